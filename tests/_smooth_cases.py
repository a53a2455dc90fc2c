"""The inputs of the particle-smoother kernel tests (tests/test_smooth_gpu.py): synthetic stored filters, no model.  Shared with
tests/test_smooth_host.py, which shows on the restatement alone that no case puts a pointer near a boundary.

Every stored value is exactly representable in fp32, so one restatement result serves the fp32 and the fp64 run of a case.
A stored filter is built the way run_filter builds one: pred[s] = a drifted copy of hist[s - 1] (slot by slot), the noise of the
case's link on top, then -- at every odd step -- a resampling (hist[s] = a gather, lwh[s] = 0), at the even ones none
(lwh[s] = random log-weights).  The cloud is as wide as the process noise, so a draw has many candidates of comparable weight.
Edges:
  q0            state 2 has q = 0 and takes three values per patient, so several candidates share a point mass
  dead          one candidate has lwh = -inf at step 0, and one pred row is NaN at every step >= 1
  patient_dead  every candidate of patient 1 is dead at step min(2, S - 1): idx = -1 and NaN from there back"""
import functools

import numpy as np

import _smooth_reference as SR

SCALE = np.array([5.0, 60.0, 80.0, 20.0, 1.0, 1.0])
TILE = 1024                        # kTile of csrc/hode_smooth.hip
LINK = {"additive": 0, "log": 1}


def _list():
    cases = []

    def add(N, M, S, B, link, edge="none"):
        cases.append(dict(N=N, M=M, S=S, B=B, link=link, edge=edge, idx=len(cases)))
    add(1, 1, 1, 1, "log")
    add(1, 65, 5, 3, "additive")
    add(2, 64, 2, 3, "additive")
    add(2, 65, 5, 1, "log", "dead")
    add(63, 65, 5, 1, "log")
    add(64, 64, 2, 3, "log", "q0")
    add(65, 300, 5, 3, "additive")
    add(65, 300, 1, 1, "log")
    add(65, 1, 5, 3, "log", "q0")
    add(257, 65, 5, 3, "log", "dead")
    add(257, 64, 5, 3, "additive", "patient_dead")
    add(257, 300, 2, 1, "additive", "q0")
    add(1000, 64, 2, 1, "additive", "dead")
    add(1000, 65, 5, 1, "log", "q0")
    add(TILE + 1, 65, 3, 1, "log", "dead")
    add(TILE + 1, 64, 2, 3, "additive")
    add(4096, 65, 3, 1, "log", "dead")
    add(4096, 1, 2, 3, "additive", "q0")
    return cases


CASES = _list()


def case_id(c):
    return f"{c['idx']}-N{c['N']}-M{c['M']}-S{c['S']}-B{c['B']}-{c['link']}-{c['edge']}"


def f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def stored_filter(rng, B, N, S, link, q, spread=0.05):
    """(hist [S, B, N, 6], lwh [S, B, N], pred [S, B, N, 6], dt [S, B]) of fp32-representable doubles."""
    truth = SCALE * (1 + 0.1 * rng.standard_normal((B, 6)))
    hist, pred, lwh = np.empty((S, B, N, 6)), np.empty((S, B, N, 6)), np.empty((S, B, N))
    dt = 1.0 + rng.random((S, B))
    dt[0] = 1.0
    quiet = ~(np.asarray(q) > 0)
    hist[0] = f32(truth[:, None, :] * np.exp(spread * rng.standard_normal((B, N, 6))))
    hist[0][:, :, quiet] = f32(truth[:, None, quiet] * (1 + 0.25 * (np.arange(N) % 3))[None, :, None])
    pred[0] = f32(truth)[:, None, :]
    lwh[0] = 0.5 * rng.standard_normal((B, N))
    for s in range(1, S):
        pred[s] = f32(hist[s - 1] * (1 + 0.01 * rng.standard_normal((B, N, 6))))
        pred[s][:, :, quiet] = hist[s - 1][:, :, quiet]
        sg = np.asarray(q) * np.sqrt(dt[s])[:, None]                            # [B, 6]
        n = rng.standard_normal((B, N, 6))
        x = pred[s] * np.exp(sg[:, None, :] * n - 0.5 * sg[:, None, :] ** 2) if link == "log" else pred[s] + sg[:, None, :] * n
        x = f32(x)
        x[:, :, quiet] = pred[s][:, :, quiet]
        if s % 2 == 1:
            anc = np.sort(rng.integers(0, N, (B, N)), axis=1)
            hist[s] = np.take_along_axis(x, anc[:, :, None], axis=1)
            lwh[s] = 0.0
        else:
            hist[s] = x
            lwh[s] = 0.5 * rng.standard_normal((B, N))
    return hist, lwh, pred, dt


@functools.lru_cache(maxsize=None)
def inputs(idx):
    c = CASES[idx]
    N, B, S = c["N"], c["B"], c["S"]
    rng = np.random.default_rng(2000 + idx)
    d = dict(c)
    q = np.array([0.05, 0.03, 0.04, 0.02, 0.1, 0.06])
    if c["edge"] == "q0":
        q[2] = 0.0
    if c["link"] == "additive":
        q = q * SCALE
    d["q"] = q
    d["hist"], d["lwh"], d["pred"], d["dt"] = stored_filter(rng, B, N, S, c["link"], q)
    d["seed"] = (0x9E3779B97F4A7C15 * (idx + 3)) & 0xFFFFFFFFFFFFFFFF
    d["id0"] = 5 * idx
    if c["edge"] == "dead" and N > 1:
        d["lwh"][0, :, N // 2] = -np.inf
        d["pred"][1:, :, N // 3] = np.nan
    if c["edge"] == "patient_dead":
        d["lwh"][min(2, S - 1), 1, :] = -np.inf
    return d


@functools.lru_cache(maxsize=None)
def reference(idx):
    """The restatement's result per patient of case idx."""
    d = inputs(idx)
    return [SR.smooth(d["hist"][:, b], d["lwh"][:, b], d["pred"][:, b], d["q"], d["dt"][:, b], d["M"], seed=d["seed"], key=d["id0"] + b,
                      link=LINK[d["link"]]) for b in range(d["B"])]

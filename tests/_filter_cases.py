"""The inputs of the particle-filter kernel tests (tests/test_filter_gpu.py), shared with tests/test_filter_host.py, which shows
on the restatement that none of them puts a resampling pointer within the summation error of a boundary.

Every value that goes to the kernel in the data's type is exactly representable in fp32, so one restatement result serves the
fp32 and the fp64 run of a case (x_out is rounded to the type when compared).  Magnitudes are those of the model's states.

The width of the particle cloud is part of the design of these cases.  The restatement draws its normals with the host's libm,
the kernel with the device's: a noised state may differ in its last bit (the GPU test allows that), and the restatement's OWN
variance therefore carries an error of 2 |x| / |x - mean| ulps for every such bit, however its sums are taken.  The stats are
held to (N + 16) * 2^-52, 18 ulps at N = 2, so the cloud is kept wide -- log-normal with a standard deviation of 0.5 on the
logarithm, 2 |x| / |x - mean| ~ 4 -- and the observation noise with it (50 % of a state's scale), so that |z| is O(1) and the
log-weights are O(10): a last-bit difference of a state then moves a log-weight by 2 ulps of z."""
import functools

import numpy as np

import _filter_reference as FR

SCALE = np.array([5.0, 60.0, 80.0, 20.0, 1.0, 1.0])
NS = (1, 2, 63, 64, 65, 256, 257, 1000, 4096)
MASKS = ("complete", "one_state", "patient_missing")
EDGES = ("none", "one_dead", "patient_dead", "one_heavy", "all_q0")


def _list():
    cases = []

    def add(N, B, link, ess, mask="complete", edge="none", n_aux=0):
        cases.append(dict(N=N, B=B, link=link, ess_frac=ess, mask=mask, edge=edge, n_aux=n_aux, idx=len(cases)))
    for k, N in enumerate(NS):                                    # every size, always resampled; B = 1 and 3 alternate
        add(N, 3 if k % 2 == 0 else 1, "log", 1.0, n_aux=(0, 3, 17)[k % 3])
        add(N, 1 if k % 2 == 0 else 3, "additive", 0.5)
    for N in (65, 257):                                           # links x thresholds x masks
        for link in ("additive", "log"):
            for ess in (0.0, 1.0, 0.5):
                for mask in MASKS:
                    add(N, 3, link, ess, mask, n_aux=3 if ess == 1.0 else 0)
    for N in (2, 257, 1000):                                      # particle edge cases, resampled
        for link in ("additive", "log"):
            for edge in EDGES[1:]:
                add(N, 3, link, 1.0, edge=edge, n_aux=17 if N == 257 else 0)
    add(4096, 3, "log", 1.0, edge="one_dead", n_aux=17)
    add(257, 3, "log", 0.0, edge="patient_dead")
    return cases


CASES = _list()


def case_id(c):
    return f"{c['idx']}-N{c['N']}-B{c['B']}-{c['link']}-ess{c['ess_frac']}-{c['mask']}-{c['edge']}-aux{c['n_aux']}"


def f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def inputs(idx):
    c = CASES[idx]
    N, B = c["N"], c["B"]
    rng = np.random.default_rng(1000 + idx)
    truth = SCALE * (1 + 0.1 * rng.standard_normal((B, 6)))
    d = dict(c)
    d["x_in"] = f32(truth[:, None, :] * np.exp(0.5 * rng.standard_normal((B, N, 6))))
    d["obs"] = f32(truth * (1 + 0.2 * rng.standard_normal((B, 6))))
    d["sigma"] = 0.5 * SCALE * (1 + 0.2 * rng.random(6))
    d["q"] = np.array([0.05, 0.03, 0.0, 0.02, 0.1, 0.0])          # two states without noise: copied bit for bit
    if c["link"] == "additive":
        d["q"] = d["q"] * SCALE
    d["dt"] = 1.0 + 4.0 * rng.random(B)
    d["lw"] = 0.5 * rng.standard_normal((B, N))
    d["status"] = None
    d["mask"] = None
    d["aux"] = f32(rng.standard_normal((B, N, c["n_aux"]))) if c["n_aux"] else None
    d["seed"] = (0x9E3779B97F4A7C15 * (idx + 1)) & 0xFFFFFFFFFFFFFFFF
    d["id0"] = 7 * idx
    d["step"] = idx % 5
    if c["mask"] == "one_state":
        d["mask"] = np.zeros((B, 6), dtype=np.uint8)
        d["mask"][:, 0] = 1
    elif c["mask"] == "patient_missing":
        d["obs"][B - 2] = np.nan                                   # by NaN for one patient ...
        d["mask"] = np.ones((B, 6), dtype=np.uint8)
        d["mask"][B - 2] = 0                                       # ... and by the mask as well
    if c["edge"] == "one_dead":
        d["status"] = np.zeros((B, N), dtype=np.int32)
        d["status"][:, N // 2] = 3
    elif c["edge"] == "patient_dead":
        d["status"] = np.zeros((B, N), dtype=np.int32)
        d["status"][1] = 3
        d["lw"][0, 0] = -np.inf                                    # and one particle dead on entry elsewhere
    elif c["edge"] == "one_heavy":
        d["lw"][:] = -800.0                                        # alive, but exp(lw - m) underflows to 0
        d["lw"][:, (2 * N) // 3] = 0.0
    elif c["edge"] == "all_q0":
        d["q"] = np.zeros(6)
    return d


@functools.lru_cache(maxsize=None)
def reference(idx):
    """The restatement's result per patient of case idx (x_out in fp64; round it to the type under test)."""
    d = inputs(idx)
    out = []
    for b in range(d["B"]):
        out.append(FR.step(d["x_in"][b], d["obs"][b], d["sigma"], d["q"], d["dt"][b], d["lw"][b], d["step"], seed=d["seed"],
                           key=d["id0"] + b, link=FR.LINK[d["link"]], ess_frac=d["ess_frac"],
                           status=None if d["status"] is None else d["status"][b],
                           mask=None if d["mask"] is None else d["mask"][b],
                           aux=None if d["aux"] is None else d["aux"][b]))
    return out

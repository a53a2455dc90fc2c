"""The inputs of the unscented smoother's tests (tests/test_ukf_smooth_host.py, tests/test_ukf_smooth_gpu.py): stored filters
built on the host by the restatement's step (tests/_ukf_reference.py), with the rows every step was handed kept as well, and the
exact Kalman RTS smoother of the two linear-Gaussian models of tests/_ukf_cases.py.  Computed once, shared, never modified.

Every value a kernel reads in the data's type (the emitted points, their constants, the propagated rows) is a float32 number, so
the fp32 and the fp64 instantiation see the same inputs and share one reference."""
import functools

import numpy as np

import _ukf_cases as UC
import _ukf_reference as UR
import _ukf_smooth_reference as SR

S_STEPS = 4
#            P, B, link, S, edge
SPECS = [dict(P=0, B=3, link=1, S=S_STEPS),
         dict(P=0, B=5, link=0, S=S_STEPS),
         dict(P=2, B=3, link=0, S=S_STEPS),
         dict(P=2, B=5, link=1, S=S_STEPS, edge="lost"),                # patient 1 is lost at step 2
         dict(P=17, B=3, link=1, S=S_STEPS),
         dict(P=17, B=5, link=0, S=S_STEPS),
         dict(P=1, B=3, link=1, S=S_STEPS, edge="zero_state"),
         dict(P=1, B=3, link=0, S=S_STEPS, edge="zero_state"),
         dict(P=2, B=3, link=1, S=1)]


def case_id(s):
    return f"P{s['P']}-B{s['B']}-{'log' if s['link'] else 'add'}-S{s['S']}" + (f"-{s['edge']}" if s.get("edge") else "")


def _carry(x, aux, cols):
    """A smooth positive map of a step's emitted rows to the rows handed to the next step (what a solve does, for the smoother's
    purposes): every state relaxes towards its scale, pulled by its neighbour and by the learned constants."""
    nxt = np.roll(x, -1, axis=1) / np.roll(UC.SCALE, -1)
    pull = np.prod(aux[:, cols], axis=1, keepdims=True) ** (0.2 / len(cols)) if cols else 1.0
    return 1.05 * UC.SCALE ** 0.1 * x ** 0.9 * nxt ** 0.2 * pull


def make_case(P, B, link, S, edge=None, seed=0):
    """A stored filter of S steps for B patients: a dict of numpy arrays, step-major as the C ABI takes them."""
    c0 = UC.make_case(P, B, link, 0, "complete", edge="zero_state" if edge == "zero_state" else None, seed=500 + seed)
    rng = np.random.default_rng(7000 + seed)
    mode, w, n, K = c0["mode"], c0["w"], c0["n"], c0["K"]
    cols, _ = UR.columns(mode)
    hist, prop, ode = np.zeros((S, B, K, 6)), np.zeros((S, B, K, 6)), np.zeros((S, B, K, 17))
    mean_f, cov_f = np.full((S, B, n), np.nan), np.full((S, B, n, n), np.nan)
    alive, dt = np.zeros((S, B), dtype=np.int32), np.ones((S, B))
    dt[1:] = 0.5 + rng.random((S - 1, B))
    for b in range(B):
        mean, cov, live = c0["mean"][b].copy(), c0["cov"][b].copy(), 1
        if edge == "zero_state":                                    # state 2 is known exactly: value 1, no spread, no noise
            mean[2] = 0.0 if link == 1 else 1.0
            cov[2, :] = 0.0
            cov[:, 2] = 0.0
        x, aux = c0["x_in"][b].copy(), c0["aux_in"][b].copy()
        for s in range(S):
            status = None
            if s > 0:
                x = UC._f32(_carry(x, aux, cols))
                if edge == "zero_state":
                    x[:, 2] = 1.0
                if edge == "lost" and b == 1 and s == 2:
                    status = np.zeros(K, dtype=np.int32)
                    status[3] = 2
            obs = UC._f32(UC.SCALE * (1 + 0.05 * rng.standard_normal(6)))
            if s == S - 2 and b == 0:
                obs[:] = np.nan                                     # a step that sees nothing
            elif (s + b) % 3 == 1:
                obs[[1, 4]] = np.nan
            prop[s, b] = x
            r = UR.step(x, aux, mode, obs, c0["sigma"], c0["q"], c0["walk"], dt[s, b], live, mean, cov, w, predict=s > 0, link=link,
                        status=status)
            live, mean, cov = r["alive"], r["mean"], r["cov"]
            x, aux = UC._f32(r["x_out"]), UC._f32(r["aux_out"])
            hist[s, b], ode[s, b], mean_f[s, b], cov_f[s, b], alive[s, b] = x, aux, mean, cov, live
    return {"P": P, "B": B, "S": S, "n": n, "K": K, "link": link, "edge": edge, "mode": mode, "w": w, "q": c0["q"], "walk": c0["walk"],
            "hist": hist, "ode": ode, "prop": prop, "mean_f": mean_f, "cov_f": cov_f, "alive": alive, "dt": dt}


@functools.lru_cache(maxsize=None)
def case(idx):
    return make_case(seed=idx, **SPECS[idx])


def smooth_patient(c, b):
    return SR.smooth(c["hist"][:, b], c["ode"][:, b], c["prop"][:, b], c["mean_f"][:, b], c["cov_f"][:, b], c["alive"][:, b], c["mode"],
                     c["q"], c["walk"], c["dt"][:, b], c["w"], c["link"])


@functools.lru_cache(maxsize=None)
def reference(idx):
    """The restatement's whole pass for every patient of a case."""
    c = case(idx)
    return [smooth_patient(c, b) for b in range(c["B"])]


# ------------------------------------------------------------------ linear-Gaussian models
def filter_linear_model(M, step_fn=None, ys=None, dead_at=None):
    """The unscented filter on a linear model of tests/_ukf_cases.py with the identity links, as UC.ukf_on_linear_model runs it,
    with everything the smoother reads kept: a one-patient case dict in the layout of make_case (B = 1).  `ys`: another record;
    `dead_at`: a step that is handed a non-zero solve status."""
    n, K, cols, S = M["n"], 2 * M["n"] + 1, M["cols"], M["S"]
    ys = M["ys"] if ys is None else ys
    w = UR.weights(n)
    x, aux = np.zeros((K, 6)), np.ones((K, 17))
    mean, cov, live = M["m0"].copy(), M["P0"].copy(), 1
    hist, prop, ode = np.zeros((S, 1, K, 6)), np.zeros((S, 1, K, 6)), np.zeros((S, 1, K, 17))
    mean_f, cov_f, alive = np.zeros((S, 1, n)), np.zeros((S, 1, n, n)), np.zeros((S, 1), dtype=np.int32)
    for s in range(S):
        if s > 0:
            x = x @ M["A"].T + aux[:, cols] @ M["Bm"].T
        status = None
        if dead_at is not None and s == dead_at:
            status = np.ones(K, dtype=np.int32)
        prop[s, 0] = x
        r = UR.step(x, aux, M["mode"], ys[s], M["sigma"], M["q"], M["walk"], M["dts"][s], live, mean, cov, w, predict=s > 0, link=0,
                    status=status)
        x, aux, mean, cov, live = r["x_out"], r["aux_out"], r["mean"], r["cov"], r["alive"]
        hist[s, 0], ode[s, 0], mean_f[s, 0], cov_f[s, 0], alive[s, 0] = x, aux, mean, cov, live
    return {"P": n - 6, "B": 1, "S": S, "n": n, "K": K, "link": 0, "edge": None, "mode": M["mode"], "w": w, "q": M["q"], "walk": M["walk"],
            "hist": hist, "ode": ode, "prop": prop, "mean_f": mean_f, "cov_f": cov_f, "alive": alive, "dt": M["dts"][:S, None].copy()}


def kalman_rts(M, ys=None):
    """The exact Rauch-Tung-Striebel smoother of a linear model on its Kalman filter UC.kalman: per step (mean, covariance)."""
    n = M["n"]
    F = np.eye(n)
    F[:6, :6], F[:6, 6:] = M["A"], M["Bm"]
    filt = UC.kalman(M if ys is None else dict(M, ys=ys))
    S = len(filt)
    out = [None] * S
    out[S - 1] = (filt[S - 1][1], filt[S - 1][2])
    for s in range(S - 2, -1, -1):
        m, P = filt[s][1], filt[s][2]
        Q = np.diag(np.concatenate([M["q"] ** 2, M["walk"][M["cols"]] ** 2]) * M["dts"][s + 1])
        mp, Pp = F @ m, F @ P @ F.T + Q
        G = np.linalg.solve(Pp, F @ P).T                            # P F^T Pp^-1 (P and Pp symmetric)
        ms, Ps = out[s + 1]
        out[s] = (m + G @ (ms - mp), P + G @ (Ps - Pp) @ G.T)
    return out

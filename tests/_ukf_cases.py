"""The inputs of the unscented Kalman filter's tests (tests/test_ukf_host.py, tests/test_ukf_gpu.py): the step kernel's cases with
their restatement results (computed once, shared, never modified), and the two linear-Gaussian models with the Kalman filter
they are held to.

Every value a kernel reads in the data's type (x_in, aux_in, obs) is a float32 number, so the fp32 and the fp64 instantiation see
the same inputs and share one reference."""
import functools
import itertools
import math

import numpy as np

import _ukf_reference as UR

SCALE = np.array([5.0, 1.0, 0.5, 2.0, 1.0, 3.0])
MODES = {0: {}, 1: {3: 2}, 2: {2: 1, 11: 2}, 17: {c: 1 + (c % 2) for c in range(17)}}      # column -> link (1 identity, 2 log)
MASKS = ("complete", "one", "none", "mixed")
COND_CAP = 1e6


def mode_of(P):
    mode = np.zeros(17, dtype=np.int32)
    for c, v in MODES[P].items():
        mode[c] = v
    return mode


def _f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def make_case(P, B, link, predict, mask, edge=None, seed=0):
    """One call of the step kernel for B patients: a dict of numpy arrays (fp64 holding float32 values where the kernel reads the
    data's type) plus the host arguments."""
    rng = np.random.default_rng(1000 + seed)
    mode = mode_of(P)
    cols, plog = UR.columns(mode)
    n, K = 6 + P, 2 * (6 + P) + 1
    slog = link == 1
    islog = np.array([slog] * 6 + plog)
    w = UR.weights(n)
    if edge == "zero_state":
        w = UR.weights(n, kappa=float(2 ** math.ceil(math.log2(n + 1)) - n))        # n + kappa a power of two: dyadic weights
    centre = np.concatenate([SCALE, np.ones(P)])
    sd = np.where(islog, 0.1, 0.05 * centre)
    x_in, aux_in, mean, cov = np.empty((B, K, 6)), np.empty((B, K, 17)), np.empty((B, n)), np.empty((B, n, n))
    for b in range(B):
        A = rng.standard_normal((n, n))
        P0 = np.diag(sd) @ (A @ A.T / n + 0.5 * np.eye(n)) @ np.diag(sd)
        m0 = np.where(islog, np.log(centre), centre) + sd * rng.standard_normal(n)
        if edge == "zero_given":                                    # state 2 and the last coordinate are known exactly
            for j in (2, n - 1):
                P0[j, :] = 0.0
                P0[:, j] = 0.0
        if edge == "zero_cov":
            P0[:] = 0.0
        mean[b], cov[b] = m0, 0.5 * (P0 + P0.T)
        L, _, _ = UR.cholesky(cov[b])
        Z = UR.draw(m0, L, w[0]) + 0.1 * sd * rng.standard_normal((K, n))
        nat = np.where(islog, np.exp(Z), Z)
        carried = 0.5 + rng.random(17)
        x_in[b] = nat[:, :6]
        aux_in[b] = carried
        aux_in[b][:, cols] = nat[:, 6:]
    x_in, aux_in = _f32(x_in), _f32(aux_in)
    obs = _f32(SCALE * (1 + 0.05 * rng.standard_normal((B, 6))))
    mk = None
    if mask == "one":
        mk = np.zeros((B, 6), dtype=np.uint8)
        mk[:, 0] = 1
    elif mask == "none":
        obs[:] = np.nan
    elif mask == "mixed":
        obs[1 % B] = np.nan
    q = np.array([0.05, 0.03, 0.0, 0.02, 0.1, 0.04]) * (1.0 if slog else SCALE)
    status = None
    alive = np.ones(B, dtype=np.int32)
    if edge == "zero_state":                                        # state 2: no spread in, no process noise -> an exact zero column
        x_in[:, :, 2] = 1.0
    elif edge == "lost_entry":
        alive[1] = 0
    elif edge == "lost_status":
        status = np.zeros((B, K), dtype=np.int32)
        status[1, 4] = 2
    elif edge == "lost_nan":
        x_in[1, 3, 2] = np.nan
    elif edge == "lost_nan_par":
        aux_in[2, K - 1, cols[0]] = np.nan
    elif edge == "lost_nonpos":
        x_in[1, 0, 5] = 0.0
    elif edge == "lost_nonpos_par":
        aux_in[0, 2, cols[-1]] = -1.0
    return {"P": P, "B": B, "n": n, "K": K, "link": link, "predict": predict, "mask_kind": mask, "edge": edge, "mode": mode, "w": w,
            "x_in": x_in, "aux_in": aux_in, "obs": obs, "mask": mk, "status": status, "sigma": 0.1 * SCALE, "q": q,
            "walk": np.full(17, 0.02), "dt": 0.5 + rng.random(B), "alive": alive, "mean": mean, "cov": cov}


def _specs():
    out = []
    # every (P, B), the other dimensions rotating through their values
    for i, (P, B) in enumerate(itertools.product((0, 1, 2, 17), (1, 3, 9))):
        out.append(dict(P=P, B=B, link=i % 2, predict=(i // 2) % 2, mask=MASKS[(i + i // 4) % 4]))
    # every (state link, predict, mask) at mixed parameter links
    for link, predict, mask in itertools.product((0, 1), (0, 1), MASKS):
        out.append(dict(P=2, B=3, link=link, predict=predict, mask=mask))
    # the edge cases
    out += [dict(P=1, B=3, link=0, predict=1, mask="complete", edge="zero_state"),
            dict(P=1, B=3, link=1, predict=1, mask="complete", edge="zero_state"),
            dict(P=2, B=3, link=1, predict=0, mask="complete", edge="zero_given"),
            dict(P=1, B=3, link=1, predict=0, mask="one", edge="zero_cov"),
            dict(P=1, B=3, link=0, predict=0, mask="complete", edge="zero_cov"),
            dict(P=1, B=3, link=1, predict=1, mask="complete", edge="lost_entry"),
            dict(P=1, B=3, link=1, predict=0, mask="complete", edge="lost_entry"),
            dict(P=1, B=3, link=1, predict=1, mask="complete", edge="lost_status"),
            dict(P=0, B=3, link=0, predict=1, mask="complete", edge="lost_nan"),
            dict(P=2, B=3, link=1, predict=1, mask="one", edge="lost_nan_par"),
            dict(P=0, B=9, link=1, predict=1, mask="complete", edge="lost_nonpos"),
            dict(P=2, B=3, link=0, predict=1, mask="mixed", edge="lost_nonpos_par")]
    return out


SPECS = _specs()


def case_id(s):
    return f"P{s['P']}-B{s['B']}-{'log' if s['link'] else 'add'}-{'predict' if s['predict'] else 'given'}-{s['mask']}" + \
        (f"-{s['edge']}" if s.get("edge") else "")


@functools.lru_cache(maxsize=None)
def case(idx):
    return make_case(seed=idx, **SPECS[idx])


def reference_of(c):
    """The restatement's result for every patient of a case."""
    return [UR.step(c["x_in"][b], c["aux_in"][b], c["mode"], c["obs"][b], c["sigma"], c["q"], c["walk"], c["dt"][b], int(c["alive"][b]),
                    c["mean"][b], c["cov"][b], c["w"], predict=bool(c["predict"]), link=c["link"],
                    status=None if c["status"] is None else c["status"][b], mask=None if c["mask"] is None else c["mask"][b])
            for b in range(c["B"])]


@functools.lru_cache(maxsize=None)
def reference(idx):
    return reference_of(case(idx))


# ------------------------------------------------------------------ linear-Gaussian models
def linear_model(which):
    """Model 1: 6 states, 9 steps, random partial masks, one step with nothing observed.  Model 2: 6 states plus 2 unknown
    constants entering linearly, 12 steps, state 3 without process noise, state 1 known exactly at the start (a singular
    covariance).  x_s = A x_{s-1} + Bm theta + N(0, diag(q^2 dt_s)), theta_s = theta_{s-1} + N(0, diag(walk^2 dt_s)),
    y_s = x_s + N(0, diag(sigma^2)) on the seen entries."""
    rng = np.random.default_rng(40 + which)
    npar, S = (0, 9) if which == 1 else (2, 12)
    A = np.eye(6) * 0.9 + 0.05 * rng.standard_normal((6, 6))
    Bm = 0.3 * rng.standard_normal((6, npar))
    q = np.array([0.3, 0.2, 0.1, 0.25, 0.3, 0.1])
    walk = np.zeros(17)
    mode = np.zeros(17, dtype=np.int32)
    cols = [4, 9][:npar]
    mode[cols] = 1
    p0 = np.concatenate([np.full(6, 0.5), np.full(npar, 0.4)])
    if which == 2:
        q[3] = 0.0
        p0[1] = 0.0
        walk[cols[1]] = 0.05
    m0 = rng.standard_normal(6 + npar)
    sigma = np.full(6, 0.7)
    dts = np.concatenate([[1.0], 0.5 + rng.random(S - 1)])
    truth = m0 + p0 * rng.standard_normal(6 + npar)
    ys = []
    for s in range(S):
        if s > 0:
            truth[:6] = A @ truth[:6] + Bm @ truth[6:] + q * math.sqrt(dts[s]) * rng.standard_normal(6)
            truth[6:] = truth[6:] + walk[cols] * math.sqrt(dts[s]) * rng.standard_normal(npar)
        y = truth[:6] + sigma * rng.standard_normal(6)
        y[rng.random(6) < 0.3] = np.nan
        ys.append(y)
    ys[4][:] = np.nan                                               # one step with nothing observed
    return {"A": A, "Bm": Bm, "q": q, "walk": walk, "mode": mode, "cols": cols, "m0": m0, "P0": np.diag(p0 ** 2), "sigma": sigma,
            "dts": dts, "ys": np.array(ys), "n": 6 + npar, "S": S}


def kalman(M):
    """The Kalman filter of a linear model: per step the evidence increment, the filtered mean and covariance."""
    n, npar = M["n"], M["n"] - 6
    F = np.eye(n)
    F[:6, :6], F[:6, 6:] = M["A"], M["Bm"]
    m, P = M["m0"].copy(), M["P0"].copy()
    out = []
    for s, y in enumerate(M["ys"]):
        if s > 0:
            Q = np.diag(np.concatenate([M["q"] ** 2, M["walk"][M["cols"]] ** 2]) * M["dts"][s])
            m, P = F @ m, F @ P @ F.T + Q
        on = np.isfinite(y)
        inc = 0.0
        if on.any():
            H = np.eye(n)[:6][on]
            S = H @ P @ H.T + np.diag(M["sigma"][on] ** 2)
            r = y[on] - H @ m
            inc = -0.5 * (r @ np.linalg.solve(S, r) + np.linalg.slogdet(S)[1] + on.sum() * math.log(2 * math.pi))
            G = P @ H.T @ np.linalg.inv(S)
            m, P = m + G @ r, (np.eye(n) - G @ H) @ P @ (np.eye(n) - G @ H).T + G @ np.diag(M["sigma"][on] ** 2) @ G.T
        out.append((inc, m.copy(), P.copy()))
    return out


def ukf_on_linear_model(M, step_fn):
    """The unscented filter on a linear model with the identity links, the propagation x_in = A chi_x + Bm chi_theta formed here.
    step_fn(x_in, aux_in, obs, dt, alive, mean, cov, predict) -> a dict as UR.step returns.  Per step (increment, mean, cov)."""
    n, K, cols = M["n"], 2 * M["n"] + 1, M["cols"]
    x, aux = np.zeros((K, 6)), np.ones((K, 17))
    mean, cov, alive = M["m0"].copy(), M["P0"].copy(), 1
    out = []
    for s in range(M["S"]):
        if s > 0:
            x = x @ M["A"].T + aux[:, cols] @ M["Bm"].T
        r = step_fn(x, aux, M["ys"][s], M["dts"][s], alive, mean, cov, s > 0)
        x, aux, mean, cov, alive = r["x_out"], r["aux_out"], r["mean"], r["cov"], r["alive"]
        out.append((r["stats"][0], mean.copy(), cov.copy()))
    return out

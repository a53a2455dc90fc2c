"""The inputs of the EM noise fit's tests (tests/test_ukf_em_host.py, tests/test_ukf_em_gpu.py): the stored filters of
tests/_ukf_smooth_cases.py with the restatement's smoother over them, the rows one E-step propagates, a record to hold the
smoothed moments against, and the restatement's statistics; and the E-step, the exact Kalman-smoother statistic and the evidence
on the linear-Gaussian models of tests/_ukf_cases.py.  Computed once, shared, never modified.

Every value a kernel reads in the data's type (the constants, the propagated rows, the record) is a float32 number, so the fp32
and the fp64 instantiation see the same inputs and share one reference."""
import functools

import numpy as np

import _ukf_cases as UC
import _ukf_em_reference as ER
import _ukf_reference as UR
import _ukf_smooth_cases as SC

SPECS = SC.SPECS                                                    # P in {0, 2, 17} x B in {3, 5}, both links, a lost patient, an
case_id = SC.case_id                                                # exact coordinate under both links, S = 1
STATUS_CASE, STATUS_PAIR, STATUS_PATIENT = 1, 1, 2                  # one pair whose solve reports a failed row
SIGMA = 0.1 * UC.SCALE
SMOOTHED = ("mean_s", "cov_s", "gain", "moments")


@functools.lru_cache(maxsize=None)
def case(idx):
    """Everything one E-step and one M-step read and give on the stored filter SC.case(idx): a dict of numpy arrays, step-major
    as the C ABI takes them (obs and mask patient-major)."""
    c, refs = SC.case(idx), SC.reference(idx)
    S, B, n, K, mode, w, link = c["S"], c["B"], c["n"], c["K"], c["mode"], c["w"], c["link"]
    cols, _ = UR.columns(mode)
    rng = np.random.default_rng(9000 + idx)
    out = {k: c[k] for k in ("P", "B", "S", "n", "K", "link", "edge", "mode", "w", "q", "walk", "dt", "alive", "ode")}
    for name in SMOOTHED:
        out[name] = np.stack([r[name] for r in refs], axis=1)
    # ---- a. the points of every pair's first step, b. their images (what a solve does, for the statistic's purposes)
    x_em, aux_em = np.zeros((S - 1, B * K, 6)), np.zeros((S - 1, B * K, 17))
    chol, cond = np.zeros((S - 1, B, n, n)), np.full((S - 1, B), np.nan)
    for s in range(S - 1):
        for b in range(B):
            p = ER.points(out["mean_s"][s, b], out["cov_s"][s, b], c["ode"][s, b, 0], mode, w, link) if c["alive"][s + 1, b] else \
                ER.dead_points(c["ode"][s, b, 0], n)
            x_em[s, b * K:(b + 1) * K], aux_em[s, b * K:(b + 1) * K], chol[s, b], cond[s, b] = p["x"], p["aux"], p["chol"], p["cond"]
    prop = np.zeros_like(x_em)
    for s in range(S - 1):
        for b in range(B):
            rows = slice(b * K, (b + 1) * K)
            prop[s, rows] = UC._f32(SC._carry(UC._f32(x_em[s, rows]), UC._f32(aux_em[s, rows]), cols))
    if c["edge"] == "zero_state":
        prop[:, :, 2] = 1.0
    status = np.zeros((max(S - 1, 0), B * K), dtype=np.int32)
    if idx == STATUS_CASE:
        status[STATUS_PAIR, STATUS_PATIENT * K + 5] = 3
    # ---- the record: one step with nothing seen, missing entries, and (odd cases) a mask with one step where one state is seen
    obs = UC._f32(UC.SCALE * (1 + 0.05 * rng.standard_normal((B, S, 6))))
    obs[0, max(S - 2, 0)] = np.nan
    for b in range(B):
        for s in range(S):
            if (s + b) % 3 == 1:
                obs[b, s, [1, 4]] = np.nan
    mask = None
    if idx % 2 == 1:
        mask = np.ones((B, S, 6), dtype=np.uint8)
        mask[:, min(1, S - 1), 1:] = 0
    out.update(x_em=x_em, aux_em=aux_em, chol=chol, cond=cond, prop=prop, status=status, obs=obs, mask=mask, sigma=SIGMA.copy())
    # ---- c, d. the statistics
    e2, pair_ok, scale = np.full((S - 1, B, n), np.nan), np.zeros((S - 1, B), dtype=np.int32), np.full((S - 1, B), np.nan)
    r2, seen = np.zeros((S, B, 6)), np.zeros((S, B), dtype=np.int32)
    for b in range(B):
        for s in range(S - 1):
            rows = slice(b * K, (b + 1) * K)
            r = ER.pair(prop[s, rows], status[s, rows], chol[s, b], out["mean_s"][s, b], out["mean_s"][s + 1, b], out["cov_s"][s + 1, b],
                        out["gain"][s, b], c["alive"][s + 1, b], w, link)
            e2[s, b], pair_ok[s, b] = r["e2"], r["ok"]
            if r["ok"]:
                scale[s, b] = r["scale"]
        for s in range(S):
            r2[s, b], seen[s, b] = ER.obs(obs[b, s], None if mask is None else mask[b, s], c["alive"][s, b], out["moments"][s, b])
    out.update(e2=e2, pair_ok=pair_ok, scale=scale, r2=r2, seen=seen)
    # ---- e. the sums and one update: two values left out of the fit, one held up by its floor
    fit_mask, floor = np.ones(ER.FIT, dtype=np.int32), np.full(ER.FIT, 1e-6)
    fit_mask[1], fit_mask[23 + 4], floor[0] = 0, 0, 10.0
    sums = ER.reduce(e2, pair_ok, r2, seen, c["dt"])
    new = ER.mstep(sums, c["q"], c["walk"], SIGMA, mode, fit_mask, floor, link)
    out.update(fit_mask=fit_mask, floor=floor, sums=sums, new_q=new[0], new_walk=new[1], new_sigma=new[2])
    return out


def select(c, b):
    """Patient b of a case alone (B = 1), for the bits of a patient beside others."""
    K = c["K"]
    rows = slice(b * K, (b + 1) * K)
    out = dict(c, B=1)
    for k in ("mean_s", "cov_s", "gain", "moments", "alive", "dt", "ode", "chol", "e2", "pair_ok", "r2", "seen"):
        out[k] = c[k][:, b:b + 1]
    for k in ("x_em", "aux_em", "prop", "status"):
        out[k] = c[k][:, rows]
    out["obs"], out["mask"] = c["obs"][b:b + 1], None if c["mask"] is None else c["mask"][b:b + 1]
    return out


# ------------------------------------------------------------------ linear-Gaussian models
def transition(M):
    F = np.eye(M["n"])
    F[:6, :6], F[:6, 6:] = M["A"], M["Bm"]
    return F


def simulate(M, S, B, seed):
    """B records of S steps from the linear model M itself (its dts drawn afresh): (M with S and dts replaced, ys [B, S, 6])."""
    rng = np.random.default_rng(seed)
    n, npar, cols = M["n"], M["n"] - 6, M["cols"]
    dts = np.concatenate([[1.0], 0.5 + rng.random(S - 1)])
    p0 = np.sqrt(np.diag(M["P0"]))
    ys = np.empty((B, S, 6))
    for b in range(B):
        truth = M["m0"] + p0 * rng.standard_normal(n)
        for s in range(S):
            if s > 0:
                truth[:6] = M["A"] @ truth[:6] + M["Bm"] @ truth[6:] + M["q"] * np.sqrt(dts[s]) * rng.standard_normal(6)
                truth[6:] = truth[6:] + M["walk"][cols] * np.sqrt(dts[s]) * rng.standard_normal(npar)
            ys[b, s] = truth[:6] + M["sigma"] * rng.standard_normal(6)
            ys[b, s][rng.random(6) < 0.2] = np.nan
    return dict(M, S=S, dts=dts, ys=ys[0]), ys


def evidence(M, ys):
    """The exact log-evidence of the records ys [B, S, 6] under the linear model M: the Kalman filter's."""
    return float(sum(sum(inc for inc, _, _ in UC.kalman(dict(M, ys=y))) for y in ys))


def estep_linear(M, ys, propagate=None):
    """One E-step of the restatement on the records ys [B, S, 6] of the linear model M with the identity links: the filter and the
    smoother of tests/_ukf_smooth_cases.py, then the points, x+ = A chi_x + Bm chi_theta, the statistics.  Returns a dict of
    step-major arrays (e2, pair_ok, r2, seen, dt, V) and the per-patient smoothed results."""
    B, S, n, cols, w = len(ys), M["S"], M["n"], M["cols"], UR.weights(M["n"])
    e2, pair_ok, V = np.zeros((S - 1, B, n)), np.zeros((S - 1, B), dtype=np.int32), np.zeros((S - 1, B, n, n))
    r2, seen, smoothed = np.zeros((S, B, 6)), np.zeros((S, B), dtype=np.int32), []
    for b in range(B):
        c = SC.filter_linear_model(M, ys=ys[b])
        sm = SC.smooth_patient(c, 0)
        smoothed.append(sm)
        for s in range(S - 1):
            p = ER.points(sm["mean_s"][s], sm["cov_s"][s], c["ode"][s, 0, 0], M["mode"], w, link=0)
            prop = p["x"] @ M["A"].T + p["aux"][:, cols] @ M["Bm"].T
            r = ER.pair(prop, None, p["chol"], sm["mean_s"][s], sm["mean_s"][s + 1], sm["cov_s"][s + 1], sm["gain"][s], c["alive"][s + 1, 0],
                        w, link=0)
            e2[s, b], pair_ok[s, b], V[s, b] = r["e2"], r["ok"], r["V"]
        for s in range(S):
            r2[s, b], seen[s, b] = ER.obs(ys[b][s], None, c["alive"][s, 0], sm["moments"][s])
    return {"e2": e2, "pair_ok": pair_ok, "r2": r2, "seen": seen, "dt": np.repeat(M["dts"][:S, None], B, axis=1), "V": V, "smoothed": smoothed}


def exact_statistics(M, y):
    """The exact Kalman-smoother values of one record y [S, 6]: e2 [S-1, n] = the diagonal of E[(x_{s+1} - F x_s)(.)^T | y] =
    Ps_{s+1} - F G_s Ps_{s+1} - (.)^T + F Ps_s F^T + (ms_{s+1} - F ms_s)(.)^T, and r2 [S, 6] = (y - H ms)^2 + diag(H Ps H^T)
    on the seen entries (0 elsewhere); `scale` [S-1] = the largest term of e2's sum."""
    n, S, F = M["n"], M["S"], transition(M)
    filt, rts = UC.kalman(dict(M, ys=y)), SC.kalman_rts(M, ys=y)
    e2, scale, r2 = np.zeros((S - 1, n)), np.zeros(S - 1), np.zeros((S, 6))
    for s in range(S - 1):
        m, P = filt[s][1], filt[s][2]
        Q = np.diag(np.concatenate([M["q"] ** 2, M["walk"][M["cols"]] ** 2]) * M["dts"][s + 1])
        G = np.linalg.solve(F @ P @ F.T + Q, F @ P).T
        (ms, Ps), (mn, Pn) = rts[s], rts[s + 1]
        cross, d = F @ G @ Pn, mn - F @ ms
        terms = (Pn, cross, F @ Ps @ F.T, np.outer(d, d))
        e2[s] = np.diag(Pn - cross - cross.T + terms[2] + terms[3])
        scale[s] = max(np.abs(np.diag(t)).max() for t in terms)
    for s in range(S):
        ms, Ps = rts[s]
        on = np.isfinite(y[s])
        r2[s][on] = (y[s][on] - ms[:6][on]) ** 2 + np.diag(Ps)[:6][on]
    return e2, r2, scale


def em_linear(M, ys, n_iter, fit_mask, floor=None):
    """n_iter EM iterations of the restatement on the linear model M from its own q, walk, sigma.  Returns ([the model before
    every iteration and after the last], [the sums of every iteration])."""
    floor = np.full(ER.FIT, 1e-6) if floor is None else floor
    models, sums = [M], []
    for _ in range(n_iter):
        e = estep_linear(M, ys)
        sm = ER.reduce(e["e2"], e["pair_ok"], e["r2"], e["seen"], e["dt"])
        q, walk, sigma = ER.mstep(sm, M["q"], M["walk"], M["sigma"], M["mode"], fit_mask, floor, link=0)
        M = dict(M, q=q, walk=walk, sigma=sigma)
        models.append(M)
        sums.append(sm)
    return models, sums

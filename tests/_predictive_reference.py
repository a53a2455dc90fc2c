"""NumPy fp64 restatement of the fold and score kernels of csrc/hode_predictive.hip (include/hode.h, "Posterior-predictive
summaries"), written from the specification: the same sequential Welford update draw by draw, the same skip rules, the same
formulae and column order.  The GPU tests compare the kernels with it; the host tests hold it to the values captured from the
reference's eval/evaluate.py (tests/golden/eval/calibration.npz) and to a two-pass long-double computation.  Plays the role of
_sobol_reference.py and _nuts_reference.py."""
import math
from statistics import NormalDist

import numpy as np

FIXED = 16            # HODE_PRED_FIXED_COLS
Z_LEVELS = (0.6744897501960817, 1.2815515655446004, 1.6448536269514722, 1.96)
_erfc = np.vectorize(math.erfc, otypes=[np.float64])
STATE_KEYS = ("n", "mean", "m2", "pit", "lmax", "lsum")


def thresholds(n_bins):
    """t_j with P(|Z| <= t_j) = j / n_bins: the half-normal quantiles sqrt(2) erfinv(j / n_bins)."""
    nd = NormalDist()
    return np.array([nd.inv_cdf(0.5 * (1.0 + j / n_bins)) for j in range(n_bins)])


def fresh_state(N):
    z = lambda: np.zeros(N, dtype=np.float64)                                                   # noqa: E731
    return {"n": np.zeros(N, dtype=np.int32), "mean": z(), "m2": z(), "pit": z(), "lmax": np.full(N, -np.inf), "lsum": z()}


def observed(obs, mask, N):
    if obs is None:
        return np.zeros(N, dtype=bool)
    on = np.isfinite(np.asarray(obs, dtype=np.float64).reshape(-1))
    if mask is not None:
        on &= np.asarray(mask).reshape(-1) != 0
    return on


def fold(state, y, obs=None, mask=None, sigma=None, status=None):
    """Fold y [S, N] into state, one draw at a time in draw order.  sigma [S, 6] or None; status [S, n_traj] or None."""
    y = np.asarray(y, dtype=np.float64)
    S, N = y.shape
    on = observed(obs, mask, N)
    o = np.zeros(N)                                    # (an unobserved entry's obs value never enters any arithmetic)
    if obs is not None:
        o[on] = np.asarray(obs, dtype=np.float64).reshape(-1)[on]
    k = np.arange(N) % 6
    n, mean, m2, pit, lmax, lsum = (state[key] for key in STATE_KEYS)
    for s in range(S):
        take = np.isfinite(y[s])
        if status is not None:
            st = np.asarray(status)[s]
            take &= np.repeat(st == 0, N // st.size)
        ys = np.where(take, y[s], 0.0)
        n1 = n + take.astype(np.int32)
        d = ys - mean
        mean1 = mean + d / np.maximum(n1, 1)
        m21 = m2 + d * (ys - mean1)
        mean[:] = np.where(take, mean1, mean)
        m2[:] = np.where(take, m21, m2)
        n[:] = n1
        seen = take & on
        if sigma is not None:
            sg = np.asarray(sigma, dtype=np.float64)[s][k]
            noisy = seen & (sg > 0)
        else:
            sg, noisy = np.ones(N), np.zeros(N, dtype=bool)
        plain = seen & ~noisy
        pit[:] = np.where(plain, pit + np.where(ys < o, 1.0, np.where(ys == o, 0.5, 0.0)), pit)
        if noisy.any():
            sgs = np.where(noisy, sg, 1.0)
            z = (o - ys) / sgs
            pit[:] = np.where(noisy, pit + 0.5 * _erfc(-z * 0.70710678118654752440), pit)
            lp = -0.5 * z * z - np.log(sgs) - 0.91893853320467274178
            up = noisy & (lp > lmax)
            keep = noisy & ~up
            with np.errstate(invalid="ignore", over="ignore"):
                ls_up = lsum * np.exp(np.where(up, lmax - lp, 0.0)) + 1.0
                ls_keep = lsum + np.exp(np.where(keep, lp - lmax, 0.0))
            lsum[:] = np.where(up, ls_up, np.where(keep, ls_keep, lsum))
            lmax[:] = np.where(up, lp, lmax)
    return state


def score(state, obs=None, mask=None, extra_var=None, thr=None):
    """(mean, sd, pit, table [6, FIXED + 2 n_bins]) of a finished state, all fp64; also the values whose distance to a decision
    boundary `clear_of_edges` checks."""
    thr = thresholds(10) if thr is None else np.asarray(thr, dtype=np.float64)
    nb = len(thr)
    n = state["n"].astype(np.int64)
    N = n.size
    k = np.arange(N) % 6
    ev = np.zeros(6) if extra_var is None else np.asarray(extra_var, dtype=np.float64)
    on = observed(obs, mask, N)
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = np.where(n >= 1, state["mean"], np.nan)
        sd = np.where(n >= 2, np.sqrt(state["m2"] / np.maximum(n - 1, 1) + ev[k]), np.nan)
        pit = np.where((n >= 2) & on, state["pit"] / np.maximum(n, 1), np.nan)
    table = np.zeros((6, FIXED + 2 * nb))
    edges = {"norm": [], "bound": [], "pit": []}
    o_all = np.asarray(obs, dtype=np.float64).reshape(-1) if obs is not None else np.zeros(N)
    for s in range(6):
        a = on & (k == s) & (n >= 1)
        o, mu = o_all[a], mean[a]
        e = mu - o
        table[s, 0:5] = a.sum(), np.sum(e * e), np.sum(np.abs(e)), np.sum(o), np.sum(o * o)
        b = on & (k == s) & (n >= 2)
        if not b.any():
            continue
        o, mu, sg, pv = o_all[b], mean[b], sd[b], pit[b]
        ae = np.abs(mu - o)
        ne = ae / (sg + 1e-6)
        lo, hi = mu - 1.96 * sg, mu + 1.96 * sg
        table[s, 5:9] = b.sum(), np.sum(sg), np.sum(ne), np.sum((hi - lo) + (2.0 / 0.05) * (np.where(o < lo, lo - o, 0.0) + np.where(o > hi, o - hi, 0.0)))
        for j, zl in enumerate(Z_LEVELS):
            table[s, 9 + j] = np.sum((o >= mu - zl * sg) & (o <= mu + zl * sg))
            edges["bound"].append((np.abs(ae - zl * sg) / np.maximum(sg, 1e-300))[sg > 0])   # (sd == 0: lo == hi == mean exactly)
        with np.errstate(divide="ignore", invalid="ignore"):
            w = (o - mu) / sg
            crps = sg * (w * (1.0 - _erfc(w * 0.70710678118654752440)) + 2.0 * 0.39894228040143267794 * np.exp(-0.5 * w * w) - 0.56418958354775628695)
        table[s, 13] = np.sum(np.where(sg > 0, crps, ae))
        ll = state["lsum"][b] > 0
        table[s, 14] = np.sum(state["lmax"][b][ll] + np.log(state["lsum"][b][ll] / n[b][ll]))
        table[s, 15] = ll.sum()
        for j in range(nb):
            table[s, FIXED + j] = np.sum(ne <= thr[j])
            edges["norm"].append(np.abs(ne - thr[j]))
        bins = np.minimum(np.floor(pv * nb).astype(np.int64), nb - 1)
        table[s, FIXED + nb:] = np.bincount(bins, minlength=nb)
        x = pv * nb
        inner = np.abs(x - np.round(x))[(np.round(x) >= 1) & (np.round(x) <= nb - 1)]          # the edges 1 .. n_bins - 1
        edges["pit"].append(inner)
    return mean, sd, pit, table, edges


def clear_of_edges(edges, tol=1e-9):
    """No |e| / (sd + 1e-6) within tol of a threshold or an interval bound and no PIT value within tol of a bin edge: then the
    counts of the table are exact whatever the last bits of the kernel's arithmetic are.  A distance of exactly 0 is not
    flagged for the threshold 0 (e == 0) and for the PIT: without noise a draw adds 0, 1/2 or 1, so pit / n is a ratio of small
    integers that both sides compute exactly (1/2 * 10 = 5.0 on either), and the bin is the same.)"""
    for key, parts in edges.items():
        for p in parts:
            p = np.asarray(p)
            p = p[p != 0.0] if key in ("norm", "pit") else p
            if p.size and float(p.min()) < tol:
                return False
    return True


def metrics(table, n_bins):
    """Pooled and per-state scores of a table; NaN where there is nothing to average."""
    t = np.asarray(table, dtype=np.float64)

    def one(r):
        ce, cu = r[0], r[5]
        div = lambda a, c: a / c if c > 0 else float("nan")                                     # noqa: E731
        out = {"rmse": math.sqrt(div(r[1], ce)) if ce > 0 else float("nan"), "mae": div(r[2], ce),
               "target_std": math.sqrt(max((r[4] - r[3] ** 2 / ce) / (ce - 1), 0.0)) if ce > 1 else float("nan"),
               "msis": div(r[8], cu), "sharpness": div(r[6], cu), "coverage_50": div(r[9], cu), "coverage_80": div(r[10], cu),
               "coverage_90": div(r[11], cu), "coverage_95": div(r[12], cu), "mean_normalized_error": div(r[7], cu), "crps": div(r[13], cu),
               "lppd": r[14] if r[15] > 0 else float("nan")}
        out["ece"] = float(np.mean(np.abs(np.arange(n_bins) / n_bins - r[FIXED:FIXED + n_bins] / cu))) if cu > 0 else float("nan")
        return out
    pooled = one(t.sum(0))
    per = [one(t[s]) for s in range(6)]
    out = dict(pooled)
    for key in pooled:
        out[key + "_per_state"] = np.array([p[key] for p in per])
    return out


def from_moments(pred, unc=None):
    """The state whose mean and sd are the given arrays (two pseudo-draws; one without unc)."""
    p = np.asarray(pred, dtype=np.float64).reshape(-1)
    st = fresh_state(p.size)
    st["mean"][:] = p
    st["n"][:] = 1 if unc is None else 2
    if unc is not None:
        st["m2"][:] = np.asarray(unc, dtype=np.float64).reshape(-1) ** 2
    return st


def calibration(pred, unc, targets, n_bins=10):
    _, _, _, table, _ = score(from_moments(pred, unc), np.asarray(targets).reshape(-1), None, None, thresholds(n_bins))
    m = metrics(table, n_bins)
    return {k: m[k] for k in ("ece", "msis", "sharpness", "coverage_95", "mean_normalized_error")}, m


# ------------------------------------------------------------------------------------------------ the tests' inputs
SCALE = np.array([120.0, 15.0, 60.0, 8.0, 0.5, 0.4])
# (n_traj, T): N = 18, less than a wave, the score pass on its scalar path; N = 390, a ragged second workgroup of the fold,
# N % 4 != 0 (the score pass by rows); N = 3348, 14 workgroups of the fold with a ragged last one, the score pass on its
# 16-byte path with 279 groups of twelve = one full workgroup and a ragged second one
SHAPES = ((1, 3), (5, 13), (9, 62))
UNSEEN_STATE = 4


def make_case(n_traj, T, S, dtype=np.float64, seed=0):
    """Seeded inputs of the kernel tests, spread 5 % of magnitude (>= 1e-3, so Welford's m2 is well conditioned): y [S, N] in
    `dtype` precision (returned as fp64 values), obs [N] with ~10 % NaN, a mask with ~10 % zeros and state UNSEEN_STATE masked
    everywhere, sigma [S, 6] > 0, status [S, n_traj].  With S >= 2 the LAST draw's trajectory 0 is non-finite from T // 2 on;
    with S >= 3 and n_traj >= 2, draw 1 of the last trajectory has status 2 and zero rows from T // 3 on."""
    rng = np.random.default_rng(1000 * seed + 10 * n_traj + T + S)
    N = n_traj * T * 6
    base = np.tile(SCALE, n_traj * T)
    y = base * (1.0 + 0.05 * rng.standard_normal((S, N)))
    obs = base * (1.0 + 0.05 * rng.standard_normal(N))
    obs[rng.random(N) < 0.1] = np.nan
    mask = (rng.random(N) >= 0.1).astype(np.uint8)
    mask[np.arange(N) % 6 == UNSEEN_STATE] = 0
    sigma = 0.05 * SCALE * (0.5 + rng.random((S, 6)))
    status = np.zeros((S, n_traj), dtype=np.int32)
    y4 = y.reshape(S, n_traj, T, 6)
    if S >= 2:
        y4[S - 1, 0, T // 2:] = np.nan
        y4[S - 1, 0, T - 1, 2] = np.inf
    if S >= 3 and n_traj >= 2:
        status[1, n_traj - 1] = 2
        y4[1, n_traj - 1, T // 3:] = 0.0
    y = y.astype(dtype).astype(np.float64)
    obs = obs.astype(dtype).astype(np.float64)
    return {"y": y, "obs": obs, "mask": mask, "sigma": sigma, "status": status, "N": N}


def two_pass(y, status, n_traj):
    """(n, mean, m2) of every entry in np.longdouble, two passes, with the fold's skip rules."""
    S, N = y.shape
    take = np.isfinite(y) & np.repeat(np.asarray(status) == 0, N // n_traj, axis=1)
    yl = np.where(take, y, 0.0).astype(np.longdouble)
    n = take.sum(0)
    mean = yl.sum(0) / np.maximum(n, 1)
    m2 = (np.where(take, yl - mean, 0.0) ** 2).sum(0)
    return n, mean, m2

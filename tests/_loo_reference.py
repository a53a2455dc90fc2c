"""NumPy restatement of csrc/hode_loo.hip (include/hode.h, "Model comparison"), written from the specification: the pointwise
log likelihood with the fold's skip rules, the streaming state of hode_pred_loo_fold_* draw by draw, and PSIS-LOO / WAIC in two
forms -- `psis_full` sorts ALL importance ratios of an entry, smooths the tail in place, renormalises and takes
logsumexp(x + l) (what arviz.psislw + arviz.loo do); `finish` is the heap form the kernel uses (the K largest ratios plus a
running log-sum-exp of the rest, numerator and denominator in log space).  Every function takes the float type `ft`
(np.float64, or np.longdouble for the precision bound).  Plays the role of _quantile_reference.py.

TOLERANCES (tests/test_loo_host.py measures them on exactly the GPU tests' inputs and holds the constants to the measurement):
the fp64 restatement against itself in np.longdouble (64-bit mantissa) differs by at most 1.35e-13 absolute in elpd_loo and
1.55e-13 in pareto_k (k from -0.6 to 14.9) over every case below; ten times that is what the GPU tests allow."""
import math
from functools import lru_cache

import numpy as np

SCALE = np.array([120.0, 15.0, 60.0, 8.0, 0.5, 0.4])
SHAPES = ((1, 3), (5, 13), (9, 62))                   # N = 18, 390, 3348 as tests/_quantile_reference.py
UNSEEN_STATE = 4
CONST_ENTRY = 2                                       # the one entry whose draws are all equal (its l is constant)
LOO_COLS = 13
EPS = 2.0 ** -52
HALF_LOG_2PI = "0.918938533204672741780329736405617639861397"
OUTPUTS = ("elpd_loo", "pareto_k", "elpd_waic", "p_waic", "lppd")
# ten times the measured fp64-against-longdouble difference of the restatement (test_loo_host.py::test_precision_bound)
TOL_ELPD = 1.4e-12
TOL_K = 1.6e-12


def tail_len(n, r_eff=1.0):
    """M = ceil(min(n / 5, 3 sqrt(n / r_eff))) in fp64, as the kernel."""
    return int(math.ceil(min(float(n) / 5.0, 3.0 * math.sqrt(float(n) / float(r_eff)))))


def loo_tail_size(n, r_eff=1.0):
    return tail_len(n, r_eff) + 1


def observed(obs, mask):
    on = np.isfinite(obs)
    if mask is not None:
        on &= np.asarray(mask) != 0
    return on


def log_lik(y, obs, mask, sigma, status=None, ft=np.float64):
    """l [S, N] in `ft`, NaN where the draw produces none: the entry unobserved, the trajectory's status non-zero, y not
    finite, sigma[s][k] not above 0.  z = (obs - y) / sigma;  l = -z^2 / 2 - log sigma - log(2 pi) / 2."""
    y = np.asarray(y, dtype=np.float64)
    S, N = y.shape
    take = np.isfinite(y) & observed(np.asarray(obs, dtype=np.float64), mask)[None]
    if status is not None:
        st = np.asarray(status)
        take &= np.repeat(st == 0, N // st.shape[1], axis=1)
    sig = np.asarray(sigma, dtype=np.float64)[:, np.arange(N) % 6]
    take &= sig > 0
    yv, ov, sg = np.where(take, y, 0.0).astype(ft), np.where(np.isfinite(obs), obs, 0.0).astype(ft)[None], np.where(take, sig, 1.0).astype(ft)
    z = (ov - yv) / sg
    l = ft(-0.5) * z * z - np.log(sg) - ft(HALF_LOG_2PI)
    return np.where(take, l, ft(np.nan))


# ---------------------------------------------------------------------------------------------------------- the fold
def _lse_add(mx, sm, v, on):
    """v into the streaming log-sum-exp {mx, sm} where `on`: v > mx ? (sm = sm exp(mx - v) + 1, mx = v) : sm += exp(v - mx)."""
    with np.errstate(invalid="ignore", over="ignore"):
        gt = v > mx
        sm_new = np.where(gt, sm * np.exp(mx - v) + 1.0, sm + np.exp(v - mx))
    return np.where(on, np.where(gt, v, mx), mx), np.where(on, sm_new, sm)


def fresh_state(N, K, ft=np.float64):
    z = lambda: np.zeros(N, dtype=ft)                                                              # noqa: E731
    return {"cnt": np.zeros(N, dtype=np.int32), "lmean": z(), "lm2": z(), "pmax": np.full(N, -np.inf, dtype=ft), "psum": z(),
            "top": np.full((K, N), np.nan, dtype=ft), "rmax": np.full(N, -np.inf, dtype=ft), "rsum": z()}


def fold(state, l):
    """The draws l [S, N] (NaN = no l) into the state, one at a time in draw order, as hode_pred_loo_fold_*.  `top` holds the
    min(cnt, K) largest r = -l in slots 0 .. min(cnt, K) - 1 in NO particular order (compare it sorted), NaN past them."""
    top = state["top"]
    K, N = top.shape
    cnt, lmean, lm2, pmax, psum, rmax, rsum = (state[k] for k in ("cnt", "lmean", "lm2", "pmax", "psum", "rmax", "rsum"))
    cols = np.arange(N)
    for v in l:
        on = ~np.isnan(v)
        lv = np.where(on, v, 0.0).astype(top.dtype)
        d = lv - lmean
        mean_new = lmean + d / (cnt + 1).astype(top.dtype)
        lm2 = np.where(on, lm2 + d * (lv - mean_new), lm2)
        lmean = np.where(on, mean_new, lmean)
        pmax, psum = _lse_add(pmax, psum, lv, on)
        r = -lv
        filling = on & (cnt < K)
        top[cnt[filling], cols[filling]] = r[filling]
        full = cols[on & ~filling]
        if full.size:
            sub = top[:, full]
            at = sub.argmin(0)
            least = sub[at, np.arange(full.size)]
            swap = least < r[full]
            top[at[swap], full[swap]] = r[full][swap]
            out = np.zeros(N, dtype=top.dtype)
            out[full] = np.where(swap, least, r[full])
            rmax, rsum = _lse_add(rmax, rsum, out, on & ~filling)
        cnt = cnt + on.astype(np.int32)
    state.update(cnt=cnt, lmean=lmean, lm2=lm2, pmax=pmax, psum=psum, rmax=rmax, rsum=rsum)
    return state


def sorted_top(state):
    """[K, N]: every entry's held ratios ascending, NaN past them."""
    return np.sort(state["top"], axis=0)


# ------------------------------------------------------------------------------------------------------------ the fit
def gpdfit(a, ft=np.float64):
    """Zhang & Stephens' estimate of the generalised Pareto shape and scale of a [G, t] (every row ascending, t >= 5), with the
    prior of Vehtari et al. 2024: (k [G], sigma [G])."""
    a = np.asarray(a, dtype=ft)
    G, t = a.shape
    m = 30 + int(math.floor(math.sqrt(t)))
    q = np.arange(1, m + 1).astype(ft)
    with np.errstate(all="ignore"):
        b = (ft(1.0) - np.sqrt(ft(m) / (q - ft(0.5))))[None, :] / (ft(3.0) * a[:, int(t / 4.0 + 0.5) - 1])[:, None] + (ft(1.0) / a[:, -1])[:, None]
        kq = np.log1p(-b[:, :, None] * a[:, None, :]).sum(-1) / ft(t)
        L = ft(t) * (np.log(-(b / kq)) - kq - ft(1.0))
        w = ft(1.0) / np.exp(L[:, None, :] - L[:, :, None]).sum(-1)
        w = np.where(w >= 10.0 * EPS, w, ft(0.0))
        w = w / w.sum(-1, keepdims=True)
        bp = (w * b).sum(-1)
        kp = np.log1p(-bp[:, None] * a).sum(-1) / ft(t)
        sigma = -kp / bp
        k = (ft(t) * kp + ft(5.0)) / (ft(t) + ft(10.0))
    return k, sigma


def _smoothed(k, sigma, t, e_cut, ft):
    """x~ [G, t]: the fitted quantiles at p_j = (j - 1/2) / t as log weights, capped at 0."""
    p = ((np.arange(1, t + 1).astype(ft) - ft(0.5)) / ft(t))[None, :]
    lp = np.log1p(-p)
    with np.errstate(all="ignore"):
        at = np.where(np.abs(k)[:, None] < EPS, -sigma[:, None] * lp, sigma[:, None] * np.expm1(-k[:, None] * lp) / k[:, None])
        return np.minimum(np.log(at + e_cut[:, None]), ft(0.0))


def _lse(v):
    """log-sum-exp along the last axis; -inf entries are empty slots."""
    mx = v.max(-1)
    with np.errstate(invalid="ignore"):
        return mx + np.log(np.exp(v - mx[..., None]).sum(-1))


def _psis_group(held, lrest_c, n, M, ft, chunk=256):
    """The heap form for G entries that share n, h and M.  held [G, h]: the h largest r ascending; lrest_c [G]: rmax + log rsum
    (the log-sum-exp of the ratios not held; -inf when there are none).  Returns (elpd, k, t, tie) with tie [G] bool: one of the M
    largest values is not above the cut (it ties the cut, or the cut was raised to log(DBL_MIN)), so t < M."""
    G, h = held.shape
    elpd, kh, ts = np.empty(G, dtype=ft), np.empty(G, dtype=ft), np.empty(G, dtype=np.int64)
    c = held[:, -1]
    x = held - c[:, None]
    x_cut = np.maximum(x[:, h - 1 - M], np.log(ft(np.finfo(np.float64).tiny)))
    e_cut = np.exp(x_cut)
    t_all = (x > x_cut[:, None]).sum(1)
    tie = t_all < M
    for t in np.unique(t_all):
        for lo in range(0, G, chunk):
            g = np.arange(lo, min(lo + chunk, G))
            g = g[t_all[g] == t]
            if not g.size:
                continue
            t = int(t)
            xt, rt = x[g, h - t:], held[g, h - t:]
            k = np.full(g.size, np.inf, dtype=ft)
            if t > 4:
                k, sigma = gpdfit(np.exp(xt) - e_cut[g, None], ft)
                ok = np.isfinite(k) & (sigma > 0)
                xt = np.where(ok[:, None], _smoothed(k, sigma, t, e_cut[g], ft), xt)
            num = _lse(np.concatenate([(np.log(ft(n - t)) - c[g])[:, None], xt - rt], axis=1))
            den = _lse(np.concatenate([(lrest_c[g] - c[g])[:, None], x[g, :h - t], xt], axis=1))
            elpd[g], kh[g], ts[g] = num - den, k, t
    return elpd, kh, ts, tie


def finish(state, r_eff=1.0, ft=np.float64):
    """hode_pred_loo_finish_* on a state of `fold`: a dict of the five outputs [N] in `ft` (NaN where n < 2 or the buffer is too
    small), `t` (tail lengths, -1 where not scored) and `tie`."""
    cnt = state["cnt"].astype(np.int64)
    top = sorted_top(state).astype(ft)
    K, N = top.shape
    out = {k: np.full(N, np.nan, dtype=ft) for k in OUTPUTS}
    out["t"], out["tie"] = np.full(N, -1, dtype=np.int64), np.zeros(N, dtype=bool)
    for n in np.unique(cnt):
        n = int(n)
        h, M = min(n, K), tail_len(n, r_eff)
        if n < 2 or M + 1 > h:
            continue
        e = np.where(cnt == n)[0]
        with np.errstate(divide="ignore"):
            lrest = state["rmax"][e].astype(ft) + np.log(state["rsum"][e].astype(ft)) if n > h else np.full(e.size, -np.inf, dtype=ft)
        out["elpd_loo"][e], out["pareto_k"][e], out["t"][e], out["tie"][e] = _psis_group(top[:h, e].T, lrest, n, M, ft)
        out["lppd"][e] = state["pmax"][e] + np.log(state["psum"][e] / ft(n))
        out["p_waic"][e] = state["lm2"][e] / ft(n - 1)
        out["elpd_waic"][e] = out["lppd"][e] - out["p_waic"][e]
    return out


def psis_full(l, r_eff=1.0, ft=np.float64):
    """The full-array form for ONE entry, l [n] (n >= 2): (elpd_loo, k, t).  Sort all r = -l, x = r - max, smooth the values
    above the cut in place, renormalise the log weights, elpd = logsumexp(x + l)."""
    l = np.asarray(l, dtype=ft)
    n = l.size
    M = tail_len(n, r_eff)
    r = np.sort(-l)
    x = r - r[-1]
    x_cut = max(x[n - 1 - M], np.log(ft(np.finfo(np.float64).tiny)))
    e_cut = np.exp(x_cut)
    t = int((x > x_cut).sum())
    k = ft(np.inf)
    if t > 4:
        kk, sg = gpdfit((np.exp(x[n - t:]) - e_cut)[None, :], ft)
        k = kk[0]
        if np.isfinite(k) and sg[0] > 0:
            x = x.copy()
            x[n - t:] = _smoothed(kk, sg, t, np.array([e_cut], dtype=ft), ft)[0]
    lw = x - _lse(x)
    return _lse(lw - r), k, t


def loo_of(l, K, r_eff=1.0, ft=np.float64):
    """The whole heap route on l [S, N]: (state, outputs)."""
    st = fold(fresh_state(l.shape[1], K, ft), l)
    return st, finish(st, r_eff, ft)


def table(out):
    """double[6][13] of include/hode.h from the outputs of `finish`."""
    tb = np.zeros((6, LOO_COLS))
    N = out["lppd"].size
    use = ~np.isnan(out["lppd"])
    for s in range(6):
        u = use & (np.arange(N) % 6 == s)
        el, ew, pw, lp, k = (np.asarray(out[key][u], dtype=np.float64) for key in ("elpd_loo", "elpd_waic", "p_waic", "lppd", "pareto_k"))
        tb[s] = (u.sum(), el.sum(), (el * el).sum(), (lp - el).sum(), ew.sum(), (ew * ew).sum(), pw.sum(), lp.sum(),
                 (k <= 0.5).sum(), ((k > 0.5) & (k <= 0.7)).sum(), ((k > 0.7) & (k <= 1.0)).sum(), (k > 1.0).sum(), (pw > 0.4).sum())
    return tb


def clear_of_thresholds(out, tol=1e-6):
    """Every k is at least tol from 0.5, 0.7 and 1, and every p_waic from 0.4: the counts of the table cannot depend on rounding."""
    k, pw = out["pareto_k"], out["p_waic"]
    k, pw = k[np.isfinite(k)], pw[np.isfinite(pw)]
    return bool(all(np.all(np.abs(k - c) >= tol) for c in (0.5, 0.7, 1.0)) and np.all(np.abs(pw - 0.4) >= tol))


# ------------------------------------------------------------------------------------------------ the tests' inputs
def make_case(n_traj, T, S, dtype=np.float64, seed=0, zero_sigma_state=None):
    """Seeded inputs in `dtype` precision (returned as fp64 values): y [S, N], obs [N] (~10 % NaN), mask (uint8, ~10 % zeros, state
    UNSEEN_STATE masked everywhere), sigma [S, 6] (states 0 and 1 vary from draw to draw like a marginal noise posterior; with
    zero_sigma_state that state's sigma is 0 in every draw), status [S, n_traj].  The draws of entry i scatter around a centre
    with spread_i sigma_k, spread_i log-uniform in [0.2, 4], and the observation sits offset_i sigma_k from the centre,
    offset_i uniform in [-2, 2]: narrow, well-placed entries get small Pareto k, wide or offset ones k far above 1.
    Skips as _quantile_reference.make_case: entry 1 is non-finite in every draw (no draw at all); with S >= 2 the last draw of
    entry 0 is +inf; with S >= 3 and n_traj >= 2, draw 1 of the last trajectory has status 2 and zero rows.  Entry CONST_ENTRY
    has the same value in every draw (state 2: constant sigma, so a constant l)."""
    rng = np.random.default_rng(9000 * seed + 10 * n_traj + T + S + 1)
    N = n_traj * T * 6
    k = np.arange(N) % 6
    sig0 = 0.05 * SCALE
    sigma = np.tile(sig0, (S, 1))
    sigma[:, :2] *= np.exp(0.1 * rng.standard_normal((S, 2)))
    if zero_sigma_state is not None:
        sigma[:, zero_sigma_state] = 0.0
    centre = SCALE[k] * (1.0 + 0.05 * rng.standard_normal(N))
    spread = np.exp(rng.uniform(np.log(0.2), np.log(4.0), N))
    y = centre + spread * sig0[k] * rng.standard_normal((S, N))
    obs = centre + rng.uniform(-2.0, 2.0, N) * sig0[k]
    y[:, CONST_ENTRY] = centre[CONST_ENTRY]
    status = np.zeros((S, n_traj), dtype=np.int32)
    y[:, 1] = np.nan
    if S >= 2:
        y[S - 1, 0] = np.inf
    if S >= 3 and n_traj >= 2:
        status[1, n_traj - 1] = 2
        y.reshape(S, n_traj, T, 6)[1, n_traj - 1] = 0.0
    y = y.astype(dtype).astype(np.float64)
    obs = obs.astype(dtype).astype(np.float64)
    miss = rng.random(N) < 0.1
    mask = (rng.random(N) >= 0.1).astype(np.uint8)
    miss[:3] = False
    mask[:3] = 1                                       # entries 0, 1, 2 are special and stay observed
    obs[miss] = np.nan
    mask[k == UNSEEN_STATE] = 0
    return {"y": y, "obs": obs, "mask": mask, "sigma": sigma, "status": status, "N": N}


@lru_cache(maxsize=None)
def case(n_traj, T, S, dt="f64", zero_sigma_state=None):
    return make_case(n_traj, T, S, np.float32 if dt == "f32" else np.float64, zero_sigma_state=zero_sigma_state)


@lru_cache(maxsize=None)
def reference(n_traj, T, S, dt, K, long=False, zero_sigma_state=None):
    """(l, state, outputs) of a case, computed once and shared (never modified by the tests)."""
    c = case(n_traj, T, S, dt, zero_sigma_state)
    ft = np.longdouble if long else np.float64
    l = log_lik(c["y"], c["obs"], c["mask"], c["sigma"], c["status"], ft)
    st, out = loo_of(l, K, 1.0, ft)
    return l, st, out


# the (shape, S) pairs the GPU tests run: every S at the two small shapes, the large shape where a second workgroup matters
GPU_CASES = tuple((sh, S) for sh in SHAPES for S in (1, 2, 7, 19, 40, 300) if not (sh == SHAPES[2] and S in (1, 2, 19)))


def l_tolerance(c, l):
    """[N]: how far a correct fp64 evaluation of l may be from this one.  (obs - y), the division, z * z, the halving (exact)
    and the two subtractions are IEEE operations, identical wherever they run; log(sigma) is the one library call, good to
    2 ulp of |log sigma| on either side.  That error passes through the two subtractions, each of which re-rounds its result
    (one ulp of the larger of |l| and |log sigma| + z^2 / 2): 2 ulp(log sigma) + 2 ulp(max) <= 4 * 2^-52 * max(1, |log sigma|,
    |l|) per draw, and the bound of an entry is the largest over its draws."""
    sig = np.asarray(c["sigma"])[:, np.arange(c["N"]) % 6]
    with np.errstate(divide="ignore", invalid="ignore"):
        ls = np.where(sig > 0, np.abs(np.log(sig)), 0.0)
    mag = np.maximum(np.maximum(np.nan_to_num(np.abs(np.asarray(l, dtype=np.float64))), ls), 1.0)
    return 4.0 * EPS * mag.max(0)

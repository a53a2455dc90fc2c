"""NumPy restatement of the tail and quantile kernels of csrc/hode_predictive.hip (include/hode.h, "Posterior bands"), written
from the specification: np.sort for the K smallest / largest values of every entry with the fold's skip rules, then the
quantile formula  h = q (n - 1), j = floor(h), g = h - j, out = a + (b - a) g  in fp64, rounded once to the working precision.
NumPy does not contract a multiply into an add, so the kernels (contraction off) are held to these bits.  The host tests hold
this restatement to np.quantile; the GPU tests hold the kernels to it.  Plays the role of _predictive_reference.py."""
import numpy as np

SCALE = np.array([120.0, 15.0, 60.0, 8.0, 0.5, 0.4])
# (n_traj, T) as tests/_predictive_reference.py: N = 18, under one wave; N = 390, a ragged second workgroup; N = 3348, fourteen
# workgroups with a ragged last wave
SHAPES = ((1, 3), (5, 13), (9, 62))
UNSEEN_STATE = 4
ORDERS = ("random", "ascending", "descending", "ties")
BAND_COLS = 4


def taken(y, status=None):
    """[S, N] bool: which values the kernel takes (finite, and the trajectory's status zero)."""
    y = np.asarray(y, dtype=np.float64)
    take = np.isfinite(y)
    if status is not None:
        st = np.asarray(status)
        take &= np.repeat(st == 0, y.shape[1] // st.shape[1], axis=1)
    return take


def tails(y, K, status=None):
    """cnt [N] int32 and (lower, upper), each [K, N] fp64: the min(cnt, K) smallest and largest taken values of every entry,
    ascending, NaN past them."""
    y = np.asarray(y, dtype=np.float64)
    S, N = y.shape
    take = taken(y, status)
    cnt = take.sum(0).astype(np.int32)
    m = np.minimum(cnt, K).astype(np.int64)
    r = np.arange(K)[:, None]
    pad = np.full((K, N), np.inf)
    up = np.concatenate([np.sort(np.where(take, y, np.inf), axis=0), pad])                        # the taken values first
    lower = np.where(r < m, up[:K], np.nan)
    # rank r of the m largest is rank cnt - m + r of all taken values
    upper = np.where(r < m, np.take_along_axis(up, np.minimum(cnt - m + r, S + K - 1), axis=0), np.nan)
    return cnt, lower, upper


def quantiles(cnt, lower, upper, levels, dtype=np.float64):
    """out [Q, N] in `dtype`: numpy's "linear" quantile from the nearer tail, NaN where cnt == 0 or a needed order statistic is
    not among the K kept values (include/hode.h)."""
    K = lower.shape[0]
    n = cnt.astype(np.int64)
    m = np.minimum(n, K)
    out = np.empty((len(levels), n.size), dtype=dtype)
    for l, q in enumerate(levels):
        h = np.float64(q) * (n - 1).astype(np.float64)
        fj = np.floor(h)
        g = h - fj
        j = np.maximum(fj.astype(np.int64), 0)
        jb = np.minimum(j + 1, np.maximum(n - 1, 0))
        if q <= 0.5:
            ok = (n > 0) & (jb < m)
            src, ia, ib = lower, j, jb
        else:
            ok = (n > 0) & (j >= n - m)
            src, ia, ib = upper, j - (n - m), jb - (n - m)
        ia, ib = np.clip(ia, 0, K - 1), np.clip(ib, 0, K - 1)
        a = np.take_along_axis(src, ia[None], axis=0)[0]
        b = np.take_along_axis(src, ib[None], axis=0)[0]
        with np.errstate(invalid="ignore"):
            v = a + (b - a) * g
        out[l] = np.where(ok, v, np.nan).astype(dtype)
    return out


def quantiles_of(y, levels, K=None, status=None, dtype=np.float64):
    """The whole route on y [S, N]: (cnt, lower, upper, out)."""
    y = np.asarray(y, dtype=np.float64)
    K = y.shape[0] if K is None else K
    cnt, lower, upper = tails(y, K, status)
    return cnt, lower, upper, quantiles(cnt, lower, upper, levels, dtype)


def tail_size(levels, n_draws):
    return min(n_draws, max(int(np.floor(min(q, 1.0 - q) * float(n_draws - 1))) + 2 for q in levels))


def observed(obs, mask):
    on = np.isfinite(obs)
    if mask is not None:
        on &= np.asarray(mask) != 0
    return on


def band_table(cnt, q_lo, q_hi, obs, mask, level_lo, level_hi):
    """[6, 4]: count, sum (hi - lo), count of lo <= obs <= hi, sum of the interval score, per state over the observed entries
    with cnt >= 2 and both bounds finite.  q_lo, q_hi: the quantiles as written (working precision)."""
    lo, hi, o = np.asarray(q_lo, dtype=np.float64), np.asarray(q_hi, dtype=np.float64), np.asarray(obs, dtype=np.float64)
    use = observed(o, mask) & (cnt >= 2) & np.isfinite(lo) & np.isfinite(hi)
    k = np.arange(lo.size) % 6
    c = 2.0 / (1.0 - (level_hi - level_lo))
    table = np.zeros((6, BAND_COLS))
    for s in range(6):
        u = use & (k == s)
        l, h, ob = lo[u], hi[u], o[u]
        table[s] = (u.sum(), np.sum(h - l), np.sum((l <= ob) & (ob <= h)),
                    np.sum((h - l) + c * (np.where(ob < l, l - ob, 0.0) + np.where(ob > h, ob - h, 0.0))))
    return table


def band_metrics(table):
    t = np.asarray(table, dtype=np.float64)

    def one(r):
        return {name: (r[i] / r[0] if r[0] > 0 else float("nan")) for i, name in ((1, "band_width"), (2, "band_coverage"), (3, "band_interval_score"))}
    out = one(t.sum(0))
    per = [one(t[s]) for s in range(6)]
    for key in list(out):
        out[key + "_per_state"] = np.array([p[key] for p in per])
    return out


# ------------------------------------------------------------------------------------------------ the tests' inputs
def make_case(n_traj, T, S, dtype=np.float64, order="random", seed=0):
    """Seeded inputs: y [S, N] of `dtype` precision (returned as fp64 values, no -0.0), status [S, n_traj].  order: "random";
    "ascending" / "descending" in the draw index (every draw enters the upper / the lower buffer); "ties": values rounded to one
    decimal.  Skips: entry 1 is non-finite in every draw (n = 0 there); with S >= 2 the last draw of entry 0 is +inf; with
    S >= 3 and n_traj >= 2, draw 1 of the last trajectory has status 2 and zero rows."""
    rng = np.random.default_rng(7000 * seed + 10 * n_traj + T + S)
    N = n_traj * T * 6
    y = np.tile(SCALE, n_traj * T) * (1.0 + 0.05 * rng.standard_normal((S, N)))
    if order == "ascending":
        y = np.sort(y, axis=0)
    elif order == "descending":
        y = np.sort(y, axis=0)[::-1].copy()
    elif order == "ties":
        y = np.round(y, 1) + 0.0
    status = np.zeros((S, n_traj), dtype=np.int32)
    y[:, 1] = np.nan
    if S >= 2:
        y[S - 1, 0] = np.inf
    if S >= 3 and n_traj >= 2:
        status[1, n_traj - 1] = 2
        y.reshape(S, n_traj, T, 6)[1, n_traj - 1] = 0.0
    y = y.astype(dtype).astype(np.float64)
    assert not np.any(np.signbit(y) & (y == 0))
    return {"y": y, "status": status, "N": N}


def make_observations(q_lo, q_hi, dtype=np.float64, seed=0):
    """obs [N] (~10 % NaN) and mask (uint8, ~10 % zeros, state UNSEEN_STATE masked everywhere) placed relative to the band
    [q_lo, q_hi]: a third below, a third inside (where the band is wide enough), a third above, every one at least 1e-3 of the
    bound's magnitude away from both bounds, so rounding cannot move it across.  `clear_of_bounds` is the tests' check."""
    lo, hi = np.asarray(q_lo, dtype=np.float64), np.asarray(q_hi, dtype=np.float64)
    N = lo.size
    rng = np.random.default_rng(seed + N)
    fin = np.isfinite(lo) & np.isfinite(hi)
    l, h = np.where(fin, lo, 1.0), np.where(fin, hi, 2.0)
    w = h - l
    where = rng.integers(0, 3, N)
    inside = (where == 1) & (w > 1e-2 * np.abs(l))
    below = where == 0
    obs = np.where(inside, l + 0.5 * w, np.where(below, l - 0.3 * w - 0.01 * np.abs(l), h + 0.3 * w + 0.01 * np.abs(h)))
    obs = obs.astype(dtype).astype(np.float64)
    obs[rng.random(N) < 0.1] = np.nan
    mask = (rng.random(N) >= 0.1).astype(np.uint8)
    mask[np.arange(N) % 6 == UNSEEN_STATE] = 0
    return obs, mask


def clear_of_bounds(obs, q_lo, q_hi, rel=1e-6):
    """Every finite obs is at least rel (relative) away from both bounds, over ALL entries with finite bounds."""
    lo, hi, o = np.asarray(q_lo, dtype=np.float64), np.asarray(q_hi, dtype=np.float64), np.asarray(obs, dtype=np.float64)
    e = np.isfinite(lo) & np.isfinite(hi) & np.isfinite(o)
    return bool(np.all(np.abs(o[e] - lo[e]) >= rel * np.abs(lo[e])) and np.all(np.abs(o[e] - hi[e]) >= rel * np.abs(hi[e])))

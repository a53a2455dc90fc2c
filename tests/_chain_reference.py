"""One plain numpy fp64 function per call of the sampler kernels (csrc/hode_hmc.hip, csrc/hode_nuts.hip), state in -> state
out, worded as include/hode.h words the call.  tests/test_chain_kernels_host.py ties these to the transition-level
restatement of tests/_nuts_reference.py and to textbook HMC; tests/test_chain_kernels_gpu.py holds every kernel to them, one
call at a time.

The functions see the LOGICAL state only: [C][D] arrays, the dst / ist / da / search tables, ckpt as a dict keyed by
(chain, level).  They know nothing of ld, padding, vector width or lanes.  Inputs are never modified; outputs are new arrays.

Every decision a call makes is also returned, as a Decision(kind, chain, margin, bound64, bound32): margin = the distance of
the compared quantity from its threshold, bound64 / bound32 = the rounding bound of that quantity when the kernel runs in
fp64 / fp32, (k + 1) u sum |terms| with k counted from the kernel's expression (the counts stand next to each bound).  A
decision that no rounding can move (a NaN, an infinity, a failed solve, a threshold met exactly by construction) has
margin = inf."""
import math
from collections import namedtuple

import numpy as np

from _nuts_reference import ACCEPT, DIR, JITTER, LEAF, MERGE, MOMENTUM, hmc_rng, momentum, normals4, u01  # noqa: F401

U64, U32 = 2.0 ** -53, 2.0 ** -24
ASSEMBLE, KICK, DRIFT, KE, PARAMS = 1, 2, 4, 8, 16
SAMPLE, ADAPT, SEARCH, DA_RESTART, DA_FINISH = range(5)
W_ACCUM, W_FINISH = 1, 2
# rows of the tree, slots of dst and ist (include/hode.h, "No-U-Turn sampling")
FZ, FP, FG, LZ, LP, LG, RZ, RP, RG, PZ, PG, SZ, SG, RHO, RHO_SUB = range(15)
H0, LOG_W, LOG_W_SUB, SUM_ACC, U_PROP, U_SUB = range(6)
J, LEAF_I, N_LEAF, ACTIVE, DIVERGENT, FAILED, DIRECTION, DEPTH = range(8)
LOG08 = math.log(0.8)

Decision = namedtuple("Decision", "kind chain margin bound64 bound32")


def unit(dtype):
    return U32 if np.dtype(dtype) == np.float32 else U64


def ode_indices(mask):
    """ODE index of sampled coordinate d: the d-th set bit of the mask, ascending."""
    return [k for k in range(17) if (mask >> k) & 1]


def uniform(seed, chain, it, tag, group):
    return u01(hmc_rng(seed, chain, it, tag, group)[0])


def _fsum(x):
    return math.fsum(float(v) for v in np.ravel(x))


def _lik_grad(c_slot, D, cmap, sd, gnn, gode):
    """The likelihood gradient in chain coordinates from slot c_slot of gnn [.][P] / gode [.][17] (None: no term)."""
    mask, sample_nn, P = cmap
    idx = ode_indices(mask)
    out = np.zeros(D)
    for d in range(D):
        if d < len(idx):
            if gode is not None:
                out[d] = gode[c_slot, idx[d]] * sd[d]
        elif gnn is not None:
            out[d] = gnn[c_slot, d - len(idx)]
    return out


def _write_params(c_slot, zrow, cmap, mu, sd, nn_p, ode_p):
    mask, sample_nn, P = cmap
    idx = ode_indices(mask)
    for d in range(zrow.shape[0]):
        if d < len(idx):
            if ode_p is not None:
                ode_p[c_slot, idx[d]] = mu[d] + sd[d] * zrow[d]
        elif sample_nn and nn_p is not None:
            nn_p[c_slot, d - len(idx)] = zrow[d]


def _natural(zrow, n_ode, mu, sd):
    out = zrow.copy()
    out[:n_ode] = mu[:n_ode] + sd[:n_ode] * zrow[:n_ode]
    return out


# ------------------------------------------------------------------------------------------------ HMC passes
def refresh(seed, it, jitter, minv, log_eps, z, g, U):
    C = z.shape[0]
    p = np.stack([momentum(seed, c, it, minv) for c in range(C)])
    ke0 = np.array([0.5 * _fsum(p[c] * p[c] * minv) for c in range(C)])
    eps = np.array([math.exp(log_eps[c]) * (1.0 + jitter * (2.0 * uniform(seed, c, it, JITTER, 0) - 1.0)) for c in range(C)])
    return dict(p=p, z0=z.copy(), g0=g.copy(), U0=U.copy(), ke0=ke0, eps=eps, failed=np.zeros(C, np.int32))


def leapfrog(flags, kick, eps, minv, z, p, g, U, ke, failed, cmap, mu=None, sd=None, gnn=None, gode=None, loss_sum=None,
             lik_scale=1.0, status=None, nn_p=None, ode_p=None):
    """The flags in the order assemble, kick, ke, drift, params.  status: [C][n_traj] or None."""
    C, D = z.shape
    z, p, g, U, ke, failed = z.copy(), p.copy(), g.copy(), U.copy(), ke.copy(), failed.copy()
    nn_p = None if nn_p is None else nn_p.copy()
    ode_p = None if ode_p is None else ode_p.copy()
    for c in range(C):
        if flags & ASSEMBLE:
            g[c] = _lik_grad(c, D, cmap, sd, gnn, gode) + z[c]
            U[c] = (lik_scale * loss_sum[c] if loss_sum is not None else 0.0) + 0.5 * _fsum(z[c] * z[c])
            if status is not None and np.any(status[c] != 0):
                failed[c] = 1
        if flags & KICK:
            p[c] = p[c] - kick * eps[c] * g[c]
        if flags & KE:
            ke[c] = 0.5 * _fsum(p[c] * p[c] * minv)
        if flags & DRIFT:
            z[c] = z[c] + eps[c] * minv * p[c]
        if flags & (DRIFT | PARAMS):
            _write_params(c, z[c], cmap, mu, sd, nn_p, ode_p)
    return dict(z=z, p=p, g=g, U=U, ke=ke, failed=failed, nn_p=nn_p, ode_p=ode_p)


def dual_average(st, delta, a):
    """One update of {mu, log eps bar, H bar, t} towards acceptance delta (Hoffman & Gelman 2014, gamma 0.05, t0 10,
    kappa 0.75).  Returns the new state and the new log eps."""
    t = st[3] + 1.0
    eta = 1.0 / (t + 10.0)
    hbar = (1.0 - eta) * st[2] + eta * (delta - a)
    le = st[0] - math.sqrt(t) / 0.05 * hbar
    w = t ** -0.75
    return np.array([st[0], w * le + (1.0 - w) * st[1], hbar, t]), le


def accept(mode, seed, it, delta, z, z0, g, g0, U, U0, ke0, ke, failed, log_eps, da, search, n_ode=0, mu=None, sd=None,
           draws=None, stats=None, slot=-1):
    """draws: [C][n_slots][D] or None; stats: [C][n_slots][4] or None."""
    C, D = z.shape
    z, g, U, log_eps, da, search = z.copy(), g.copy(), U.copy(), log_eps.copy(), da.copy(), search.copy()
    draws = None if draws is None else draws.copy()
    stats = None if stats is None else stats.copy()
    dec = []
    out = dict(z=z, g=g, U=U, log_eps=log_eps, da=da, search=search, draws=draws, stats=stats, decisions=dec)
    for c in range(C):
        if mode == DA_RESTART:
            da[c] = [math.log(10.0) + log_eps[c], 0.0, 0.0, 0.0]
            search[c] = 0
            continue
        if mode == DA_FINISH:
            if da[c, 3] > 0:
                log_eps[c] = da[c, 1]
            continue
        Hs, H1 = U0[c] + ke0[c], U[c] + ke[c]
        dH = H1 - Hs
        fail = failed[c] != 0
        # dH: three roundings in fp64 in both dtypes, (3 + 1) u64 over the four energies
        b_dH = 4 * U64 * (abs(U0[c]) + abs(ke0[c]) + abs(U[c]) + abs(ke[c])) if math.isfinite(dH) else 0.0
        keep = False
        if mode == SEARCH:
            lw = -math.inf if (fail or not math.isfinite(dH)) else -dH
            if not search[c, 1]:
                d = int(search[c, 0])
                if d == 0:
                    d = search[c, 0] = 1 if lw > LOG08 else -1
                dec.append(Decision("search", c, abs(lw - LOG08) if math.isfinite(lw) else math.inf, b_dH, b_dH))
                if (d == 1 and not lw > LOG08) or (d == -1 and not lw < LOG08):
                    search[c, 1] = 1
                else:
                    log_eps[c] += d * math.log(2.0)
        else:
            finite = math.isfinite(H1) and math.isfinite(dH)
            div = bool(fail or not math.isfinite(H1) or dH > 1000.0)
            dec.append(Decision("divergence", c, abs(dH - 1000.0) if (finite and not fail) else math.inf, b_dH, b_dH))
            a = 0.0 if div else (1.0 if dH <= 0 else math.exp(-dH))
            u = uniform(seed, c, it, ACCEPT, 0)
            # a = exp(-dH): the error of dH scaled by a, and two roundings of exp
            b_a = 0.0 if (div or dH <= 0) else a * b_dH + 2 * U64 * a
            dec.append(Decision("metropolis", c, math.inf if (div or dH <= 0) else abs(u - a), b_a, b_a))
            keep = (not div) and u < a
            if mode == ADAPT:
                da[c], log_eps[c] = dual_average(da[c], delta, a)
            if slot >= 0:
                stats[c, slot] = [a, -(U[c] if keep else U0[c]), 1.0 if div else 0.0, 1.0 if fail else 0.0]
        if not keep:
            U[c], z[c], g[c] = U0[c], z0[c], g0[c]
        if draws is not None and slot >= 0 and mode != SEARCH:
            draws[c, slot] = _natural(z[c], n_ode, mu, sd)
    return out


def welford(flags, z, wf, minv):
    """wf [3][D] = {count, mean, M2}.  ACCUM pools the C rows of z into it (Chan et al.'s merge of two-pass batch moments);
    FINISH sets minv = n/(n+5) var + 1e-3 * 5/(n+5) where n > 1, then zeroes wf."""
    wf, minv = wf.copy(), minv.copy()
    if flags & W_ACCUM:
        nb = z.shape[0]
        mb = z.mean(axis=0)
        m2b = ((z - mb) ** 2).sum(axis=0)
        na = wf[0]
        n = na + nb
        dl = mb - wf[1]
        wf = np.stack([n, wf[1] + dl * nb / n, wf[2] + m2b + dl * dl * na * nb / n])
    if flags & W_FINISH:
        n = wf[0]
        on = n > 1.0
        var = wf[2][on] / (n[on] - 1.0)
        minv[on] = (n[on] / (n[on] + 5.0)) * var + 1e-3 * (5.0 / (n[on] + 5.0))
        wf = np.zeros_like(wf)
    return wf, minv


# ------------------------------------------------------------------------------------------------ NUTS passes
def _copy_tree(T):
    return dict(tree=T["tree"].copy(), ckpt=dict(T["ckpt"]), dst=T["dst"].copy(), ist=T["ist"].copy())


def nuts_begin(z, p, g, U, U0, ke0, tree=None, dst=None, ist=None):
    """tree / dst / ist: what the buffers held before (rows and slots the call does not write keep it); None = NaN / 0."""
    C, D = z.shape
    tree = np.full((15, C, D), np.nan) if tree is None else tree.copy()
    dst = np.full((C, 8), np.nan) if dst is None else dst.copy()
    ist = np.zeros((C, 8), np.int32) if ist is None else ist.copy()
    for r, src in ((LZ, z), (LP, p), (LG, g), (RZ, z), (RP, p), (RG, g), (PZ, z), (PG, g), (RHO, p)):
        tree[r] = src
    dst[:, H0] = U0 + ke0
    dst[:, LOG_W] = 0.0
    dst[:, LOG_W_SUB] = -math.inf
    dst[:, SUM_ACC] = 0.0
    dst[:, U_PROP] = U
    dst[:, U_SUB] = U
    ist[:, :] = [0, 0, 0, 1, 0, 0, 1, 0]
    return dict(tree=tree, ckpt={}, dst=dst, ist=ist)


def nuts_pre(T, seed, it, eps, minv, rank, cmap, mu=None, sd=None, nn_p=None, ode_p=None):
    T = _copy_tree(T)
    tree, ist = T["tree"], T["ist"]
    nn_p = None if nn_p is None else nn_p.copy()
    ode_p = None if ode_p is None else ode_p.copy()
    dec = []
    for c in range(ist.shape[0]):
        if not ist[c, ACTIVE]:
            continue
        leaf, j, v = int(ist[c, LEAF_I]), int(ist[c, J]), int(ist[c, DIRECTION])
        if leaf == 0:
            u = uniform(seed, c, it, DIR, j)
            dec.append(Decision("direction", c, abs(u - 0.5), 0.0, 0.0))       # a Philox word against a constant: exact
            v = 1 if u < 0.5 else -1
            ist[c, DIRECTION], ist[c, DEPTH] = v, j + 1
        src = FZ if leaf else (RZ if v > 0 else LZ)
        sz, sp, sg = tree[src, c], tree[src + 1, c], tree[src + 2, c]
        fp = sp - 0.5 * v * eps[c] * sg
        fz = sz + v * eps[c] * minv * fp
        tree[FP, c], tree[FZ, c] = fp, fz
        _write_params(int(rank[c]), fz, cmap, mu, sd, nn_p, ode_p)
    return T, nn_p, ode_p, dec


def post_bounds(c, T, eps, minv, glik, n_ode):
    """Rounding bounds, per dtype unit u, of what hode_nuts_post computes in the kernel's real type R for chain c: returns
    (b_g [D], b_p [D]) as multiples of u.  g = lik + z with lik = gode (R)sd for a constant (the conversion, the product, the
    sum: k_g = 3) or gnn (the sum: k_g = 1): (k_g + 1) (|lik| + |z|).  p' = p - eh g with eh = (R)(v eps / 2): the roundings of
    eh, of the product and of the difference on top of g's, (k_g + 3 + 1) (|p| + |eh| (|lik| + |z|))."""
    fz, fp = T["tree"][FZ, c], T["tree"][FP, c]
    eh = abs(0.5 * eps[c])
    k_g = np.where(np.arange(fz.shape[0]) < n_ode, 3, 1)
    b_g = (k_g + 1) * (np.abs(glik) + np.abs(fz))
    b_p = (k_g + 4) * (np.abs(fp) + eh * (np.abs(glik) + np.abs(fz)))
    return b_g, b_p


def nuts_post(T, seed, it, eps, minv, rank, cmap, max_depth, sd=None, gnn=None, gode=None, loss_sum=None, lik_scale=1.0,
              status=None, fp_stored=None):
    """fp_stored [C][D]: the kernel's own stored p' (checked entry by entry first), which the chain sums ke and H are then
    taken over, so that they are bounded by the fp64 summation alone.  T["info"][c] holds the call's rounding bounds."""
    T = _copy_tree(T)
    info = T["info"] = {}
    tree, ckpt, dst, ist = T["tree"], T["ckpt"], T["dst"], T["ist"]
    C, D = tree.shape[1:]
    dec = []
    written = []                                         # the (chain, level) checkpoints this call wrote
    for c in range(C):
        if not ist[c, ACTIVE]:
            continue
        leaf, j, v, n_leaf = int(ist[c, LEAF_I]), int(ist[c, J]), int(ist[c, DIRECTION]), int(ist[c, N_LEAF]) + 1
        s = int(rank[c])
        fz = tree[FZ, c]
        glik = _lik_grad(s, D, cmap, sd, gnn, gode)
        b_g, b_p = post_bounds(c, T, eps, minv, glik, len(ode_indices(cmap[0])))
        fg = glik + fz
        fp = tree[FP, c] - 0.5 * v * eps[c] * fg
        tree[FG, c], tree[FP, c] = fg, fp
        U = (lik_scale * loss_sum[s] if loss_sum is not None else 0.0) + 0.5 * _fsum(fz * fz)
        fp_sum = fp if fp_stored is None else fp_stored[c]
        ke_terms = fp_sum * fp_sum * minv
        H = U + 0.5 * _fsum(ke_terms)
        ist[c, N_LEAF] = n_leaf
        bad = status is not None and bool(np.any(status[s] != 0))
        if bad:
            ist[c, FAILED] = 1
        # H: the stored p' carries b_p u per entry, so ke moves by sum minv (2 |p'| + b_p u) b_p u / 2; on top the fp64 sums
        # and products of 2 D + 4 terms, (2 D + 4) u64 sum |terms|
        mag = abs(U) + 0.5 * _fsum(np.abs(ke_terms)) + abs(dst[c, H0])
        b_sum = (2 * D + 4) * U64 * mag
        b_H = {u: (0.5 * _fsum(minv * (2 * np.abs(fp) + b_p * u) * b_p * u) if fp_stored is None else 0.0) + b_sum for u in (U64, U32)}
        info[c] = dict(b_g=b_g, b_p=b_p, b_H=b_H, mag=mag, rho_sub_in=np.abs(tree[RHO_SUB, c]) * (leaf != 0), rho_in=np.abs(tree[RHO, c]),
                       minv_b_p=minv * b_p)
        finite = math.isfinite(H)
        div = bool(bad or not finite or H - dst[c, H0] > 1000.0)
        dec.append(Decision("divergence", c, abs(H - dst[c, H0] - 1000.0) if (finite and not bad) else math.inf, b_H[U64], b_H[U32]))
        if div:
            ist[c, DIVERGENT], ist[c, ACTIVE] = 1, 0
            continue
        lw = dst[c, H0] - H
        dst[c, SUM_ACC] += 1.0 if lw >= 0.0 else math.exp(lw)
        lws = lw if leaf == 0 else float(np.logaddexp(dst[c, LOG_W_SUB], lw))
        dst[c, LOG_W_SUB] = lws
        u = uniform(seed, c, it, LEAF, n_leaf)
        thr = math.exp(lw - lws)
        # thr = exp(lw - lws): d thr = thr d(lw - lws), |d(lw - lws)| <= |d H|; four roundings of log1p, exp, the sums
        bt = (lambda bh: 0.0 if leaf == 0 else thr * bh + 5 * U64 * thr * (1 + abs(lw) + abs(lws)))
        dec.append(Decision("leaf", c, math.inf if leaf == 0 else abs(u - thr), bt(b_H[U64]), bt(b_H[U32])))
        if u < thr:
            tree[SZ, c], tree[SG, c] = fz, fg
            dst[c, U_SUB] = U
        ps = minv * fp
        before = np.zeros(D) if leaf == 0 else tree[RHO_SUB, c]
        for k in range(1, j + 1):
            if leaf % 2 ** k == 0:
                ckpt[(c, k)] = (ps.copy(), before.copy())
                written.append((c, k))
        rho_sub = before + fp
        tree[RHO_SUB, c] = rho_sub
        turn = False
        for k in range(1, j + 1):
            if (leaf + 1) % 2 ** k == 0 and not turn:
                first_p, rb = ckpt[(c, k)]
                blk = rho_sub - rb
                # blk from the stored rho_sub' = rho_sub + p' (one rounding in R on top of b_p u) and rb; the dot products
                # in fp64: (D + 1) u64 sum |terms|
                for name, w in (("uturn_first", first_p), ("uturn_last", ps)):
                    val = _fsum(w * blk)
                    bb = {uu: _fsum(np.abs(w) * ((b_p + np.abs(rho_sub)) * uu)) + _fsum(np.abs(blk) * minv * b_p * uu) * (name == "uturn_last")
                          + (D + 1) * U64 * _fsum(np.abs(w * blk)) for uu in (U64, U32)}
                    dec.append(Decision(name, c, abs(val), bb[U64], bb[U32]))
                    turn = turn or not val > 0.0
        if turn:
            ist[c, ACTIVE] = 0
            continue
        if leaf + 1 < 2 ** j:
            ist[c, LEAF_I] = leaf + 1
            continue
        lw_t = dst[c, LOG_W]
        u = uniform(seed, c, it, MERGE, j)
        thr = math.exp(lws - lw_t)
        bt = (lambda bh: thr * bh + 5 * U64 * thr * (1 + abs(lw_t) + abs(lws)))    # as the leaf choice; lw_t is an input
        dec.append(Decision("merge", c, abs(u - thr), bt(b_H[U64]), bt(b_H[U32])))
        if u < thr:
            tree[PZ, c], tree[PG, c] = tree[SZ, c], tree[SG, c]
            dst[c, U_PROP] = dst[c, U_SUB]
        dst[c, LOG_W] = float(np.logaddexp(lw_t, lws))
        e, o = (RZ, LZ) if v > 0 else (LZ, RZ)
        tree[e, c], tree[e + 1, c], tree[e + 2, c] = fz, fp, fg
        rho = tree[RHO, c] + rho_sub
        tree[RHO, c] = rho
        ends = False
        for name, pe, own in (("uturn_tree_v", fp, True), ("uturn_tree_opp", tree[o + 1, c], False)):
            val = _fsum(minv * pe * rho)
            # rho' = rho + rho_sub': one rounding in R on top of rho_sub's (b_p + |rho_sub|) u
            b_rho = b_p + np.abs(rho_sub) + np.abs(rho)
            bb = {uu: _fsum(np.abs(minv * pe) * b_rho * uu) + _fsum(np.abs(rho) * minv * b_p * uu) * own
                  + (2 * D + 1) * U64 * _fsum(np.abs(minv * pe * rho)) for uu in (U64, U32)}
            dec.append(Decision(name, c, abs(val), bb[U64], bb[U32]))
            ends = ends or not val > 0.0
        ist[c, J], ist[c, LEAF_I] = j + 1, 0
        if ends or j + 1 >= max_depth:
            ist[c, ACTIVE] = 0
    T["written"] = written
    return T, dec


def nuts_compact(ist):
    on = ist[:, ACTIVE] != 0
    rank = np.where(on, np.cumsum(on) - on, -1).astype(np.int32)
    return rank, int(on.sum())


def nuts_finish(T, adapt, delta, z, g, U, log_eps, da, n_ode=0, mu=None, sd=None, draws=None, stats=None, slot=-1):
    """draws: [C][n_slots][D] or None; stats: [C][n_slots][6] or None."""
    tree, dst, ist = T["tree"], T["dst"], T["ist"]
    C = tree.shape[1]
    z, g, U = tree[PZ].copy(), tree[PG].copy(), dst[:, U_PROP].copy()
    log_eps, da = log_eps.copy(), da.copy()
    draws = None if draws is None else draws.copy()
    stats = None if stats is None else stats.copy()
    for c in range(C):
        n_leaf = int(ist[c, N_LEAF])
        acc = dst[c, SUM_ACC] / n_leaf if n_leaf > 0 else 0.0
        if adapt:
            da[c], log_eps[c] = dual_average(da[c], delta, acc)
        if slot >= 0:
            stats[c, slot] = [acc, -dst[c, U_PROP], float(ist[c, DIVERGENT] != 0), float(ist[c, FAILED] != 0), float(ist[c, DEPTH]),
                              float(n_leaf)]
            if draws is not None:
                draws[c, slot] = _natural(z[c], n_ode, mu, sd)
    return dict(z=z, g=g, U=U, log_eps=log_eps, da=da, draws=draws, stats=stats)

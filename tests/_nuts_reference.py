"""A plain-numpy restatement of the No-U-Turn transition that inference/nuts.py runs on the GPU, and
a numpy Philox4x32-10 that gives the same random words as csrc/hode_philox.h.  tests/test_nuts_host.py checks the
restatement on a Gaussian; tests/test_nuts_gpu.py checks the kernels against it.

The transition, for one chain (multinomial NUTS, generalised U-turn criterion; Hoffman & Gelman 2014, Betancourt 2017):
  - H0 = U0 + ke0; left edge = right edge = (z, p, g); proposal = (z, g, U); log_w = 0 (leaf weights relative to H0);
    rho = p; j = 0; n_leaf = 0; sum_acc = 0.
  - while j < max_depth: direction v = +1 if u(DIR, j) < 0.5 else -1; 2^j leaves from the edge on side v, each one leapfrog
    step of signed size v eps.  At every leaf n_leaf += 1, then
      divergent (failed solve, H not finite, H - H0 > 1000): the subtree is rejected and the tree ends (adds 0 to sum_acc);
      sum_acc += min(1, exp(H0 - H)); log_w_sub = logaddexp(log_w_sub, H0 - H);
      the leaf becomes the subtree proposal if u(LEAF, n_leaf) < exp(H0 - H - log_w_sub); rho_sub += p;
      every aligned block of 2^k leaves (k >= 1) that ends here turns if p#_first . rho_blk <= 0 or p#_last . rho_blk <= 0:
      the subtree is rejected and the tree ends.
    A complete subtree is merged: its proposal replaces the tree's if u(MERGE, j) < exp(log_w_sub - log_w); log_w =
    logaddexp(log_w, log_w_sub); rho += rho_sub; the edge on side v = the last leaf; j += 1; the tree ends if
    p#_left . rho <= 0 or p#_right . rho <= 0.
  - (z, g, U) = the proposal; accept statistic = sum_acc / n_leaf; tree_depth = doublings started; n_leapfrog = n_leaf.
p# = M^-1 p with the diagonal minv.  Stan's extra checks across merged subtrees (2.26+) are not part of this definition."""
import math

import numpy as np

# stream tags of csrc/hode_philox.h
MOMENTUM, ACCEPT, JITTER, INIT, DIR, LEAF, MERGE = range(7)
_M32 = 0xFFFFFFFF


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & _M32, p1 & _M32, ((p0 >> 32) ^ c3 ^ k1) & _M32, p0 & _M32
        k0, k1 = (k0 + 0x9E3779B9) & _M32, (k1 + 0xBB67AE85) & _M32
    return c0, c1, c2, c3


def hmc_rng(seed, chain, it, tag, group):
    """key (seed bits 0..31, chain), counter (group, tag, iteration, seed bits 32..63)."""
    return philox4x32_10(group & _M32, tag, it & _M32, (seed >> 32) & _M32, seed & _M32, chain & _M32)


def u01(x):
    return (x + 0.5) * 2.3283064365386963e-10


def normals4(r):
    r0, r1 = math.sqrt(-2.0 * math.log(u01(r[0]))), math.sqrt(-2.0 * math.log(u01(r[2])))
    a0, a1 = 6.283185307179586 * u01(r[1]), 6.283185307179586 * u01(r[3])
    return [r0 * math.cos(a0), r0 * math.sin(a0), r1 * math.cos(a1), r1 * math.sin(a1)]


def momentum(seed, chain, it, minv):
    """hode_hmc_refresh's p = M^(1/2) xi, xi from four-coordinate groups of the momentum stream."""
    D = minv.shape[0]
    xi = np.concatenate([normals4(hmc_rng(seed, chain, it, MOMENTUM, grp)) for grp in range((D + 3) // 4)])[:D]
    return xi / np.sqrt(minv)


def philox_uniform(seed, chain, it):
    """u(tag, group) of one chain and iteration: the first word of the block, as the kernels take it."""
    return lambda tag, group: u01(hmc_rng(seed, chain, it, tag, group)[0])


def transition(z, p, g, U, eps, minv, u_grad, uniform, max_depth):
    """One NUTS transition from (z, p) with grad U = g and energy U.  u_grad(z) -> (U, grad U, solve failed);
    uniform(tag, group) -> a number in (0, 1).  Returns a dict: z, g, U, accept_stat, tree_depth, n_leapfrog, divergent,
    failed."""
    H0 = U + 0.5 * float(np.sum(p * p * minv))
    left, right = (z, p, g), (z, p, g)
    prop = (z, g, U)
    log_w, rho = 0.0, p.copy()
    j = n_leaf = depth = 0
    sum_acc = 0.0
    divergent = failed = False
    while j < max_depth:
        v = 1 if uniform(DIR, j) < 0.5 else -1
        depth += 1
        fz, fp, fg = right if v > 0 else left
        h, e = 0.5 * v * eps, v * eps
        log_w_sub, rho_sub, sub = -math.inf, np.zeros_like(p), None
        ckpt = {}                                       # level k -> (p# at the block's first leaf, rho_sub before it)
        ended = False
        for i in range(2 ** j):
            fp = fp - h * fg
            fz = fz + e * minv * fp
            Ul, gl, bad = u_grad(fz)
            fp, fg = fp - h * gl, gl
            H = Ul + 0.5 * float(np.sum(fp * fp * minv))
            n_leaf += 1
            failed = failed or bool(bad)
            if bad or not math.isfinite(H) or H - H0 > 1000.0:
                divergent = ended = True
                break
            lw = H0 - H
            sum_acc += 1.0 if lw >= 0 else math.exp(lw)
            log_w_sub = float(np.logaddexp(log_w_sub, lw))
            if uniform(LEAF, n_leaf) < math.exp(lw - log_w_sub):
                sub = (fz, fg, Ul)
            ps = minv * fp
            for k in range(1, j + 1):
                if i % 2 ** k == 0:
                    ckpt[k] = (ps, rho_sub.copy())
            rho_sub = rho_sub + fp
            for k in range(1, j + 1):
                if (i + 1) % 2 ** k == 0:
                    first, before = ckpt[k]
                    blk = rho_sub - before
                    if float(first @ blk) <= 0 or float(ps @ blk) <= 0:
                        ended = True
            if ended:
                break
        if ended:
            break
        if uniform(MERGE, j) < math.exp(log_w_sub - log_w):
            prop = sub
        log_w = float(np.logaddexp(log_w, log_w_sub))
        rho = rho + rho_sub
        if v > 0:
            right = (fz, fp, fg)
        else:
            left = (fz, fp, fg)
        j += 1
        if float((minv * left[1]) @ rho) <= 0 or float((minv * right[1]) @ rho) <= 0:
            break
    return {"z": prop[0], "g": prop[1], "U": prop[2], "accept_stat": sum_acc / n_leaf, "tree_depth": depth, "n_leapfrog": n_leaf,
            "divergent": divergent, "failed": failed}

"""A plain-numpy fp64 restatement of the EM noise fit over the unscented smoother (include/hode_ukf_em.h; csrc/hode_ukf_em.hip;
DESIGN.md section 4.24), written from the header's text on the pieces of tests/_ukf_reference.py.  tests/test_ukf_em_host.py
checks its properties (on linear-Gaussian models its statistic is the exact Kalman-smoother expectation, and its iterations
raise the exact evidence); tests/test_ukf_em_gpu.py holds the kernels and inference.fit_ukf_noise to it.

One patient per call up to `reduce`, everything fp64, explicit loops in the header's orders (numpy adds whole rows per index,
which is that order entry by entry).
  points   the sigma points of a step's smoothed moments in natural space, their constants and the Cholesky factor; `cond` = the
           2-norm condition number of the covariance on its non-zero columns, what the GPU test's tolerance scales with
  pair     the pair statistic e2 and pair_ok; `scale` = the largest magnitude among the terms e2 sums
  obs      the observation statistic r2 and the seen bits of one step
  reduce   the sums A, N, D, R, M over all patients in the header's fixed shape
  mstep    the new values from the sums"""
import math

import numpy as np

import _ukf_reference as UR

SLOTS, SUMS, FIT = 256, 37, 29
AT_A, AT_N, AT_D, AT_R, AT_M = 0, 23, 24, 25, 31


def points(mean, cov, ode_row, mode, w, link=1):
    """mean [n], cov [n, n]: the smoothed moments of step s; ode_row [17]: ode_history[s] row b * K.  Returns a dict: x [K, 6] and
    aux [K, 17] (fp64, not yet rounded to a storage type), chol [n, n], zero (its zero columns), cond."""
    gamma = w[0]
    cols, plog = UR.columns(mode)
    n = 6 + len(cols)
    K = 2 * n + 1
    islog = [link == 1] * 6 + plog
    with np.errstate(all="ignore"):
        L, zero, _ = UR.cholesky(cov)
        X = UR.draw(np.asarray(mean, dtype=np.float64), L, gamma)
        nat = np.stack([np.array([UR._exp(X[k, j]) if islog[j] else X[k, j] for j in range(n)]) for k in range(K)])
        aux = np.tile(np.asarray(ode_row, dtype=np.float64), (K, 1))
        aux[:, cols] = nat[:, 6:]
        keep = [j for j in range(n) if j not in zero]
        cond = UR._cond(np.asarray(cov)[np.ix_(keep, keep)])
    return {"x": nat[:, :6].copy(), "aux": aux, "chol": L, "zero": zero, "cond": cond}


def dead_points(ode_row, n):
    """What a pair into a dead step gets: rows a solve can take."""
    K = 2 * n + 1
    return {"x": np.ones((K, 6)), "aux": np.tile(np.asarray(ode_row, dtype=np.float64), (K, 1)), "chol": np.full((n, n), np.nan),
            "zero": [], "cond": np.nan}


def pair(prop, status, chol, mean_s, mean_n, cov_n, G, alive_n, w, link=1):
    """prop [K, 6]: the images of the points' states; status [K] or None; chol, mean_s: the factor and the smoothed mean of step
    s; mean_n, cov_n: the smoothed moments of step s + 1; G: the smoother gain of the pair; alive_n: alive[s + 1].
    Returns a dict: e2 [n], ok, and for a counted pair fbar, F, U, V, cross, scale."""
    gamma, wm0, wc0, wi = w
    n = len(mean_s)
    K = 2 * n + 1
    slog = link == 1
    prop = np.asarray(prop, dtype=np.float64)
    ok = bool(alive_n) and (status is None or not np.any(np.asarray(status) != 0)) and bool(np.isfinite(prop).all()) \
        and (not slog or bool((prop > 0).all()))
    if not ok:
        return {"e2": np.full(n, np.nan), "ok": 0}
    with np.errstate(all="ignore"):
        Z = UR.draw(np.asarray(mean_s, dtype=np.float64), chol, gamma)
        for k in range(K):
            for j in range(6):
                Z[k, j] = math.log(prop[k, j]) if slog else prop[k, j]
        fbar = UR._wsum(wm0, wi, [Z[k] for k in range(K)])
        F = UR._wsum(wc0, wi, [(Z[k] - fbar) * (Z[k] - fbar) for k in range(K)])
        wg = wi * gamma
        U = np.zeros((n, n))
        for j in range(n):
            if chol[j, j] != 0.0:
                U[j] = wg * (Z[1 + j] - Z[1 + n + j])
        V = np.zeros((n, n))
        for p in range(n - 1, -1, -1):                          # every column i at once: the same order entry by entry
            t = U[p].copy()
            for c in range(p + 1, n):
                t = t - chol[c, p] * V[c]
            V[p] = 0.0 if chol[p, p] == 0.0 else t / chol[p, p]
        W = np.zeros((n, n))
        for a in range(n):                                      # W[i][b] = sum_a Ps_{s+1}[i][a] G[b][a]
            W = W + np.outer(cov_n[:, a], G[:, a])
        cross, mag = np.zeros(n), np.zeros(n)
        for b in range(n):
            cross = cross + W[:, b] * V[b, :]
            mag = mag + np.abs(W[:, b] * V[b, :])
        d = np.asarray(mean_n, dtype=np.float64) - fbar
        pd = np.diag(cov_n)
        e2 = ((pd + d * d) - 2.0 * cross) + F
        scale = float(max(np.abs(pd).max(), (d * d).max(), 2.0 * mag.max(), F.max()))
    return {"e2": e2, "ok": 1, "fbar": fbar, "F": F, "U": U, "V": V, "cross": cross, "scale": scale}


def obs(y, mask, alive, moments):
    """y [6] (NaN = missing), mask [6] or None, alive, moments [12] of one step.  Returns (r2 [6], the seen bits)."""
    r2, bits = np.zeros(6), 0
    for j in range(6):
        if math.isfinite(y[j]) and (mask is None or bool(mask[j])) and bool(alive):
            r = float(y[j]) - moments[j]
            r2[j] = r * r + moments[6 + j]
            bits |= 1 << j
    return r2, bits


def reduce(e2, pair_ok, r2, seen, dt):
    """e2 [S-1, B, n], pair_ok [S-1, B], r2 [S, B, 6], seen [S, B], dt [S, B] -> sums [37]: per patient over s ascending, the
    patients of slot b mod 256 ascending, then the slots folded by halves."""
    S, B = r2.shape[:2]
    n = e2.shape[2] if S > 1 else 6
    slots = np.zeros((SLOTS, SUMS))
    for b in range(B):
        part = np.zeros(SUMS)
        for s in range(S - 1):
            if pair_ok[s, b]:
                for i in range(n):
                    part[AT_A + i] += e2[s, b, i] / dt[s + 1, b]
                part[AT_N] += 1.0
                part[AT_D] += dt[s + 1, b]
        for s in range(S):
            for j in range(6):
                if (int(seen[s, b]) >> j) & 1:
                    part[AT_R + j] += r2[s, b, j]
                    part[AT_M + j] += 1.0
        slots[b % SLOTS] = slots[b % SLOTS] + part
    h = SLOTS // 2
    while h >= 1:
        slots[:h] = slots[:h] + slots[h:2 * h]
        h //= 2
    return slots[0].copy()


def log_link_variance(A, N, D):
    """The maximiser of -(N / 2) log v - A / (2 v) - v D / 8 over v > 0, v = 2 (sqrt(N^2 + A D) - N) / D, in the form without the
    cancellation."""
    return (2.0 * A) / (math.sqrt(N * N + A * D) + N)


def mstep(sums, q, walk, sigma, mode, fit_mask, floor, link=1):
    """The new (q [6], walk [17], sigma [6]) from the sums; fit_mask, floor [29]: q, walk by column, sigma."""
    cols, _ = UR.columns(mode)
    q, walk, sigma = np.array(q, dtype=np.float64), np.array(walk, dtype=np.float64), np.array(sigma, dtype=np.float64)
    N, D = sums[AT_N], sums[AT_D]
    for v in range(FIT):
        if not fit_mask[v]:
            continue
        var = None
        if v < 23:
            i = v if v < 6 else (6 + cols.index(v - 6) if (v - 6) in cols else -1)
            if i >= 0 and N > 0:
                A = sums[AT_A + i]
                var = log_link_variance(A, N, D) if (v < 6 and link == 1) else A / N
            arr, at = (q, v) if v < 6 else (walk, v - 6)
        else:
            j = v - 23
            if sums[AT_M + j] > 0:
                var = sums[AT_R + j] / sums[AT_M + j]
            arr, at = sigma, j
        if var is not None and var >= 0.0 and arr[at] != 0.0:
            arr[at] = max(math.sqrt(var), float(floor[v]))
    return q, walk, sigma

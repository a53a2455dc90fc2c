"""A plain-numpy fp64 restatement of the unscented Rauch-Tung-Striebel smoother (include/hode_ukf_smooth.h;
csrc/hode_ukf_smooth.hip), written from the header's text on the pieces of tests/_ukf_reference.py.
tests/test_ukf_smooth_host.py checks its properties (on linear-Gaussian models it is the Kalman RTS smoother);
tests/test_ukf_smooth_gpu.py holds the kernels and UKFResult.smooth to it.

One patient per call, everything fp64, explicit loops in the header's orders.
  pair     phases a-d for the steps (s, s + 1): the predicted moments m-, P- of step s + 1, the cross covariance C, the gain
           G = C (P-)^-1 through the column Cholesky factor of P- and its zero columns; `cond` = the 2-norm condition number of
           P- on its non-zero columns, what the GPU test's tolerance scales with
  back     phase e, one step of the recursion; `scale` = the largest entry of |G| |D| |G^T|, the magnitude the terms of the
           smoothed covariance's update reach before they cancel
  moments  phase f: the natural-space mean and variance of the six states
  smooth   the whole pass over one patient's stored filter, lost steps included"""
import numpy as np

import _ukf_reference as UR


def link_points(x, aux, cols, islog):
    """[K, n] in link space from the rows x [K, 6] and aux [K, 17] in natural space."""
    raw = np.concatenate([np.asarray(x, dtype=np.float64), np.asarray(aux, dtype=np.float64)[:, cols]], axis=1)
    with np.errstate(all="ignore"):
        return np.stack([np.array([np.log(raw[k, j]) if islog[j] else raw[k, j] for j in range(raw.shape[1])]) for k in range(raw.shape[0])])


def pair(hist_s, ode_s, prop_n, mean_s, mode, q, walk, dt_n, w, link=1):
    """hist_s [K, 6], ode_s [K, 17]: what step s emitted; prop_n [K, 6]: the rows handed to step s + 1; mean_s [n]: the filtered
    mean of step s; dt_n: the dt of step s + 1.  Returns a dict: m_pred, P_pred, C, gain, cond."""
    gamma, wm0, wc0, wi = w
    cols, plog = UR.columns(mode)
    n = 6 + len(cols)
    K = 2 * n + 1
    slog = link == 1
    islog = [slog] * 6 + plog
    with np.errstate(all="ignore"):
        ZA, ZB = link_points(hist_s, ode_s, cols, islog), link_points(prop_n, ode_s, cols, islog)
        assert ZA.shape == (K, n)
        mt = UR._wsum(wm0, wi, [ZB[k] for k in range(K)])
        P = UR._wsum(wc0, wi, [np.outer(ZB[k] - mt, ZB[k] - mt) for k in range(K)])
        s = np.array([float(q[j]) for j in range(6)] + [float(walk[c]) for c in cols])
        s2 = (s * s) * float(dt_n)
        P[np.diag_indices(n)] += s2
        m = mt.copy()
        if slog:
            m[:6] = m[:6] - 0.5 * s2[:6]
        ms = np.asarray(mean_s, dtype=np.float64)
        Cx = UR._wsum(wc0, wi, [np.outer(ZA[k] - ms, ZB[k] - mt) for k in range(K)])
        L, zero, _ = UR.cholesky(P)
        G = np.zeros((n, n))
        for i in range(n):
            g = Cx[i].copy()
            for p in range(n):
                t = g[p]
                for c in range(p):
                    t -= L[p, c] * g[c]
                g[p] = 0.0 if p in zero else t / L[p, p]
            for p in range(n - 1, -1, -1):
                t = g[p]
                for c in range(p + 1, n):
                    t -= L[c, p] * g[c]
                g[p] = 0.0 if p in zero else t / L[p, p]
            G[i] = g
        keep = [j for j in range(n) if j not in zero]
        cond = UR._cond(P[np.ix_(keep, keep)])
    return {"m_pred": m, "P_pred": P, "C": Cx, "gain": G, "cond": cond, "zero": zero}


def back(mean_f, cov_f, G, m_pred, P_pred, mean_next, cov_next):
    """One step of the recursion: (ms_s, Ps_s, scale) from the filtered moments of step s and the smoothed ones of step s + 1."""
    n = len(mean_f)
    with np.errstate(all="ignore"):
        delta, D = mean_next - m_pred, cov_next - P_pred
        ms = np.empty(n)
        for i in range(n):
            acc = 0.0
            for j in range(n):
                acc += G[i, j] * delta[j]
            ms[i] = mean_f[i] + acc
        T, U = np.zeros((n, n)), np.zeros((n, n))
        for j in range(n):                                      # T_ik = sum_j G_ij D_jk, j ascending, whole matrices per j
            T = T + np.outer(G[:, j], D[j, :])
        for k in range(n):                                      # U_ij = sum_k T_ik G_jk, k ascending
            U = U + np.outer(T[:, k], G[:, k])
        A = cov_f + U
        Ps = 0.5 * (A + A.T)
        scale = float((np.abs(G) @ np.abs(D) @ np.abs(G).T).max()) if np.isfinite(G).all() and np.isfinite(D).all() else np.nan
    return ms, Ps, scale


def moments(mean, cov, mode, w, link=1):
    """[12]: the unscented mean and variance of the six states in natural space of the points of (mean, cov)."""
    gamma, wm0, wc0, wi = w
    cols, plog = UR.columns(mode)
    n = 6 + len(cols)
    K = 2 * n + 1
    with np.errstate(all="ignore"):
        L, _, _ = UR.cholesky(cov)
        X = UR.draw(mean, L, gamma)
        nat = np.stack([np.array([UR._exp(X[k, j]) if link == 1 else X[k, j] for j in range(6)]) for k in range(K)])
        mu = UR._wsum(wm0, wi, [nat[k] for k in range(K)])
        var = UR._wsum(wc0, wi, [(nat[k] - mu) * (nat[k] - mu) for k in range(K)])
    return np.concatenate([mu, var])


def smooth(hist, ode, prop, mean_f, cov_f, alive, mode, q, walk, dt, w, link=1):
    """One patient's stored filter: hist / prop [S, K, 6], ode [S, K, 17], mean_f [S, n], cov_f [S, n, n], alive [S], dt [S].
    Returns a dict of mean_s [S, n], cov_s [S, n, n], gain [S-1, n, n], pred_mean [S-1, n], pred_cov [S-1, n, n], moments [S, 12],
    cond [S-1], scale [S-1] (NaN where the header says NaN) and `terminal`."""
    S, n = mean_f.shape
    alive = [bool(v) for v in alive]
    term = max([s for s in range(S) if alive[s]], default=-1)
    out = {"mean_s": np.full((S, n), np.nan), "cov_s": np.full((S, n, n), np.nan), "gain": np.full((S - 1, n, n), np.nan),
           "pred_mean": np.full((S - 1, n), np.nan), "pred_cov": np.full((S - 1, n, n), np.nan), "moments": np.full((S, 12), np.nan),
           "cond": np.full(S - 1, np.nan), "scale": np.full(S - 1, np.nan), "terminal": term}
    for s in range(S - 1):
        if alive[s + 1]:
            p = pair(hist[s], ode[s], prop[s + 1], mean_f[s], mode, q, walk, dt[s + 1], w, link)
            out["gain"][s], out["pred_mean"][s], out["pred_cov"][s], out["cond"][s] = p["gain"], p["m_pred"], p["P_pred"], p["cond"]
    if term >= 0:
        out["mean_s"][term], out["cov_s"][term] = mean_f[term], cov_f[term]
    for s in range(term - 1, -1, -1):
        out["mean_s"][s], out["cov_s"][s], out["scale"][s] = back(mean_f[s], cov_f[s], out["gain"][s], out["pred_mean"][s],
                                                                  out["pred_cov"][s], out["mean_s"][s + 1], out["cov_s"][s + 1])
    for s in range(term + 1):
        out["moments"][s] = moments(out["mean_s"][s], out["cov_s"][s], mode, w, link)
    return out

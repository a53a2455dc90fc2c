"""A plain-numpy fp64 restatement of one step of the unscented Kalman filter (include/hode.h "Unscented Kalman filter";
csrc/hode_ukf.hip), written from the header's text.  tests/test_ukf_host.py checks its properties (on
linear-Gaussian models it is a Kalman filter); tests/test_ukf_gpu.py holds the kernel and inference.run_ukf to it.

One patient per call, everything fp64.  Every sum over the sigma points runs from 0.0 over k = 0, 1, ... in order with the weight
multiplied first (numpy adds whole matrices per k, which is that order entry by entry); the Cholesky factor and the substitutions
subtract their terms in index order.
  a. predict  zeta_k = (g(x_in[k]), phi(aux_in[k][cols])), m- and P- with diag(s^2) added, then the log link's -s^2 / 2 drift
  b. redraw   column Cholesky without pivoting, zero column at a pivot <= n 2^-52 |P_jj|, chi = m-, m- +- gamma L[:, i]
  c. update   Y = g^-1(chi) on the seen states, S, C; z = L_S^-1 r, W = C L_S^-T, m = m- + W z, P = sym(P- - W W^T)
  d. emit     the points of (m, P), in natural space
`cond` = the larger 2-norm condition number of P- (restricted to its non-zero columns) and of S: what the tolerance of the GPU
test scales with."""
import math

import numpy as np

COLS = 16
LINK = {"additive": 0, "log": 1}
MOVE = {"carried": 0, "identity": 1, "log": 2}
LOG_2PI = 1.8378770664093453
EPS = 2.0 ** -52


def _exp(v):
    return float(np.exp(v))                                     # (inf on overflow, where math.exp raises)


def weights(n, alpha=1.0, beta=0.0, kappa=1.0):
    lam = alpha * alpha * (n + kappa) - n
    wm0 = lam / (n + lam)
    return math.sqrt(n + lam), wm0, wm0 + 1.0 - alpha * alpha + beta, 1.0 / (2.0 * (n + lam))


def columns(mode):
    mode = [int(v) for v in mode]
    assert len(mode) == 17 and all(v in (0, 1, 2) for v in mode)
    cols = [c for c in range(17) if mode[c]]
    return cols, [mode[c] == 2 for c in cols]


def cholesky(A):
    """(L, zero columns, lost): the header's column Cholesky of the symmetric A."""
    n = A.shape[0]
    L = np.zeros((n, n))
    zero, lost = [], False
    for j in range(n):
        piv = A[j, j]
        for k in range(j):
            piv -= L[j, k] * L[j, k]
        if not math.isfinite(piv):
            lost = True
        if not math.isfinite(piv) or not piv > n * EPS * abs(A[j, j]):
            zero.append(j)
            continue
        root = math.sqrt(piv)
        L[j, j] = root
        for i in range(j + 1, n):
            t = A[i, j]
            for k in range(j):
                t -= L[i, k] * L[j, k]
            L[i, j] = t / root
    return L, zero, lost


def draw(m, L, gamma):
    n = m.shape[0]
    Z = np.empty((2 * n + 1, n))
    Z[0] = m
    for i in range(n):
        Z[1 + i] = m + gamma * L[:, i]
        Z[1 + n + i] = m - gamma * L[:, i]
    return Z


def _wsum(w0, wi, terms):
    acc = np.zeros_like(terms[0])
    for k, t in enumerate(terms):
        acc = acc + (w0 if k == 0 else wi) * t
    return acc


def _cond(A):
    if A.size == 0:
        return 1.0
    with np.errstate(all="ignore"):
        s = np.linalg.svd(A, compute_uv=False)
    return float(s[0] / s[-1]) if s[-1] > 0 else math.inf


def step(x_in, aux_in, mode, obs, sigma, q, walk, dt, alive, mean, cov, w, predict=True, link=1, status=None, mask=None):
    """x_in [K, 6], aux_in [K, 17], mode [17], obs [6], sigma / q [6], walk [17], dt scalar, alive 0 / 1, mean [n], cov [n, n]
    (read with predict=False), w = (gamma, wm0, wc0, wi).  Returns a dict: alive, mean, cov, x_out [K, 6] and aux_out [K, 17]
    (fp64, not yet rounded to a storage type), stats [16], m_pred, P_pred (the moments the update started from), cond."""
    gamma, wm0, wc0, wi = w
    cols, plog = columns(mode)
    n = 6 + len(cols)
    K = 2 * n + 1
    x_in, aux_in, obs = np.asarray(x_in, dtype=np.float64), np.asarray(aux_in, dtype=np.float64), np.asarray(obs, dtype=np.float64)
    assert x_in.shape == (K, 6) and aux_in.shape == (K, 17)
    slog = link == 1
    islog = [slog] * 6 + plog
    seen = [j for j in range(6) if math.isfinite(obs[j]) and (mask is None or bool(mask[j]))]
    d = len(seen)
    lost = not alive
    cond = 1.0

    def result():
        stats = np.full(COLS, np.nan)
        stats[0], stats[2], stats[3] = -math.inf, d, 0.0
        return {"alive": 0, "mean": np.full(n, np.nan), "cov": np.full((n, n), np.nan), "x_out": x_in.copy(), "aux_out": aux_in.copy(),
                "stats": stats, "cond": cond, "m_pred": None, "P_pred": None}

    with np.errstate(all="ignore"):
        # ---- a
        if predict:
            raw = np.concatenate([x_in, aux_in[:, cols]], axis=1)                    # [K, n]
            ok = np.isfinite(raw).all() and all((raw[:, j] > 0).all() for j in range(n) if islog[j])
            if status is not None and np.any(np.asarray(status) != 0):
                ok = False
            if not ok:
                lost = True
            if lost:
                return result()
            Z = np.stack([np.array([math.log(raw[k, j]) if islog[j] else raw[k, j] for j in range(n)]) for k in range(K)])
            m = _wsum(wm0, wi, [Z[k] for k in range(K)])
            P = _wsum(wc0, wi, [np.outer(Z[k] - m, Z[k] - m) for k in range(K)])
            s = np.array([float(q[j]) for j in range(6)] + [float(walk[c]) for c in cols])
            s2 = (s * s) * float(dt)
            P[np.diag_indices(n)] += s2
            if slog:
                m[:6] = m[:6] - 0.5 * s2[:6]
        else:
            if lost:
                return result()
            m, P = np.array(mean, dtype=np.float64).reshape(n), np.array(cov, dtype=np.float64).reshape(n, n)
        m_pred, P_pred = m.copy(), P.copy()
        # ---- b
        L, zero, bad = cholesky(P)
        if bad:
            return result()
        keep = [j for j in range(n) if j not in zero]
        cond = _cond(P[np.ix_(keep, keep)])
        X = draw(m, L, gamma)
        # ---- c
        inc = nis = 0.0
        if d:
            Y = np.stack([np.array([_exp(X[k, j]) if slog else X[k, j] for j in seen]) for k in range(K)])
            yh = _wsum(wm0, wi, [Y[k] for k in range(K)])
            S = _wsum(wc0, wi, [np.outer(Y[k] - yh, Y[k] - yh) for k in range(K)])
            S[np.diag_indices(d)] += np.array([float(sigma[j]) * float(sigma[j]) for j in seen])
            C = _wsum(wc0, wi, [np.outer(X[k] - m, Y[k] - yh) for k in range(K)])
            r = obs[seen] - yh
            LS = np.zeros((d, d))
            for j in range(d):
                piv = S[j, j]
                for k in range(j):
                    piv -= LS[j, k] * LS[j, k]
                if not (math.isfinite(piv) and piv > 0):
                    return result()
                LS[j, j] = math.sqrt(piv)
                for i in range(j + 1, d):
                    t = S[i, j]
                    for k in range(j):
                        t -= LS[i, k] * LS[j, k]
                    LS[i, j] = t / LS[j, j]
            cond = max(cond, _cond(S))
            z, ld = np.zeros(d), 0.0
            for p in range(d):
                t = r[p]
                for c in range(p):
                    t -= LS[p, c] * z[c]
                z[p] = t / LS[p, p]
                nis += z[p] * z[p]
                ld += math.log(LS[p, p])
            inc = -0.5 * ((nis + 2.0 * ld) + d * LOG_2PI)
            W = np.zeros((n, d))
            m = m.copy()
            for i in range(n):
                acc = 0.0
                for p in range(d):
                    t = C[i, p]
                    for c in range(p):
                        t -= LS[p, c] * W[i, c]
                    W[i, p] = t / LS[p, p]
                    acc += W[i, p] * z[p]
                m[i] = m[i] + acc
            T = P.copy()
            for p in range(d):
                T = T - np.outer(W[:, p], W[:, p])
            P = 0.5 * (T + T.T)
        # ---- d
        L, zero, bad = cholesky(P)
        if bad:
            return result()
        X = draw(m, L, gamma)
        nat = np.stack([np.array([_exp(X[k, j]) if islog[j] else X[k, j] for j in range(n)]) for k in range(K)])
        if not np.isfinite(nat).all():
            return result()
        aux_out = np.tile(aux_in[0], (K, 1))
        aux_out[:, cols] = nat[:, 6:]
        stats = np.empty(COLS)
        stats[0:4] = [inc, nis, d, 1.0]
        mu = _wsum(wm0, wi, [nat[k, :6] for k in range(K)])
        stats[4:10] = mu
        stats[10:16] = _wsum(wc0, wi, [(nat[k, :6] - mu) * (nat[k, :6] - mu) for k in range(K)])
    return {"alive": 1, "mean": m, "cov": P, "x_out": nat[:, :6].copy(), "aux_out": aux_out, "stats": stats, "cond": cond,
            "m_pred": m_pred, "P_pred": P_pred}

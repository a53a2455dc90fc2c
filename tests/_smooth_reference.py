"""A numpy fp64 restatement of backward-simulation smoothing over a stored particle filter (include/hode.h "Particle smoother";
csrc/hode_smooth.hip), written from the header's text, with the numpy Philox of tests/_nuts_reference.py.
tests/test_smooth_host.py checks its properties; tests/test_smooth_gpu.py holds the kernel and FilterResult.smooth to it.

One patient per call, vectorised over the N candidates, loops over (m, s).  For trajectory m:
  last step    l_i = lwh[S-1][i]
  step s       x~ = hist[s+1][k_{s+1}], sg_j = q_j sqrt(dt[s+1]), r_j = 1 / sg_j, p = pred[s+1][i];
               l_i = lwh[s][i] + sum_j tau_j (j from 0 in order); sg_j > 0: tau_j = -0.5 (z z), z = (x~_j - p_j) r_j (additive) or
               (log x~_j - (log p_j - 0.5 (sg_j sg_j))) r_j (log); otherwise tau_j = 0 if p_j == x~_j else -inf; non-finite l = -inf
  draw         mx = max l, w = exp(l - mx), c = the sequential running sum (numpy's cumsum is one), u = u01(word 0 of
               block(seed, key, step s, tag 10, group m)), k_s = min{k : c_k >= u c_{N-1}}; nobody alive: -1 / NaN from here back.
Besides idx and paths the call returns what the tie condition of the GPU test needs, each the extreme over all draws of the call:
  tie      the smallest distance of any pointer u c_{N-1} to any boundary c_k, relative to c_{N-1};
  spread   the largest |l_i - mx| of a candidate alive;
  logamp   the largest |log v| |z_j| r_j over the log-link terms, v being p_j or x~_j (0 under the additive link).
`transition=False` drops the transition term (the control of the host test: that is genealogy-free resampling of the FILTER
weights at every step, which is not the smoothing distribution)."""
import math

import numpy as np

from _nuts_reference import hmc_rng, u01

SMOOTH = 10                        # stream tag kRngFilterSmooth of csrc/hode_philox.h


def smooth(hist, lwh, pred, q, dt, M, seed=0, key=0, link=1, transition=True):
    """hist / pred [S, N, 6] (the stored values, any float type), lwh [S, N], q [6], dt [S].  Returns a dict: idx [S, M] int32,
    paths [S, M, 6] of hist's dtype, tie, spread, logamp."""
    hist, pred = np.asarray(hist), np.asarray(pred)
    S, N, _ = hist.shape
    h64, p64, lwh = hist.astype(np.float64), pred.astype(np.float64), np.asarray(lwh, dtype=np.float64)
    idx = np.full((S, M), -1, dtype=np.int32)
    paths = np.full((S, M, 6), np.nan, dtype=hist.dtype)
    tie, spread, logamp = math.inf, 0.0, 0.0
    # per step: the candidates' side of the density, once (as the kernel stages it)
    cand = []
    for s in range(S - 1):
        sg = np.array([float(q[j]) * math.sqrt(float(dt[s + 1])) for j in range(6)])
        pos = sg > 0.0
        r = np.where(pos, 1.0 / np.where(pos, sg, 1.0), 0.0)
        c = p64[s + 1].copy()
        if link == 1:
            with np.errstate(invalid="ignore", divide="ignore"):
                c[:, pos] = np.log(p64[s + 1][:, pos]) - 0.5 * (sg[pos] * sg[pos])
        cand.append((pos, r, c))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for m in range(M):
            k = -1
            for s in range(S - 1, -1, -1):
                l = lwh[s].copy()
                if s < S - 1 and transition:
                    pos, r, c = cand[s]
                    xt = h64[s + 1][k]
                    a = np.where(pos, np.log(xt), xt) if link == 1 else xt
                    acc = np.zeros(N)
                    for j in range(6):
                        if pos[j]:
                            z = (a[j] - c[:, j]) * r[j]
                            acc = acc + -0.5 * (z * z)
                            if link == 1:
                                za = np.abs(z[np.isfinite(z)])
                                if za.size:
                                    amp = np.abs(np.log(p64[s + 1][:, j][np.isfinite(z)]))
                                    logamp = max(logamp, float((np.maximum(amp, abs(a[j])) * za).max() * r[j]))
                        else:
                            acc = acc + np.where(a[j] == c[:, j], 0.0, -np.inf)
                    l = l + acc
                l = np.where(np.isfinite(l), l, -np.inf)
                mx = l.max()
                if mx == -np.inf:
                    break                                          # lost: -1 / NaN at this step and every earlier one
                w = np.where(l > -np.inf, np.exp(l - mx), 0.0)
                c_run = np.cumsum(w)
                target = u01(hmc_rng(seed, key, s, SMOOTH, m)[0]) * c_run[N - 1]
                k = int(np.searchsorted(c_run, target, side="left"))           # min{k : c_k >= target}
                assert k < N and w[k] > 0.0
                near = c_run[k] - target
                if k > 0:
                    near = min(near, target - c_run[k - 1])
                tie = min(tie, float(near) / c_run[N - 1])
                spread = max(spread, float(np.abs(l[l > -np.inf] - mx).max()))
                idx[s, m] = k
                paths[s, m] = hist[s, k]
    return {"idx": idx, "paths": paths, "tie": tie, "spread": spread, "logamp": logamp}


def tie_bound(N, spread, logamp):
    """How far the kernel's and the restatement's c_k / c_{N-1} can differ (derived in tests/test_smooth_gpu.py)."""
    eps = 2.0 ** -52
    return N * 2.0 ** -53 + 2.0 * (eps * (2.0 + spread) + 12.0 * eps * logamp)

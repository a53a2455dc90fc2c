"""A plain-numpy fp64 restatement of one step of the bootstrap particle filter (include/hode.h "Particle filter"; csrc/hode_filter.hip;
DESIGN.md section 4.19), written from the header's text, with the numpy Philox of tests/_nuts_reference.py.
tests/test_filter_host.py checks its properties; tests/test_filter_gpu.py holds the kernel and inference.run_filter to it.

One patient per call.  Everything is fp64; `x_out` is rounded once, to `dtype`.
  a. noise     s_j = q_j sqrt(dt) > 0: xi = normals4(block(seed, key, step, tag 8, group 2 i + (j >> 2)))[j & 3];
               additive x += s xi, log x *= exp(s xi - s^2 / 2); s == 0 copies.
  b. weight    lw_i += sum_j seen_j [-z^2 / 2 - log sigma_j - log(2 pi) / 2], z = (obs_j - x_ij) / sigma_j; dead = status != 0,
               non-finite state, lw -inf or NaN on entry.
  c. normalise m = max lw, w = exp(lw - m); the stats use math.fsum (the exactly rounded sum), so they are the reference every
               summation order is within (terms) * 2^-53 of; c_k is the SEQUENTIAL running sum, as the header defines anc on it.
  d. resample  iff ESS < ess_frac N: u = u01(word 0 of block(seed, key, step, tag 9, group 0)),
               anc_i = min{k : c_k >= (i + u) / N * c_{N-1}}; lw = 0.
  e. gather.
`tie`: the smallest distance of any pointer (i + u) / N * c_{N-1} to any boundary c_k, relative to c_{N-1} (inf when nothing
was resampled): where it is far above the summation error N * 2^-53 of c, every correct scan gives the same ancestors."""
import math

import numpy as np

from _nuts_reference import hmc_rng, normals4, u01

NOISE, RESAMPLE = 8, 9            # stream tags kRngFilterNoise, kRngFilterResample of csrc/hode_philox.h
HALF_LOG_2PI = 0.9189385332046727
COLS = 16
LINK = {"additive": 0, "log": 1}


def noise(x_row, s, link, seed, key, step, i):
    """The fp64 state of particle i after the process noise."""
    x = [float(v) for v in x_row]
    n = [0.0] * 8
    if any(s[j] > 0.0 for j in range(4)):
        n[0:4] = normals4(hmc_rng(seed, key, step, NOISE, 2 * i))
    if s[4] > 0.0 or s[5] > 0.0:
        n[4:8] = normals4(hmc_rng(seed, key, step, NOISE, 2 * i + 1))
    for j in range(6):
        if s[j] > 0.0:
            if link == 1:
                x[j] = x[j] * math.exp(s[j] * n[j] - 0.5 * (s[j] * s[j]))
            else:
                x[j] = x[j] + s[j] * n[j]
    return x


def _lse(v):
    """(max, fsum exp(v - max)) of the finite-or--inf entries of v; (-inf, 0) when all are -inf."""
    m = max(v)
    if m == -math.inf:
        return m, 0.0
    return m, math.fsum(math.exp(a - m) for a in v if a > -math.inf)


def step(x_in, obs, sigma, q, dt, lw, step, seed=0, key=0, link=1, ess_frac=0.5, status=None, mask=None, aux=None, dtype=np.float64):
    """x_in [N, 6], obs [6], sigma / q [6], dt scalar, lw [N] (not modified), aux [N, n_aux] or None.
    Returns a dict: x (fp64, after the noise, before the gather), x_out [N, 6] of `dtype`, lw [N], anc [N] int32, stats [16],
    aux_out, tie."""
    x_in = np.asarray(x_in)
    N = x_in.shape[0]
    obs = np.asarray(obs)
    rdt = math.sqrt(float(dt))
    s = [float(q[j]) * rdt for j in range(6)]
    seen = [bool(np.isfinite(obs[j])) and (mask is None or bool(mask[j])) for j in range(6)]
    lsig = [math.log(float(sigma[j])) for j in range(6)]
    lw_in = [(-math.inf if not (float(v) > -math.inf) else float(v)) for v in lw]
    x = np.empty((N, 6))
    new = []
    for i in range(N):
        xi = noise(x_in[i], s, link, seed, key, step, i)
        x[i] = xi
        ok = (status is None or int(status[i]) == 0) and all(math.isfinite(v) for v in xi)
        acc = 0.0
        for j in range(6):
            if seen[j]:
                z = (float(obs[j]) - xi[j]) / float(sigma[j])
                acc += (-0.5 * (z * z) - lsig[j]) - HALF_LOG_2PI
        v = lw_in[i] + acc
        new.append(v if ok and math.isfinite(v) else -math.inf)
    stats = np.full(COLS, np.nan)
    anc = np.arange(N, dtype=np.int32)
    m_in, c_in = _lse(lw_in)
    m, tot = _lse(new)
    alive = [v > -math.inf for v in new]
    tie = math.inf
    if not any(alive):
        stats[0:4] = [-math.inf, 0.0, 0.0, 0.0]
        lw_out = np.full(N, -np.inf)
    else:
        w = [math.exp(v - m) if a else 0.0 for v, a in zip(new, alive)]
        sw2 = math.fsum(a * a for a in w)
        ess = (tot * tot) / sw2
        stats[0] = (m + math.log(tot)) - (m_in + math.log(c_in))
        stats[1], stats[3] = ess, float(sum(alive))
        for j in range(6):
            mean = math.fsum(w[i] * x[i, j] for i in range(N) if alive[i]) / tot
            stats[4 + j] = mean
            stats[10 + j] = math.fsum(w[i] * ((x[i, j] - mean) * (x[i, j] - mean)) for i in range(N) if alive[i]) / tot
        resample = ess < ess_frac * N
        stats[2] = 1.0 if resample else 0.0
        lw_out = np.array(new)
        if resample:
            c = np.empty(N)
            run = 0.0
            for k in range(N):
                run += w[k]
                c[k] = run
            u = u01(hmc_rng(seed, key, step, RESAMPLE, 0)[0])
            target = np.array([(i + u) / N * c[N - 1] for i in range(N)])
            anc = np.searchsorted(c, target, side="left").astype(np.int32)        # min{k : c_k >= target}
            assert anc.max() < N and all(alive[k] for k in anc)
            lo = np.abs(target - c[np.maximum(anc - 1, 0)])
            hi = np.abs(c[anc] - target)
            tie = float(min(lo[anc > 0].min() if (anc > 0).any() else math.inf, hi.min())) / c[N - 1]
            lw_out = np.zeros(N)
    return {"x": x, "x_out": x[anc].astype(dtype), "lw": lw_out, "anc": anc, "stats": stats,
            "aux_out": None if aux is None else np.asarray(aux)[anc], "tie": tie}


def systematic(weights, u):
    """Systematic resampling alone (sequential c_k): the ancestors of normalised or unnormalised weights."""
    c = np.cumsum(np.asarray(weights, dtype=np.float64))      # numpy's cumsum is the sequential running sum
    N = len(c)
    target = np.array([(i + u) / N * c[N - 1] for i in range(N)])
    return np.searchsorted(c, target, side="left").astype(np.int32)

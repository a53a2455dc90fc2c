"""A plain-numpy fp64 restatement of the particle filter's parameter move (include/hode.h "Particle filter: parameter move";
csrc/hode_pf_params.hip), written from the header's text, with the numpy Philox of
tests/_nuts_reference.py.  tests/test_pf_params_host.py checks its properties and the method on a linear-Gaussian model;
tests/test_pf_params_gpu.py holds the kernel and inference.run_filter(learn=...) to it.

One patient per call.  Everything is fp64; the moved rows are rounded once, to `dtype`.
  counting   particle i counts iff lw_i > -inf (false for NaN) and every selected value of its row is finite and, under the log
             link, positive; m = max lw over those, w = exp(lw - m).  Nobody counts: pstats all NaN, nothing moves.
  moments    phi = theta or log theta; mean = sum(w phi) / sum(w); var = sum(w (phi - mean)^2) / sum(w).  The sums are
             `total` = math.fsum, the exactly rounded sum that every summation order is within (terms) * 2^-53 of; a test
             passes another `total` to show what the order of the sum can change.
  move       unless a == 1 and walk_k == 0: sd = sqrt((1 - a a) var + walk_k^2 dt),
             eps = normals4(block(seed, key, step, tag 11, group 5 i + (k >> 2)))[k & 3],
             phi' = (mean + a (phi - mean)) + sd eps; theta' = phi' or exp(phi').
`shrinkage=False` drops the shrinkage from the move (phi' = phi + sd eps): the control of the method test, not the kernel's."""
import math

import numpy as np

from _nuts_reference import hmc_rng, normals4

PARAM = 11                        # stream tag kRngFilterParam of csrc/hode_philox.h
CARRIED, IDENTITY, LOG = 0, 1, 2  # HODE_PF_MOVE_*


def epsilon(seed, key, step, i, k):
    """The draw of particle i, column k."""
    return normals4(hmc_rng(seed, key, step, PARAM, 5 * i + (k >> 2)))[k & 3]


def move(lw, aux, mode, walk, dt, shrink, step, seed=0, key=0, dtype=np.float64, total=math.fsum, shrinkage=True):
    """lw [N], aux [N, n_aux] (not modified), mode / walk [n_aux], dt and shrink scalars.
    Returns a dict: aux (the moved rows, of `dtype`; untouched entries are the input's values cast to `dtype`), phi_new [N, n_aux]
    fp64 (phi' where a value was moved, else NaN), pstats [2 n_aux], counts [N] bool, sd [n_aux] (NaN where nothing moved)."""
    aux_in = np.asarray(aux)
    N, n_aux = aux_in.shape
    out = aux_in.astype(dtype).copy()
    phi_new = np.full((N, n_aux), np.nan)
    pstats = np.full(2 * n_aux, np.nan)
    sds = np.full(n_aux, np.nan)
    sel = [k for k in range(n_aux) if int(mode[k]) in (IDENTITY, LOG)]
    a = float(shrink)

    def usable(i):
        if not (float(lw[i]) > -math.inf):
            return False
        for k in sel:
            v = float(aux_in[i, k])
            if not math.isfinite(v) or (int(mode[k]) == LOG and not v > 0.0):
                return False
        return True
    counts = np.array([usable(i) for i in range(N)], dtype=bool)
    res = {"aux": out, "phi_new": phi_new, "pstats": pstats, "counts": counts, "sd": sds}
    live = [i for i in range(N) if counts[i]]
    if not live:
        return res
    m = max(float(lw[i]) for i in live)
    if not math.isfinite(m):
        return res
    w = {i: math.exp(float(lw[i]) - m) for i in live}
    sw = total([w[i] for i in live])
    for k in sel:
        lg = int(mode[k]) == LOG
        phi = {i: (math.log(float(aux_in[i, k])) if lg else float(aux_in[i, k])) for i in live}
        mean = total([w[i] * phi[i] for i in live]) / sw
        var = total([w[i] * ((phi[i] - mean) * (phi[i] - mean)) for i in live]) / sw
        pstats[2 * k], pstats[2 * k + 1] = mean, var
        wk = float(walk[k])
        if a == 1.0 and wk == 0.0:
            continue
        sd = math.sqrt((1.0 - a * a) * var + (wk * wk) * float(dt))
        sds[k] = sd
        for i in live:
            e = epsilon(seed, key, step, i, k)
            p = ((mean + a * (phi[i] - mean)) if shrinkage else phi[i]) + sd * e
            phi_new[i, k] = p
            out[i, k] = math.exp(p) if lg else p            # (one rounding, to `dtype`, on the store)
    return res

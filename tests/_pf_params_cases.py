"""The inputs of the parameter-move kernel tests (tests/test_pf_params_gpu.py): synthetic clouds, no model, and for each case
the error bound that kernel and restatement (tests/_pf_params_reference.py) may differ by.  Shared with
tests/test_pf_params_host.py, which shows on the restatement alone that another summation order stays inside the bound.

Every payload value is exactly representable in fp32, so one restatement result serves the fp32 and the fp64 run of a case.
Clouds are wide (a relative spread of 0.3), so the variance is well conditioned and the bounds stay far below an fp32 ulp.
  cols     one           one column, log link                       c16   column 16 alone (n_aux = 17), identity link
           all           every column, the links alternating        mix   some columns of either link, the rest carried
  weights  weighted      lw = 0.5 * normal                          zero  lw = 0 everywhere, as after a resampling
  edge     dead          one particle has lw = -inf, another lw = NaN
           patient_dead  every particle of patient 1 is dead (B = 3): its pstats are NaN, its rows untouched
           nonpos        one particle holds 0 and another a negative value in a log-link column: they do not count
  move     walk          a = 1, walk > 0      shrink   a < 1, walk = 0      both   a < 1, walk > 0
           (columns with walk_k = 0 inside a `walk` case are skipped: they keep their bits)

The bound, from the case's own numbers (e = (N + 16) * 2^-52: a sum of N non-negative fp64 terms in any order is within
N * 2^-53 of the exact sum, relatively; the 16 pays for the libm calls and roundings around it; u = 2^-52):
  mean   |sum w phi| carries e * sum w |phi| <= e * sw * max|phi|, sw carries e: 4 e max|phi| absolutely (log's error, u |phi|,
         included);
  var    sum w d^2 carries 2 e V for its own sum and weights; an error t in the mean changes it by t^2 at second order and, through
         the rounding of every d, by at most 2 t E|d| <= 2 t sqrt(V) at first: e (4 V + 8 max|phi| sqrt(V)) + (mean bound)^2 --
         relative to V the conditioning max|phi| / sqrt(V) of a variance computed from unshifted values;
  sd     X = (1 - a^2) V + walk^2 dt carries (1 - a^2) (var bound) + 4 u X; |sqrt x - sqrt y| <= min(sqrt|x - y|, |x - y| / sqrt x);
  eps    Box-Muller through another libm (log, sqrt, cos / sin of the same fp64 arguments, each within 2 ulp): 64 u, the
         radius being at most sqrt(-2 log 2^-33) < 7;
  phi'   2 (mean bound) + 7 (sd bound) + sd * 64 u + 8 u (max|phi| + 7 sd);
  theta' identity link: phi's bound; log link: relative phi's bound + 4 u (exp through another libm).
fp32 data: the bound is far below an fp32 ulp, so the one rounding can differ by one fp32 ulp and no more."""
import functools
import math

import numpy as np

import _pf_params_reference as PR

U = 2.0 ** -52
SCALE = np.array([0.01, 0.05, 1.4, 0.2, 6.0, 0.003, 0.08, 0.5, 0.02, 0.9, 0.004, 11.0, 0.06, 0.3, 0.015, 2.5, 0.07])
MAX_EPS = 7.0


def _list():
    cases = []

    def add(N, B, n_aux, cols, weights="weighted", edge="none", move="both"):
        cases.append(dict(N=N, B=B, n_aux=n_aux, cols=cols, weights=weights, edge=edge, move=move, idx=len(cases)))
    add(1, 1, 1, "one", "zero", "none", "walk")
    add(1, 3, 4, "mix", "weighted", "none", "shrink")
    add(2, 3, 5, "all", "weighted", "none", "both")
    add(2, 1, 17, "c16", "zero", "dead", "walk")
    add(63, 1, 4, "one", "weighted", "dead", "shrink")
    add(63, 3, 17, "all", "zero", "none", "walk")
    add(64, 3, 1, "one", "weighted", "none", "both")
    add(64, 1, 5, "mix", "zero", "nonpos", "shrink")
    add(65, 3, 5, "mix", "weighted", "patient_dead", "both")
    add(65, 1, 17, "c16", "weighted", "none", "shrink")
    add(256, 1, 17, "all", "weighted", "nonpos", "both")
    add(256, 3, 4, "all", "zero", "dead", "shrink")
    add(257, 3, 17, "mix", "weighted", "dead", "walk")
    add(257, 1, 1, "one", "zero", "none", "shrink")
    add(257, 3, 4, "mix", "weighted", "patient_dead", "shrink")
    add(1000, 1, 17, "all", "weighted", "dead", "shrink")
    add(1000, 3, 5, "one", "zero", "nonpos", "both")
    add(1000, 3, 17, "c16", "weighted", "patient_dead", "walk")
    add(4096, 1, 4, "mix", "weighted", "nonpos", "both")
    add(4096, 3, 1, "one", "weighted", "dead", "shrink")
    add(4096, 1, 17, "c16", "zero", "none", "walk")
    return cases


CASES = _list()


def case_id(c):
    return f"{c['idx']}-N{c['N']}-B{c['B']}-aux{c['n_aux']}-{c['cols']}-{c['weights']}-{c['edge']}-{c['move']}"


def f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def _mode(cols, n_aux):
    mode = np.zeros(n_aux, dtype=np.int32)
    if cols == "one":
        mode[min(2, n_aux - 1)] = PR.LOG
    elif cols == "c16":
        mode[16] = PR.IDENTITY
    elif cols == "all":
        mode[:] = [PR.LOG if k % 2 == 0 else PR.IDENTITY for k in range(n_aux)]
    else:
        for k, md in ((0, PR.LOG), (3, PR.IDENTITY), (4, PR.LOG), (7, PR.IDENTITY), (16, PR.LOG)):
            if k < n_aux:
                mode[k] = md
    return mode


@functools.lru_cache(maxsize=None)
def inputs(idx):
    c = CASES[idx]
    N, B, n_aux = c["N"], c["B"], c["n_aux"]
    rng = np.random.default_rng(4100 + idx)
    d = dict(c)
    d["mode"] = mode = _mode(c["cols"], n_aux)
    centre = SCALE[:n_aux] * (1 + 0.1 * rng.standard_normal((B, 1, n_aux)))
    aux = centre * np.exp(0.3 * rng.standard_normal((B, N, n_aux)))
    ident = mode == PR.IDENTITY
    aux[:, :, ident] = (centre * (1 + 0.3 * rng.standard_normal((B, N, n_aux))))[:, :, ident]     # (may be negative: identity link)
    d["aux"] = f32(aux)
    d["lw"] = 0.5 * rng.standard_normal((B, N)) if c["weights"] == "weighted" else np.zeros((B, N))
    d["dt"] = 0.5 + rng.random(B)
    walk = np.zeros(n_aux)
    if c["move"] in ("walk", "both"):
        sel = np.nonzero(mode)[0]
        walk[sel] = 0.05 + 0.1 * rng.random(len(sel))
        walk[ident] *= SCALE[:n_aux][ident]
        if c["move"] == "walk" and len(sel) > 1:
            walk[sel[1]] = 0.0                                         # a selected column that is skipped
    d["walk"] = walk
    d["shrink"] = 1.0 if c["move"] == "walk" else (3 * 0.95 - 1) / (2 * 0.95)
    d["step"] = 3 + idx
    d["seed"] = (0x9E3779B97F4A7C15 * (idx + 5)) & 0xFFFFFFFFFFFFFFFF
    d["id0"] = 7 * idx
    logcols = np.nonzero(mode == PR.LOG)[0]
    if c["edge"] == "dead" and N > 1:
        d["lw"][:, N // 2] = -np.inf
        if N > 2:
            d["lw"][:, 0] = np.nan
    if c["edge"] == "patient_dead":
        d["lw"][1, :] = -np.inf
    if c["edge"] == "nonpos":
        d["aux"][:, N // 3, logcols[0]] = 0.0
        d["aux"][:, N // 5, logcols[-1]] = -d["aux"][:, N // 5, logcols[-1]]
    return d


def restate(d, b, dtype=np.float64, **kw):
    return PR.move(d["lw"][b], d["aux"][b], d["mode"], d["walk"], d["dt"][b], d["shrink"], d["step"], seed=d["seed"], key=d["id0"] + b,
                   dtype=dtype, **kw)


@functools.lru_cache(maxsize=None)
def reference(idx):
    """The restatement's result per patient of case idx (fp64 rows; the fp32 test rounds them)."""
    d = inputs(idx)
    return [restate(d, b) for b in range(d["B"])]


def bounds(d, b, ref):
    """Per column k of patient b: dict(mean=, var=) absolute bounds on pstats, value_abs / value_rel on a moved value (fp64 data).
    From the reference's numbers alone (module docstring)."""
    N, a = d["N"], d["shrink"]
    e = (N + 16) * U
    out = {}
    live = ref["counts"]
    for k in np.nonzero(d["mode"])[0]:
        if not live.any():
            continue
        v = d["aux"][b][live, k]
        phi = np.log(v) if d["mode"][k] == PR.LOG else v
        mx = float(np.abs(phi).max())
        V = float(ref["pstats"][2 * k + 1])
        bm = 4 * e * mx
        bv = e * (4 * V + 8 * mx * math.sqrt(V)) + bm * bm
        o = {"mean": bm, "var": bv}
        sd = ref["sd"][k]
        if np.isfinite(sd):
            X = sd * sd
            dX = (1 - a * a) * bv + 4 * U * X
            dsd = min(math.sqrt(dX), dX / math.sqrt(X)) if X > 0 else math.sqrt(dX)
            bp = 2 * bm + MAX_EPS * dsd + sd * 64 * U + 8 * U * (mx + MAX_EPS * sd)
            o["value_abs"], o["value_rel"] = (0.0, bp + 4 * U) if d["mode"][k] == PR.LOG else (bp, 0.0)
        out[int(k)] = o
    return out

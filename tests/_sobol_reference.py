"""A plain-numpy fp64 restatement of the Sobol estimators that csrc/hode_sobol.hip runs on the GPU (include/hode.h, "Sobol
indices") -- what SALib.analyze.sobol.analyze computes, SALib not being installed.  tests/
test_sobol_indices_host.py checks the restatement on the Ishigami function; tests/test_sobol_indices_gpu.py checks the kernel
against it.

Per output column, with the rows of the design in SALib's block order (A, AB_1..AB_D, [BA_1..BA_D,] B per base sample):
  z = (Y - mean) / std over all rows (ddof 0);  V = var(A u B) (ddof 0);
  S1_j = mean(B (AB_j - A)) / V;  ST_j = mean((A - AB_j)^2) / (2 V);
  S2_jk = mean(BA_j AB_k - A B) / V - S1_j - S1_k for j < k, NaN elsewhere;
  conf = conf_z * std(the same estimates on R resamples of the base samples, ddof 1), NaN for R < 2.
A column that is constant or holds a non-finite value: NaN everywhere, variance 0 or NaN.
Resample r takes base sample (word * N) >> 32 at position q, word = element q & 3 of the Philox block of counter
(q >> 2, 7, r, seed >> 32), key (seed & 0xffffffff, 0)."""
import numpy as np

from _nuts_reference import philox4x32_10

SOBOL_TAG = 7
ISHIGAMI_S1 = np.array([0.3139, 0.4424, 0.0])
ISHIGAMI_ST = np.array([0.5576, 0.4424, 0.2437])
ISHIGAMI_S2_13 = 0.2437


def resample_indices(seed, r, N):
    """rho_r(q), q < N (the Philox rounds run on whole arrays of uint64)."""
    q = np.arange(N, dtype=np.uint64)
    blk = philox4x32_10(q >> np.uint64(2), SOBOL_TAG, r, (seed >> 32) & 0xFFFFFFFF, seed & 0xFFFFFFFF, 0)
    words = np.stack([np.asarray(w, dtype=np.uint64) for w in blk], 1)
    word = words[np.arange(N), (q & np.uint64(3)).astype(np.int64)]
    return ((word * np.uint64(N)) >> np.uint64(32)).astype(np.int64)


def _estimates(A, AB, BA, B, second):
    D = AB.shape[1]
    V = np.var(np.r_[A, B])
    S1 = np.array([np.mean(B * (AB[:, j] - A)) / V for j in range(D)])
    ST = np.array([0.5 * np.mean((A - AB[:, j]) ** 2) / V for j in range(D)])
    S2 = np.full((D, D), np.nan)
    if second:
        for j in range(D):
            for k in range(j + 1, D):
                S2[j, k] = np.mean(BA[:, j] * AB[:, k] - A * B) / V - S1[j] - S1[k]
    return S1, ST, S2


def analyze_column(y, D, second=True, R=100, seed=0, conf_z=1.959963984540054):
    """One column y [N * nb] -> dict S1, ST, S1_conf, ST_conf [D], S2, S2_conf [D, D], variance."""
    y = np.asarray(y, dtype=np.float64)
    nb = 2 * D + 2 if second else D + 2
    N = y.shape[0] // nb
    assert N * nb == y.shape[0] and N >= 1
    nanD, nanDD = np.full(D, np.nan), np.full((D, D), np.nan)
    bad = not np.all(np.isfinite(y))
    if bad or y.max() == y.min():
        return {"S1": nanD, "ST": nanD, "S2": nanDD, "S1_conf": nanD, "ST_conf": nanD, "S2_conf": nanDD,
                "variance": np.nan if bad else 0.0}
    with np.errstate(all="ignore"):
        z = ((y - y.mean()) / y.std()).reshape(N, nb)
        A, AB, B = z[:, 0], z[:, 1:1 + D], z[:, -1]
        BA = z[:, 1 + D:1 + 2 * D] if second else None
        S1, ST, S2 = _estimates(A, AB, BA, B, second)
        out = {"S1": S1, "ST": ST, "S2": S2, "S1_conf": nanD, "ST_conf": nanD, "S2_conf": nanDD, "variance": float(np.var(y))}
        if R >= 2:
            est = []
            for r in range(R):
                rho = resample_indices(seed, r, N)
                est.append(_estimates(A[rho], AB[rho], BA[rho] if second else None, B[rho], second))
            for i, k in enumerate(("S1_conf", "ST_conf", "S2_conf")):
                out[k] = conf_z * np.std(np.stack([e[i] for e in est]), axis=0, ddof=1)
    return out


def analyze(Y, D, second=True, R=100, seed=0, conf_z=1.959963984540054):
    """Y [N * nb, M] -> dict of arrays with a leading M."""
    Y = np.asarray(Y, dtype=np.float64)
    cols = [analyze_column(Y[:, m], D, second, R, seed, conf_z) for m in range(Y.shape[1])]
    return {k: np.stack([np.asarray(c[k]) for c in cols]) for k in cols[0]}


def ishigami(x, a=7.0, b=0.1):
    return np.sin(x[:, 0]) + a * np.sin(x[:, 1]) ** 2 + b * x[:, 2] ** 4 * np.sin(x[:, 0])

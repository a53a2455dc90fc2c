// hode_ukf_linalg.h -- the two pieces of per-wave linear algebra that the unscented filter's step (hode_ukf.hip), its smoother
// (hode_ukf_smooth.hip) and the EM statistics over it (hode_ukf_em.hip) share: the column Cholesky factor with its zero-column
// rule, and the sigma points of a mean and a factor.  Both work on one wave's slice of LDS and end on a workgroup barrier, so
// every wave of the workgroup calls them with the same n.  Contraction is off from here on in the including file: a * b + c below
// is two roundings.  At the end, the two host helpers that size a launch whose waves each own a slice of the dynamic LDS.
#pragma once
#include "hode_chains.h"
#include <cmath>

#pragma clang fp contract(off)

namespace hode {
namespace {

constexpr double kEps = 2.220446049250313e-16;                 // 2^-52

// The lower Cholesky factor L of the n x n matrix A (row-major, both in this wave's LDS), column by column without pivoting; the
// upper triangle of L is written as zeros.  pivot_j = A_jj - sum_{k<j} L_jk^2, the sum from k = 0 in order; a pivot
// <= n 2^-52 |A_jj| gives a zero column.  A non-finite pivot: returns true (L is then arbitrary, but every entry is written).
__device__ __forceinline__ bool ukf_chol(const double *A, double *L, int n, int lane)
{
    bool bad = false;
    for (int j = 0; j < n; ++j) {
        double piv = A[j * n + j];
        for (int k = 0; k < j; ++k) piv -= L[j * n + k] * L[j * n + k];
        const bool finite = __builtin_isfinite(piv);
        bad = bad || !finite;
        const bool zero = !finite || !(piv > (double)n * kEps * fabs(A[j * n + j]));
        const double root = zero ? 1.0 : sqrt(piv);
        for (int i = lane; i < n; i += 64) {
            double t = 0.0;
            if (i == j && !zero) t = root;
            if (i > j && !zero) {
                t = A[i * n + j];
                for (int k = 0; k < j; ++k) t -= L[i * n + k] * L[j * n + k];
                t = t / root;
            }
            L[i * n + j] = t;
        }
        __syncthreads();
    }
    return bad;
}

// Z [K][n] <- the sigma points of (M, L): row 0 the mean, rows 1..n the mean + gamma * column, rows n+1..2n the mean - it
__device__ __forceinline__ void ukf_draw(double *Z, const double *M, const double *L, int n, double gamma, int lane)
{
    const int K = 2 * n + 1;
    for (int e = lane; e < K * n; e += 64) {
        const int k = e / n, j = e - k * n;
        double v = M[j];
        if (k >= 1 && k <= n) v = v + gamma * L[j * n + (k - 1)];
        else if (k > n) v = v - gamma * L[j * n + (k - n - 1)];
        Z[e] = v;
    }
    __syncthreads();
}

// ---- launching a kernel whose waves each own a slice of the dynamic LDS (the smoother, the EM statistics)
constexpr size_t kCuLds = 160 * 1024;                           // the LDS of a gfx950 CU: what a workgroup may ask for

// the waves of a workgroup whose slices of `doubles` doubles stay inside a CU's LDS
inline int waves_for(int doubles)
{
    const size_t fit = kCuLds / ((size_t)doubles * sizeof(double));
    return fit >= (size_t)(kThreads / 64) ? kThreads / 64 : fit < 1 ? 1 : (int)fit;
}

// (more than 64 KiB of dynamic LDS has to be asked for)
template <typename F> bool lds_ok(F *kernel, size_t bytes)
{
    if (bytes <= 64 * 1024) return true;
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) == hipSuccess)
        return true;
    (void)hipGetLastError();
    return false;
}

}  // namespace
}  // namespace hode

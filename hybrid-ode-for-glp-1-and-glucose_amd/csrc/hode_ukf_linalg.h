// hode_ukf_linalg.h -- the two pieces of per-wave linear algebra that the unscented filter's step (hode_ukf.hip) and its
// smoother (hode_ukf_smooth.hip) share: the column Cholesky factor with its zero-column rule, and the sigma points of a mean and a
// factor.  Both work on one wave's slice of LDS and end on a workgroup barrier, so every wave of the workgroup calls them with
// the same n.  Contraction is off from here on in the including file: a * b + c below is two roundings.
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

}  // namespace
}  // namespace hode

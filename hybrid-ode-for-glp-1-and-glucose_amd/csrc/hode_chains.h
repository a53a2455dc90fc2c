// hode_chains.h -- helpers shared by the per-chain sampler passes (hode_hmc.hip, hode_nuts.hip): one workgroup of kThreads
// lanes per chain, rows of `ld` reals moved four at a time, chain reductions in a fixed order (a butterfly inside each wave,
// then the four wave sums in order), Stan's dual averaging.
#pragma once
#include "hode_kernels.h"

namespace hode {
namespace {

constexpr int kThreads = 256;

__device__ __forceinline__ double block_sum(double v, double *sh)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    const double r = (sh[0] + sh[1]) + (sh[2] + sh[3]);
    __syncthreads();
    return r;
}

// two chain sums at once (sh: 8 doubles), each in the order of block_sum
__device__ __forceinline__ void block_sum2(double &a, double &b, double *sh)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_xor(a, o, 64);
        b += __shfl_xor(b, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        sh[threadIdx.x >> 6] = a;
        sh[4 + (threadIdx.x >> 6)] = b;
    }
    __syncthreads();
    a = (sh[0] + sh[1]) + (sh[2] + sh[3]);
    b = (sh[4] + sh[5]) + (sh[6] + sh[7]);
    __syncthreads();
}

// six chain sums at once (sh: 24 doubles), each in the order of block_sum: the per-state sums of hode_obs.hip
__device__ __forceinline__ void block_sum6(double (&v)[6], double *sh)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int k = 0; k < 6; ++k) v[k] += __shfl_xor(v[k], o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) sh[4 * k + (threadIdx.x >> 6)] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 6; ++k) v[k] = (sh[4 * k] + sh[4 * k + 1]) + (sh[4 * k + 2] + sh[4 * k + 3]);
    __syncthreads();
}

__device__ __forceinline__ int block_or(int v, int *sh)
{
    v = __any(v != 0) ? 1 : 0;
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    const int r = sh[0] | sh[1] | sh[2] | sh[3];
    __syncthreads();
    return r;
}

// four consecutive reals: one 16-byte access (fp32) / two (fp64) when `vec`, else up to `n` scalars (nothing past the row)
template <typename R> __device__ __forceinline__ void ld4(const R *p, bool vec, int n, R (&o)[4])
{
    if (vec) {
        if constexpr (sizeof(R) == 4) {
            const float4 a = *reinterpret_cast<const float4 *>(p);
            o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w;
        } else {
            const double2 a = reinterpret_cast<const double2 *>(p)[0], b = reinterpret_cast<const double2 *>(p)[1];
            o[0] = a.x; o[1] = a.y; o[2] = b.x; o[3] = b.y;
        }
        return;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = k < n ? p[k] : R(0);
}

template <typename R> __device__ __forceinline__ void st4(R *p, bool vec, int n, const R (&o)[4])
{
    if (vec) {
        if constexpr (sizeof(R) == 4) {
            *reinterpret_cast<float4 *>(p) = make_float4(o[0], o[1], o[2], o[3]);
        } else {
            reinterpret_cast<double2 *>(p)[0] = make_double2(o[0], o[1]);
            reinterpret_cast<double2 *>(p)[1] = make_double2(o[2], o[3]);
        }
        return;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (k < n) p[k] = o[k];
}

// ODE index of sampled coordinate d (< n_ode): the d-th set bit of the mask
__device__ __forceinline__ int ode_index(uint32_t mask, int d)
{
    for (int k = 0; k < 17; ++k)
        if ((mask >> k) & 1u) {
            if (d == 0) return k;
            --d;
        }
    return 0;
}

// one dual-averaging update of a chain's step size towards acceptance `delta` (Hoffman & Gelman 2014, Stan's constants
// gamma 0.05, t0 10, kappa 0.75).  st: {mu, log eps bar, H bar, t}; a: this iteration's acceptance statistic
__device__ __forceinline__ void dual_average(double *st, double delta, double a, double *log_eps)
{
    const double t = st[3] + 1.0, eta = 1.0 / (t + 10.0);
    st[2] = (1.0 - eta) * st[2] + eta * (delta - a);
    const double le = st[0] - sqrt(t) / 0.05 * st[2];
    const double w = pow(t, -0.75);
    st[1] = w * le + (1.0 - w) * st[1];
    st[3] = t;
    *log_eps = le;
}

template <typename R> bool rows_vec(int ld, std::initializer_list<const void *> ptrs)
{
    if (ld % 4) return false;
    for (const void *p : ptrs)
        if (p && ((uintptr_t)p & 15)) return false;
    return true;
}

inline int done() { return hipGetLastError() == hipSuccess ? HODE_OK : HODE_ELAUNCH; }

}  // namespace
}  // namespace hode

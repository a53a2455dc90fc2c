// hode_population.hip -- the hierarchical population layer between the samplers' chain coordinates and the solve's per-set
// constants (inference/population.py; include/hode.h, "Population model").
//
// A row of chain coordinates holds D = K (B + 2) values with an N(0, 1) prior each,
//     [ m_0..m_{K-1} | s_0..s_{K-1} | z_{0,0}..z_{0,K-1} | ... | z_{B-1,K-1} ],
// k in ascending ODE-index order (the set bits of ode_mask, as in hode_hmc.hip).  The map (pop_params) is
//     mu_pop_k = mu0_k + sd0_k m_k,  tau_k = tau0_k exp(omega s_k),  theta_{b,k} = mu_pop_k + tau_k z_{b,k}
// into ode_p[A * B][17], one parameter set per (row, patient); its transpose (pop_grad) takes the adjoint's per-set gode to
// the likelihood gradient of the row.  Both compute in double and round once to R.  They are memory-bound over A x B x 17
// values; pop_grad is one workgroup per row with its sums in block_sum's fixed order: no floating-point atomics, the same
// call gives the same bits, and a row's result depends on nothing but that row.
#include "hode_chains.h"

namespace hode {
namespace {

constexpr int kOde = 17;

// mu_pop_k and tau_k of the row into LDS (hyp[k], hyp[kOde + k]) and the ODE index of coordinate k (idx[k]), k < K
template <typename R>
__device__ __forceinline__ void row_hyper(const R *__restrict__ row, int K, uint32_t ode_mask, const double *__restrict__ mu0,
                                          const double *__restrict__ sd0, const double *__restrict__ tau0, double omega, double *hyp,
                                          int *idx)
{
    const int k = threadIdx.x;
    if (k < K) {
        hyp[k] = mu0 ? mu0[k] + sd0[k] * (double)row[k] : 0.0;
        hyp[kOde + k] = tau0[k] * exp(omega * (double)row[K + k]);
        idx[k] = ode_index(ode_mask, k);
    }
    __syncthreads();
}

// ---------------------------------------------------------------- coords -> ode_p: grid (row, tile of 4 * kThreads entries)
template <typename R>
__global__ __launch_bounds__(kThreads) void pop_params_kernel(int B, int K, int ld, bool vec, const R *__restrict__ coords,
                                                              uint32_t ode_mask, const double *__restrict__ mu0,
                                                              const double *__restrict__ sd0, const double *__restrict__ tau0,
                                                              double omega, const R *__restrict__ ode_base, R *__restrict__ ode_p)
{
    __shared__ double hyp[2 * kOde];
    __shared__ int idx[kOde];
    const int a = blockIdx.x;
    const R *row = coords + (int64_t)a * ld;
    row_hyper(row, K, ode_mask, mu0, sd0, tau0, omega, hyp, idx);
    const int64_t len = (int64_t)B * kOde;                       // the row's entries of ode_p: patient b, constant j at b * 17 + j
    const int64_t e0 = 4 * ((int64_t)blockIdx.y * kThreads + threadIdx.x);
    if (e0 >= len) return;
    const int n = len - e0 < 4 ? (int)(len - e0) : 4;
    R out[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        out[q] = R(0);
        if (q < n) {
            const int64_t e = e0 + q;
            const int b = (int)(e / kOde), j = (int)(e % kOde);
            if ((ode_mask >> j) & 1u) {
                const int k = __popc(ode_mask & ((1u << j) - 1u));
                out[q] = (R)(hyp[k] + hyp[kOde + k] * (double)row[2 * K + (int64_t)b * K + k]);
            } else {
                out[q] = ode_base[j];
            }
        }
    }
    st4(ode_p + (int64_t)a * len + e0, vec, n, out);
}

// ---------------------------------------------------------------- gode -> likelihood gradient of the row: one workgroup per row
template <typename R>
__global__ __launch_bounds__(kThreads) void pop_grad_kernel(int B, int K, int ld, const R *__restrict__ coords,
                                                            const R *__restrict__ gode, uint32_t ode_mask,
                                                            const double *__restrict__ sd0, const double *__restrict__ tau0,
                                                            double omega, R *__restrict__ glik)
{
    __shared__ double hyp[2 * kOde];
    __shared__ int idx[kOde];
    __shared__ double sh[24];
    __shared__ double red[36];
    const int a = blockIdx.x;
    const R *row = coords + (int64_t)a * ld;
    R *out = glik + (int64_t)a * ld;
    row_hyper(row, K, ode_mask, (const double *)nullptr, sd0, tau0, omega, hyp, idx);
    double acc[36];                                              // acc[2 k] = sum_b G_bk, acc[2 k + 1] = sum_b G_bk z_bk
#pragma unroll
    for (int i = 0; i < 36; ++i) acc[i] = 0.0;
    for (int b = threadIdx.x; b < B; b += kThreads) {            // patients t, t + 256, ... in ascending order
        const R *G = gode + ((int64_t)a * B + b) * kOde;
        const int64_t zo = 2 * K + (int64_t)b * K;
#pragma unroll
        for (int k = 0; k < kOde; ++k) {
            if (k < K) {
                const double g = (double)G[idx[k]], z = (double)row[zo + k];
                acc[2 * k] += g;
                acc[2 * k + 1] += g * z;
                out[zo + k] = (R)(hyp[kOde + k] * g);
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 6; ++q) {                                // the 2 K sums, six at a time, each in block_sum's order
        if (6 * q < 2 * K) {
            double v[6];
#pragma unroll
            for (int i = 0; i < 6; ++i) v[i] = acc[6 * q + i];
            block_sum6(v, sh);
            if (threadIdx.x == 0) {
#pragma unroll
                for (int i = 0; i < 6; ++i) red[6 * q + i] = v[i];
            }
        }
    }
    __syncthreads();
    const int k = threadIdx.x;
    if (k < K) {
        out[k] = (R)(sd0[k] * red[2 * k]);
        out[K + k] = (R)(omega * hyp[kOde + k] * red[2 * k + 1]);
    }
    for (int d = K * (B + 2) + threadIdx.x; d < ld; d += kThreads) out[d] = R(0);
}

}  // namespace

template <typename R> int launch_pop_params(hipStream_t s, int A, int B, int K, int ld, const R *coords, uint32_t ode_mask, const double *mu0,
                                            const double *sd0, const double *tau0, double tau_log_sd, const R *ode_base, R *ode_p)
{
    const int64_t len = (int64_t)B * kOde;
    const bool vec = len % 4 == 0 && ((uintptr_t)ode_p & 15) == 0;
    const unsigned tiles = (unsigned)((len + 4 * kThreads - 1) / (4 * kThreads));
    hipLaunchKernelGGL(pop_params_kernel<R>, dim3(A, tiles), dim3(kThreads), 0, s, B, K, ld, vec, coords, ode_mask, mu0, sd0, tau0,
                       tau_log_sd, ode_base, ode_p);
    return done();
}

template <typename R> int launch_pop_grad(hipStream_t s, int A, int B, int K, int ld, const R *coords, const R *gode, uint32_t ode_mask,
                                          const double *sd0, const double *tau0, double tau_log_sd, R *glik)
{
    hipLaunchKernelGGL(pop_grad_kernel<R>, dim3(A), dim3(kThreads), 0, s, B, K, ld, coords, gode, ode_mask, sd0, tau0, tau_log_sd, glik);
    return done();
}

#define HODE_POP_INST(R)                                                                                                          \
    template int launch_pop_params<R>(hipStream_t, int, int, int, int, const R *, uint32_t, const double *, const double *,       \
                                      const double *, double, const R *, R *);                                                    \
    template int launch_pop_grad<R>(hipStream_t, int, int, int, int, const R *, const R *, uint32_t, const double *,             \
                                    const double *, double, R *);
HODE_POP_INST(float)
HODE_POP_INST(double)

}  // namespace hode

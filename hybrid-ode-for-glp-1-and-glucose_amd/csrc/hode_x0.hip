// hode_x0.hip -- the initial-state layer between the samplers' chain coordinates and the solve's per-trajectory initial states
// (inference/initial_state.py; include/hode.h, "Initial-state model").
//
// A row of chain coordinates holds, from column `off`, B n_lat values w_{b,i} with an N(0, 1) prior each, patient-major, i over
// the latent states (the set bits of lat_mask, ascending).  The map (x0_params) is
//     x0_{b,j} = m_{b,j} + s_{b,j} w_{b,rank(j)}            (link 0)
//     x0_{b,j} = m_{b,j} exp(s_{b,j} w_{b,rank(j)})         (link 1)
// for the latent j and x0_base[b][j] for the others, into x0_out[A * B][6]; optionally the global constants of the row
// (theta_k = mu_k + sd_k coords[k], k < K) into ode_p[A][17].  Its transpose (x0_grad) takes the adjoint's per-trajectory gx0
// (and per-row gode) to the likelihood gradient of the row.  Both compute in double and round once to R.  There is no sum:
// one lane per entry, grid (row, tile of kThreads entries), scalar accesses only (a row of x0 is 24 or 48 bytes and `off` is
// arbitrary, so nothing is assumed about alignment); the same call gives the same bits.
#include "hode_chains.h"

namespace hode {
namespace {

constexpr int kOde = 17;
constexpr int kState = 6;

// the r-th set bit of a mask over the six states
__device__ __forceinline__ int state_index(uint32_t mask, int r)
{
    for (int j = 0; j < kState; ++j)
        if ((mask >> j) & 1u) {
            if (r == 0) return j;
            --r;
        }
    return 0;
}

__device__ __forceinline__ double link_value(int link, double m, double s, double w) { return link ? m * exp(s * w) : m + s * w; }

// ---------------------------------------------------------------- coords -> x0_out (and ode_p): entries 0..6 B-1 are x0, then 17 of ode_p
template <typename R>
__global__ __launch_bounds__(kThreads) void x0_params_kernel(int B, int n_lat, int ld, int off, const R *__restrict__ coords,
                                                             uint32_t lat_mask, int link, const double *__restrict__ m,
                                                             const double *__restrict__ s, const R *__restrict__ x0_base,
                                                             R *__restrict__ x0_out, uint32_t ode_mask,
                                                             const double *__restrict__ mu, const double *__restrict__ sd,
                                                             const R *__restrict__ ode_base, R *__restrict__ ode_p)
{
    const int a = blockIdx.x;
    const R *row = coords + (int64_t)a * ld;
    const int64_t nx = (int64_t)B * kState;
    const int64_t e = (int64_t)blockIdx.y * kThreads + threadIdx.x;
    if (e < nx) {
        const int64_t b = e / kState;
        const int j = (int)(e % kState);
        R v;
        if ((lat_mask >> j) & 1u) {
            const int r = __popc(lat_mask & ((1u << j) - 1u));
            v = (R)link_value(link, m[e], s[e], (double)row[off + b * n_lat + r]);
        } else {
            v = x0_base[e];
        }
        x0_out[(int64_t)a * nx + e] = v;
    } else if (ode_p && e < nx + kOde) {
        const int j = (int)(e - nx);
        R v;
        if ((ode_mask >> j) & 1u) {
            const int k = __popc(ode_mask & ((1u << j) - 1u));
            v = (R)(mu[k] + sd[k] * (double)row[k]);
        } else {
            v = ode_base[j];
        }
        ode_p[(int64_t)a * kOde + j] = v;
    }
}

// ---------------------------------------------------------------- gx0 (and gode) -> glik: entries 0..B n_lat-1 are w, then K constants
template <typename R>
__global__ __launch_bounds__(kThreads) void x0_grad_kernel(int B, int n_lat, int ld, int off, const R *__restrict__ coords,
                                                           uint32_t lat_mask, int link, const double *__restrict__ m,
                                                           const double *__restrict__ s, const R *__restrict__ gx0, int K,
                                                           uint32_t ode_mask, const double *__restrict__ sd,
                                                           const R *__restrict__ gode, R *__restrict__ glik)
{
    const int a = blockIdx.x;
    const R *row = coords + (int64_t)a * ld;
    R *out = glik + (int64_t)a * ld;
    const int64_t nw = (int64_t)B * n_lat;
    const int64_t e = (int64_t)blockIdx.y * kThreads + threadIdx.x;
    if (e < nw) {
        const int64_t b = e / n_lat;
        const int j = state_index(lat_mask, (int)(e % n_lat));
        const int64_t q = b * kState + j;
        const double sj = s[q];
        const double d = link ? sj * link_value(1, m[q], sj, (double)row[off + e]) : sj;
        out[off + e] = (R)((double)gx0[((int64_t)a * B) * kState + q] * d);
    } else if (gode && e < nw + K) {
        const int k = (int)(e - nw);
        out[k] = (R)(sd[k] * (double)gode[(int64_t)a * kOde + ode_index(ode_mask, k)]);
    }
}

inline unsigned tiles_of(int64_t n) { return (unsigned)((n + kThreads - 1) / kThreads); }

}  // namespace

template <typename R> int launch_x0_params(hipStream_t st, int A, int B, int n_lat, int ld, int off, const R *coords, uint32_t lat_mask,
                                           int link, const double *m, const double *s, const R *x0_base, R *x0_out, uint32_t ode_mask,
                                           const double *mu, const double *sd, const R *ode_base, R *ode_p)
{
    const int64_t n = (int64_t)B * kState + (ode_p ? kOde : 0);
    hipLaunchKernelGGL(x0_params_kernel<R>, dim3(A, tiles_of(n)), dim3(kThreads), 0, st, B, n_lat, ld, off, coords, lat_mask, link, m, s,
                       x0_base, x0_out, ode_mask, mu, sd, ode_base, ode_p);
    return done();
}

template <typename R> int launch_x0_grad(hipStream_t st, int A, int B, int n_lat, int ld, int off, const R *coords, uint32_t lat_mask,
                                         int link, const double *m, const double *s, const R *gx0, int K, uint32_t ode_mask,
                                         const double *sd, const R *gode, R *glik)
{
    const int64_t n = (int64_t)B * n_lat + (gode ? K : 0);
    hipLaunchKernelGGL(x0_grad_kernel<R>, dim3(A, tiles_of(n)), dim3(kThreads), 0, st, B, n_lat, ld, off, coords, lat_mask, link, m, s,
                       gx0, K, ode_mask, sd, gode, glik);
    return done();
}

#define HODE_X0_INST(R)                                                                                                           \
    template int launch_x0_params<R>(hipStream_t, int, int, int, int, int, const R *, uint32_t, int, const double *, const double *, \
                                     const R *, R *, uint32_t, const double *, const double *, const R *, R *);                   \
    template int launch_x0_grad<R>(hipStream_t, int, int, int, int, int, const R *, uint32_t, int, const double *, const double *,  \
                                   const R *, int, uint32_t, const double *, const R *, R *);
HODE_X0_INST(float)
HODE_X0_INST(double)

}  // namespace hode

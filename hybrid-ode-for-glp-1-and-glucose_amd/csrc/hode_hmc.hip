// hode_hmc.hip -- the per-chain passes of multi-chain HMC (inference/hmc.py; include/hode.h, "MCMC").
//
// C chains of D coordinates each, row-major [C][ld] (ld >= D; ld % 4 == 0 with 16-byte aligned rows lets every lane move
// four coordinates per 16-byte load).  Every kernel is memory-bound over C x D values.  Chain reductions (kinetic energy,
// |z|^2, failed solves) are one workgroup per chain, in a fixed order: a butterfly inside each wave, then the four wave sums
// in order.  There are no floating-point atomics anywhere in this file: the same call gives the same bits.
//
// Coordinates (z): d < n_ode are the sampled mechanistic constants, in ascending ODE-index order (the set bits of ode_mask),
// theta = mu + sd z; the next P coordinates (sample_nn) are the MLP weights themselves, theta = z.
#include "hode_chains.h"
#include "hode_philox.h"

namespace hode {
namespace {

// ---------------------------------------------------------------- per-set sum of squares + cotangent
template <typename R, bool VEC>
__global__ __launch_bounds__(kThreads) void mse_sets_kernel(int64_t len, const R *__restrict__ y, const R *__restrict__ obs,
                                                            R scale, double *__restrict__ loss_sum, R *__restrict__ gy)
{
    __shared__ double sh[4];
    const int s = blockIdx.x;
    const R *ys = y + (int64_t)s * len;
    R *gs = gy ? gy + (int64_t)s * len : nullptr;
    double acc = 0.0;
    const R two = R(2) * scale;
    if (VEC) {
        for (int64_t i = 4 * (int64_t)threadIdx.x; i < len; i += 4 * kThreads) {
            R a[4], b[4], g[4];
            ld4(ys + i, true, 4, a);
            ld4(obs + i, true, 4, b);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const R d = a[k] - b[k];
                acc += (double)d * (double)d;
                g[k] = two * d;
            }
            if (gs) st4(gs + i, true, 4, g);
        }
    } else {
        for (int64_t i = threadIdx.x; i < len; i += kThreads) {
            const R d = ys[i] - obs[i];
            acc += (double)d * (double)d;
            if (gs) gs[i] = two * d;
        }
    }
    acc = block_sum(acc, sh);
    if (threadIdx.x == 0) loss_sum[s] += acc;
}

// ---------------------------------------------------------------- momentum refresh + trajectory start
template <typename R>
__global__ __launch_bounds__(kThreads) void refresh_kernel(int D, int ld, bool vec, uint64_t seed, uint32_t iter, double jitter,
                                                           const R *__restrict__ minv, const double *__restrict__ log_eps,
                                                           const R *__restrict__ z, const R *__restrict__ g,
                                                           const double *__restrict__ U, R *__restrict__ p, R *__restrict__ z0,
                                                           R *__restrict__ g0, double *__restrict__ U0, double *__restrict__ ke0,
                                                           double *__restrict__ eps, int32_t *__restrict__ failed)
{
    __shared__ double sh[4];
    const int c = blockIdx.x;
    const int64_t row = (int64_t)c * ld;
    double ke = 0.0;
    for (int d0 = 4 * threadIdx.x; d0 < D; d0 += 4 * kThreads) {
        const int n = D - d0 < 4 ? D - d0 : 4;
        R mi[4], zz[4], gg[4], pp[4];
        ld4(minv + d0, vec, n, mi);
        ld4(z + row + d0, vec, n, zz);
        ld4(g + row + d0, vec, n, gg);
        double xi[4];
        normals4(hmc_rng(seed, (uint32_t)c, iter, kRngMomentum, (uint32_t)(d0 >> 2)), xi);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double m = k < n ? (double)mi[k] : 1.0;
            pp[k] = k < n ? (R)(xi[k] / sqrt(m)) : R(0);          // p = M^{1/2} xi, M = diag(1 / minv)
            ke += (double)pp[k] * (double)pp[k] * m;
        }
        st4(p + row + d0, vec, n, pp);
        st4(z0 + row + d0, vec, n, zz);
        st4(g0 + row + d0, vec, n, gg);
    }
    ke = block_sum(ke, sh);
    if (threadIdx.x == 0) {
        ke0[c] = 0.5 * ke;
        U0[c] = U[c];
        const Philox4 r = hmc_rng(seed, (uint32_t)c, iter, kRngJitter, 0);
        eps[c] = exp(log_eps[c]) * (1.0 + jitter * (2.0 * u01(r.x) - 1.0));
        failed[c] = 0;
    }
}

// ---------------------------------------------------------------- gradient assembly, kick, drift, parameters of the next solve
template <typename R>
__global__ __launch_bounds__(kThreads) void leapfrog_kernel(int D, int ld, bool vec, int flags, double kick, const double *__restrict__ eps,
                                                            const R *__restrict__ minv, R *__restrict__ z, R *__restrict__ p,
                                                            R *__restrict__ g, const R *__restrict__ gnn, const R *__restrict__ gode,
                                                            int P, const double *__restrict__ loss_sum, double lik_scale,
                                                            const int32_t *__restrict__ status, int n_traj, double *__restrict__ U,
                                                            double *__restrict__ ke_out, int32_t *__restrict__ failed, uint32_t ode_mask,
                                                            int n_ode, const double *__restrict__ mu, const double *__restrict__ sd,
                                                            int sample_nn, R *__restrict__ nn_p, R *__restrict__ ode_p)
{
    __shared__ double sh[4];
    __shared__ int shi[4];
    const int c = blockIdx.x;
    const int64_t row = (int64_t)c * ld;
    const bool assemble = flags & HODE_HMC_ASSEMBLE, do_kick = flags & HODE_HMC_KICK, drift = flags & HODE_HMC_DRIFT;
    const bool want_ke = flags & HODE_HMC_KE, params = (flags & (HODE_HMC_DRIFT | HODE_HMC_PARAMS)) != 0;
    const double e = eps[c];
    const R ek = (R)(kick * e), ed = (R)e;
    double zz2 = 0.0, ke = 0.0;
    for (int d0 = 4 * threadIdx.x; d0 < D; d0 += 4 * kThreads) {
        const int n = D - d0 < 4 ? D - d0 : 4;
        R zz[4], gg[4], pp[4], mi[4];
        ld4(z + row + d0, vec, n, zz);
        if (assemble) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int d = d0 + k;
                R lik = R(0);
                if (k < n) {
                    if (d < n_ode) {
                        if (gode) lik = gode[(int64_t)c * 17 + ode_index(ode_mask, d)] * (R)sd[d];
                    } else if (gnn) {
                        lik = gnn[(int64_t)c * P + (d - n_ode)];
                    }
                }
                gg[k] = k < n ? lik + zz[k] : R(0);                    // grad U = grad (likelihood) + z (N(0, 1) prior)
                if (k < n) zz2 += (double)zz[k] * (double)zz[k];
            }
            st4(g + row + d0, vec, n, gg);
        } else {
            ld4(g + row + d0, vec, n, gg);
        }
        if (do_kick || drift || want_ke) {
            ld4(p + row + d0, vec, n, pp);
            ld4(minv + d0, vec, n, mi);
            if (do_kick) {
#pragma unroll
                for (int k = 0; k < 4; ++k) pp[k] -= ek * gg[k];
                st4(p + row + d0, vec, n, pp);
            }
            if (want_ke) {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (k < n) ke += (double)pp[k] * (double)pp[k] * (double)mi[k];
            }
            if (drift) {
#pragma unroll
                for (int k = 0; k < 4; ++k) zz[k] += ed * mi[k] * pp[k];
                st4(z + row + d0, vec, n, zz);
            }
        }
        if (params) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int d = d0 + k;
                if (k < n) {
                    if (d < n_ode) ode_p[(int64_t)c * 17 + ode_index(ode_mask, d)] = (R)(mu[d] + sd[d] * (double)zz[k]);
                    else if (sample_nn) nn_p[(int64_t)c * P + (d - n_ode)] = zz[k];
                }
            }
        }
    }
    if (assemble) {
        int bad = 0;
        if (status)
            for (int b = threadIdx.x; b < n_traj; b += kThreads) bad |= status[(int64_t)c * n_traj + b] != 0;
        bad = block_or(bad, shi);
        zz2 = block_sum(zz2, sh);
        if (threadIdx.x == 0) {
            U[c] = (loss_sum ? lik_scale * loss_sum[c] : 0.0) + 0.5 * zz2;
            if (bad) failed[c] = 1;
        }
    }
    if (want_ke) {
        ke = block_sum(ke, sh);
        if (threadIdx.x == 0) ke_out[c] = 0.5 * ke;
    }
}

// ---------------------------------------------------------------- Metropolis test, dual averaging, draws
template <typename R>
__global__ __launch_bounds__(kThreads) void accept_kernel(int D, int ld, bool vec, int mode, uint64_t seed, uint32_t iter, double delta,
                                                          R *__restrict__ z, const R *__restrict__ z0, R *__restrict__ g,
                                                          const R *__restrict__ g0, double *__restrict__ U, const double *__restrict__ U0,
                                                          const double *__restrict__ ke0, const double *__restrict__ ke,
                                                          const int32_t *__restrict__ failed, double *__restrict__ log_eps,
                                                          double *__restrict__ da, int32_t *__restrict__ search, int n_ode,
                                                          const double *__restrict__ mu, const double *__restrict__ sd,
                                                          R *__restrict__ draws, double *__restrict__ stats, int n_slots, int slot)
{
    __shared__ int keep_sh;
    const int c = blockIdx.x;
    const int64_t row = (int64_t)c * ld;
    double *st = da + 4 * (int64_t)c;                        // {mu, log eps bar, H bar, t}
    if (mode == HODE_HMC_DA_RESTART || mode == HODE_HMC_DA_FINISH) {
        if (threadIdx.x == 0) {
            if (mode == HODE_HMC_DA_RESTART) {
                st[0] = log(10.0) + log_eps[c];
                st[1] = 0.0; st[2] = 0.0; st[3] = 0.0;
                search[2 * c] = 0; search[2 * c + 1] = 0;
            } else if (st[3] > 0) {
                log_eps[c] = st[1];
            }
        }
        return;
    }
    if (threadIdx.x == 0) {
        const double H0 = U0[c] + ke0[c], H1 = U[c] + ke[c];
        const bool fail = failed[c] != 0;
        const double dH = H1 - H0;
        int keep = 0;                                        // 1: the proposal replaces the state
        if (mode == HODE_HMC_SEARCH) {
            // Stan's initial step size heuristic, per chain: double / halve until the one-step acceptance crosses 0.8
            const double lw = (fail || !isfinite(dH)) ? -INFINITY : -dH;  // log acceptance weight of one leapfrog step
            int dir = search[2 * c];
            if (!search[2 * c + 1]) {
                if (dir == 0) dir = search[2 * c] = lw > log(0.8) ? 1 : -1;
                if ((dir == 1 && !(lw > log(0.8))) || (dir == -1 && !(lw < log(0.8)))) search[2 * c + 1] = 1;
                else log_eps[c] += dir * log(2.0);
            }
        } else {
            const bool div = fail || !isfinite(H1) || dH > 1000.0;
            const double a = div ? 0.0 : (dH <= 0 ? 1.0 : exp(-dH));
            const double u = u01(hmc_rng(seed, (uint32_t)c, iter, kRngAccept, 0).x);
            keep = !div && u < a;
            if (mode == HODE_HMC_ADAPT) dual_average(st, delta, a, &log_eps[c]);
            if (slot >= 0) {
                double *s = stats + ((int64_t)c * n_slots + slot) * 4;
                s[0] = a;
                s[1] = -(keep ? U[c] : U0[c]);
                s[2] = div ? 1.0 : 0.0;
                s[3] = fail ? 1.0 : 0.0;
            }
        }
        if (!keep) U[c] = U0[c];
        keep_sh = keep;
    }
    __syncthreads();
    const bool keep = keep_sh != 0;
    for (int d0 = 4 * threadIdx.x; d0 < D; d0 += 4 * kThreads) {
        const int n = D - d0 < 4 ? D - d0 : 4;
        R zz[4];
        if (!keep) {
            R gg[4];
            ld4(z0 + row + d0, vec, n, zz);
            ld4(g0 + row + d0, vec, n, gg);
            st4(z + row + d0, vec, n, zz);
            st4(g + row + d0, vec, n, gg);
        } else if (draws && slot >= 0) {
            ld4(z + row + d0, vec, n, zz);
        }
        if (draws && slot >= 0 && mode != HODE_HMC_SEARCH) {
            R *dr = draws + ((int64_t)c * n_slots + slot) * D;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int d = d0 + k;
                if (k < n) dr[d] = d < n_ode ? (R)(mu[d] + sd[d] * (double)zz[k]) : zz[k];
            }
        }
    }
}

// ---------------------------------------------------------------- pooled cross-chain variance (mass matrix)
template <typename R>
__global__ __launch_bounds__(64) void welford_kernel(int C, int D, int ld, int flags, const R *__restrict__ z, double *__restrict__ wf,
                                                     R *__restrict__ minv)
{
    const int d = blockIdx.x * 64 + threadIdx.x;
    if (d >= D) return;
    double n = wf[d], m = wf[D + d], m2 = wf[2 * D + d];
    if (flags & HODE_HMC_WELFORD_ACCUM) {
        for (int c = 0; c < C; ++c) {                        // chains in order: a fixed summation order
            const double x = (double)z[(int64_t)c * ld + d];
            n += 1.0;
            const double dl = x - m;
            m += dl / n;
            m2 += dl * (x - m);
        }
    }
    if (flags & HODE_HMC_WELFORD_FINISH) {
        if (n > 1.0) {
            const double var = m2 / (n - 1.0);
            minv[d] = (R)((n / (n + 5.0)) * var + 1e-3 * (5.0 / (n + 5.0)));   // Stan's regularisation
        }
        n = 0.0; m = 0.0; m2 = 0.0;
    }
    wf[d] = n; wf[D + d] = m; wf[2 * D + d] = m2;
}


}  // namespace

template <typename R> int launch_mse_sets(hipStream_t s, int n_sets, int64_t len, const R *y, const R *obs, R scale, double *loss_sum, R *gy)
{
    const bool vec = len % 4 == 0 && ((((uintptr_t)y | (uintptr_t)obs | (uintptr_t)gy) & 15) == 0);
    if (vec) hipLaunchKernelGGL((mse_sets_kernel<R, true>), dim3(n_sets), dim3(kThreads), 0, s, len, y, obs, scale, loss_sum, gy);
    else hipLaunchKernelGGL((mse_sets_kernel<R, false>), dim3(n_sets), dim3(kThreads), 0, s, len, y, obs, scale, loss_sum, gy);
    return done();
}

template <typename R> int launch_hmc_refresh(hipStream_t s, const HmcRefreshArgs<R> &a)
{
    const bool vec = rows_vec<R>(a.ld, {a.minv, a.z, a.g, a.p, a.z0, a.g0});
    hipLaunchKernelGGL(refresh_kernel<R>, dim3(a.C), dim3(kThreads), 0, s, a.D, a.ld, vec, a.seed, a.iter, a.jitter, a.minv, a.log_eps,
                       a.z, a.g, a.U, a.p, a.z0, a.g0, a.U0, a.ke0, a.eps, a.failed);
    return done();
}

template <typename R> int launch_hmc_leapfrog(hipStream_t s, const HmcLeapfrogArgs<R> &a)
{
    const bool vec = rows_vec<R>(a.ld, {a.minv, a.z, a.p, a.g});
    hipLaunchKernelGGL(leapfrog_kernel<R>, dim3(a.C), dim3(kThreads), 0, s, a.D, a.ld, vec, a.flags, a.kick, a.eps, a.minv, a.z, a.p,
                       a.g, a.gnn, a.gode, a.P, a.loss_sum, a.lik_scale, a.status, a.n_traj, a.U, a.ke, a.failed, a.ode_mask, a.n_ode,
                       a.mu, a.sd, a.sample_nn, a.nn_p, a.ode_p);
    return done();
}

template <typename R> int launch_hmc_accept(hipStream_t s, const HmcAcceptArgs<R> &a)
{
    const bool vec = rows_vec<R>(a.ld, {a.z, a.z0, a.g, a.g0});
    hipLaunchKernelGGL(accept_kernel<R>, dim3(a.C), dim3(kThreads), 0, s, a.D, a.ld, vec, a.mode, a.seed, a.iter, a.delta, a.z, a.z0,
                       a.g, a.g0, a.U, a.U0, a.ke0, a.ke, a.failed, a.log_eps, a.da, a.search, a.n_ode, a.mu, a.sd, a.draws,
                       a.stats, a.n_slots, a.slot);
    return done();
}

template <typename R> int launch_hmc_welford(hipStream_t s, int C, int D, int ld, int flags, const R *z, double *wf, R *minv)
{
    hipLaunchKernelGGL(welford_kernel<R>, dim3((D + 63) / 64), dim3(64), 0, s, C, D, ld, flags, z, wf, minv);
    return done();
}

#define HODE_HMC_INST(R)                                                                                                          \
    template int launch_mse_sets<R>(hipStream_t, int, int64_t, const R *, const R *, R, double *, R *);                         \
    template int launch_hmc_refresh<R>(hipStream_t, const HmcRefreshArgs<R> &);                                                 \
    template int launch_hmc_leapfrog<R>(hipStream_t, const HmcLeapfrogArgs<R> &);                                               \
    template int launch_hmc_accept<R>(hipStream_t, const HmcAcceptArgs<R> &);                                                   \
    template int launch_hmc_welford<R>(hipStream_t, int, int, int, int, const R *, double *, R *);
HODE_HMC_INST(float)
HODE_HMC_INST(double)

}  // namespace hode

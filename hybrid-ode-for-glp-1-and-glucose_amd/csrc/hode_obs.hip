// hode_obs.hip -- the observation model's negative log-likelihood and cotangent per parameter set (inference/observation.py;
// include/hode.h, "Observation model").
//
// y[n_sets][len] against ONE obs[len] (len = n_traj * T * 6, element i belongs to state i % 6).  An entry is observed when
// obs is finite and, with a mask, the mask byte is non-zero; an unobserved entry is SELECTED away (no arithmetic ever touches
// its obs value): it adds exactly 0 to every sum and its cotangent is 0.  One workgroup of kThreads lanes per set:
//   sweep 1   six fp64 sums of squares per lane (one per state), reduced in a fixed order (block_sum6: a butterfly inside
//             each wave, then the four wave sums in order), added to sse[s][0..5];
//   then      the six cotangent coefficients and the set's negative log-likelihood from the finished sums;
//   sweep 2   gy = coefficient[state] * (y - obs) over the same elements (a set of the samplers' size, 47 KB, is still in L2).
// The 16-byte path gives a lane 12 consecutive elements (three 16-byte loads in fp32 = two rows of six states), so every
// register has a compile-time state and there is no `% 6` select; what is left of a set (len % 12) and every set whose pointers
// or length rule the wide accesses out go row by row (six scalars per lane, the state again a compile-time index).
// There are no floating-point atomics in this file: the same call gives the same bits.
#include "hode_chains.h"

namespace hode {
namespace {

template <typename R> struct ObsKernelArgs {
    int64_t len;
    const R *y, *obs;
    const uint8_t *mask;
    int mode, flags;
    double c0[6], c1[6], c2[6];      // fixed: c0 = 1 / sigma^2;  marginal: c0 = a, c1 = b, c2 = n
    double *sse, *loss_sum;
    R *gy;
};

template <typename R> __device__ __forceinline__ bool seen(R o, unsigned m) { return m != 0u && __builtin_isfinite(o); }

// the 12 mask bytes of a lane's group as three words (mask + i is 4-byte aligned on the 16-byte path), or all ones
__device__ __forceinline__ void ld_mask12(const uint8_t *mask, int64_t i, uint32_t (&w)[3])
{
    if (mask) {
        const uint32_t *p = reinterpret_cast<const uint32_t *>(mask + i);
        w[0] = p[0]; w[1] = p[1]; w[2] = p[2];
    } else {
        w[0] = w[1] = w[2] = 0xffffffffu;
    }
}

// One sweep over a set.  SUMS: acc[k] += (y - obs)^2 of the observed entries of state k.  !SUMS: gs = coef[k] * (y - obs), 0 where
// unobserved.  Both sweeps visit the same elements from the same lanes.
template <typename R, bool VEC, bool SUMS>
__device__ __forceinline__ void sweep(int64_t len, const R *__restrict__ ys, const R *__restrict__ obs, const uint8_t *__restrict__ mask,
                                      double (&acc)[6], const R (&coef)[6], R *__restrict__ gs)
{
    int64_t row0 = 0;                                  // first row (of six) the scalar loop takes
    if (VEC) {
        const int64_t n12 = len / 12;
        for (int64_t grp = threadIdx.x; grp < n12; grp += kThreads) {
            const int64_t i = 12 * grp;
            R a[3][4], b[3][4], g[3][4];
            uint32_t mw[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                ld4(ys + i + 4 * j, true, 4, a[j]);
                ld4(obs + i + 4 * j, true, 4, b[j]);
            }
            ld_mask12(mask, i, mw);
#pragma unroll
            for (int j = 0; j < 3; ++j) {
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int k = (4 * j + c) % 6;                 // compile-time after unrolling
                    const bool on = seen(b[j][c], (mw[j] >> (8 * c)) & 0xffu);
                    const R d = on ? a[j][c] - b[j][c] : R(0);
                    if (SUMS) acc[k] += (double)d * (double)d;
                    else g[j][c] = on ? coef[k] * d : R(0);
                }
            }
            if (!SUMS) {
#pragma unroll
                for (int j = 0; j < 3; ++j) st4(gs + i + 4 * j, true, 4, g[j]);
            }
        }
        row0 = 2 * n12;
    }
    for (int64_t row = row0 + threadIdx.x; 6 * row < len; row += kThreads) {
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const int64_t i = 6 * row + k;
            if (i < len) {
                const R o = obs[i];
                const bool on = seen(o, mask ? mask[i] : 1u);
                const R d = on ? ys[i] - o : R(0);
                if (SUMS) acc[k] += (double)d * (double)d;
                else gs[i] = on ? coef[k] * d : R(0);
            }
        }
    }
}

template <typename R, bool VEC>
__global__ __launch_bounds__(kThreads) void obs_nll_sets_kernel(const ObsKernelArgs<R> a)
{
    __shared__ double sh[24];
    __shared__ double tot[6];
    const int s = blockIdx.x;
    const R *ys = a.y + (int64_t)s * a.len;
    R *gs = a.gy ? a.gy + (int64_t)s * a.len : nullptr;
    double *sse = a.sse + 6 * (int64_t)s;
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    R coef[6] = {R(0), R(0), R(0), R(0), R(0), R(0)};
    const bool from_sse = a.flags == HODE_OBS_FROM_SSE;
    if (!from_sse) {
        sweep<R, VEC, true>(a.len, ys, a.obs, a.mask, acc, coef, nullptr);
        block_sum6(acc, sh);
    }
    // the set's sums so far: lane 0 adds this call's share to sse, every lane then reads the same six totals
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const double t = from_sse ? sse[k] : sse[k] + acc[k];
            if (!from_sse) sse[k] = t;
            tot[k] = t;
        }
    }
    if (a.flags == HODE_OBS_SUMS_ONLY) return;
    __syncthreads();
    // fixed:    nll = sum_k S_k / (2 sigma_k^2) over THIS call's sums (pieces of a set add up), coefficient 1 / sigma_k^2
    // marginal: nll = sum_{n_k > 0} (a_k + n_k / 2) log(b_k + SSE_k / 2) of the set's finished sums, coefficient
    //           (a_k + n_k / 2) / (b_k + SSE_k / 2)
    double nll = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        if (a.mode == HODE_OBS_FIXED) {
            nll += 0.5 * a.c0[k] * (from_sse ? tot[k] : acc[k]);
            coef[k] = (R)a.c0[k];
        } else if (a.c2[k] > 0.0) {
            const double sh_k = a.c0[k] + 0.5 * a.c2[k], rate = a.c1[k] + 0.5 * tot[k];
            nll += sh_k * log(rate);
            coef[k] = (R)(sh_k / rate);
        }
    }
    if (threadIdx.x == 0 && a.loss_sum) a.loss_sum[s] += nll;
    if (gs) sweep<R, VEC, false>(a.len, ys, a.obs, a.mask, acc, coef, gs);
}

}  // namespace

template <typename R> int launch_obs_nll_sets(hipStream_t s, const ObsArgs<R> &h)
{
    ObsKernelArgs<R> a{};
    a.len = h.len; a.y = h.y; a.obs = h.obs; a.mask = h.mask; a.mode = h.mode; a.flags = h.flags;
    a.sse = h.sse; a.loss_sum = h.loss_sum; a.gy = h.gy;
    for (int k = 0; k < 6; ++k) {
        a.c0[k] = h.mode == HODE_OBS_FIXED ? h.w[k] : h.a[k];
        a.c1[k] = h.mode == HODE_OBS_FIXED ? 0.0 : h.b[k];
        a.c2[k] = h.mode == HODE_OBS_FIXED ? 0.0 : h.n[k];
    }
    // 16-byte rows: every set starts on a 16-byte boundary (len % 4 == 0 covers fp32 and fp64) and the mask on a word
    const bool vec = h.len % 4 == 0 && ((((uintptr_t)h.y | (uintptr_t)h.obs | (uintptr_t)h.gy) & 15) == 0) && (((uintptr_t)h.mask & 3) == 0);
    if (vec) hipLaunchKernelGGL((obs_nll_sets_kernel<R, true>), dim3(h.n_sets), dim3(kThreads), 0, s, a);
    else hipLaunchKernelGGL((obs_nll_sets_kernel<R, false>), dim3(h.n_sets), dim3(kThreads), 0, s, a);
    return done();
}

template int launch_obs_nll_sets<float>(hipStream_t, const ObsArgs<float> &);
template int launch_obs_nll_sets<double>(hipStream_t, const ObsArgs<double> &);

}  // namespace hode

// hode_pf_params.hip -- the parameter move of the particle filter (inference/filter.py, run_filter(learn=...); include/hode.h,
// "Particle filter: parameter move"): Liu & West's kernel shrinkage and / or a random walk on chosen
// columns of the payload rows that hode_pf_step_* gathered, launched after it.
//
// One workgroup of kThreads lanes per patient; lane t owns particles t, t + kThreads, ... in every pass, so a lane re-reads only
// what it wrote and the move can be in place.
//   pass 0   which particles count (alive, every selected value usable), from the rows as they came in; the maximum of their
//            log-weights;
//   pass 1   w = exp(lw - m) into LDS, sum w;
//   then, column by column (a column's move writes that column only):
//   pass 2   sum w phi;  pass 3   sum w (phi - mean)^2;  pass 4   the move (Philox stream kRngFilterParam).
// A patient has at most 17 columns of a few thousand values, which stay in cache between the passes; the column loop keeps the
// live state to a handful of doubles.  Every sum is fp64 in block_sum's order (lane-serial, a butterfly inside each wave, then
// the four wave sums in order), floating-point contraction is off and there are no floating-point atomics: the same call gives
// the same bits, and a patient's bits depend on its key id0 + b alone.
#include "hode_chains.h"
#include "hode_philox.h"
#include <limits>

#pragma clang fp contract(off)

namespace hode {
namespace {

constexpr int kPfMax = HODE_PF_MAX_PARTICLES;

template <typename R> struct PfParamArgs {
    int N, n_aux;
    uint32_t step, id0;
    uint64_t seed;
    double shrink;
    const double *lw, *walk, *dt;
    const int32_t *mode;
    R *aux;
    double *pstats;
};

__device__ __forceinline__ double block_max(double v, double *sh)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    const double r = fmax(fmax(sh[0], sh[1]), fmax(sh[2], sh[3]));
    __syncthreads();
    return r;
}

// normal number k & 3 of normals4(block): the same operations on the same words, the unused pair left out
__device__ __forceinline__ double normal_of(const Philox4 &r, int k)
{
    const bool hi = (k & 2) != 0;
    const double rad = sqrt(-2.0 * log(u01(hi ? r.z : r.x))), ang = 6.283185307179586 * u01(hi ? r.w : r.y);
    return (k & 1) ? rad * sin(ang) : rad * cos(ang);
}

template <typename R> __global__ __launch_bounds__(kThreads) void pf_params_kernel(const PfParamArgs<R> a)
{
    extern __shared__ __align__(16) double w[];            // [N]: the weights of the particles that count, 0 for the others
    __shared__ double sh[4];
    __shared__ uint8_t counts[kPfMax];
    const double ninf = -std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const int N = a.N, n_aux = a.n_aux, b = blockIdx.x, tid = threadIdx.x;
    const uint32_t key = a.id0 + (uint32_t)b;
    const int64_t base = (int64_t)b * N;
    const double *lw = a.lw + base;
    R *aux = a.aux + base * n_aux;
    double *pstats = a.pstats + (int64_t)b * 2 * n_aux;

    // the selected columns and their links, as bit masks (n_aux <= 17); the same in every lane
    uint32_t sel = 0, lg = 0;
    for (int k = 0; k < n_aux; ++k) {
        const int32_t md = a.mode[k];
        if (md == HODE_PF_MOVE_IDENTITY || md == HODE_PF_MOVE_LOG) sel |= 1u << k;
        if (md == HODE_PF_MOVE_LOG) lg |= 1u << k;
    }

    // ---- pass 0
    double m = ninf, n_count = 0.0;
    for (int i = tid; i < N; i += kThreads) {
        const double l = lw[i];
        bool ok = l > ninf;                                 // (false for NaN)
        for (int k = 0; k < n_aux; ++k) {
            if ((sel >> k) & 1u) {
                const double v = (double)aux[(int64_t)i * n_aux + k];
                ok = ok && __builtin_isfinite(v) && (!((lg >> k) & 1u) || v > 0.0);
            }
        }
        counts[i] = ok ? 1 : 0;
        if (ok) {
            m = fmax(m, l);
            n_count += 1.0;
        }
    }
    m = block_max(m, sh);
    n_count = block_sum(n_count, sh);
    if (!(n_count > 0.0) || !__builtin_isfinite(m)) {
        // nobody counts (or a log-weight of +inf: no weights can be formed): nothing is moved
        for (int k = tid; k < 2 * n_aux; k += kThreads) pstats[k] = nan;
        return;
    }

    // ---- pass 1
    double sw = 0.0;
    for (int i = tid; i < N; i += kThreads) {
        const double wi = counts[i] ? exp(lw[i] - m) : 0.0;
        w[i] = wi;
        sw += wi;
    }
    sw = block_sum(sw, sh);

    const double sh_a = a.shrink, dtb = a.dt[b];
    for (int k = 0; k < n_aux; ++k) {
        if (!((sel >> k) & 1u)) {
            if (tid == 0) pstats[2 * k] = pstats[2 * k + 1] = nan;
            continue;
        }
        const bool islog = (lg >> k) & 1u;
        // ---- pass 2
        double s1 = 0.0;
        for (int i = tid; i < N; i += kThreads) {
            if (counts[i]) {
                const double v = (double)aux[(int64_t)i * n_aux + k];
                const double phi = islog ? log(v) : v;
                s1 += w[i] * phi;
            }
        }
        const double mean = block_sum(s1, sh) / sw;
        // ---- pass 3
        double s2 = 0.0;
        for (int i = tid; i < N; i += kThreads) {
            if (counts[i]) {
                const double v = (double)aux[(int64_t)i * n_aux + k];
                const double d = (islog ? log(v) : v) - mean;
                s2 += w[i] * (d * d);
            }
        }
        const double var = block_sum(s2, sh) / sw;
        if (tid == 0) {
            pstats[2 * k] = mean;
            pstats[2 * k + 1] = var;
        }
        const double wk = a.walk[k];
        if (sh_a == 1.0 && wk == 0.0) continue;             // nothing to do: the column keeps its bits
        // ---- pass 4
        const double sd = sqrt((1.0 - sh_a * sh_a) * var + (wk * wk) * dtb);
        for (int i = tid; i < N; i += kThreads) {
            if (counts[i]) {
                const double v = (double)aux[(int64_t)i * n_aux + k];
                const double phi = islog ? log(v) : v;
                const double eps = normal_of(hmc_rng(a.seed, key, a.step, kRngFilterParam, 5u * (uint32_t)i + (uint32_t)(k >> 2)), k);
                const double moved = (mean + sh_a * (phi - mean)) + sd * eps;
                aux[(int64_t)i * n_aux + k] = (R)(islog ? exp(moved) : moved);
            }
        }
    }
}

template <typename R>
int pf_params(void *stream, int B, int N, uint32_t step, uint64_t seed, uint32_t id0, const double *lw, int n_aux, R *aux,
              const int32_t *mode, const double *walk, const double *dt, double shrink, double *pstats)
{
    if (B < 1 || N < 1 || n_aux < 1 || n_aux > HODE_PF_MAX_AUX) return HODE_EINVAL;
    if (!(shrink >= 0.0 && shrink <= 1.0)) return HODE_EINVAL;
    if (!lw || !aux || !mode || !walk || !dt || !pstats) return HODE_EINVAL;
    if (N > HODE_PF_MAX_PARTICLES) return HODE_EUNSUPPORTED;
    PfParamArgs<R> a{};
    a.N = N; a.n_aux = n_aux; a.step = step; a.id0 = id0; a.seed = seed; a.shrink = shrink;
    a.lw = lw; a.walk = walk; a.dt = dt; a.mode = mode; a.aux = aux; a.pstats = pstats;
    hipLaunchKernelGGL((pf_params_kernel<R>), dim3(B), dim3(kThreads), (size_t)N * sizeof(double), (hipStream_t)stream, a);
    return done();
}

}  // namespace
}  // namespace hode

extern "C" {

int hode_pf_params_f32(void *stream, int B, int N, uint32_t step, uint64_t seed, uint32_t id0, const double *lw, int n_aux, float *aux,
                       const int32_t *mode, const double *walk, const double *dt, double shrink, double *pstats)
{
    return hode::pf_params<float>(stream, B, N, step, seed, id0, lw, n_aux, aux, mode, walk, dt, shrink, pstats);
}
int hode_pf_params_f64(void *stream, int B, int N, uint32_t step, uint64_t seed, uint32_t id0, const double *lw, int n_aux, double *aux,
                       const int32_t *mode, const double *walk, const double *dt, double shrink, double *pstats)
{
    return hode::pf_params<double>(stream, B, N, step, seed, id0, lw, n_aux, aux, mode, walk, dt, shrink, pstats);
}

}  // extern "C"

// hode_filter.hip -- one step of the bootstrap particle filter per patient (inference/filter.py, run_filter; include/hode.h,
// "Particle filter"): what happens between two forward solves of a patient's N particles.
//
// One workgroup of kThreads lanes per patient; lane t owns particles t, t + kThreads, ... in every pass (so a lane re-reads only
// what it wrote), except in the scan, where it owns a contiguous chunk of the LDS array.
//   pass A   process noise (Philox stream kRngFilterNoise), x_out = the noised state, the new log-weight into LDS;
//            the maxima of the log-weights on entry and now, the number of particles alive;
//   pass B   w = exp(lw - m) into LDS in place of lw; sum w^2, sum w x_j, sum exp(lw_in - m_in); lw written back;
//   pass C   sum w (x_j - mean_j)^2;
//   scan     c_k = sum_{i <= k} w_i in place: sequential inside a lane's chunk, Kogge-Stone across the lanes of a wave, the four
//            wave totals in order;
//   resample iff ESS < ess_frac * N: slot i searches c for its pointer (i + u) / N * c_{N-1} (one u per patient, stream
//            kRngFilterResample) and gathers its ancestor's noised state and payload.
// The noised state of a particle is a pure function of (x_in row, seed, key, step, particle), so the passes that need its fp64
// value again recompute it (fp64 data: read it back from x_out, which then holds all of its bits) and the gather recomputes the
// ancestor's: nothing of size N * 6 has to stay on chip, and x_out may therefore not alias x_in.
// Every sum is fp64 in a fixed order (lane-serial, a butterfly inside each wave, then the four wave sums in order), floating-
// point contraction is off (an a * b + c here is two roundings, as in the restatement of the tests), and there are no
// floating-point atomics: the same call gives the same bits, and a patient's bits depend on its key id0 + b alone.
#include "hode_chains.h"
#include "hode_philox.h"
#include <limits>

#pragma clang fp contract(off)

namespace hode {
namespace {

constexpr int kPfMax = HODE_PF_MAX_PARTICLES;
constexpr double kHalfLog2Pi = 0.9189385332046727;

template <typename R> struct PfArgs {
    int N, link, n_aux;
    uint32_t step, id0;
    uint64_t seed;
    double ess_frac;
    const R *x_in, *obs, *aux_in;
    const int32_t *status;
    const uint8_t *mask;
    const double *sigma, *q, *dt;
    double *lw, *stats;
    R *x_out, *aux_out;
    int32_t *anc;
};

// K sums at once (sh: 4 * K doubles), each in the order of block_sum (hode_chains.h)
template <int K> __device__ __forceinline__ void block_sum_n(double (&v)[K], double *sh)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] += __shfl_xor(v[k], o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) sh[4 * k + (threadIdx.x >> 6)] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = (sh[4 * k] + sh[4 * k + 1]) + (sh[4 * k + 2] + sh[4 * k + 3]);
    __syncthreads();
}

// two maxima at once (sh: 8 doubles); a maximum does not depend on the order
__device__ __forceinline__ void block_max2(double &a, double &b, double *sh)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a = fmax(a, __shfl_xor(a, o, 64));
        b = fmax(b, __shfl_xor(b, o, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        sh[threadIdx.x >> 6] = a;
        sh[4 + (threadIdx.x >> 6)] = b;
    }
    __syncthreads();
    a = fmax(fmax(sh[0], sh[1]), fmax(sh[2], sh[3]));
    b = fmax(fmax(sh[4], sh[5]), fmax(sh[6], sh[7]));
    __syncthreads();
}

// the state of particle i after the process noise, in fp64.  s[j] = q_j sqrt(dt); s[j] > 0 is false for 0, negatives and NaN,
// and such a state is the input's value exactly.
template <typename R>
__device__ __forceinline__ void noised(const R *__restrict__ row, uint64_t seed, uint32_t key, uint32_t step, uint32_t i,
                                       const double (&s)[6], int link, double (&x)[6])
{
#pragma unroll
    for (int j = 0; j < 6; ++j) x[j] = (double)row[j];
    double n[8];
    if (s[0] > 0.0 || s[1] > 0.0 || s[2] > 0.0 || s[3] > 0.0) {
        double t[4];
        normals4(hmc_rng(seed, key, step, kRngFilterNoise, 2u * i), t);
        n[0] = t[0]; n[1] = t[1]; n[2] = t[2]; n[3] = t[3];
    } else {
        n[0] = n[1] = n[2] = n[3] = 0.0;
    }
    if (s[4] > 0.0 || s[5] > 0.0) {
        double t[4];
        normals4(hmc_rng(seed, key, step, kRngFilterNoise, 2u * i + 1u), t);
        n[4] = t[0]; n[5] = t[1];
    } else {
        n[4] = n[5] = 0.0;
    }
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        if (s[j] > 0.0) {
            if (link == HODE_PF_LINK_LOG) x[j] = x[j] * exp(s[j] * n[j] - 0.5 * (s[j] * s[j]));
            else x[j] = x[j] + s[j] * n[j];
        }
    }
}

template <typename R> __global__ __launch_bounds__(kThreads) void pf_step_kernel(const PfArgs<R> a)
{
    extern __shared__ __align__(16) double c[];            // [N]: log-weights, then weights, then cumulative weights
    __shared__ double sh[36];
    __shared__ uint8_t dead[kPfMax];
    const double ninf = -std::numeric_limits<double>::infinity();
    const int N = a.N, b = blockIdx.x, tid = threadIdx.x;
    const uint32_t key = a.id0 + (uint32_t)b;
    const int64_t base = (int64_t)b * N;
    const R *xin = a.x_in + 6 * base;
    R *xout = a.x_out + 6 * base;
    double *lw = a.lw + base;
    int32_t *anc = a.anc + base;
    double *stats = a.stats + (int64_t)b * HODE_PF_COLS;

    const double rdt = sqrt(a.dt[b]);
    double s[6], o[6], sig[6], lsig[6];
    bool seen[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        s[j] = a.q[j] * rdt;
        const R ob = a.obs[6 * (int64_t)b + j];
        seen[j] = __builtin_isfinite(ob) && (!a.mask || a.mask[6 * (int64_t)b + j] != 0);
        o[j] = seen[j] ? (double)ob : 0.0;
        sig[j] = a.sigma[j];
        lsig[j] = log(a.sigma[j]);
    }

    // ---- pass A
    double m_in = ninf, m = ninf, n_alive = 0.0;
    for (int i = tid; i < N; i += kThreads) {
        double x[6];
        noised<R>(xin + 6 * (int64_t)i, a.seed, key, a.step, (uint32_t)i, s, a.link, x);
        bool ok = !a.status || a.status[base + i] == 0;
        double acc = 0.0;
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            xout[6 * (int64_t)i + j] = (R)x[j];
            ok = ok && __builtin_isfinite(x[j]);
            if (seen[j]) {
                const double z = (o[j] - x[j]) / sig[j];
                acc += (-0.5 * (z * z) - lsig[j]) - kHalfLog2Pi;
            }
        }
        double l_in = lw[i];
        if (!(l_in > ninf)) l_in = ninf;                   // NaN on entry counts as dead
        double l = l_in + acc;
        if (!ok || !(l > ninf) || !__builtin_isfinite(l)) l = ninf;
        c[i] = l;
        dead[i] = l > ninf ? 0 : 1;
        m_in = fmax(m_in, l_in);
        m = fmax(m, l);
        n_alive += l > ninf ? 1.0 : 0.0;
    }
    block_max2(m_in, m, sh);
    {
        double v[1] = {n_alive};
        block_sum_n<1>(v, sh);
        n_alive = v[0];
    }

    if (!(n_alive > 0.0)) {
        // nobody is left: the states keep their noise, the weights stay dead, nothing is resampled
        for (int i = tid; i < N; i += kThreads) {
            lw[i] = ninf;
            anc[i] = i;
            for (int k = 0; k < a.n_aux; ++k) a.aux_out[(base + i) * a.n_aux + k] = a.aux_in[(base + i) * a.n_aux + k];
        }
        if (tid < HODE_PF_COLS) {
            const double nan = std::numeric_limits<double>::quiet_NaN();
            stats[tid] = tid == 0 ? ninf : tid < 4 ? 0.0 : nan;
        }
        return;
    }

    // ---- pass B
    double sb[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};      // sum w, sum w^2, sum exp(lw_in - m_in), sum w x_j
    for (int i = tid; i < N; i += kThreads) {
        const double l = c[i], l_in = lw[i];
        const double w = l > ninf ? exp(l - m) : 0.0;
        c[i] = w;
        lw[i] = l;
        sb[0] += w;
        sb[1] += w * w;
        if (l_in > ninf) sb[2] += exp(l_in - m_in);
        if (l > ninf) {
            double x[6];
            if constexpr (sizeof(R) == 8) {
#pragma unroll
                for (int j = 0; j < 6; ++j) x[j] = (double)xout[6 * (int64_t)i + j];
            } else {
                noised<R>(xin + 6 * (int64_t)i, a.seed, key, a.step, (uint32_t)i, s, a.link, x);
            }
#pragma unroll
            for (int j = 0; j < 6; ++j) sb[3 + j] += w * x[j];
        }
    }
    block_sum_n<9>(sb, sh);
    double mean[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) mean[j] = sb[3 + j] / sb[0];

    // ---- pass C
    double sv[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = tid; i < N; i += kThreads) {
        const double w = c[i];
        if (!dead[i]) {
            double x[6];
            if constexpr (sizeof(R) == 8) {
#pragma unroll
                for (int j = 0; j < 6; ++j) x[j] = (double)xout[6 * (int64_t)i + j];
            } else {
                noised<R>(xin + 6 * (int64_t)i, a.seed, key, a.step, (uint32_t)i, s, a.link, x);
            }
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                const double d = x[j] - mean[j];
                sv[j] += w * (d * d);
            }
        }
    }
    block_sum_n<6>(sv, sh);          // (its barriers also order pass B's writes of c before the scan's reads)

    // ---- scan: lane t owns c[t * per .. (t + 1) * per)
    const int per = (N + kThreads - 1) / kThreads;
    const int lo = min(tid * per, N), hi = min(lo + per, N);
    double run = 0.0;
    for (int k = lo; k < hi; ++k) {
        run += c[k];
        c[k] = run;
    }
    double incl = run;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double up = __shfl_up(incl, d, 64);
        if ((tid & 63) >= d) incl = up + incl;
    }
    if ((tid & 63) == 63) sh[tid >> 6] = incl;
    __syncthreads();
    double wave_base = 0.0;
    for (int w = 0; w < (tid >> 6); ++w) wave_base += sh[w];
    double excl = __shfl_up(incl, 1, 64);
    if ((tid & 63) == 0) excl = 0.0;
    excl = wave_base + excl;
    for (int k = lo; k < hi; ++k) c[k] = excl + c[k];
    __syncthreads();
    const double ctot = c[N - 1];

    const double ess = (sb[0] * sb[0]) / sb[1];
    const bool resample = ess < a.ess_frac * (double)N;
    if (tid == 0) {
        // both sums in block_sum's order, not the scan's: a patient nothing was observed of gets exactly 0
        stats[0] = (m + log(sb[0])) - (m_in + log(sb[2]));
        stats[1] = ess;
        stats[2] = resample ? 1.0 : 0.0;
        stats[3] = n_alive;
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            stats[4 + j] = mean[j];
            stats[10 + j] = sv[j] / sb[0];
        }
    }

    // ---- resample + gather
    const double u = u01(hmc_rng(a.seed, key, a.step, kRngFilterResample, 0u).x);
    for (int i = tid; i < N; i += kThreads) {
        int k = i;
        if (resample) {
            const double target = ((double)i + u) / (double)N * ctot;
            int l0 = 0, h0 = N - 1;                         // min{k : c_k >= target}; c_{N-1} >= target always
            while (l0 < h0) {
                const int mid = (l0 + h0) >> 1;
                if (c[mid] >= target) h0 = mid;
                else l0 = mid + 1;
            }
            k = l0;
            // c is the exact cumulative sum only up to rounding: where a pointer falls into such a gap in front of a dead
            // particle, the alive one before it is meant (one exists: in front of the first alive particle c is exactly 0)
            while (k > 0 && dead[k]) --k;
            lw[i] = 0.0;
            if (k != i) {
                double x[6];
                noised<R>(xin + 6 * (int64_t)k, a.seed, key, a.step, (uint32_t)k, s, a.link, x);
#pragma unroll
                for (int j = 0; j < 6; ++j) xout[6 * (int64_t)i + j] = (R)x[j];
            }
        }
        anc[i] = k;
        for (int j = 0; j < a.n_aux; ++j) a.aux_out[(base + i) * a.n_aux + j] = a.aux_in[(base + k) * a.n_aux + j];
    }
}

template <typename R>
int pf_step(void *stream, int B, int N, uint32_t step, uint64_t seed, uint32_t id0, const R *x_in, const int32_t *status, const R *obs,
            const uint8_t *mask, const double *sigma, const double *q, const double *dt, int link, double ess_frac, double *lw, R *x_out,
            int32_t *anc, double *stats, int n_aux, const R *aux_in, R *aux_out)
{
    if (B < 1 || N < 1 || n_aux < 0 || n_aux > HODE_PF_MAX_AUX || (link != HODE_PF_LINK_ADD && link != HODE_PF_LINK_LOG)) return HODE_EINVAL;
    if (!(ess_frac >= 0.0 && ess_frac <= 1.0)) return HODE_EINVAL;
    if (!x_in || !obs || !sigma || !q || !dt || !lw || !x_out || !anc || !stats) return HODE_EINVAL;
    if (n_aux > 0 && (!aux_in || !aux_out)) return HODE_EINVAL;
    if (x_out == x_in || (n_aux > 0 && aux_out == aux_in)) return HODE_EINVAL;
    if (N > HODE_PF_MAX_PARTICLES) return HODE_EUNSUPPORTED;
    PfArgs<R> a{};
    a.N = N; a.link = link; a.n_aux = n_aux; a.step = step; a.id0 = id0; a.seed = seed; a.ess_frac = ess_frac;
    a.x_in = x_in; a.obs = obs; a.aux_in = aux_in; a.status = status; a.mask = mask; a.sigma = sigma; a.q = q; a.dt = dt;
    a.lw = lw; a.stats = stats; a.x_out = x_out; a.aux_out = aux_out; a.anc = anc;
    hipLaunchKernelGGL((pf_step_kernel<R>), dim3(B), dim3(kThreads), (size_t)N * sizeof(double), (hipStream_t)stream, a);
    return done();
}

}  // namespace
}  // namespace hode

extern "C" {

int hode_pf_step_f32(void *stream, int B, int N, uint32_t step, uint64_t seed, uint32_t id0, const float *x_in, const int32_t *status,
                     const float *obs, const uint8_t *mask, const double *sigma, const double *q, const double *dt, int link,
                     double ess_frac, double *lw, float *x_out, int32_t *anc, double *stats, int n_aux, const float *aux_in,
                     float *aux_out)
{
    return hode::pf_step<float>(stream, B, N, step, seed, id0, x_in, status, obs, mask, sigma, q, dt, link, ess_frac, lw, x_out, anc, stats,
                                n_aux, aux_in, aux_out);
}
int hode_pf_step_f64(void *stream, int B, int N, uint32_t step, uint64_t seed, uint32_t id0, const double *x_in, const int32_t *status,
                     const double *obs, const uint8_t *mask, const double *sigma, const double *q, const double *dt, int link,
                     double ess_frac, double *lw, double *x_out, int32_t *anc, double *stats, int n_aux, const double *aux_in,
                     double *aux_out)
{
    return hode::pf_step<double>(stream, B, N, step, seed, id0, x_in, status, obs, mask, sigma, q, dt, link, ess_frac, lw, x_out, anc, stats,
                                 n_aux, aux_in, aux_out);
}

}  // extern "C"

// hode_sobol.hip -- Sobol indices of a Saltelli design's outputs with bootstrap confidence (inference/sobol.py; include/hode.h,
// "Sobol indices"): the analysis that follows the one-launch solve of HybridODENN.forward_ode_sets.
//
// One workgroup of kThreads lanes per output column.  The column's N * nb raw values are staged in LDS in the input's type when
// they fit (the reference size, 1 024 x 16 fp32, is 64 KiB) and read from global memory when not; every value is normalised in
// fp64 as it is used, so both routes feed the same operands to the same sums.  Then, for the base estimate (rho = identity) and
// for each of the R resamples:
//   rho     the N resampled base-sample indices (Philox stream kRngSobol), kept in LDS when there is room, else recomputed;
//   pass 0  the mean of the resampled A u B;
//   pass 1  per group of kGroup parameters j: sum B (AB_j - A) and sum (A - AB_j)^2; with the first group also the centred sum
//           of squares of A u B and sum A B;
//   pass 2  (second order) per j and group of kGroup parameters k > j: sum BA_j AB_k;
//   finish  lane o owns output o (S1_j, ST_j, S2_jk): the base estimate is stored, a resample updates the output's Welford
//           state, from which the ddof-1 standard deviation comes.
// Lane t takes base samples t, t + kThreads, ...; a sum is a butterfly inside each wave, then the four wave sums in order
// (block_sum's order, hode_chains.h).  Nothing depends on M or on the route: no floating-point atomics, the same bits every time.
#include "hode_chains.h"
#include "hode_philox.h"
#include <limits>

namespace hode {
namespace {

constexpr int kGroup = 8;                       // accumulators of one kind a lane carries through a pass
constexpr size_t kLdsBudget = 160 * 1024;       // what one workgroup may declare on gfx950

template <typename R> struct SobolArgs {
    int N, D, nb, second, n_res;
    int staged, rho_lds;                        // the column / the resample indices live in LDS
    int64_t ldy;
    const R *Y;
    uint64_t seed;
    double conf_z;
    double *S1, *ST, *S2, *S1c, *STc, *S2c, *variance;
};

// doubles in the fixed part of the workgroup's LDS: block_sum scratch, wave partials of every sum, Welford state of every output
__host__ __device__ inline int n_outputs(int D, int second) { return 2 * D + (second ? D * (D - 1) / 2 : 0); }
__host__ __device__ inline size_t fixed_doubles(int D, int second) { return 8 + 4 * (size_t)(2 + n_outputs(D, second)) + 2 * (size_t)n_outputs(D, second); }

__device__ __forceinline__ uint32_t resample_index(uint64_t seed, uint32_t r, uint32_t q, uint32_t N)
{
    const Philox4 b = hmc_rng(seed, 0u, r, kRngSobol, q >> 2);
    const uint32_t w = (q & 3u) == 0u ? b.x : (q & 3u) == 1u ? b.y : (q & 3u) == 2u ? b.z : b.w;
    return (uint32_t)(((uint64_t)w * N) >> 32);
}

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// the workgroup's maximum, in block_sum's order: a column's extremes (min = -max(-v)) and its finiteness flag
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

// pair (j, k), j < k, in j-major order
__device__ __forceinline__ int pair_slot(int D, int j, int k) { return j * D - j * (j + 1) / 2 + (k - j - 1); }

template <typename R>
__global__ __launch_bounds__(kThreads) void sobol_indices_kernel(const SobolArgs<R> a)
{
    extern __shared__ double lds[];
    const int D = a.D, N = a.N, nb = a.nb, m = blockIdx.x, t = threadIdx.x;
    const int nP = a.second ? D * (D - 1) / 2 : 0, O = 2 * D + nP;
    const int64_t n = (int64_t)N * nb;
    double *red = lds;                               // [8]
    double *part = red + 8;                          // [2 + O][4]: {centred squares of A u B, A B, S1 sums, ST sums, pair sums} per wave
    double *wf = part + 4 * (2 + O);                 // [O][2]: {mean, M2} of the resampled estimates
    uint32_t *rho = reinterpret_cast<uint32_t *>(wf + 2 * O);
    R *stage = reinterpret_cast<R *>(rho + (a.rho_lds ? (N + 1) / 2 * 2 : 0));
    const R *col = a.Y + m;
    double *S1 = a.S1 + (int64_t)m * D, *ST = a.ST + (int64_t)m * D;
    double *S2 = a.second ? a.S2 + (int64_t)m * D * D : nullptr;
    double *S1c = a.S1c ? a.S1c + (int64_t)m * D : nullptr, *STc = a.STc ? a.STc + (int64_t)m * D : nullptr;
    double *S2c = a.second && a.S2c ? a.S2c + (int64_t)m * D * D : nullptr;
    const double nan = std::numeric_limits<double>::quiet_NaN();

    // ---- the column: staged, its sum, extremes and finiteness; then mean and ddof-0 variance in two passes
    double sum = 0.0, hi = -INFINITY, nlo = -INFINITY, bad = 0.0;
    for (int64_t i = t; i < n; i += kThreads) {
        const R raw = col[i * a.ldy];
        if (a.staged) stage[i] = raw;
        const double v = (double)raw;
        if (!__builtin_isfinite(v)) bad = 1.0;
        sum += v;
        hi = fmax(hi, v);
        nlo = fmax(nlo, -v);
    }
    bad = block_max(bad, red);                       // (also the barrier that publishes the staged column)
    hi = block_max(hi, red);
    nlo = block_max(nlo, red);
    const bool degenerate = bad != 0.0 || hi == -nlo;
    double mean = 0.0, inv_std = 0.0;
    if (!degenerate) {
        mean = block_sum(sum, red) / (double)n;
        double ss = 0.0;
        for (int64_t i = t; i < n; i += kThreads) {
            const double d = (double)(a.staged ? stage[i] : col[i * a.ldy]) - mean;
            ss += d * d;
        }
        const double var = block_sum(ss, red) / (double)n;
        inv_std = 1.0 / sqrt(var);
        if (t == 0 && a.variance) a.variance[m] = var;
    } else if (t == 0 && a.variance) {
        a.variance[m] = bad != 0.0 ? nan : 0.0;
    }
    // what no estimate fills: S2 off the pairs j < k, and everything of a degenerate column
    for (int e = t; e < D * D; e += kThreads) {
        if (degenerate || !(e / D < e % D)) {
            if (S2) S2[e] = nan;
            if (S2c) S2c[e] = nan;
        }
    }
    if (degenerate) {
        for (int j = t; j < D; j += kThreads) {
            S1[j] = nan; ST[j] = nan;
            if (S1c) S1c[j] = nan;
            if (STc) STc[j] = nan;
        }
        return;                                      // (the whole workgroup: `degenerate` is the same in every lane)
    }
    auto z = [&](int64_t row) -> double { return ((double)(a.staged ? stage[row] : col[row * a.ldy]) - mean) * inv_std; };
    for (int o = t; o < O; o += kThreads) { wf[2 * o] = 0.0; wf[2 * o + 1] = 0.0; }     // (lane o is the only one to touch wf[o])

    const int wave = t >> 6;
    const bool lead = (t & 63) == 0;
    for (int r = -1; r < a.n_res; ++r) {
        auto row_of = [&](int q) -> int64_t {
            const uint32_t i = a.rho_lds ? rho[q] : r < 0 ? (uint32_t)q : resample_index(a.seed, (uint32_t)r, (uint32_t)q, (uint32_t)N);
            return (int64_t)i * nb;
        };
        if (a.rho_lds)                               // (a lane reads back only the entries it wrote: no barrier)
            for (int q = t; q < N; q += kThreads) rho[q] = r < 0 ? (uint32_t)q : resample_index(a.seed, (uint32_t)r, (uint32_t)q, (uint32_t)N);
        // pass 0: the mean of A u B
        double s = 0.0;
        for (int q = t; q < N; q += kThreads) {
            const int64_t b = row_of(q);
            s += z(b) + z(b + nb - 1);
        }
        const double mab = block_sum(s, red) / (2.0 * N);   // (its barriers also fence the previous finish off the partials)
        // pass 1: first-order and total sums, kGroup parameters at a time
        for (int j0 = 0; j0 < D; j0 += kGroup) {
            const int cnt = min(kGroup, D - j0);
            double s1[kGroup], st[kGroup], vv = 0.0, sab = 0.0;
#pragma unroll
            for (int c = 0; c < kGroup; ++c) { s1[c] = 0.0; st[c] = 0.0; }
            for (int q = t; q < N; q += kThreads) {
                const int64_t b = row_of(q);
                const double A = z(b), B = z(b + nb - 1);
                if (j0 == 0) {
                    const double da = A - mab, db = B - mab;
                    vv += da * da + db * db;
                    sab += A * B;
                }
#pragma unroll
                for (int c = 0; c < kGroup; ++c) {
                    if (c < cnt) {
                        const double ab = z(b + 1 + j0 + c), d = A - ab;
                        s1[c] += B * (ab - A);
                        st[c] += d * d;
                    }
                }
            }
            if (j0 == 0) {
                vv = wave_sum(vv);
                sab = wave_sum(sab);
                if (lead) { part[wave] = vv; part[4 + wave] = sab; }
            }
#pragma unroll
            for (int c = 0; c < kGroup; ++c) {
                if (c < cnt) {
                    const double u = wave_sum(s1[c]), w = wave_sum(st[c]);
                    if (lead) { part[4 * (2 + j0 + c) + wave] = u; part[4 * (2 + D + j0 + c) + wave] = w; }
                }
            }
        }
        // pass 2: the second-order cross sums
        if (a.second) {
            for (int j = 0; j + 1 < D; ++j) {
                for (int k0 = j + 1; k0 < D; k0 += kGroup) {
                    const int cnt = min(kGroup, D - k0);
                    double cs[kGroup];
#pragma unroll
                    for (int c = 0; c < kGroup; ++c) cs[c] = 0.0;
                    for (int q = t; q < N; q += kThreads) {
                        const int64_t b = row_of(q);
                        const double ba = z(b + 1 + D + j);
#pragma unroll
                        for (int c = 0; c < kGroup; ++c)
                            if (c < cnt) cs[c] += ba * z(b + 1 + k0 + c);
                    }
#pragma unroll
                    for (int c = 0; c < kGroup; ++c) {
                        if (c < cnt) {
                            const double u = wave_sum(cs[c]);
                            if (lead) part[4 * (2 + 2 * D + pair_slot(D, j, k0 + c)) + wave] = u;
                        }
                    }
                }
            }
        }
        __syncthreads();
        // finish: output o from the finished sums
        auto total = [&](int slot) -> double { const double *p = part + 4 * slot; return (p[0] + p[1]) + (p[2] + p[3]); };
        const double V = total(0) / (2.0 * N);
        auto first = [&](int j) -> double { return total(2 + j) / (double)N / V; };
        for (int o = t; o < O; o += kThreads) {
            double e;
            double *out, *conf;
            if (o < D) {
                e = first(o);
                out = S1 + o; conf = S1c ? S1c + o : nullptr;
            } else if (o < 2 * D) {
                e = 0.5 * (total(2 + o) / (double)N) / V;
                out = ST + (o - D); conf = STc ? STc + (o - D) : nullptr;
            } else {
                int j = 0, p = o - 2 * D;
                while (p >= D - 1 - j) { p -= D - 1 - j; ++j; }
                const int k = j + 1 + p;
                e = (total(2 + o) - total(1)) / (double)N / V - first(j) - first(k);
                out = S2 + j * D + k; conf = S2c ? S2c + j * D + k : nullptr;
            }
            if (r < 0) {
                *out = e;
                if (conf && a.n_res < 2) *conf = nan;
            } else {
                // Welford: mean and sum of squared deviations of the estimates so far
                const double cntr = (double)(r + 1), d = e - wf[2 * o];
                const double mu = wf[2 * o] + d / cntr;
                wf[2 * o] = mu;
                wf[2 * o + 1] += d * (e - mu);
                if (conf && r == a.n_res - 1 && a.n_res >= 2) *conf = a.conf_z * sqrt(wf[2 * o + 1] / (double)(a.n_res - 1));
            }
        }
    }
}

template <typename R>
int sobol_indices(void *stream, int N, int D, int M, const R *Y, int64_t ldy, int second_order, int n_res, uint64_t seed, double conf_z,
                  double *S1, double *ST, double *S2, double *S1c, double *STc, double *S2c, double *variance)
{
    if (N < 1 || D < 1 || M < 1 || ldy < M || n_res < 0 || !Y || !S1 || !ST || (second_order && !S2)) return HODE_EINVAL;
    if (n_res > 0 && (!S1c || !STc || (second_order && !S2c))) return HODE_EINVAL;
    if (D > HODE_SOBOL_MAX_D) return HODE_EUNSUPPORTED;
    const int nb = second_order ? 2 * D + 2 : D + 2;
    if ((int64_t)N * nb > (((int64_t)1 << 62) / ldy)) return HODE_EINVAL;          // row * ldy stays inside int64
    SobolArgs<R> a{};
    a.N = N; a.D = D; a.nb = nb; a.second = second_order ? 1 : 0; a.n_res = n_res; a.ldy = ldy; a.Y = Y; a.seed = seed;
    a.conf_z = conf_z; a.S1 = S1; a.ST = ST; a.S2 = S2; a.S1c = S1c; a.STc = STc; a.S2c = S2c; a.variance = variance;
    // LDS: the fixed part, then the column if it fits, then the resample indices if they still fit
    size_t bytes = fixed_doubles(D, a.second) * sizeof(double);
    const size_t col_bytes = (size_t)N * nb * sizeof(R), rho_bytes = ((size_t)N + 1) / 2 * 2 * sizeof(uint32_t);
    if (bytes + col_bytes <= kLdsBudget) { a.staged = 1; bytes += col_bytes; }
    if (bytes + rho_bytes <= kLdsBudget) { a.rho_lds = 1; bytes += rho_bytes; }
    // (more than 64 KiB of dynamic LDS has to be asked for)
    if (bytes > 64 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void *>(&sobol_indices_kernel<R>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBudget) != hipSuccess) {
        (void)hipGetLastError();
        return HODE_ELAUNCH;
    }
    hipLaunchKernelGGL((sobol_indices_kernel<R>), dim3(M), dim3(kThreads), bytes, (hipStream_t)stream, a);
    return done();
}

}  // namespace
}  // namespace hode

extern "C" {

int hode_sobol_indices_f32(void *stream, int N, int D, int M, const float *Y, int64_t ldy, int second_order, int R, uint64_t seed,
                           double conf_z, double *S1, double *ST, double *S2, double *S1_conf, double *ST_conf, double *S2_conf,
                           double *variance)
{
    return hode::sobol_indices<float>(stream, N, D, M, Y, ldy, second_order, R, seed, conf_z, S1, ST, S2, S1_conf, ST_conf, S2_conf, variance);
}
int hode_sobol_indices_f64(void *stream, int N, int D, int M, const double *Y, int64_t ldy, int second_order, int R, uint64_t seed,
                           double conf_z, double *S1, double *ST, double *S2, double *S1_conf, double *ST_conf, double *S2_conf,
                           double *variance)
{
    return hode::sobol_indices<double>(stream, N, D, M, Y, ldy, second_order, R, seed, conf_z, S1, ST, S2, S1_conf, ST_conf, S2_conf, variance);
}

}  // extern "C"

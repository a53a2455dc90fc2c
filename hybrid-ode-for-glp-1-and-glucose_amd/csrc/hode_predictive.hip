// hode_predictive.hip -- posterior-predictive summaries folded draw by draw, and their scores against the data
// (inference/predictive.py, eval/evaluate.py; include/hode.h, "Posterior-predictive summaries").
//
// y[n_draws][N] are trajectories of n_draws parameter draws (N = n_traj * T * 6, element i belongs to state i % 6).
//   pred_fold   folds the draws of a call into a per-entry state {n, mean, m2, pit, lmax, lsum} that lives in the caller's
//               device memory: a lane OWNS one entry, loads its state once, takes the draws one at a time in draw order
//               (Welford's update; contraction is off inside the update, so one draw is the same arithmetic wherever the
//               loop boundaries of a call fall), and stores the state once.  The state is fp64 in registers and fp64 in
//               memory, so a store and a load between two draws change nothing: any split of the draws into consecutive
//               calls gives the bits of one call.  kFly draws' loads are issued before the first of them is used; across
//               the lanes of a wave every load is 64 consecutive reals.
//   pred_score  turns a finished state into mean / sd / pit and a table [6][K] of per-state sums: lane sums, a block sum in
//               the order of block_sum6, one partial row per workgroup, and a last pass that adds the rows in index order.
//               The histogram columns are integer counts (LDS integer adds: exact in any order).  Its 16-byte path gives a
//               lane 12 consecutive entries (two rows of six states), so the state of every accumulator is a compile-time
//               index, as in hode_obs.hip; a call whose length (N % 4 != 0) or pointers rule the wide accesses out goes row
//               by row, six scalars per lane, the state again a compile-time index.
//   pred_tails  folds the draws into the K smallest and the K largest values of every entry (two binary heaps per entry in
//               global memory, slot-major so a wave's accesses at one depth coalesce): a lane owns one entry as in pred_fold,
//               keeps the count and the two heap roots in registers, and only a value that passes a root -- about
//               K (1 + ln(S / K)) of S draws per tail -- walks a heap, O(log K) loads and stores.  A draw is a pure update of
//               the state in memory, so any split of the draws gives the same bits and any order the same multisets.
//   pred_quantiles  sorts the two buffers in place (heapsort, then reversed: a sorted buffer is still a heap, so folding may
//               go on) and interpolates every level between two order statistics in fp64 (numpy's "linear" method); the band
//               table [6][4] of the outer pair of levels against the data is reduced as the score table is.
// There are no floating-point atomics in this file: the same call gives the same bits.
#include "hode_pred_heap.h"

namespace hode {
namespace {

constexpr int kScoreBlocks = HODE_PRED_SCORE_BLOCKS;
constexpr int kFixedCols = HODE_PRED_FIXED_COLS;
constexpr double kInvSqrt2 = 0.70710678118654752440, kInvSqrtPi = 0.56418958354775628695, kInvSqrt2Pi = 0.39894228040143267794;

template <typename R> struct FoldArgs {
    int n_draws;
    int64_t N, row_len, n_traj;
    const R *y, *obs;
    const uint8_t *mask;
    const double *sigma;
    const int32_t *status;
    int32_t *n;
    double *mean, *m2, *pit, *lmax, *lsum;
};

// G consecutive values (G = 12 or 6) from p + i: 16-byte accesses when VEC (then G = 12 and p + i is 16-byte aligned)
template <typename V, int G, bool VEC> __device__ __forceinline__ void ldg(const V *p, int64_t i, V (&o)[G])
{
    if constexpr (VEC) {
        if constexpr (sizeof(V) == 4) {
#pragma unroll
            for (int j = 0; j < G / 4; ++j) {
                const int4 a = reinterpret_cast<const int4 *>(p + i)[j];
                const int w[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
                for (int c = 0; c < 4; ++c) o[4 * j + c] = __builtin_bit_cast(V, w[c]);
            }
        } else {
#pragma unroll
            for (int j = 0; j < G / 2; ++j) {
                const double2 a = reinterpret_cast<const double2 *>(p + i)[j];
                o[2 * j] = a.x; o[2 * j + 1] = a.y;
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < G; ++j) o[j] = p[i + j];
    }
}

template <typename V, int G, bool VEC> __device__ __forceinline__ void stg(V *p, int64_t i, const V (&o)[G])
{
    if constexpr (VEC) {
        if constexpr (sizeof(V) == 4) {
#pragma unroll
            for (int j = 0; j < G / 4; ++j)
                reinterpret_cast<int4 *>(p + i)[j] = make_int4(__builtin_bit_cast(int, o[4 * j]), __builtin_bit_cast(int, o[4 * j + 1]),
                                                               __builtin_bit_cast(int, o[4 * j + 2]), __builtin_bit_cast(int, o[4 * j + 3]));
        } else {
#pragma unroll
            for (int j = 0; j < G / 2; ++j) reinterpret_cast<double2 *>(p + i)[j] = make_double2(o[2 * j], o[2 * j + 1]);
        }
    } else {
#pragma unroll
        for (int j = 0; j < G; ++j) p[i + j] = o[j];
    }
}

// bit j set: entry i + j is observed
template <typename R, int G, bool VEC> __device__ __forceinline__ unsigned seen_bits(const R (&o)[G], const uint8_t *mask, int64_t i)
{
    unsigned bits = 0;
    if (mask) {
        if constexpr (VEC) {
            const uint32_t *p = reinterpret_cast<const uint32_t *>(mask + i);
#pragma unroll
            for (int j = 0; j < G; ++j) bits |= (seen(o[j], (p[j / 4] >> (8 * (j % 4))) & 0xffu) ? 1u : 0u) << j;
        } else {
#pragma unroll
            for (int j = 0; j < G; ++j) bits |= (seen(o[j], mask[i + j]) ? 1u : 0u) << j;
        }
    } else {
#pragma unroll
        for (int j = 0; j < G; ++j) bits |= (seen(o[j], 1u) ? 1u : 0u) << j;
    }
    return bits;
}

struct EntryState {
    int32_t n;
    double mean, m2, pit, lmax, lsum;
};

// ONE draw into ONE entry.  Contraction is off: the update is the same arithmetic whether the draw is the first of a call, in the
// middle of a batch of in-flight loads or in the remainder loop, and it is what tests/_predictive_reference.py restates.
__device__ __forceinline__ void fold_one(EntryState &e, double yv, bool on, double ov, bool noise, double sig, double log_sig)
{
#pragma clang fp contract(off)
    if (!__builtin_isfinite(yv)) return;
    e.n += 1;
    const double d = yv - e.mean;
    e.mean += d / (double)e.n;
    e.m2 += d * (yv - e.mean);
    if (!on) return;
    if (noise && sig > 0.0) {
        const double z = (ov - yv) / sig;
        e.pit += 0.5 * erfc(-z * kInvSqrt2);
        const double lp = -0.5 * z * z - log_sig - kHalfLog2Pi;
        if (lp > e.lmax) {
            e.lsum = e.lsum * exp(e.lmax - lp) + 1.0;
            e.lmax = lp;
        } else {
            e.lsum += exp(lp - e.lmax);
        }
    } else {
        e.pit += yv < ov ? 1.0 : (yv == ov ? 0.5 : 0.0);
    }
}

// One lane, one entry, all draws of the call.  The update chain of an entry is serial in the draws, so the parallelism of a
// fold is its number of entries: a lane takes ONE (twelve per lane, the layout of hode_obs.hip, left 31 workgroups for 256 CUs
// at 64 x 241 x 6 entries and measured 6.5 times slower).  A wave's load of a draw is 64 consecutive
// reals, whole cache lines whatever the alignment of y, so there is one path for every N and every pointer.
template <typename R> __global__ __launch_bounds__(kThreads) void pred_fold_kernel(const FoldArgs<R> a)
{
    constexpr int kFly = 16;                           // draws whose loads are in flight together
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= a.N) return;
    EntryState e{a.n[i], a.mean[i], a.m2[i], a.pit[i], a.lmax[i], a.lsum[i]};
    const int k = (int)(i % 6);
    const int64_t tr = i / a.row_len;
    const double ov = a.obs ? (double)a.obs[i] : 0.0;
    const bool on = a.obs && seen(a.obs[i], a.mask ? (unsigned)a.mask[i] : 1u);
    const bool noise = a.sigma != nullptr;

    auto take = [&](int s, R yv, int32_t st) {
        if (st != 0) return;                                                   // a failed trajectory is skipped whole
        const double sig = noise ? a.sigma[6 * (int64_t)s + k] : 0.0;
        fold_one(e, (double)yv, on, ov, noise, sig, sig > 0.0 ? log(sig) : 0.0);
    };

    int s = 0;
    for (; s + kFly <= a.n_draws; s += kFly) {
        R yv[kFly];
        int32_t st[kFly];
#pragma unroll
        for (int f = 0; f < kFly; ++f) {
            yv[f] = a.y[(int64_t)(s + f) * a.N + i];
            st[f] = a.status ? a.status[(int64_t)(s + f) * a.n_traj + tr] : 0;
        }
#pragma unroll
        for (int f = 0; f < kFly; ++f) take(s + f, yv[f], st[f]);
    }
    for (; s < a.n_draws; ++s) take(s, a.y[(int64_t)s * a.N + i], a.status ? a.status[(int64_t)s * a.n_traj + tr] : 0);

    a.n[i] = e.n; a.mean[i] = e.mean; a.m2[i] = e.m2;
    if (a.obs) {                                       // without observations these three are never written
        a.pit[i] = e.pit; a.lmax[i] = e.lmax; a.lsum[i] = e.lsum;
    }
}

inline bool aligned16(std::initializer_list<const void *> ptrs)
{
    for (const void *p : ptrs)
        if (p && ((uintptr_t)p & 15)) return false;
    return true;
}

template <typename R>
int pred_fold(void *stream, int n_draws, int64_t N, const R *y, const R *obs, const uint8_t *mask, const double *sigma,
              const int32_t *status, int64_t row_len, int32_t *n, double *mean, double *m2, double *pit, double *lmax, double *lsum)
{
    if (n_draws < 0 || N < 6 || N % 6 || !n || !mean || !m2 || !pit || !lmax || !lsum) return HODE_EINVAL;
    if (n_draws > 0 && !y) return HODE_EINVAL;
    if (mask && !obs) return HODE_EINVAL;
    if (status && (row_len < 6 || row_len % 6 || N % row_len)) return HODE_EINVAL;
    if (n_draws > 0 && N > (((int64_t)1 << 62) / n_draws)) return HODE_EINVAL;          // draw * N stays inside int64
    if (n_draws == 0) return HODE_OK;
    FoldArgs<R> a{};
    a.n_draws = n_draws; a.N = N; a.row_len = status ? row_len : N; a.n_traj = N / a.row_len;
    a.y = y; a.obs = obs; a.mask = mask; a.sigma = sigma; a.status = status;
    a.n = n; a.mean = mean; a.m2 = m2; a.pit = pit; a.lmax = lmax; a.lsum = lsum;
    const int64_t blocks = (N + kThreads - 1) / kThreads;
    if (blocks > 0x7fffffff) return HODE_EUNSUPPORTED;
    hipLaunchKernelGGL((pred_fold_kernel<R>), dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, a);
    return done();
}

// ------------------------------------------------------------------------------------------------------------ score
template <typename R> struct ScoreArgs {
    int64_t N;
    const int32_t *n;
    const double *mean, *m2, *pit, *lmax, *lsum;
    const R *obs;
    const uint8_t *mask;
    double extra_var[6];
    double thr[HODE_PRED_MAX_BINS];
    int n_bins, K;
    R *out_mean, *out_sd, *out_pit;
    double *table, *work;
};

// the lane's sums: nine fp64 columns and seven counts per state (the columns of include/hode.h in their order)
struct LaneSums {
    double s[6][9];
    int c[6][7];
};

template <typename R, int G, bool VEC>
__device__ __forceinline__ void score_entries(const ScoreArgs<R> &a, int64_t i0, LaneSums &L, unsigned *hist)
{
    int32_t n[G];
    double mean[G], m2[G], pit[G], lmax[G], lsum[G];
    R ob[G], om[G], os[G], op[G];
    ldg<int32_t, G, VEC>(a.n, i0, n);
    ldg<double, G, VEC>(a.mean, i0, mean);
    ldg<double, G, VEC>(a.m2, i0, m2);
    ldg<double, G, VEC>(a.pit, i0, pit);
    ldg<double, G, VEC>(a.lmax, i0, lmax);
    ldg<double, G, VEC>(a.lsum, i0, lsum);
    unsigned on = 0;
    if (a.obs) {
        ldg<R, G, VEC>(a.obs, i0, ob);
        on = seen_bits<R, G, VEC>(ob, a.mask, i0);
    } else {
#pragma unroll
        for (int j = 0; j < G; ++j) ob[j] = R(0);
    }
    const double nan = __builtin_nan("");
#pragma unroll
    for (int j = 0; j < G; ++j) {
        const int k = j % 6;                                                   // compile-time after unrolling
        const bool seen_j = (on >> j) & 1u;
        const int cnt = n[j];
        const double mu = cnt >= 1 ? mean[j] : nan;
        const double sd = cnt >= 2 ? sqrt(m2[j] / (double)(cnt - 1) + a.extra_var[k]) : nan;
        const double pv = (cnt >= 2 && seen_j) ? pit[j] / (double)cnt : nan;
        om[j] = (R)mu; os[j] = (R)sd; op[j] = (R)pv;
        if (!seen_j || cnt < 1) continue;
        const double o = (double)ob[j], e = mu - o, ae = fabs(e);
        L.c[k][0] += 1;
        L.s[k][0] += e * e;
        L.s[k][1] += ae;
        L.s[k][2] += o;
        L.s[k][3] += o * o;
        if (cnt < 2) continue;
        const double ne = ae / (sd + 1e-6);
        const double lo = mu - 1.96 * sd, hi = mu + 1.96 * sd;
        L.c[k][1] += 1;
        L.s[k][4] += sd;
        L.s[k][5] += ne;
        L.s[k][6] += (hi - lo) + (2.0 / 0.05) * ((o < lo ? lo - o : 0.0) + (o > hi ? o - hi : 0.0));
        L.c[k][2] += (o >= mu - 0.6744897501960817 * sd && o <= mu + 0.6744897501960817 * sd) ? 1 : 0;
        L.c[k][3] += (o >= mu - 1.2815515655446004 * sd && o <= mu + 1.2815515655446004 * sd) ? 1 : 0;
        L.c[k][4] += (o >= mu - 1.6448536269514722 * sd && o <= mu + 1.6448536269514722 * sd) ? 1 : 0;
        L.c[k][5] += (o >= lo && o <= hi) ? 1 : 0;
        if (sd > 0.0) {                                                        // Gaussian CRPS (Gneiting & Raftery 2007, eq. 21)
            const double w = (o - mu) / sd;
            L.s[k][7] += sd * (w * (1.0 - erfc(w * kInvSqrt2)) + 2.0 * kInvSqrt2Pi * exp(-0.5 * w * w) - kInvSqrtPi);
        } else {
            L.s[k][7] += ae;
        }
        if (lsum[j] > 0.0) {
            L.s[k][8] += lmax[j] + log(lsum[j] / (double)cnt);
            L.c[k][6] += 1;
        }
        unsigned *h = hist + k * 2 * a.n_bins;
        for (int b = 0; b < a.n_bins; ++b)
            if (ne <= a.thr[b]) atomicAdd(h + b, 1u);
        int bin = (int)(pv * (double)a.n_bins);
        bin = bin < 0 ? 0 : (bin > a.n_bins - 1 ? a.n_bins - 1 : bin);
        atomicAdd(h + a.n_bins + bin, 1u);
    }
    stg<R, G, VEC>(a.out_mean, i0, om);
    stg<R, G, VEC>(a.out_sd, i0, os);
    stg<R, G, VEC>(a.out_pit, i0, op);
}

template <typename R, bool VEC> __global__ __launch_bounds__(kThreads) void pred_score_kernel(const ScoreArgs<R> a)
{
    __shared__ double sh[24];
    __shared__ unsigned hist[6 * 2 * HODE_PRED_MAX_BINS];
    for (int i = threadIdx.x; i < 6 * 2 * a.n_bins; i += kThreads) hist[i] = 0u;
    __syncthreads();
    LaneSums L;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
#pragma unroll
        for (int c = 0; c < 9; ++c) L.s[k][c] = 0.0;
#pragma unroll
        for (int c = 0; c < 7; ++c) L.c[k][c] = 0;
    }
    const int64_t units = VEC ? a.N / 12 : a.N / 6;
    for (int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x; g < units; g += (int64_t)gridDim.x * kThreads) {
        if (VEC) score_entries<R, 12, true>(a, 12 * g, L, hist);
        else score_entries<R, 6, false>(a, 6 * g, L, hist);
    }
    // block sums, column by column, each in the order of block_sum6; the row of this workgroup: work[block][6][K]
    double *row = a.work + (int64_t)blockIdx.x * 6 * a.K;
    // table column of the nine fp64 sums and of the seven counts
    constexpr int scol[9] = {1, 2, 3, 4, 6, 7, 8, 13, 14};
    constexpr int ccol[7] = {0, 5, 9, 10, 11, 12, 15};
#pragma unroll
    for (int c = 0; c < 9; ++c) {
        double v[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) v[k] = L.s[k][c];
        block_sum6(v, sh);
        if (threadIdx.x == 0) {
#pragma unroll
            for (int k = 0; k < 6; ++k) row[k * a.K + scol[c]] = v[k];
        }
    }
#pragma unroll
    for (int c = 0; c < 7; ++c) {
        double v[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) v[k] = (double)L.c[k][c];
        block_sum6(v, sh);
        if (threadIdx.x == 0) {
#pragma unroll
            for (int k = 0; k < 6; ++k) row[k * a.K + ccol[c]] = v[k];
        }
    }
    for (int i = threadIdx.x; i < 6 * 2 * a.n_bins; i += kThreads)
        row[(i / (2 * a.n_bins)) * a.K + kFixedCols + i % (2 * a.n_bins)] = (double)hist[i];
}

template <typename R>
int pred_score(void *stream, int64_t N, const int32_t *n, const double *mean, const double *m2, const double *pit, const double *lmax,
               const double *lsum, const R *obs, const uint8_t *mask, const double *extra_var, const double *thr, int n_bins,
               R *out_mean, R *out_sd, R *out_pit, double *table, double *work)
{
    if (N < 6 || N % 6 || n_bins < 1 || n_bins > HODE_PRED_MAX_BINS) return HODE_EINVAL;
    if (!n || !mean || !m2 || !pit || !lmax || !lsum || !thr || !out_mean || !out_sd || !out_pit || !table || !work) return HODE_EINVAL;
    if (mask && !obs) return HODE_EINVAL;
    ScoreArgs<R> a{};
    a.N = N; a.n = n; a.mean = mean; a.m2 = m2; a.pit = pit; a.lmax = lmax; a.lsum = lsum; a.obs = obs; a.mask = mask;
    for (int k = 0; k < 6; ++k) a.extra_var[k] = extra_var ? extra_var[k] : 0.0;
    for (int b = 0; b < n_bins; ++b) a.thr[b] = thr[b];
    a.n_bins = n_bins; a.K = kFixedCols + 2 * n_bins;
    a.out_mean = out_mean; a.out_sd = out_sd; a.out_pit = out_pit; a.table = table; a.work = work;
    const bool vec = N % 4 == 0 && aligned16({n, mean, m2, pit, lmax, lsum, obs, out_mean, out_sd, out_pit}) && (((uintptr_t)mask & 3) == 0);
    const int64_t units = vec ? N / 12 : N / 6;
    const int64_t want = (units + kThreads - 1) / kThreads;
    const int blocks = (int)(want < kScoreBlocks ? want : kScoreBlocks);
    if (vec) hipLaunchKernelGGL((pred_score_kernel<R, true>), dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL((pred_score_kernel<R, false>), dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(pred_score_finish_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, blocks, 6 * a.K, work, table);
    return done();
}

// ------------------------------------------------------------------------------------------------------------ tails
// The K smallest and the K largest values of every entry across the draws: what an empirical tail quantile needs of them.
// lo[K][N] is a binary max-heap of the smallest values taken (its root, slot 0, the largest of them: the threshold a new value
// must be below to enter), hi[K][N] a min-heap of the largest; slot j of entry i is at j * N + i, so the lanes of a wave touch
// consecutive addresses at the same depth.  Values are copied and compared with <, never computed with.
template <typename R> struct TailArgs {
    int n_draws;
    int64_t N, row_len, n_traj, K;
    const R *y;
    const int32_t *status;
    int32_t *cnt;
    R *lo, *hi;
};

// One lane, one entry, all draws of the call, as pred_fold_kernel.  cnt and the two roots stay in registers; a draw that
// passes neither root (all but about K (1 + ln(S / K)) of S draws per tail) costs its load and two compares.
template <typename R> __global__ __launch_bounds__(kThreads) void pred_tails_kernel(const TailArgs<R> a)
{
    constexpr int kFly = 16;                           // draws whose loads are in flight together
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= a.N) return;
    const int64_t tr = i / a.row_len;
    int32_t cnt = a.cnt[i];
    R top_lo = cnt > 0 ? a.lo[i] : R(0), top_hi = cnt > 0 ? a.hi[i] : R(0);

    auto take = [&](R v, int32_t st) {
        if (st != 0 || !__builtin_isfinite(v)) return;
        const bool filling = cnt < a.K;                                        // both buffers still take everything
        unsigned need = filling ? 3u : ((v < top_lo ? 1u : 0u) | (top_hi < v ? 2u : 0u));          // bit 0: into lo, bit 1: into hi
        while (need) {                                 // ONE loop for both buffers: a lane in lo and a lane in hi walk together
            const bool max = need & 1u;
            R *h = max ? a.lo : a.hi;
            const R top = max ? top_lo : top_hi;
            R root;
            if (filling) {
                sift_up(h, max, a.N, i, cnt, v);
                root = (cnt == 0 || below(max, top, v)) ? v : top;
            } else {
                root = sift_down(h, max, a.N, i, a.K, v);
            }
            if (max) top_lo = root;
            else top_hi = root;
            need &= max ? 2u : 0u;
        }
        cnt += 1;
    };

    int s = 0;
    for (; s + kFly <= a.n_draws; s += kFly) {
        R yv[kFly];
        int32_t st[kFly];
#pragma unroll
        for (int f = 0; f < kFly; ++f) {
            yv[f] = a.y[(int64_t)(s + f) * a.N + i];
            st[f] = a.status ? a.status[(int64_t)(s + f) * a.n_traj + tr] : 0;
        }
#pragma unroll
        for (int f = 0; f < kFly; ++f) take(yv[f], st[f]);
    }
    for (; s < a.n_draws; ++s) take(a.y[(int64_t)s * a.N + i], a.status ? a.status[(int64_t)s * a.n_traj + tr] : 0);
    a.cnt[i] = cnt;
}

template <typename R>
int pred_tails(void *stream, int n_draws, int64_t N, const R *y, const int32_t *status, int64_t row_len, int64_t K, int32_t *cnt, R *lo,
               R *hi)
{
    if (n_draws < 0 || N < 1 || K < 1 || !cnt || !lo || !hi) return HODE_EINVAL;
    if (n_draws > 0 && !y) return HODE_EINVAL;
    if (status && (row_len < 1 || N % row_len)) return HODE_EINVAL;
    if ((n_draws > 0 && N > (((int64_t)1 << 62) / n_draws)) || N > (((int64_t)1 << 62) / K)) return HODE_EINVAL;   // inside int64
    if (n_draws == 0) return HODE_OK;
    TailArgs<R> a{};
    a.n_draws = n_draws; a.N = N; a.row_len = status ? row_len : N; a.n_traj = N / a.row_len; a.K = K;
    a.y = y; a.status = status; a.cnt = cnt; a.lo = lo; a.hi = hi;
    const int64_t blocks = (N + kThreads - 1) / kThreads;
    if (blocks > 0x7fffffff) return HODE_EUNSUPPORTED;
    hipLaunchKernelGGL((pred_tails_kernel<R>), dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, a);
    return done();
}

// -------------------------------------------------------------------------------------------------------- quantiles
template <typename R> struct QuantArgs {
    int64_t N, K;
    const int32_t *cnt;
    R *lo, *hi;
    int n_levels;
    double levels[HODE_PRED_MAX_LEVELS];
    R *out;
};

// One lane, one entry: sort both buffers, then numpy's "linear" quantile of every level from the nearer one.
template <typename R> __global__ __launch_bounds__(kThreads) void pred_quantiles_kernel(const QuantArgs<R> a)
{
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= a.N) return;
    const int64_t n = a.cnt[i], m = n < a.K ? n : a.K;
    sort_heap(a.lo, true, a.N, i, m);
    sort_heap(a.hi, false, a.N, i, m);
    for (int l = 0; l < a.n_levels; ++l) {
        const double q = a.levels[l];
        double r = __builtin_nan("");
        if (n > 0) {
            const double h = q * (double)(n - 1), fj = floor(h), g = h - fj;
            const int64_t j = (int64_t)fj, jb = j + 1 < n - 1 ? j + 1 : n - 1;
            if (q <= 0.5) {                            // rank r (ascending) is slot m - 1 - r of lo
                if (jb < m) {
                    const double va = (double)a.lo[(m - 1 - j) * a.N + i], vb = (double)a.lo[(m - 1 - jb) * a.N + i];
                    r = va + (vb - va) * g;
                }
            } else {                                   // rank r is slot r - (n - m) of hi
                if (j >= n - m) {
                    const double va = (double)a.hi[(j - (n - m)) * a.N + i], vb = (double)a.hi[(jb - (n - m)) * a.N + i];
                    r = va + (vb - va) * g;
                }
            }
        }
        a.out[(int64_t)l * a.N + i] = (R)r;
    }
}

template <typename R> struct BandArgs {
    int64_t N;
    const int32_t *cnt;
    const R *qlo, *qhi, *obs;
    const uint8_t *mask;
    double two_over_alpha;
    double *work;
};

// per-state sums of the band [qlo, qhi] against the observations, a lane taking rows of six entries (the state a compile-time
// index), reduced as pred_score_kernel reduces: work[block][6][4]
template <typename R> __global__ __launch_bounds__(kThreads) void pred_band_kernel(const BandArgs<R> a)
{
#pragma clang fp contract(off)
    __shared__ double sh[24];
    double s[6][2];
    int c[6][2];
#pragma unroll
    for (int k = 0; k < 6; ++k) s[k][0] = s[k][1] = 0.0, c[k][0] = c[k][1] = 0;
    for (int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x; g < a.N / 6; g += (int64_t)gridDim.x * kThreads) {
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const int64_t i = 6 * g + k;
            const R ob = a.obs[i];
            if (!seen(ob, a.mask ? (unsigned)a.mask[i] : 1u) || a.cnt[i] < 2) continue;
            const double lo = (double)a.qlo[i], hi = (double)a.qhi[i], o = (double)ob;
            if (!__builtin_isfinite(lo) || !__builtin_isfinite(hi)) continue;
            c[k][0] += 1;
            s[k][0] += hi - lo;
            c[k][1] += (lo <= o && o <= hi) ? 1 : 0;
            s[k][1] += (hi - lo) + a.two_over_alpha * ((o < lo ? lo - o : 0.0) + (o > hi ? o - hi : 0.0));
        }
    }
    double *row = a.work + (int64_t)blockIdx.x * 6 * HODE_PRED_BAND_COLS;
#pragma unroll
    for (int col = 0; col < HODE_PRED_BAND_COLS; ++col) {
        double v[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) v[k] = (col & 1) ? s[k][col >> 1] : (double)c[k][col >> 1];
        block_sum6(v, sh);
        if (threadIdx.x == 0) {
#pragma unroll
            for (int k = 0; k < 6; ++k) row[k * HODE_PRED_BAND_COLS + col] = v[k];
        }
    }
}

template <typename R>
int pred_quantiles(void *stream, int64_t N, int64_t K, const int32_t *cnt, R *lo, R *hi, int n_levels, const double *levels, R *out,
                   const R *obs, const uint8_t *mask, double *band_table, double *work)
{
    if (N < 1 || K < 1 || !cnt || !lo || !hi || !levels || !out || n_levels < 1 || n_levels > HODE_PRED_MAX_LEVELS) return HODE_EINVAL;
    if (N > (((int64_t)1 << 62) / K) || N > (((int64_t)1 << 62) / n_levels)) return HODE_EINVAL;
    for (int l = 0; l < n_levels; ++l)
        if (!(levels[l] > 0.0 && levels[l] < 1.0) || (l > 0 && !(levels[l - 1] < levels[l]))) return HODE_EINVAL;
    if (mask && !obs) return HODE_EINVAL;
    if (band_table && (N % 6 || !obs || !work || n_levels < 2 || !(levels[0] < 0.5 && 0.5 < levels[n_levels - 1]))) return HODE_EINVAL;
    QuantArgs<R> a{};
    a.N = N; a.K = K; a.cnt = cnt; a.lo = lo; a.hi = hi; a.n_levels = n_levels; a.out = out;
    for (int l = 0; l < n_levels; ++l) a.levels[l] = levels[l];
    const int64_t blocks = (N + kThreads - 1) / kThreads;
    if (blocks > 0x7fffffff) return HODE_EUNSUPPORTED;
    hipLaunchKernelGGL((pred_quantiles_kernel<R>), dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, a);
    if (band_table) {
        BandArgs<R> b{};
        b.N = N; b.cnt = cnt; b.qlo = out; b.qhi = out + (int64_t)(n_levels - 1) * N; b.obs = obs; b.mask = mask; b.work = work;
        b.two_over_alpha = 2.0 / (1.0 - (levels[n_levels - 1] - levels[0]));
        const int64_t want = (N / 6 + kThreads - 1) / kThreads;
        const int nb = (int)(want < kScoreBlocks ? want : kScoreBlocks);
        hipLaunchKernelGGL((pred_band_kernel<R>), dim3(nb), dim3(kThreads), 0, (hipStream_t)stream, b);
        hipLaunchKernelGGL(pred_score_finish_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, nb, 6 * HODE_PRED_BAND_COLS, work,
                           band_table);
    }
    return done();
}

}  // namespace
}  // namespace hode

extern "C" {

int hode_pred_fold_f32(void *stream, int n_draws, int64_t N, const float *y, const float *obs, const uint8_t *mask, const double *sigma,
                       const int32_t *status, int64_t row_len, int32_t *n, double *mean, double *m2, double *pit, double *lmax,
                       double *lsum)
{
    return hode::pred_fold<float>(stream, n_draws, N, y, obs, mask, sigma, status, row_len, n, mean, m2, pit, lmax, lsum);
}
int hode_pred_fold_f64(void *stream, int n_draws, int64_t N, const double *y, const double *obs, const uint8_t *mask, const double *sigma,
                       const int32_t *status, int64_t row_len, int32_t *n, double *mean, double *m2, double *pit, double *lmax,
                       double *lsum)
{
    return hode::pred_fold<double>(stream, n_draws, N, y, obs, mask, sigma, status, row_len, n, mean, m2, pit, lmax, lsum);
}
int hode_pred_score_f32(void *stream, int64_t N, const int32_t *n, const double *mean, const double *m2, const double *pit,
                        const double *lmax, const double *lsum, const float *obs, const uint8_t *mask, const double *extra_var,
                        const double *thr, int n_bins, float *out_mean, float *out_sd, float *out_pit, double *table, double *work)
{
    return hode::pred_score<float>(stream, N, n, mean, m2, pit, lmax, lsum, obs, mask, extra_var, thr, n_bins, out_mean, out_sd, out_pit,
                                   table, work);
}
int hode_pred_score_f64(void *stream, int64_t N, const int32_t *n, const double *mean, const double *m2, const double *pit,
                        const double *lmax, const double *lsum, const double *obs, const uint8_t *mask, const double *extra_var,
                        const double *thr, int n_bins, double *out_mean, double *out_sd, double *out_pit, double *table, double *work)
{
    return hode::pred_score<double>(stream, N, n, mean, m2, pit, lmax, lsum, obs, mask, extra_var, thr, n_bins, out_mean, out_sd, out_pit,
                                    table, work);
}
int hode_pred_tails_f32(void *stream, int n_draws, int64_t N, const float *y, const int32_t *status, int64_t row_len, int K, int32_t *cnt,
                        float *lo, float *hi)
{
    return hode::pred_tails<float>(stream, n_draws, N, y, status, row_len, K, cnt, lo, hi);
}
int hode_pred_tails_f64(void *stream, int n_draws, int64_t N, const double *y, const int32_t *status, int64_t row_len, int K, int32_t *cnt,
                        double *lo, double *hi)
{
    return hode::pred_tails<double>(stream, n_draws, N, y, status, row_len, K, cnt, lo, hi);
}
int hode_pred_quantiles_f32(void *stream, int64_t N, int K, const int32_t *cnt, float *lo, float *hi, int n_levels, const double *levels,
                            float *out, const float *obs, const uint8_t *mask, double *band_table, double *work)
{
    return hode::pred_quantiles<float>(stream, N, K, cnt, lo, hi, n_levels, levels, out, obs, mask, band_table, work);
}
int hode_pred_quantiles_f64(void *stream, int64_t N, int K, const int32_t *cnt, double *lo, double *hi, int n_levels, const double *levels,
                            double *out, const double *obs, const uint8_t *mask, double *band_table, double *work)
{
    return hode::pred_quantiles<double>(stream, N, K, cnt, lo, hi, n_levels, levels, out, obs, mask, band_table, work);
}

}  // extern "C"

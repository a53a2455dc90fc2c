// hode_loo.hip -- model comparison folded draw by draw: PSIS-LOO and WAIC of the pointwise log likelihood
// (inference/predictive.py `loo=`, inference.compare; include/hode.h, "Model comparison").
//
// l = log N(obs | y, sigma_k^2) of one draw at one observed entry is the arithmetic of pred_fold (hode_predictive.hip), and
// r = -l is the log importance ratio of leaving that observation out.
//   pred_loo_fold    a lane OWNS one entry as in pred_fold / pred_tails: it keeps the count, Welford's mean and m2 of l, the
//                    streaming log-sum-exp of l, the streaming log-sum-exp of every r that is NOT among the K largest, and the
//                    root of a min-heap top[K][N] of the K largest r in registers, and takes the draws one at a time in draw
//                    order.  A draw's r goes into the heap or into the running sum, never both, and what the heap evicts
//                    goes into the sum: no subtraction ever forms the sum of the non-tail ratios.
//   pred_loo_finish  one lane, one entry: sorts the heap in place (ascending, still a heap), fits the generalised Pareto
//                    distribution to the M largest ratios (Zhang & Stephens 2009, with the weakly informative prior of
//                    Vehtari et al. 2024), replaces them by the fitted quantiles, and forms elpd_loo in log space.  The
//                    per-entry intermediates (the tail a_j, then its smoothed values; the m profile likelihoods L_q) live
//                    in a caller-provided buffer fit[rows][N] in global memory, slot-major like the heap: nothing here is a
//                    run-time-indexed array in registers.  The five results are also left in fp64 in fit[0..4][N];
//   pred_loo_table   reduces them to the per-state table as pred_band_kernel does: a lane takes rows of six entries (the state
//                    a compile-time index), block sums in the order of block_sum6, one partial row per workgroup, and
//                    pred_score_finish_kernel adds the rows in index order.
// There are no atomics in this file: the same call gives the same bits.
#include <cfloat>

#include "hode_pred_heap.h"

namespace hode {
namespace {

constexpr int kLooCols = HODE_PRED_LOO_COLS;
constexpr int kLooBlocks = HODE_PRED_SCORE_BLOCKS;

template <typename R> struct LooFoldArgs {
    int n_draws;
    int64_t N, row_len, n_traj, K;
    const R *y, *obs;
    const uint8_t *mask;
    const double *sigma;
    const int32_t *status;
    int32_t *cnt;
    double *lmean, *lm2, *pmax, *psum, *top, *rmax, *rsum;
};

// v into a streaming log-sum-exp {mx, sm}: sum_j exp(v_j) = exp(mx) sm
__device__ __forceinline__ void lse_add(double &mx, double &sm, double v)
{
#pragma clang fp contract(off)
    if (v > mx) {
        sm = sm * exp(mx - v) + 1.0;
        mx = v;
    } else {
        sm += exp(v - mx);
    }
}

// One lane, one entry, all draws of the call.  An entry that is not observed never produces an l: its lane leaves at once.
template <typename R> __global__ __launch_bounds__(kThreads) void pred_loo_fold_kernel(const LooFoldArgs<R> a)
{
    constexpr int kFly = 16;                           // draws whose loads are in flight together
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= a.N) return;
    if (!seen(a.obs[i], a.mask ? (unsigned)a.mask[i] : 1u)) return;
    const double ov = (double)a.obs[i];
    const int k = (int)(i % 6);
    const int64_t tr = i / a.row_len;
    int32_t cnt = a.cnt[i];
    double lmean = a.lmean[i], lm2 = a.lm2[i], pmax = a.pmax[i], psum = a.psum[i], rmax = a.rmax[i], rsum = a.rsum[i];
    double root = cnt > 0 ? a.top[i] : 0.0;

    auto take = [&](int s, R yr, int32_t st) {
#pragma clang fp contract(off)
        const double yv = (double)yr;
        if (st != 0 || !__builtin_isfinite(yv)) return;                        // the skip rules of pred_fold
        const double sig = a.sigma[6 * (int64_t)s + k];
        if (!(sig > 0.0)) return;                                              // no observation noise, no likelihood
        const double z = (ov - yv) / sig;
        const double l = -0.5 * z * z - log(sig) - kHalfLog2Pi;                // fold_one's lp, operation for operation
        const double r = -l;
        const double d = l - lmean;
        lmean += d / (double)(cnt + 1);
        lm2 += d * (l - lmean);
        lse_add(pmax, psum, l);
        if (cnt < a.K) {
            sift_up(a.top, false, a.N, i, (int64_t)cnt, r);
            root = (cnt == 0 || r < root) ? r : root;
        } else if (root < r) {
            const double out = root;
            root = sift_down(a.top, false, a.N, i, a.K, r);
            lse_add(rmax, rsum, out);
        } else {
            lse_add(rmax, rsum, r);
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
        for (int f = 0; f < kFly; ++f) take(s + f, yv[f], st[f]);
    }
    for (; s < a.n_draws; ++s) take(s, a.y[(int64_t)s * a.N + i], a.status ? a.status[(int64_t)s * a.n_traj + tr] : 0);

    a.cnt[i] = cnt; a.lmean[i] = lmean; a.lm2[i] = lm2; a.pmax[i] = pmax; a.psum[i] = psum; a.rmax[i] = rmax; a.rsum[i] = rsum;
}

template <typename R>
int pred_loo_fold(void *stream, int n_draws, int64_t N, const R *y, const R *obs, const uint8_t *mask, const double *sigma,
                  const int32_t *status, int64_t row_len, int K, int32_t *cnt, double *lmean, double *lm2, double *pmax, double *psum,
                  double *top, double *rmax, double *rsum)
{
    if (n_draws < 0 || N < 6 || N % 6 || K < 2) return HODE_EINVAL;
    if (!cnt || !lmean || !lm2 || !pmax || !psum || !top || !rmax || !rsum || !obs || !sigma) return HODE_EINVAL;
    if (n_draws > 0 && !y) return HODE_EINVAL;
    if (status && (row_len < 6 || row_len % 6 || N % row_len)) return HODE_EINVAL;
    if ((n_draws > 0 && N > (((int64_t)1 << 62) / n_draws)) || N > (((int64_t)1 << 62) / K)) return HODE_EINVAL;   // inside int64
    if (n_draws == 0) return HODE_OK;
    LooFoldArgs<R> a{};
    a.n_draws = n_draws; a.N = N; a.row_len = status ? row_len : N; a.n_traj = N / a.row_len; a.K = K;
    a.y = y; a.obs = obs; a.mask = mask; a.sigma = sigma; a.status = status;
    a.cnt = cnt; a.lmean = lmean; a.lm2 = lm2; a.pmax = pmax; a.psum = psum; a.top = top; a.rmax = rmax; a.rsum = rsum;
    const int64_t blocks = (N + kThreads - 1) / kThreads;
    if (blocks > 0x7fffffff) return HODE_EUNSUPPORTED;
    hipLaunchKernelGGL((pred_loo_fold_kernel<R>), dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, a);
    return done();
}

// ----------------------------------------------------------------------------------------------------------- finish
template <typename R> struct LooFinishArgs {
    int64_t N, K, L0;                                  // L0: the first row of fit that holds an L_q (the rows before it: the tail)
    double r_eff;
    const int32_t *cnt;
    const double *lmean, *lm2, *pmax, *psum, *rmax, *rsum;
    double *top, *fit;
    R *elpd_loo, *pareto_k, *elpd_waic, *p_waic, *lppd;
};

// the rows of fit a state of K slots needs: K - 1 for the tail (M <= K - 1) and 30 + floor(sqrt(K - 1)) for the L_q
inline int64_t loo_fit_rows(int64_t K)
{
    int64_t s = 0;
    while ((s + 1) * (s + 1) <= K - 1) ++s;
    return (K - 1) + 30 + s;
}

template <typename R> __global__ __launch_bounds__(kThreads) void pred_loo_finish_kernel(const LooFinishArgs<R> a)
{
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= a.N) return;
    const int64_t N = a.N;
    const int64_t n = a.cnt[i], h = n < a.K ? n : a.K;
    double *top = a.top, *fit = a.fit;
    sort_heap(top, false, N, i, h);                    // ascending: slot h - 1 is the largest ratio
    const double nan = __builtin_nan(""), inf = __builtin_inf();
    const double dn = (double)n;
    const double fm = ceil(fmin(dn / 5.0, 3.0 * sqrt(dn / a.r_eff)));
    double elpd = nan, kh = nan, ewaic = nan, pwaic = nan, lppd = nan;
    if (n >= 2 && fm + 1.0 <= (double)h) {
        const int64_t M = (int64_t)fm;
        const double c = top[(h - 1) * N + i];
        const double x_cut = fmax(top[(h - 1 - M) * N + i] - c, log(DBL_MIN));
        const double e_cut = exp(x_cut);
        int64_t t = 0;                                 // held values strictly above the cut: slots h - t .. h - 1
        while (t < M && top[(h - 1 - t) * N + i] - c > x_cut) ++t;
        const int64_t t0 = h - t;
        const double dt = (double)t;
        kh = inf;
        bool smooth = false;
        double sigma = 0.0;
        if (t > 4) {
            // the tail above the cut, ascending: a_j at fit[j - 1]
            for (int64_t j = 0; j < t; ++j) fit[j * N + i] = exp(top[(t0 + j) * N + i] - c) - e_cut;
            const int64_t m = 30 + (int64_t)sqrt(dt);
            const double dm = (double)m;
            const double a_q = fit[((int64_t)(dt / 4.0 + 0.5) - 1) * N + i], a_t = fit[(t - 1) * N + i];
            auto b_of = [&](int64_t q) { return (1.0 - sqrt(dm / ((double)q - 0.5))) / (3.0 * a_q) + 1.0 / a_t; };
            auto k_of = [&](double b) {
                double s = 0.0;
                for (int64_t j = 0; j < t; ++j) s += log1p(-b * fit[j * N + i]);
                return s / dt;
            };
            for (int64_t q = 1; q <= m; ++q) {
                const double b = b_of(q), kq = k_of(b);
                fit[(a.L0 + q - 1) * N + i] = dt * (log(-(b / kq)) - kq - 1.0);
            }
            double sw = 0.0, sb = 0.0;
            for (int64_t q = 1; q <= m; ++q) {
                const double Lq = fit[(a.L0 + q - 1) * N + i];
                double den = 0.0;
                for (int64_t p = 0; p < m; ++p) den += exp(fit[(a.L0 + p) * N + i] - Lq);
                const double w = 1.0 / den;
                if (w >= 10.0 * DBL_EPSILON) {
                    sw += w;
                    sb += w * b_of(q);
                }
            }
            const double b = sb / sw;
            const double kp = k_of(b);
            sigma = -kp / b;
            kh = (dt * kp + 5.0) / (dt + 10.0);
            smooth = __builtin_isfinite(kh) && sigma > 0.0;
        }
        // the tail's log weights, smoothed or as they are, at fit[j - 1]; their maxima for the two log-sum-exps
        const double ln_non = log((double)(n - t)) - c;
        const bool rest = n > h;                       // some ratios are in the running sum and not in the heap
        const double lrest = rest ? a.rmax[i] + log(a.rsum[i]) - c : -inf;
        double nmax = ln_non, dmax = lrest;
        if (t0 > 0) dmax = fmax(dmax, top[(t0 - 1) * N + i] - c);
        for (int64_t j = 0; j < t; ++j) {
            const double rj = top[(t0 + j) * N + i];
            double x = rj - c;
            if (smooth) {
                const double lp = log1p(-((double)j + 0.5) / dt);
                const double at = fabs(kh) < DBL_EPSILON ? -sigma * lp : sigma * expm1(-kh * lp) / kh;
                x = fmin(log(at + e_cut), 0.0);
            }
            fit[j * N + i] = x;
            nmax = fmax(nmax, x - rj);
            dmax = fmax(dmax, x);
        }
        double num = exp(ln_non - nmax), den = rest ? exp(lrest - dmax) : 0.0;
        for (int64_t j = 0; j < t0; ++j) den += exp((top[j * N + i] - c) - dmax);
        for (int64_t j = 0; j < t; ++j) {
            const double x = fit[j * N + i];
            num += exp((x - top[(t0 + j) * N + i]) - nmax);
            den += exp(x - dmax);
        }
        elpd = (nmax + log(num)) - (dmax + log(den));
        lppd = a.pmax[i] + log(a.psum[i] / dn);
        pwaic = a.lm2[i] / (double)(n - 1);
        ewaic = lppd - pwaic;
    }
    a.elpd_loo[i] = (R)elpd; a.pareto_k[i] = (R)kh; a.elpd_waic[i] = (R)ewaic; a.p_waic[i] = (R)pwaic; a.lppd[i] = (R)lppd;
    fit[i] = elpd; fit[N + i] = kh; fit[2 * N + i] = ewaic; fit[3 * N + i] = pwaic; fit[4 * N + i] = lppd;
}

// per-state sums of the five fp64 results in res[5][N] over the scored entries (lppd not NaN): work[block][6][kLooCols]
__global__ __launch_bounds__(kThreads) void pred_loo_table_kernel(int64_t N, const double *res, double *work)
{
#pragma clang fp contract(off)
    __shared__ double sh[24];
    double s[6][7];
    int c[6][6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
#pragma unroll
        for (int j = 0; j < 7; ++j) s[k][j] = 0.0;
#pragma unroll
        for (int j = 0; j < 6; ++j) c[k][j] = 0;
    }
    for (int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x; g < N / 6; g += (int64_t)gridDim.x * kThreads) {
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const int64_t i = 6 * g + k;
            const double lppd = res[4 * N + i];
            if (lppd != lppd) continue;
            const double el = res[i], kh = res[N + i], ew = res[2 * N + i], pw = res[3 * N + i];
            c[k][0] += 1;
            s[k][0] += el; s[k][1] += el * el; s[k][2] += lppd - el;
            s[k][3] += ew; s[k][4] += ew * ew; s[k][5] += pw;
            s[k][6] += lppd;
            c[k][1] += kh <= 0.5 ? 1 : 0;
            c[k][2] += (kh > 0.5 && kh <= 0.7) ? 1 : 0;
            c[k][3] += (kh > 0.7 && kh <= 1.0) ? 1 : 0;
            c[k][4] += kh > 1.0 ? 1 : 0;
            c[k][5] += pw > 0.4 ? 1 : 0;
        }
    }
    double *row = work + (int64_t)blockIdx.x * 6 * kLooCols;
#pragma unroll
    for (int col = 0; col < kLooCols; ++col) {
        double v[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) v[k] = col == 0 ? (double)c[k][0] : (col <= 7 ? s[k][col - 1] : (double)c[k][col - 7]);
        block_sum6(v, sh);
        if (threadIdx.x == 0) {
#pragma unroll
            for (int k = 0; k < 6; ++k) row[k * kLooCols + col] = v[k];
        }
    }
}

template <typename R>
int pred_loo_finish(void *stream, int64_t N, int K, double r_eff, const int32_t *cnt, const double *lmean, const double *lm2,
                    const double *pmax, const double *psum, double *top, const double *rmax, const double *rsum, R *elpd_loo, R *pareto_k,
                    R *elpd_waic, R *p_waic, R *lppd, double *table, double *fit, double *work)
{
    if (N < 6 || N % 6 || K < 2 || !(r_eff > 0.0 && r_eff <= 1.0)) return HODE_EINVAL;
    if (!cnt || !lmean || !lm2 || !pmax || !psum || !top || !rmax || !rsum) return HODE_EINVAL;
    if (!elpd_loo || !pareto_k || !elpd_waic || !p_waic || !lppd || !table || !fit || !work) return HODE_EINVAL;
    const int64_t rows = loo_fit_rows(K);
    if (N > (((int64_t)1 << 62) / rows)) return HODE_EINVAL;
    LooFinishArgs<R> a{};
    a.N = N; a.K = K; a.L0 = K - 1; a.r_eff = r_eff;
    a.cnt = cnt; a.lmean = lmean; a.lm2 = lm2; a.pmax = pmax; a.psum = psum; a.rmax = rmax; a.rsum = rsum; a.top = top; a.fit = fit;
    a.elpd_loo = elpd_loo; a.pareto_k = pareto_k; a.elpd_waic = elpd_waic; a.p_waic = p_waic; a.lppd = lppd;
    const int64_t blocks = (N + kThreads - 1) / kThreads;
    if (blocks > 0x7fffffff) return HODE_EUNSUPPORTED;
    hipLaunchKernelGGL((pred_loo_finish_kernel<R>), dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, a);
    const int64_t want = (N / 6 + kThreads - 1) / kThreads;
    const int nb = (int)(want < kLooBlocks ? want : kLooBlocks);
    hipLaunchKernelGGL(pred_loo_table_kernel, dim3(nb), dim3(kThreads), 0, (hipStream_t)stream, N, (const double *)fit, work);
    hipLaunchKernelGGL(pred_score_finish_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, nb, 6 * kLooCols, work, table);
    return done();
}

}  // namespace
}  // namespace hode

extern "C" {

int hode_pred_loo_fold_f32(void *stream, int n_draws, int64_t N, const float *y, const float *obs, const uint8_t *mask, const double *sigma,
                           const int32_t *status, int64_t row_len, int K, int32_t *cnt, double *lmean, double *lm2, double *pmax,
                           double *psum, double *top, double *rmax, double *rsum)
{
    return hode::pred_loo_fold<float>(stream, n_draws, N, y, obs, mask, sigma, status, row_len, K, cnt, lmean, lm2, pmax, psum, top, rmax,
                                      rsum);
}
int hode_pred_loo_fold_f64(void *stream, int n_draws, int64_t N, const double *y, const double *obs, const uint8_t *mask, const double *sigma,
                           const int32_t *status, int64_t row_len, int K, int32_t *cnt, double *lmean, double *lm2, double *pmax,
                           double *psum, double *top, double *rmax, double *rsum)
{
    return hode::pred_loo_fold<double>(stream, n_draws, N, y, obs, mask, sigma, status, row_len, K, cnt, lmean, lm2, pmax, psum, top, rmax,
                                       rsum);
}
int hode_pred_loo_finish_f32(void *stream, int64_t N, int K, double r_eff, const int32_t *cnt, const double *lmean, const double *lm2,
                             const double *pmax, const double *psum, double *top, const double *rmax, const double *rsum, float *elpd_loo,
                             float *pareto_k, float *elpd_waic, float *p_waic, float *lppd, double *table, double *fit, double *work)
{
    return hode::pred_loo_finish<float>(stream, N, K, r_eff, cnt, lmean, lm2, pmax, psum, top, rmax, rsum, elpd_loo, pareto_k, elpd_waic,
                                        p_waic, lppd, table, fit, work);
}
int hode_pred_loo_finish_f64(void *stream, int64_t N, int K, double r_eff, const int32_t *cnt, const double *lmean, const double *lm2,
                             const double *pmax, const double *psum, double *top, const double *rmax, const double *rsum, double *elpd_loo,
                             double *pareto_k, double *elpd_waic, double *p_waic, double *lppd, double *table, double *fit, double *work)
{
    return hode::pred_loo_finish<double>(stream, N, K, r_eff, cnt, lmean, lm2, pmax, psum, top, rmax, rsum, elpd_loo, pareto_k, elpd_waic,
                                         p_waic, lppd, table, fit, work);
}

}  // extern "C"

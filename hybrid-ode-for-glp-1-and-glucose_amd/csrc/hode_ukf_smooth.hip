// hode_ukf_smooth.hip -- the unscented Rauch-Tung-Striebel smoother over a stored run of the unscented Kalman filter
// (inference/ukf.py, UKFResult.smooth; include/hode_ukf_smooth.h): from the points every
// filter step emitted and the rows the solve carried them to, the state at every step given the whole record.  Three launches,
// whatever the number of steps S:
//   gain     one wave per pair (s, s + 1) of a patient, several per workgroup: the predicted moments m-, P- of step s + 1 (the
//            step kernel's, bit for bit), the cross covariance C of the emitted points of step s with their images, and the gain
//            G = C (P-)^-1 through the Cholesky factor of P-.  Its slice of LDS (fp64):
//              ZA, ZB [K][n]  the emitted points and their images in link space;  MS, MT [n]  their means (the filtered mean of
//              step s, the pre-drift mean of the images);  PP, L [n][n]  P- and its factor;  C [n][n]  C, then G row by row
//   pass     one wave (one workgroup) per patient walks s = S - 2 .. 0: ms_s = m_s + G (ms_{s+1} - m-),
//            Ps_s = sym(P_s + G (Ps_{s+1} - P-) G^T), the smoothed moments of step s + 1 carried in LDS
//   moments  one wave per (s, patient): the points of (ms, Ps), mapped to natural space, their unscented mean and variance
// A lane owns output entries (i, j), (i, j) + 64, ... and loops over the points or the inner index in order: no sum needs a
// cross-lane reduction, and every sum has the order of the restatement of the tests.  Waves never exchange data; the barriers
// are workgroup barriers all the same, so control flow is uniform across the workgroup (loop bounds depend on n and S alone,
// a dead step and a wave past the last item are predicated at the stores).  Contraction is off, there are no atomics: the same
// call gives the same bits, and an item's bits depend neither on B nor on its row.
#include "hode_ukf_linalg.h"
#include "../../include/hode_ukf_smooth.h"
#include <limits>

#pragma clang fp contract(off)

namespace hode {
namespace {

template <typename R> struct UkfSmoothArgs {
    int S, B, link, n_par;
    double gamma, wm0, wc0, wi;
    const R *hist, *ode, *prop;
    const double *mean_f, *cov_f;
    const int32_t *alive;
    const double *q, *walk, *dt;
    double *mean_s, *cov_s, *gain, *pred_mean, *pred_cov, *moments;
    int8_t col[HODE_PF_MAX_AUX];                                // the learned columns, ascending
    int8_t plog[HODE_PF_MAX_AUX];                               // 1: that column has the log link
};

// doubles of LDS per wave
__host__ __device__ constexpr int gain_doubles(int n) { return 2 * (2 * n + 1) * n + 2 * n + 3 * n * n; }
__host__ __device__ constexpr int pass_doubles(int n) { return 3 * n * n + 2 * n; }
__host__ __device__ constexpr int moments_doubles(int n) { return (2 * n + 1) * n + n + 2 * n * n; }

template <typename R> __global__ __launch_bounds__(kThreads) void ukf_gain_kernel(const UkfSmoothArgs<R> a)
{
    extern __shared__ __align__(16) double lds[];
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    const int n = 6 + a.n_par, K = 2 * n + 1;
    const int64_t items = (int64_t)(a.S - 1) * a.B;
    const int64_t raw = (int64_t)blockIdx.x * waves + wave;
    const bool valid = raw < items;                             // a wave past the last pair repeats it and stores nothing
    const int64_t it = valid ? raw : items - 1;
    const int64_t s = it / a.B, b = it - s * a.B;
    const int64_t row_s = (s * a.B + b) * K, row_n = ((s + 1) * a.B + b) * K;
    const bool slog = a.link == HODE_PF_LINK_LOG;
    const bool live = a.alive[(s + 1) * a.B + b] != 0;          // the gain into a dead step is NaN
    const double dtb = a.dt[(s + 1) * a.B + b];

    double *ZA = lds + (size_t)wave * gain_doubles(n);
    double *ZB = ZA + K * n, *MS = ZB + K * n, *MT = MS + n, *PP = MT + n, *L = PP + n * n, *C = L + n * n;

    // ---- a. the emitted points of step s and their images, in link space
    for (int e = lane; e < K * n; e += 64) {
        const int k = e / n, j = e - k * n;
        const bool lg = j < 6 ? slog : a.plog[j - 6] != 0;
        double va, vb;
        if (j < 6) {
            va = (double)a.hist[6 * (row_s + k) + j];
            vb = (double)a.prop[6 * (row_n + k) + j];
        } else {
            va = vb = (double)a.ode[HODE_PF_MAX_AUX * (row_s + k) + a.col[j - 6]];
        }
        ZA[e] = lg ? log(va) : va;
        ZB[e] = lg ? log(vb) : vb;
    }
    for (int j = lane; j < n; j += 64) MS[j] = a.mean_f[(s * a.B + b) * n + j];
    __syncthreads();

    // ---- b. the predicted moments: the step kernel's phase (a) on the same values in the same order
    for (int j = lane; j < n; j += 64) {
        double acc = 0.0;
        for (int k = 0; k < K; ++k) acc += (k == 0 ? a.wm0 : a.wi) * ZB[k * n + j];
        MT[j] = acc;
    }
    __syncthreads();
    // ---- c. the cross covariance, about the filtered mean of step s and the pre-drift mean of the images
    for (int e = lane; e < n * n; e += 64) {
        const int i = e / n, j = e - i * n;
        double acc = 0.0, cc = 0.0;
        for (int k = 0; k < K; ++k) {
            const double w = k == 0 ? a.wc0 : a.wi;
            acc += w * ((ZB[k * n + i] - MT[i]) * (ZB[k * n + j] - MT[j]));
            cc += w * ((ZA[k * n + i] - MS[i]) * (ZB[k * n + j] - MT[j]));
        }
        if (i == j) {
            const double sd = i < 6 ? a.q[i] : a.walk[a.col[i - 6]];
            acc += (sd * sd) * dtb;
        }
        PP[e] = acc;
        C[e] = cc;
    }
    __syncthreads();

    // ---- d. the gain G = C (P-)^-1 through L = chol(P-): row i forward, then backward; a zero column passes nothing
    (void)ukf_chol(PP, L, n, lane);
    for (int i = lane; i < n; i += 64) {
        double *g = C + i * n;
        for (int p = 0; p < n; ++p) {
            double t = g[p];
            for (int c = 0; c < p; ++c) t -= L[p * n + c] * g[c];
            const double dg = L[p * n + p];
            g[p] = dg == 0.0 ? 0.0 : t / dg;
        }
        for (int p = n - 1; p >= 0; --p) {
            double t = g[p];
            for (int c = p + 1; c < n; ++c) t -= L[c * n + p] * g[c];
            const double dg = L[p * n + p];
            g[p] = dg == 0.0 ? 0.0 : t / dg;
        }
    }
    __syncthreads();

    if (valid) {
        double *pm = a.pred_mean + it * n, *pc = a.pred_cov + it * n * n, *gn = a.gain + it * n * n;
        for (int j = lane; j < n; j += 64) {
            double m = MT[j];
            if (slog && j < 6) m = m - 0.5 * ((a.q[j] * a.q[j]) * dtb);
            pm[j] = live ? m : nan;
        }
        for (int e = lane; e < n * n; e += 64) {
            pc[e] = live ? PP[e] : nan;
            gn[e] = live ? C[e] : nan;
        }
    }
}

// one workgroup of one wave per patient
template <typename R> __global__ __launch_bounds__(64) void ukf_pass_kernel(const UkfSmoothArgs<R> a)
{
    extern __shared__ __align__(16) double lds[];
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const int lane = threadIdx.x;
    const int n = 6 + a.n_par, nn = n * n;
    const int64_t b = blockIdx.x;
    double *MS = lds, *DL = MS + n, *A = DL + n, *G = A + nn, *T = G + nn;

    int term = -1;                                              // the terminal step: the last one the filter left alive
    for (int s = 0; s < a.S; ++s)
        if (a.alive[(int64_t)s * a.B + b] != 0) term = s;

    for (int s = a.S - 1; s >= 0; --s) {
        const int64_t at = (int64_t)s * a.B + b;
        double *ms = a.mean_s + at * n, *ps = a.cov_s + at * nn;
        const double *mf = a.mean_f + at * n, *pf = a.cov_f + at * nn;
        if (s > term) {                                         // (the same in every lane: term depends on the patient alone)
            for (int j = lane; j < n; j += 64) ms[j] = nan;
            for (int e = lane; e < nn; e += 64) ps[e] = nan;
            continue;
        }
        if (s == term) {                                        // copies, bit for bit
            for (int j = lane; j < n; j += 64) ms[j] = MS[j] = mf[j];
            for (int e = lane; e < nn; e += 64) ps[e] = A[e] = pf[e];
            __syncthreads();
            continue;
        }
        // ---- e. delta = ms_{s+1} - m-, D = Ps_{s+1} - P- (in place), G
        for (int j = lane; j < n; j += 64) DL[j] = MS[j] - a.pred_mean[at * n + j];
        for (int e = lane; e < nn; e += 64) {
            A[e] = A[e] - a.pred_cov[at * nn + e];
            G[e] = a.gain[at * nn + e];
        }
        __syncthreads();
        for (int i = lane; i < n; i += 64) {
            double acc = 0.0;
            for (int j = 0; j < n; ++j) acc += G[i * n + j] * DL[j];
            ms[i] = MS[i] = mf[i] + acc;
        }
        for (int e = lane; e < nn; e += 64) {
            const int i = e / n, k = e - i * n;
            double acc = 0.0;
            for (int j = 0; j < n; ++j) acc += G[i * n + j] * A[j * n + k];
            T[e] = acc;
        }
        __syncthreads();
        for (int e = lane; e < nn; e += 64) {
            const int i = e / n, j = e - i * n;
            double u1 = 0.0, u2 = 0.0;
            for (int k = 0; k < n; ++k) {
                u1 += T[i * n + k] * G[j * n + k];
                u2 += T[j * n + k] * G[i * n + k];
            }
            ps[e] = A[e] = 0.5 * ((pf[i * n + j] + u1) + (pf[j * n + i] + u2));
        }
        __syncthreads();
    }
}

template <typename R> __global__ __launch_bounds__(kThreads) void ukf_moments_kernel(const UkfSmoothArgs<R> a)
{
    extern __shared__ __align__(16) double lds[];
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    const int n = 6 + a.n_par, K = 2 * n + 1;
    const int64_t items = (int64_t)a.S * a.B;
    const int64_t raw = (int64_t)blockIdx.x * waves + wave;
    const bool valid = raw < items;                             // a wave past the last item repeats it and stores nothing
    const int64_t it = valid ? raw : items - 1;
    const bool slog = a.link == HODE_PF_LINK_LOG;
    const bool live = a.alive[it] != 0;

    double *Z = lds + (size_t)wave * moments_doubles(n);
    double *M = Z + K * n, *P = M + n, *L = P + n * n;
    for (int j = lane; j < n; j += 64) M[j] = a.mean_s[it * n + j];
    for (int e = lane; e < n * n; e += 64) P[e] = a.cov_s[it * n * n + e];
    __syncthreads();

    // ---- f. the step kernel's phase (d) and its statistics on (ms, Ps)
    (void)ukf_chol(P, L, n, lane);
    ukf_draw(Z, M, L, n, a.gamma, lane);
    for (int e = lane; e < K * n; e += 64) {
        const int j = e % n;
        const bool lg = j < 6 ? slog : a.plog[j - 6] != 0;
        Z[e] = lg ? exp(Z[e]) : Z[e];
    }
    __syncthreads();
    if (valid && lane < 6) {
        double mu = 0.0, var = 0.0;
        for (int k = 0; k < K; ++k) mu += (k == 0 ? a.wm0 : a.wi) * Z[k * n + lane];
        for (int k = 0; k < K; ++k) {
            const double dv = Z[k * n + lane] - mu;
            var += (k == 0 ? a.wc0 : a.wi) * (dv * dv);
        }
        a.moments[it * 12 + lane] = live ? mu : nan;
        a.moments[it * 12 + 6 + lane] = live ? var : nan;
    }
}

template <typename R>
int ukf_smooth(void *stream, int S, int B, int link, const int32_t *mode, double gamma, double wm0, double wc0, double wi, const R *hist,
               const R *ode, const R *prop, const double *mean_f, const double *cov_f, const int32_t *alive, const double *q,
               const double *walk, const double *dt, double *mean_s, double *cov_s, double *gain, double *pred_mean, double *pred_cov,
               double *moments)
{
    if (S < 1 || B < 1 || (link != HODE_PF_LINK_ADD && link != HODE_PF_LINK_LOG)) return HODE_EINVAL;
    if (!(gamma > 0.0) || !std::isfinite(gamma) || !std::isfinite(wm0) || !std::isfinite(wc0) || !std::isfinite(wi)) return HODE_EINVAL;
    if (!mode || !hist || !ode || !prop || !mean_f || !cov_f || !alive || !q || !walk || !dt || !mean_s || !cov_s || !moments)
        return HODE_EINVAL;
    if (S > 1 && (!gain || !pred_mean || !pred_cov)) return HODE_EINVAL;
    const void *ins[] = {hist, ode, prop, mean_f, cov_f, alive, q, walk, dt};
    const void *outs[] = {mean_s, cov_s, moments, gain, pred_mean, pred_cov};
    for (int o = 0; o < (S > 1 ? 6 : 3); ++o) {
        for (const void *p : ins)
            if (outs[o] == p) return HODE_EINVAL;
        for (int o2 = 0; o2 < o; ++o2)
            if (outs[o] == outs[o2]) return HODE_EINVAL;
    }
    UkfSmoothArgs<R> a{};
    for (int c = 0; c < HODE_PF_MAX_AUX; ++c) {
        if (mode[c] < HODE_PF_MOVE_CARRIED || mode[c] > HODE_PF_MOVE_LOG) return HODE_EINVAL;
        if (mode[c] != HODE_PF_MOVE_CARRIED) {
            a.col[a.n_par] = (int8_t)c;
            a.plog[a.n_par] = mode[c] == HODE_PF_MOVE_LOG ? 1 : 0;
            ++a.n_par;
        }
    }
    a.S = S; a.B = B; a.link = link; a.gamma = gamma; a.wm0 = wm0; a.wc0 = wc0; a.wi = wi;
    a.hist = hist; a.ode = ode; a.prop = prop; a.mean_f = mean_f; a.cov_f = cov_f; a.alive = alive; a.q = q; a.walk = walk; a.dt = dt;
    a.mean_s = mean_s; a.cov_s = cov_s; a.gain = gain; a.pred_mean = pred_mean; a.pred_cov = pred_cov; a.moments = moments;
    const int n = 6 + a.n_par;
    hipStream_t st = (hipStream_t)stream;
    if (S > 1) {
        const int waves = waves_for(gain_doubles(n));
        const size_t bytes = (size_t)waves * gain_doubles(n) * sizeof(double);
        const int64_t items = (int64_t)(S - 1) * B;
        if (!lds_ok(&ukf_gain_kernel<R>, bytes)) return HODE_ELAUNCH;
        hipLaunchKernelGGL((ukf_gain_kernel<R>), dim3((unsigned)((items + waves - 1) / waves)), dim3(64 * waves), bytes, st, a);
    }
    hipLaunchKernelGGL((ukf_pass_kernel<R>), dim3(B), dim3(64), (size_t)pass_doubles(n) * sizeof(double), st, a);
    {
        const int waves = waves_for(moments_doubles(n));
        const size_t bytes = (size_t)waves * moments_doubles(n) * sizeof(double);
        const int64_t items = (int64_t)S * B;
        if (!lds_ok(&ukf_moments_kernel<R>, bytes)) return HODE_ELAUNCH;
        hipLaunchKernelGGL((ukf_moments_kernel<R>), dim3((unsigned)((items + waves - 1) / waves)), dim3(64 * waves), bytes, st, a);
    }
    return done();
}

}  // namespace
}  // namespace hode

extern "C" {

int hode_ukf_smooth_f32(void *stream, int S, int B, int link, const int32_t *mode, double gamma, double wm0, double wc0, double wi,
                        const float *history, const float *ode_history, const float *propagated, const double *mean_f,
                        const double *cov_f, const int32_t *alive, const double *q, const double *walk, const double *dt,
                        double *mean_s, double *cov_s, double *gain, double *pred_mean, double *pred_cov, double *moments)
{
    return hode::ukf_smooth<float>(stream, S, B, link, mode, gamma, wm0, wc0, wi, history, ode_history, propagated, mean_f, cov_f, alive, q,
                                   walk, dt, mean_s, cov_s, gain, pred_mean, pred_cov, moments);
}
int hode_ukf_smooth_f64(void *stream, int S, int B, int link, const int32_t *mode, double gamma, double wm0, double wc0, double wi,
                        const double *history, const double *ode_history, const double *propagated, const double *mean_f,
                        const double *cov_f, const int32_t *alive, const double *q, const double *walk, const double *dt,
                        double *mean_s, double *cov_s, double *gain, double *pred_mean, double *pred_cov, double *moments)
{
    return hode::ukf_smooth<double>(stream, S, B, link, mode, gamma, wm0, wc0, wi, history, ode_history, propagated, mean_f, cov_f, alive,
                                    q, walk, dt, mean_s, cov_s, gain, pred_mean, pred_cov, moments);
}

}  // extern "C"

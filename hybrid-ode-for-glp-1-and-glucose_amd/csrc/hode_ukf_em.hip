// hode_ukf_em.hip -- EM for the noise of the unscented Kalman filter over its smoother (inference/ukf.py, fit_ukf_noise;
// include/hode_ukf_em.h): the expected squared residual of every coordinate over every pair of steps,
// that of every seen observation, and the process noise, walk and observation noise that maximise the expected likelihood.
// Three kernels, one launch each whatever the number of steps S:
//   points   one wave per pair (s, s + 1) of a patient: the sigma points of the smoothed moments of step s, in natural space with
//            their constants -- the rows a forward solve carries over the segment of step s + 1 -- and their Cholesky factor.
//            Its slice of LDS (fp64): Z [K][n] the points, M [n], P, L [n][n] the moments and the factor
//   stats    one wave per (s, patient): from the images of those rows the pair's statistic e2 (fbar, F, the cross term through
//            U = L^-1 Cov(x_s, f) and V = L^-T U) and the step's observation statistic r2.  Its slice of LDS:
//              Z [K][n] the points, then their images in link space;  PS, G [n][n] the smoothed covariance of step s + 1 and the
//              gain;  L [n][n] the factor, then W = PS G^T;  U [n][n] U, then V in place;  FB, FF, MN [n] fbar, F (first the mean
//              of step s), the mean of step s + 1
//   mstep    one workgroup of 4 x 256 threads: slot t of group g sums quantity 4 r + g in round r over the patients b = t
//            (mod 256), the slots are folded in LDS, and the first 29 threads write the new values
// A lane owns output entries and loops over the points or the inner index in order: no sum needs a cross-lane reduction, and
// every sum has the order of the restatement of the tests.  Waves never exchange data (the M-step's fold apart); the barriers are
// workgroup barriers all the same, so control flow is uniform across the workgroup (loop bounds depend on n, S and B alone, a
// dead pair and a wave past the last item are predicated at the stores).  Contraction is off, there are no atomics: the same call
// gives the same bits.
#include "hode_ukf_linalg.h"
#include "../../include/hode_ukf_em.h"
#include <limits>

#pragma clang fp contract(off)

namespace hode {
namespace {

constexpr int kEmSlots = HODE_UKF_EM_SLOTS, kEmGroups = 4;
constexpr int kEmA = 0, kEmN = 23, kEmD = 24, kEmR = 25, kEmM = 31;  // the layout of sums

template <typename R> struct UkfEmArgs {
    int S, B, link, n_par;
    double gamma, wm0, wc0, wi;
    const double *mean_s, *cov_s, *gain, *chol_in, *moments;
    const int32_t *alive, *status;
    const R *ode, *prop, *obs;
    const uint8_t *mask;
    R *x_em, *aux_em;
    double *chol, *e2, *r2;
    int32_t *pair_ok, *seen;
    int8_t col[HODE_PF_MAX_AUX];                                // the learned columns, ascending
    int8_t plog[HODE_PF_MAX_AUX];                               // 1: that column has the log link
};

struct UkfEmStepArgs {
    int S, B, link, n;
    const double *e2, *r2, *dt;
    const int32_t *pair_ok, *seen;
    double *q, *walk, *sigma, *sums;
    double floor[HODE_UKF_EM_FIT];
    int8_t fit[HODE_UKF_EM_FIT];
    int8_t coord[HODE_PF_MAX_AUX];                              // the coordinate of a learned column, -1 for a carried one
};

// doubles of LDS per wave
__host__ __device__ constexpr int points_doubles(int n) { return (2 * n + 1) * n + n + 2 * n * n; }
__host__ __device__ constexpr int stats_doubles(int n) { return (2 * n + 1) * n + 4 * n * n + 3 * n; }

template <typename R> __global__ __launch_bounds__(kThreads) void ukf_em_points_kernel(const UkfEmArgs<R> a)
{
    extern __shared__ __align__(16) double lds[];
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    const int n = 6 + a.n_par, K = 2 * n + 1;
    const int64_t items = (int64_t)(a.S - 1) * a.B;
    const int64_t raw = (int64_t)blockIdx.x * waves + wave;
    const bool valid = raw < items;                             // a wave past the last pair repeats it and stores nothing
    const int64_t it = valid ? raw : items - 1;
    const bool slog = a.link == HODE_PF_LINK_LOG;
    const bool live = a.alive[it + a.B] != 0;                   // (step s + 1 of the same patient)

    double *Z = lds + (size_t)wave * points_doubles(n);
    double *M = Z + K * n, *P = M + n, *L = P + n * n;
    for (int j = lane; j < n; j += 64) M[j] = a.mean_s[it * n + j];
    for (int e = lane; e < n * n; e += 64) P[e] = a.cov_s[it * n * n + e];
    __syncthreads();

    // ---- a. the step kernel's phase (d) on (ms, Ps)
    (void)ukf_chol(P, L, n, lane);
    ukf_draw(Z, M, L, n, a.gamma, lane);
    for (int e = lane; e < K * n; e += 64) {
        const int j = e % n;
        const bool lg = j < 6 ? slog : a.plog[j - 6] != 0;
        Z[e] = lg ? exp(Z[e]) : Z[e];
    }
    __syncthreads();

    if (valid) {
        R *xo = a.x_em + 6 * it * K, *ao = a.aux_em + HODE_PF_MAX_AUX * it * K;
        const R *ai = a.ode + HODE_PF_MAX_AUX * it * K;         // the centre row's carried columns
        for (int e = lane; e < K * 6; e += 64) {
            const int k = e / 6, j = e - k * 6;
            xo[e] = live ? (R)Z[k * n + j] : (R)1;
        }
        for (int e = lane; e < K * HODE_PF_MAX_AUX; e += 64) {
            const int k = e / HODE_PF_MAX_AUX, c = e - k * HODE_PF_MAX_AUX;
            R v = ai[c];
            for (int p = 0; p < a.n_par; ++p)
                if (live && a.col[p] == c) v = (R)Z[k * n + 6 + p];
            ao[e] = v;
        }
        for (int e = lane; e < n * n; e += 64) a.chol[it * n * n + e] = live ? L[e] : nan;
    }
}

template <typename R> __global__ __launch_bounds__(kThreads) void ukf_em_stats_kernel(const UkfEmArgs<R> a)
{
    extern __shared__ __align__(16) double lds[];
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    const int n = 6 + a.n_par, K = 2 * n + 1, nn = n * n;
    const int64_t items = (int64_t)a.S * a.B;
    const int64_t raw = (int64_t)blockIdx.x * waves + wave;
    const bool valid = raw < items;                             // a wave past the last item repeats it and stores nothing
    const int64_t it = valid ? raw : items - 1;
    const int64_t s = it / a.B, b = it - s * a.B;
    const bool slog = a.link == HODE_PF_LINK_LOG;

    if (a.S > 1) {                                              // (the same in every wave of the launch)
        // the last step starts no pair: its wave repeats the pair before it and stores nothing of it
        const bool has_pair = s < a.S - 1;
        const int64_t pit = has_pair ? it : it - a.B, nit = pit + a.B;
        double *Z = lds + (size_t)wave * stats_doubles(n);
        double *PS = Z + K * n, *G = PS + nn, *L = G + nn, *U = L + nn, *FB = U + nn, *FF = FB + n, *MN = FF + n;
        for (int j = lane; j < n; j += 64) {
            FF[j] = a.mean_s[pit * n + j];
            MN[j] = a.mean_s[nit * n + j];
        }
        for (int e = lane; e < nn; e += 64) {
            PS[e] = a.cov_s[nit * nn + e];
            G[e] = a.gain[pit * nn + e];
            L[e] = a.chol_in[pit * nn + e];
        }
        __syncthreads();

        // ---- c. the points of step s again, their states replaced by the images in link space
        ukf_draw(Z, FF, L, n, a.gamma, lane);
        bool bad = false;
        for (int e = lane; e < K * 6; e += 64) {
            const int k = e / 6, j = e - k * 6;
            const double v = (double)a.prop[6 * (pit * K + k) + j];
            const bool ok = __builtin_isfinite(v) && (!slog || v > 0.0);
            bad = bad || !ok;
            Z[k * n + j] = ok ? (slog ? log(v) : v) : 0.0;
        }
        if (lane < K && a.status[pit * K + lane] != 0) bad = true;
        const bool ok = a.alive[nit] != 0 && __any(bad ? 1 : 0) == 0;
        __syncthreads();
        for (int i = lane; i < n; i += 64) {
            double acc = 0.0;
            for (int k = 0; k < K; ++k) acc += (k == 0 ? a.wm0 : a.wi) * Z[k * n + i];
            FB[i] = acc;
        }
        __syncthreads();
        for (int i = lane; i < n; i += 64) {
            double acc = 0.0;
            for (int k = 0; k < K; ++k) {
                const double dv = Z[k * n + i] - FB[i];
                acc += (k == 0 ? a.wc0 : a.wi) * (dv * dv);
            }
            FF[i] = acc;
        }
        const double wg = a.wi * a.gamma;
        for (int e = lane; e < nn; e += 64) {
            const int j = e / n, i = e - j * n;
            U[e] = L[j * n + j] == 0.0 ? 0.0 : wg * (Z[(1 + j) * n + i] - Z[(1 + n + j) * n + i]);
        }
        __syncthreads();
        // V = L^-T U, column i by backward substitution, in place
        for (int i = lane; i < n; i += 64) {
            for (int p = n - 1; p >= 0; --p) {
                double t = U[p * n + i];
                for (int c = p + 1; c < n; ++c) t -= L[c * n + p] * U[c * n + i];
                const double dg = L[p * n + p];
                U[p * n + i] = dg == 0.0 ? 0.0 : t / dg;
            }
        }
        __syncthreads();
        // W = Ps_{s+1} G^T over the factor, which is done with
        for (int e = lane; e < nn; e += 64) {
            const int i = e / n, c = e - i * n;
            double acc = 0.0;
            for (int k = 0; k < n; ++k) acc += PS[i * n + k] * G[c * n + k];
            L[e] = acc;
        }
        __syncthreads();
        if (valid && has_pair) {
            for (int i = lane; i < n; i += 64) {
                double cross = 0.0;
                for (int c = 0; c < n; ++c) cross += L[i * n + c] * U[c * n + i];
                const double d = MN[i] - FB[i];
                const double v = ((PS[i * n + i] + d * d) - 2.0 * cross) + FF[i];
                a.e2[pit * n + i] = ok ? v : nan;
            }
            if (lane == 0) a.pair_ok[pit] = ok ? 1 : 0;
        }
    }

    // ---- d. the observation statistic of step s
    bool sn = false;
    if (lane < 6) {
        const R o = a.obs[(b * a.S + s) * 6 + lane];
        sn = __builtin_isfinite(o) && (!a.mask || a.mask[(b * a.S + s) * 6 + lane] != 0) && a.alive[it] != 0;
        double v = 0.0;
        if (sn) {
            const double r = (double)o - a.moments[it * 12 + lane];
            v = r * r + a.moments[it * 12 + 6 + lane];
        }
        if (valid) a.r2[it * 6 + lane] = v;
    }
    const unsigned long long bits = __ballot(sn ? 1 : 0);
    if (valid && lane == 0) a.seen[it] = (int32_t)(bits & 63ull);
}

__global__ __launch_bounds__(kEmSlots *kEmGroups) void ukf_em_mstep_kernel(const UkfEmStepArgs a)
{
    __shared__ double red[kEmGroups][kEmSlots];
    __shared__ double tot[HODE_UKF_EM_SUMS];
    const int t = threadIdx.x % kEmSlots, g = threadIdx.x / kEmSlots;
    const int n = a.n;
    constexpr int rounds = (HODE_UKF_EM_SUMS + kEmGroups - 1) / kEmGroups;

    // ---- e. the sums: per patient over s ascending, the patients of a slot ascending, the slots folded
    for (int r = 0; r < rounds; ++r) {
        const int qn = r * kEmGroups + g;
        double acc = 0.0;
        // (a pair or an entry that does not count adds +0.0, which leaves a sum that started at +0.0 bit for bit: the loads of
        // several steps are then in flight at once, where a skipped iteration would have each wait for the one before)
        if (qn < n) {                                           // A_i over the counted pairs
            for (int64_t b = t; b < a.B; b += kEmSlots) {
                double part = 0.0;
#pragma unroll 4
                for (int64_t s = 0; s + 1 < a.S; ++s) {
                    const double v = a.e2[(s * a.B + b) * n + qn] / a.dt[(s + 1) * a.B + b];
                    part += a.pair_ok[s * a.B + b] != 0 ? v : 0.0;
                }
                acc += part;
            }
        } else if (qn == kEmN || qn == kEmD) {                  // their number, their dt
            for (int64_t b = t; b < a.B; b += kEmSlots) {
                double part = 0.0;
#pragma unroll 4
                for (int64_t s = 0; s + 1 < a.S; ++s) {
                    const double v = qn == kEmN ? 1.0 : a.dt[(s + 1) * a.B + b];
                    part += a.pair_ok[s * a.B + b] != 0 ? v : 0.0;
                }
                acc += part;
            }
        } else if (qn >= kEmR && qn < HODE_UKF_EM_SUMS) {       // R_j and M_j over the seen entries
            const int j = qn < kEmM ? qn - kEmR : qn - kEmM;
            for (int64_t b = t; b < a.B; b += kEmSlots) {
                double part = 0.0;
#pragma unroll 4
                for (int64_t s = 0; s < a.S; ++s) {
                    const double v = qn < kEmM ? a.r2[(s * a.B + b) * 6 + j] : 1.0;
                    part += ((a.seen[s * a.B + b] >> j) & 1) != 0 ? v : 0.0;
                }
                acc += part;
            }
        }                                                       // (a coordinate past n: 0)
        red[g][t] = acc;
        for (int h = kEmSlots / 2; h >= 1; h >>= 1) {
            __syncthreads();
            if (t < h) red[g][t] = red[g][t] + red[g][t + h];
        }
        if (t == 0 && qn < HODE_UKF_EM_SUMS) {
            tot[qn] = red[g][0];
            a.sums[qn] = red[g][0];
        }
        __syncthreads();
    }

    // ---- the new values: thread v of the first HODE_UKF_EM_FIT owns one
    const int v = threadIdx.x;
    if (v < HODE_UKF_EM_FIT && a.fit[v] != 0) {
        const double N = tot[kEmN], D = tot[kEmD];
        double *dst = v < 6 ? a.q + v : v < 6 + HODE_PF_MAX_AUX ? a.walk + (v - 6) : a.sigma + (v - 6 - HODE_PF_MAX_AUX);
        double var = -1.0;                                      // (negative: nothing to write)
        if (v < 6 + HODE_PF_MAX_AUX) {
            const int i = v < 6 ? v : a.coord[v - 6];
            if (i >= 0 && N > 0.0) {
                const double A = tot[kEmA + i];
                var = (v < 6 && a.link == HODE_PF_LINK_LOG) ? (2.0 * A) / (sqrt(N * N + A * D) + N) : A / N;
            }
        } else {
            const int j = v - 6 - HODE_PF_MAX_AUX;
            if (tot[kEmM + j] > 0.0) var = tot[kEmR + j] / tot[kEmM + j];
        }
        if (var >= 0.0 && *dst != 0.0) {
            const double sd = sqrt(var);
            *dst = sd > a.floor[v] ? sd : a.floor[v];
        }
    }
}

// the host arguments every entry shares; HODE_EINVAL or the number of learned columns
template <typename A> int em_head(A &a, int S, int B, int link, const int32_t *mode)
{
    if (S < 1 || B < 1 || (link != HODE_PF_LINK_ADD && link != HODE_PF_LINK_LOG) || !mode) return HODE_EINVAL;
    int n_par = 0;
    for (int c = 0; c < HODE_PF_MAX_AUX; ++c) {
        if (mode[c] < HODE_PF_MOVE_CARRIED || mode[c] > HODE_PF_MOVE_LOG) return HODE_EINVAL;
        if (mode[c] != HODE_PF_MOVE_CARRIED) {
            a.col[n_par] = (int8_t)c;
            a.plog[n_par] = mode[c] == HODE_PF_MOVE_LOG ? 1 : 0;
            ++n_par;
        }
    }
    a.S = S; a.B = B; a.link = link; a.n_par = n_par;
    return n_par;
}

inline bool distinct(const void *const *outs, int n_out, const void *const *ins, int n_in)
{
    for (int o = 0; o < n_out; ++o) {
        if (!outs[o]) continue;
        for (int i = 0; i < n_in; ++i)
            if (outs[o] == ins[i]) return false;
        for (int o2 = 0; o2 < o; ++o2)
            if (outs[o] == outs[o2]) return false;
    }
    return true;
}

template <typename R>
int ukf_em_points(void *stream, int S, int B, int link, const int32_t *mode, double gamma, const double *mean_s, const double *cov_s,
                  const int32_t *alive, const R *ode, R *x_em, R *aux_em, double *chol)
{
    UkfEmArgs<R> a{};
    if (em_head(a, S, B, link, mode) < 0) return HODE_EINVAL;
    if (!(gamma > 0.0) || !std::isfinite(gamma)) return HODE_EINVAL;
    if (!mean_s || !cov_s || !alive || !ode) return HODE_EINVAL;
    if (S > 1 && (!x_em || !aux_em || !chol)) return HODE_EINVAL;
    const void *ins[] = {mean_s, cov_s, alive, ode};
    const void *outs[] = {x_em, aux_em, chol};
    if (!distinct(outs, 3, ins, 4)) return HODE_EINVAL;
    if (S == 1) return HODE_OK;
    a.gamma = gamma; a.mean_s = mean_s; a.cov_s = cov_s; a.alive = alive; a.ode = ode; a.x_em = x_em; a.aux_em = aux_em; a.chol = chol;
    const int n = 6 + a.n_par;
    const int waves = waves_for(points_doubles(n));
    const size_t bytes = (size_t)waves * points_doubles(n) * sizeof(double);
    const int64_t items = (int64_t)(S - 1) * B;
    if (!lds_ok(&ukf_em_points_kernel<R>, bytes)) return HODE_ELAUNCH;
    hipLaunchKernelGGL((ukf_em_points_kernel<R>), dim3((unsigned)((items + waves - 1) / waves)), dim3(64 * waves), bytes, (hipStream_t)stream, a);
    return done();
}

template <typename R>
int ukf_em_stats(void *stream, int S, int B, int link, const int32_t *mode, double gamma, double wm0, double wc0, double wi, const R *prop,
                 const int32_t *status, const double *chol, const double *mean_s, const double *cov_s, const double *gain,
                 const int32_t *alive, const R *obs, const uint8_t *mask, const double *moments, double *e2, int32_t *pair_ok, double *r2,
                 int32_t *seen)
{
    UkfEmArgs<R> a{};
    if (em_head(a, S, B, link, mode) < 0) return HODE_EINVAL;
    if (!(gamma > 0.0) || !std::isfinite(gamma) || !std::isfinite(wm0) || !std::isfinite(wc0) || !std::isfinite(wi)) return HODE_EINVAL;
    if (!mean_s || !cov_s || !alive || !obs || !moments || !r2 || !seen) return HODE_EINVAL;
    if (S > 1 && (!prop || !status || !chol || !gain || !e2 || !pair_ok)) return HODE_EINVAL;
    const void *ins[] = {prop, status, chol, mean_s, cov_s, gain, alive, obs, mask, moments};
    const void *outs[] = {r2, seen, e2, pair_ok};
    if (!distinct(outs, 4, ins, 10)) return HODE_EINVAL;
    a.gamma = gamma; a.wm0 = wm0; a.wc0 = wc0; a.wi = wi;
    a.prop = prop; a.status = status; a.chol_in = chol; a.mean_s = mean_s; a.cov_s = cov_s; a.gain = gain; a.alive = alive; a.obs = obs;
    a.mask = mask; a.moments = moments; a.e2 = e2; a.pair_ok = pair_ok; a.r2 = r2; a.seen = seen;
    const int n = 6 + a.n_par;
    const int waves = waves_for(stats_doubles(n));
    const size_t bytes = (size_t)waves * stats_doubles(n) * sizeof(double);
    const int64_t items = (int64_t)S * B;
    if (!lds_ok(&ukf_em_stats_kernel<R>, bytes)) return HODE_ELAUNCH;
    hipLaunchKernelGGL((ukf_em_stats_kernel<R>), dim3((unsigned)((items + waves - 1) / waves)), dim3(64 * waves), bytes, (hipStream_t)stream, a);
    return done();
}

int ukf_em_mstep(void *stream, int S, int B, int link, const int32_t *mode, const int32_t *fit_mask, const double *floor, const double *e2,
                 const int32_t *pair_ok, const double *r2, const int32_t *seen, const double *dt, double *q, double *walk, double *sigma,
                 double *sums)
{
    UkfEmArgs<double> head{};
    if (em_head(head, S, B, link, mode) < 0) return HODE_EINVAL;
    if (!fit_mask || !floor || !r2 || !seen || !dt || !q || !walk || !sigma || !sums) return HODE_EINVAL;
    if (S > 1 && (!e2 || !pair_ok)) return HODE_EINVAL;
    UkfEmStepArgs a{};
    for (int v = 0; v < HODE_UKF_EM_FIT; ++v) {
        if (fit_mask[v] != 0 && fit_mask[v] != 1) return HODE_EINVAL;
        if (!std::isfinite(floor[v]) || floor[v] < 0.0) return HODE_EINVAL;
        a.fit[v] = (int8_t)fit_mask[v];
        a.floor[v] = floor[v];
    }
    const void *ins[] = {e2, pair_ok, r2, seen, dt};
    const void *outs[] = {q, walk, sigma, sums};
    if (!distinct(outs, 4, ins, 5)) return HODE_EINVAL;
    for (int c = 0; c < HODE_PF_MAX_AUX; ++c) a.coord[c] = -1;
    for (int p = 0; p < head.n_par; ++p) a.coord[head.col[p]] = (int8_t)(6 + p);
    a.S = S; a.B = B; a.link = link; a.n = 6 + head.n_par;
    a.e2 = e2; a.pair_ok = pair_ok; a.r2 = r2; a.seen = seen; a.dt = dt; a.q = q; a.walk = walk; a.sigma = sigma; a.sums = sums;
    hipLaunchKernelGGL(ukf_em_mstep_kernel, dim3(1), dim3(kEmSlots * kEmGroups), 0, (hipStream_t)stream, a);
    return done();
}

}  // namespace
}  // namespace hode

extern "C" {

int hode_ukf_em_points_f32(void *stream, int S, int B, int link, const int32_t *mode, double gamma, const double *mean_s,
                           const double *cov_s, const int32_t *alive, const float *ode_history, float *x_em, float *aux_em, double *chol)
{
    return hode::ukf_em_points<float>(stream, S, B, link, mode, gamma, mean_s, cov_s, alive, ode_history, x_em, aux_em, chol);
}
int hode_ukf_em_points_f64(void *stream, int S, int B, int link, const int32_t *mode, double gamma, const double *mean_s,
                           const double *cov_s, const int32_t *alive, const double *ode_history, double *x_em, double *aux_em, double *chol)
{
    return hode::ukf_em_points<double>(stream, S, B, link, mode, gamma, mean_s, cov_s, alive, ode_history, x_em, aux_em, chol);
}
int hode_ukf_em_stats_f32(void *stream, int S, int B, int link, const int32_t *mode, double gamma, double wm0, double wc0, double wi,
                          const float *prop_em, const int32_t *status, const double *chol, const double *mean_s, const double *cov_s,
                          const double *gain, const int32_t *alive, const float *obs, const uint8_t *mask, const double *moments,
                          double *e2, int32_t *pair_ok, double *r2, int32_t *seen)
{
    return hode::ukf_em_stats<float>(stream, S, B, link, mode, gamma, wm0, wc0, wi, prop_em, status, chol, mean_s, cov_s, gain, alive, obs,
                                     mask, moments, e2, pair_ok, r2, seen);
}
int hode_ukf_em_stats_f64(void *stream, int S, int B, int link, const int32_t *mode, double gamma, double wm0, double wc0, double wi,
                          const double *prop_em, const int32_t *status, const double *chol, const double *mean_s, const double *cov_s,
                          const double *gain, const int32_t *alive, const double *obs, const uint8_t *mask, const double *moments,
                          double *e2, int32_t *pair_ok, double *r2, int32_t *seen)
{
    return hode::ukf_em_stats<double>(stream, S, B, link, mode, gamma, wm0, wc0, wi, prop_em, status, chol, mean_s, cov_s, gain, alive, obs,
                                      mask, moments, e2, pair_ok, r2, seen);
}
int hode_ukf_em_mstep(void *stream, int S, int B, int link, const int32_t *mode, const int32_t *fit_mask, const double *floor,
                      const double *e2, const int32_t *pair_ok, const double *r2, const int32_t *seen, const double *dt, double *q,
                      double *walk, double *sigma, double *sums)
{
    return hode::ukf_em_mstep(stream, S, B, link, mode, fit_mask, floor, e2, pair_ok, r2, seen, dt, q, walk, sigma, sums);
}

}  // extern "C"

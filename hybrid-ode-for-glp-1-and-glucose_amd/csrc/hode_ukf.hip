// hode_ukf.hip -- one step of the unscented (sigma-point) Kalman filter per patient (inference/ukf.py, run_ukf; include/hode.h,
// "Unscented Kalman filter"): what happens between two forward solves of a patient's K = 2 n + 1 sigma
// points -- the unscented mean and covariance of the propagated points, the redraw, the measurement update through the Cholesky
// factor of the innovation covariance, and the points for the next solve.
//
// One wave of 64 lanes per patient, kUkfPatients patients per workgroup; a patient's working set (fp64) is its wave's slice of
// the dynamic LDS, sized by n at launch:
//   Z [K][n]  the points in link space (the propagated ones, then the redrawn ones, then the emitted ones in natural space)
//   M [n]     the mean;  PA, PB [n][n]  covariance and Cholesky factor (they swap roles after the update)
//   Y [K][6]  the natural-space seen states of the points;  W [n][6]  the cross covariance C, then W = C L_S^-T
//   S, LS [6][6]  the innovation covariance and its factor;  YH, RZ [6]  the predicted observation, the residual
// A lane owns output entries (i, j), (i, j) + 64, ... and loops over the points in order: no sum needs a cross-lane reduction,
// and every sum has the order of the restatement of the tests.  Waves never exchange data; the barriers between the phases are
// workgroup barriers all the same, so control flow is uniform across the workgroup (loop bounds depend on n alone, everything
// that depends on the patient -- the seen states, a lost patient, a wave past the last patient -- is predicated) and no wave
// returns in front of one.  Floating-point contraction is off (an a * b + c here is two roundings), there are no atomics: the
// same call gives the same bits, and a patient's bits depend neither on B nor on its row.
#include "hode_ukf_linalg.h"
#include <limits>

#pragma clang fp contract(off)

namespace hode {
namespace {

constexpr int kUkfPatients = kThreads / 64;
constexpr double kLog2Pi = 1.8378770664093453;

template <typename R> struct UkfArgs {
    int B, predict, link, n_par;
    double gamma, wm0, wc0, wi;
    const R *x_in, *aux_in, *obs;
    const int32_t *status;
    const uint8_t *mask;
    const double *sigma, *q, *walk, *dt;
    int32_t *alive;
    double *mean, *cov, *stats;
    R *x_out, *aux_out;
    int8_t col[HODE_PF_MAX_AUX];                                // the learned columns, ascending
    int8_t plog[HODE_PF_MAX_AUX];                               // 1: that column has the log link
};

// doubles of LDS per patient
__host__ __device__ constexpr int ukf_doubles(int n) { return (2 * n + 1) * n + n + 2 * n * n + (2 * n + 1) * 6 + n * 6 + 36 + 36 + 6 + 6; }

// the a-th set bit of a 6-bit mask
__device__ __forceinline__ int nth_seen(uint32_t m, int a)
{
    for (int j = 0; j < 6; ++j)
        if ((m >> j) & 1u) {
            if (a == 0) return j;
            --a;
        }
    return 0;
}

template <typename R> __global__ __launch_bounds__(kThreads) void ukf_step_kernel(const UkfArgs<R> a)
{
    extern __shared__ __align__(16) double lds[];
    const double nan = std::numeric_limits<double>::quiet_NaN(), ninf = -std::numeric_limits<double>::infinity();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = 6 + a.n_par, K = 2 * n + 1;
    const int b_raw = blockIdx.x * kUkfPatients + wave;
    const bool valid = b_raw < a.B;                             // a wave past the last patient repeats it and stores nothing
    const int64_t b = valid ? b_raw : a.B - 1;
    const int64_t row0 = b * K;
    const bool slog = a.link == HODE_PF_LINK_LOG;

    double *Z = lds + (size_t)wave * ukf_doubles(n);
    double *M = Z + K * n, *PA = M + n, *PB = PA + n * n, *Y = PB + n * n, *W = Y + K * 6, *S = W + n * 6, *LS = S + 36, *YH = LS + 36,
           *RZ = YH + 6;

    // the seen states (the same in every lane of the wave)
    uint32_t seen = 0;
    int d = 0;
    for (int j = 0; j < 6; ++j) {
        const bool s = __builtin_isfinite(a.obs[6 * b + j]) && (!a.mask || a.mask[6 * b + j] != 0);
        seen |= (s ? 1u : 0u) << j;
        d += s ? 1 : 0;
    }
    bool lost = a.alive[b] == 0;

    // ---- a. predict
    if (a.predict) {
        const double dtb = a.dt[b];
        bool bad = false;
        for (int e = lane; e < K * n; e += 64) {
            const int k = e / n, j = e - k * n;
            const double v = j < 6 ? (double)a.x_in[6 * (row0 + k) + j] : (double)a.aux_in[HODE_PF_MAX_AUX * (row0 + k) + a.col[j - 6]];
            const bool lg = j < 6 ? slog : a.plog[j - 6] != 0;
            const bool ok = __builtin_isfinite(v) && (!lg || v > 0.0);
            bad = bad || !ok;
            Z[e] = ok ? (lg ? log(v) : v) : 0.0;
        }
        if (a.status && lane < K && a.status[row0 + lane] != 0) bad = true;
        lost = lost || __any(bad ? 1 : 0) != 0;
        __syncthreads();
        for (int j = lane; j < n; j += 64) {
            double acc = 0.0;
            for (int k = 0; k < K; ++k) acc += (k == 0 ? a.wm0 : a.wi) * Z[k * n + j];
            M[j] = acc;
        }
        __syncthreads();
        for (int e = lane; e < n * n; e += 64) {
            const int i = e / n, j = e - i * n;
            double acc = 0.0;
            for (int k = 0; k < K; ++k) acc += (k == 0 ? a.wc0 : a.wi) * ((Z[k * n + i] - M[i]) * (Z[k * n + j] - M[j]));
            if (i == j) {
                const double s = i < 6 ? a.q[i] : a.walk[a.col[i - 6]];
                acc += (s * s) * dtb;
            }
            PA[e] = acc;
        }
        __syncthreads();
        if (slog && lane < 6) M[lane] = M[lane] - 0.5 * ((a.q[lane] * a.q[lane]) * dtb);
    } else {
        for (int j = lane; j < n; j += 64) M[j] = a.mean[b * n + j];
        for (int e = lane; e < n * n; e += 64) PA[e] = a.cov[b * n * n + e];
    }
    __syncthreads();

    // ---- b. redraw
    lost = ukf_chol(PA, PB, n, lane) || lost;
    ukf_draw(Z, M, PB, n, a.gamma, lane);

    // ---- c. update (d == 0: nothing below changes M or PA, the increment is exactly 0)
    double inc = 0.0, nis = 0.0;
    double *P = PA, *L = PB;
    for (int e = lane; e < K * 6; e += 64) {
        const int k = e / 6, c = e - k * 6;
        double y = 0.0;
        if (c < d) {
            const double v = Z[k * n + nth_seen(seen, c)];
            y = slog ? exp(v) : v;
        }
        Y[e] = y;
    }
    __syncthreads();
    if (lane < 6) {
        double acc = 0.0;
        for (int k = 0; k < K; ++k) acc += (k == 0 ? a.wm0 : a.wi) * Y[k * 6 + lane];
        YH[lane] = acc;
    }
    __syncthreads();
    if (lane < 36) {
        const int p = lane / 6, c = lane - p * 6;
        double acc = 0.0;
        for (int k = 0; k < K; ++k) acc += (k == 0 ? a.wc0 : a.wi) * ((Y[k * 6 + p] - YH[p]) * (Y[k * 6 + c] - YH[c]));
        if (p == c && p < d) {
            const double sg = a.sigma[nth_seen(seen, p)];
            acc += sg * sg;
        }
        S[lane] = acc;
    }
    for (int e = lane; e < n * 6; e += 64) {
        const int i = e / 6, c = e - i * 6;
        double acc = 0.0;
        for (int k = 0; k < K; ++k) acc += (k == 0 ? a.wc0 : a.wi) * ((Z[k * n + i] - M[i]) * (Y[k * 6 + c] - YH[c]));
        W[e] = acc;
    }
    if (lane < 6) RZ[lane] = lane < d ? (double)a.obs[6 * b + nth_seen(seen, lane)] - YH[lane] : 0.0;
    __syncthreads();
    // the factor of S: its leading d x d block, in 6 x 6 storage
    {
        bool bad = false;
        for (int j = 0; j < 6; ++j) {
            double piv = S[j * 6 + j];
            for (int k = 0; k < j; ++k) piv -= LS[j * 6 + k] * LS[j * 6 + k];
            const bool live = j < d;
            if (live && !(piv > 0.0 && __builtin_isfinite(piv))) bad = true;
            const double root = live && piv > 0.0 ? sqrt(piv) : 1.0;
            if (lane < 6) {
                double t = 0.0;
                if (live && lane >= j && lane < d) {
                    if (lane == j) {
                        t = root;
                    } else {
                        t = S[lane * 6 + j];
                        for (int k = 0; k < j; ++k) t -= LS[lane * 6 + k] * LS[j * 6 + k];
                        t = t / root;
                    }
                }
                LS[lane * 6 + j] = t;
            }
            __syncthreads();
        }
        lost = lost || (d > 0 && bad);
    }
    if (d > 0) {
        // z = L_S^-1 r (every lane, the same values); row i of W = C L_S^-T by forward substitution; m += W z
        double z[6];
        double ld = 0.0;
#pragma unroll
        for (int p = 0; p < 6; ++p) {
            double t = RZ[p];
#pragma unroll
            for (int c = 0; c < p; ++c) t -= LS[p * 6 + c] * z[c];
            const double dg = p < d ? LS[p * 6 + p] : 1.0;
            z[p] = p < d ? t / dg : 0.0;
            nis += z[p] * z[p];
            ld += log(dg);
        }
        inc = -0.5 * ((nis + 2.0 * ld) + (double)d * kLog2Pi);
        for (int i = lane; i < n; i += 64) {
            double w[6];
            double acc = 0.0;
#pragma unroll
            for (int p = 0; p < 6; ++p) {
                double t = W[i * 6 + p];
#pragma unroll
                for (int c = 0; c < p; ++c) t -= LS[p * 6 + c] * w[c];
                w[p] = p < d ? t / LS[p * 6 + p] : 0.0;
                acc += w[p] * z[p];
            }
#pragma unroll
            for (int p = 0; p < 6; ++p) W[i * 6 + p] = w[p];
            M[i] = M[i] + acc;
        }
    }
    __syncthreads();
    if (d > 0) {
        // P = P- - W W^T, symmetrised, into the other matrix (a lane reads entries of P- that another lane's entry mirrors)
        for (int e = lane; e < n * n; e += 64) {
            const int i = e / n, j = e - i * n;
            double t1 = PA[i * n + j], t2 = PA[j * n + i];
            for (int p = 0; p < 6; ++p) {
                t1 -= W[i * 6 + p] * W[j * 6 + p];
                t2 -= W[j * 6 + p] * W[i * 6 + p];
            }
            PB[e] = 0.5 * (t1 + t2);
        }
        P = PB;
        L = PA;
    }
    __syncthreads();

    // ---- d. emit: the points of (M, P), in natural space
    lost = ukf_chol(P, L, n, lane) || lost;
    ukf_draw(Z, M, L, n, a.gamma, lane);
    {
        bool bad = false;
        for (int e = lane; e < K * n; e += 64) {
            const int j = e % n;
            const bool lg = j < 6 ? slog : a.plog[j - 6] != 0;
            const double v = lg ? exp(Z[e]) : Z[e];
            bad = bad || !__builtin_isfinite(v);
            Z[e] = v;
        }
        lost = lost || __any(bad ? 1 : 0) != 0;
    }
    __syncthreads();

    // ---- outputs
    if (valid) {
        R *xo = a.x_out + 6 * row0, *ao = a.aux_out + HODE_PF_MAX_AUX * row0;
        const R *xi = a.x_in + 6 * row0, *ai = a.aux_in + HODE_PF_MAX_AUX * row0;
        double *st = a.stats + b * HODE_UKF_COLS;
        if (lost) {
            for (int e = lane; e < K * 6; e += 64) xo[e] = xi[e];
            for (int e = lane; e < K * HODE_PF_MAX_AUX; e += 64) ao[e] = ai[e];
            for (int j = lane; j < n; j += 64) a.mean[b * n + j] = nan;
            for (int e = lane; e < n * n; e += 64) a.cov[b * n * n + e] = nan;
            if (lane < HODE_UKF_COLS) st[lane] = lane == 0 ? ninf : lane == 2 ? (double)d : lane == 3 ? 0.0 : nan;
            if (lane == 0) a.alive[b] = 0;
        } else {
            for (int e = lane; e < K * 6; e += 64) {
                const int k = e / 6, j = e - k * 6;
                xo[e] = (R)Z[k * n + j];
            }
            for (int e = lane; e < K * HODE_PF_MAX_AUX; e += 64) {
                const int k = e / HODE_PF_MAX_AUX, c = e - k * HODE_PF_MAX_AUX;
                R v = ai[c];                                    // the centre row's carried columns
                for (int p = 0; p < a.n_par; ++p)
                    if (a.col[p] == c) v = (R)Z[k * n + 6 + p];
                ao[e] = v;
            }
            for (int j = lane; j < n; j += 64) a.mean[b * n + j] = M[j];
            for (int e = lane; e < n * n; e += 64) a.cov[b * n * n + e] = P[e];
            if (lane < 6) {
                double mu = 0.0, var = 0.0;
                for (int k = 0; k < K; ++k) mu += (k == 0 ? a.wm0 : a.wi) * Z[k * n + lane];
                for (int k = 0; k < K; ++k) {
                    const double dv = Z[k * n + lane] - mu;
                    var += (k == 0 ? a.wc0 : a.wi) * (dv * dv);
                }
                st[4 + lane] = mu;
                st[10 + lane] = var;
            }
            if (lane == 0) {
                st[0] = inc;
                st[1] = nis;
                st[2] = (double)d;
                st[3] = 1.0;
                a.alive[b] = 1;
            }
        }
    }
}

template <typename R>
int ukf_step(void *stream, int B, int predict, int link, const int32_t *mode, double gamma, double wm0, double wc0, double wi, const R *x_in,
             const int32_t *status, const R *aux_in, const R *obs, const uint8_t *mask, const double *sigma, const double *q,
             const double *walk, const double *dt, int32_t *alive, double *mean, double *cov, R *x_out, R *aux_out, double *stats)
{
    if (B < 1 || (predict != 0 && predict != 1) || (link != HODE_PF_LINK_ADD && link != HODE_PF_LINK_LOG)) return HODE_EINVAL;
    if (!(gamma > 0.0) || !std::isfinite(gamma) || !std::isfinite(wm0) || !std::isfinite(wc0) || !std::isfinite(wi)) return HODE_EINVAL;
    if (!mode || !x_in || !aux_in || !obs || !sigma || !q || !walk || !dt || !alive || !mean || !cov || !x_out || !aux_out || !stats)
        return HODE_EINVAL;
    if (x_out == x_in || aux_out == aux_in) return HODE_EINVAL;
    UkfArgs<R> a{};
    for (int c = 0; c < HODE_PF_MAX_AUX; ++c) {
        if (mode[c] < HODE_PF_MOVE_CARRIED || mode[c] > HODE_PF_MOVE_LOG) return HODE_EINVAL;
        if (mode[c] != HODE_PF_MOVE_CARRIED) {
            a.col[a.n_par] = (int8_t)c;
            a.plog[a.n_par] = mode[c] == HODE_PF_MOVE_LOG ? 1 : 0;
            ++a.n_par;
        }
    }
    a.B = B; a.predict = predict; a.link = link; a.gamma = gamma; a.wm0 = wm0; a.wc0 = wc0; a.wi = wi;
    a.x_in = x_in; a.aux_in = aux_in; a.obs = obs; a.status = status; a.mask = mask; a.sigma = sigma; a.q = q; a.walk = walk; a.dt = dt;
    a.alive = alive; a.mean = mean; a.cov = cov; a.stats = stats; a.x_out = x_out; a.aux_out = aux_out;
    const size_t bytes = (size_t)kUkfPatients * ukf_doubles(6 + a.n_par) * sizeof(double);
    // (more than 64 KiB of dynamic LDS has to be asked for; n = 23 needs 86 KiB)
    if (bytes > 64 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void *>(&ukf_step_kernel<R>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 (int)(kUkfPatients * ukf_doubles(6 + HODE_PF_MAX_AUX) * sizeof(double))) != hipSuccess) {
        (void)hipGetLastError();
        return HODE_ELAUNCH;
    }
    hipLaunchKernelGGL((ukf_step_kernel<R>), dim3((B + kUkfPatients - 1) / kUkfPatients), dim3(kThreads), bytes, (hipStream_t)stream, a);
    return done();
}

}  // namespace
}  // namespace hode

extern "C" {

int hode_ukf_step_f32(void *stream, int B, int predict, int link, const int32_t *mode, double gamma, double wm0, double wc0, double wi,
                      const float *x_in, const int32_t *status, const float *aux_in, const float *obs, const uint8_t *mask,
                      const double *sigma, const double *q, const double *walk, const double *dt, int32_t *alive, double *mean,
                      double *cov, float *x_out, float *aux_out, double *stats)
{
    return hode::ukf_step<float>(stream, B, predict, link, mode, gamma, wm0, wc0, wi, x_in, status, aux_in, obs, mask, sigma, q, walk, dt,
                                 alive, mean, cov, x_out, aux_out, stats);
}
int hode_ukf_step_f64(void *stream, int B, int predict, int link, const int32_t *mode, double gamma, double wm0, double wc0, double wi,
                      const double *x_in, const int32_t *status, const double *aux_in, const double *obs, const uint8_t *mask,
                      const double *sigma, const double *q, const double *walk, const double *dt, int32_t *alive, double *mean,
                      double *cov, double *x_out, double *aux_out, double *stats)
{
    return hode::ukf_step<double>(stream, B, predict, link, mode, gamma, wm0, wc0, wi, x_in, status, aux_in, obs, mask, sigma, q, walk, dt,
                                  alive, mean, cov, x_out, aux_out, stats);
}

}  // extern "C"

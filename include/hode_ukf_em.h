/* hode_ukf_em.h -- the C ABI of the EM noise fit over the unscented RTS smoother, an extension of include/hode.h (which it
 * includes: the constants, the return codes and the conventions are that header's).  libhode.so exports these entries beside
 * those of hode.h; the Python binding keeps their prototypes in its own table (hode/_abi.py, EXTENSIONS). */
#ifndef HODE_UKF_EM_H
#define HODE_UKF_EM_H
#include "hode.h"
#ifdef __cplusplus
extern "C" {
#endif

#define HODE_UKF_EM_SUMS 37  /* sums: A [23] by coordinate (0 past n), N, D, R [6], M [6] */
#define HODE_UKF_EM_FIT 29   /* fit_mask / floor: q [6], walk [17] by column, sigma [6] */
#define HODE_UKF_EM_SLOTS 256 /* the patient slots of the M-step's reduction */

/* =====================================================================================================
 * EM for the noise of the unscented filter (inference/ukf.py, fit_ukf_noise): the expected sufficient statistics of
 * process_noise, the learned constants' walk and noise_sigma over a smoothed run (include/hode_ukf_smooth.h), and their
 * maximiser.  One E-step is hode_ukf_em_points, a forward solve of the rows it wrote over the segment of every pair,
 * hode_ukf_em_stats; hode_ukf_em_mstep reduces and updates.  One launch each, no seed, nothing on the host.
 *
 * Sizes and layout: n, K, the coordinates (0..5 the states, 6..n-1 the learned columns, ascending), mode [17] and the links as
 * for hode_ukf_step; S >= 1 steps, step-major as in hode_ukf_smooth.h: step s of patient b is item s * B + b, a pair (s, s + 1),
 * 0 <= s < S - 1, is item s * B + b of x_em, aux_em, chol, prop_em, status, gain, e2, pair_ok.  mean_s, cov_s, gain, moments
 * are the smoother's outputs, alive and dt its inputs.  mode, gamma, wm0, wc0, wi, fit_mask, floor are on the HOST, every
 * other array on the DEVICE.  With S == 1 there are no pairs: the pair arrays may be NULL and are not touched.
 *
 * Everything is computed in fp64; a * b + c is two roundings; every sum starts at 0.0 and runs in index order, a sum over the
 * points with the weight multiplied first, a substitution subtracting its terms from the right-hand side in index order.
 *
 * hode_ukf_em_points: a wave per pair.  L = the column Cholesky factor of cov_s[s] as in phase b of hode_ukf_step, zero columns
 *   included; chi_k = the points of (mean_s[s], L) with gamma as there; x_em[k] = g^-1(chi_k) on the states and aux_em[k] = the
 *   row ode_history[s][b * K] with the learned columns replaced by phi^-1(chi_k), rounded to the data type, exactly as phase d
 *   of hode_ukf_step forms x_out / aux_out.  chol = L.  A pair into a dead step (alive[s + 1] == 0): x_em is 1 everywhere,
 *   aux_em the row ode_history[s][b * K] unchanged, chol NaN -- rows a solve can take, whose images are not read.
 *   x_em [S-1][B*K][6], aux_em [S-1][B*K][17] in the data type, chol [S-1][B][n][n] fp64.
 *
 * hode_ukf_em_stats: a wave per (s, b), S * B of them.  prop_em [S-1][B*K][6]: the end of the solve of x_em / aux_em over the
 *   segment of step s + 1; status [S-1][B*K] int32: that solve's.
 *   c. Pair statistic (s < S - 1).  chi_k again from (mean_s[s], chol); zeta+_k = (g(prop_em[k]), chi_k[6..n-1]);
 *      fbar = sum wm_k zeta+_k; F_i = sum wc_k (zeta+_k,i - fbar_i)^2; U[j][i] = (wi * gamma) * (zeta+_{1+j},i - zeta+_{1+n+j},i),
 *      a zero row for a zero column j of chol (chol[j][j] == 0); V = L^-T U column by column, p descending,
 *      V[p][i] = (U[p][i] - sum_{c>p} L[c][p] V[c][i]) / L[p][p], c ascending, a zero column p gives V[p][i] = 0;
 *      W[i][b] = sum_a cov_s[s+1][i][a] gain[s][b][a]; cross_i = sum_b W[i][b] V[b][i]; d_i = mean_s[s+1][i] - fbar_i;
 *      e2[i] = ((cov_s[s+1][i][i] + d_i * d_i) - 2 cross_i) + F_i: the expected squared residual of coordinate i over the pair.
 *      pair_ok = 1 if alive[s + 1] != 0, every status row of the pair is 0 and every state of prop_em is finite (and positive
 *      under the log link); otherwise pair_ok = 0 and e2 is NaN.  e2 [S-1][B][n] fp64, pair_ok [S-1][B] int32.
 *   d. Observation statistic (every s).  Entry j is seen if obs[b][s][j] is finite, mask is NULL or mask[b][s][j] != 0, and
 *      alive[s] != 0: r2[j] = (obs_j - moments[j])^2 + moments[6 + j]; an unseen entry is 0.0 and no arithmetic touches its obs.
 *      obs [B][S][6] in the data type and mask [B][S][6] uint8 or NULL are PATIENT-major (the rows of the record at the steps);
 *      r2 [S][B][6] fp64; seen [S][B] int32: bit j set for a seen entry.
 *
 * hode_ukf_em_mstep: one workgroup.  Per patient, s ascending from 0.0: a_i = sum e2[s][i] / dt[s+1] over the pairs with
 *   pair_ok, their number n_b and d_b = sum dt[s+1]; r_j = sum r2[s][j] and m_j = the count over the seen entries.  Over the
 *   patients: slot t = b mod 256 adds its patients' values in ascending b from 0.0; then for h = 128, 64, .. 1 slot t < h adds
 *   slot t + h to itself; slot 0 is the total.  The shape depends on B alone.  sums = A [23] (0 past n), N, D, R [6], M [6].
 *   New values, written in place: q[i] of a state under the additive link and walk[c] of a learned column c at coordinate i:
 *   v = A_i / N; q[i] under the log link, whose -v dt / 2 drift depends on v: the maximiser of -(N/2) log v - A / (2 v) - v D / 8,
 *   v = 2 (sqrt(N^2 + A D) - N) / D, evaluated as (2 A) / (sqrt(N * N + A * D) + N) (the same number without the cancellation);
 *   the new value is max(sqrt(v), floor).  sigma[j] = max(sqrt(R_j / M_j), floor).  A value stays as it is, bit for bit, when its
 *   fit_mask flag is 0, when it is exactly 0, when N == 0 (M_j == 0 for sigma), and walk[c] of a carried column always.
 *
 * There are no atomics and every sum runs in a fixed order: the same call gives the same bits, and an item's bits of
 * x_em, aux_em, chol, e2, pair_ok, r2, seen depend neither on B nor on its row.
 *
 * HODE_EINVAL (nothing launched): S < 1, B < 1, link not 0 or 1, a NULL mode or a mode value outside 0..2, gamma not finite or
 * not positive, a non-finite wm0, wc0 or wi; a NULL among the arrays (the pair arrays only with S > 1; mask may always be NULL);
 * an output that is an input or another output; for the M-step also a NULL fit_mask or floor, a fit_mask value outside 0..1, a
 * floor that is not finite or negative.  HODE_EUNSUPPORTED: never.
 * ===================================================================================================== */
int hode_ukf_em_points_f32(void *stream, int S, int B, int link, const int32_t *mode, double gamma, const double *mean_s,
                           const double *cov_s, const int32_t *alive, const float *ode_history, float *x_em, float *aux_em, double *chol);
int hode_ukf_em_points_f64(void *stream, int S, int B, int link, const int32_t *mode, double gamma, const double *mean_s,
                           const double *cov_s, const int32_t *alive, const double *ode_history, double *x_em, double *aux_em, double *chol);
int hode_ukf_em_stats_f32(void *stream, int S, int B, int link, const int32_t *mode, double gamma, double wm0, double wc0, double wi,
                          const float *prop_em, const int32_t *status, const double *chol, const double *mean_s, const double *cov_s,
                          const double *gain, const int32_t *alive, const float *obs, const uint8_t *mask, const double *moments,
                          double *e2, int32_t *pair_ok, double *r2, int32_t *seen);
int hode_ukf_em_stats_f64(void *stream, int S, int B, int link, const int32_t *mode, double gamma, double wm0, double wc0, double wi,
                          const double *prop_em, const int32_t *status, const double *chol, const double *mean_s, const double *cov_s,
                          const double *gain, const int32_t *alive, const double *obs, const uint8_t *mask, const double *moments,
                          double *e2, int32_t *pair_ok, double *r2, int32_t *seen);
int hode_ukf_em_mstep(void *stream, int S, int B, int link, const int32_t *mode, const int32_t *fit_mask, const double *floor,
                      const double *e2, const int32_t *pair_ok, const double *r2, const int32_t *seen, const double *dt, double *q,
                      double *walk, double *sigma, double *sums);

#ifdef __cplusplus
}
#endif
#endif /* HODE_UKF_EM_H */

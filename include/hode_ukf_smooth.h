/* hode_ukf_smooth.h -- the C ABI of the unscented RTS smoother, an extension of include/hode.h (which it includes: the constants,
 * the return codes and the conventions are that header's).  libhode.so exports these entries beside those of hode.h; the Python
 * binding keeps their prototypes in its own table (hode/_abi.py, EXTENSIONS). */
#ifndef HODE_UKF_SMOOTH_H
#define HODE_UKF_SMOOTH_H
#include "hode.h"
#ifdef __cplusplus
extern "C" {
#endif

/* =====================================================================================================
 * Unscented RTS smoother (inference/ukf.py, UKFResult.smooth): the unscented Rauch-Tung-Striebel pass (Sarkka 2008) over a stored
 * run of hode_ukf_step -- the mean and covariance of every step given the whole record, the smoother gains and the predicted
 * moments they were formed from.  Three launches on the stream whatever S is (two with S == 1), no seed, nothing on the host.
 *
 * Sizes and layout: n, K, the coordinates and mode [17] as for hode_ukf_step.  S >= 1 filter steps, step-major: step s of patient
 * b is item s * B + b of every array below; a pair (s, s + 1), 0 <= s < S - 1, is item s * B + b of gain, pred_mean, pred_cov.
 *
 * Arguments (DEVICE unless noted): S, B, link on the host; mode [17] int32, gamma, wm0, wc0, wi on the HOST as for
 * hode_ukf_step; history [S][B*K][6] and ode_history [S][B*K][17]: x_out and aux_out of every step as stored; propagated
 * [S][B*K][6]: the x_in handed to every step (slab 0, and whatever slab belongs to a step without a prediction, is not read);
 * mean_f [S][B][n], cov_f [S][B][n][n] fp64: mean and cov after every step; alive [S][B] int32: the flag after every step (once
 * 0 it stays 0); q [6], walk [17] fp64; dt [S][B] fp64: the dt every step received (row 0 is not read).  Outputs, all fp64:
 * mean_s [S][B][n], cov_s [S][B][n][n], gain [S-1][B][n][n], pred_mean [S-1][B][n], pred_cov [S-1][B][n][n] (the three may be
 * NULL with S == 1), moments [S][B][12].
 *
 * Everything is computed in fp64; a * b + c is two roundings; every sum starts at 0.0 and runs in index order, a sum over the
 * points with the weight multiplied first, a substitution subtracting its terms from the right-hand side in index order.
 *  a. Points (per pair).  zeta_k = (g(history[s][k]), phi(ode_history[s][k][cols])): the emitted points of step s in link space;
 *     zeta+_k = (g(propagated[s+1][k]), phi(ode_history[s][k][cols])): their images (a solve does not change the constants).
 *  b. Predicted moments.  mt = sum wm_k zeta+_k; P- = sum wc_k (zeta+_k - mt)(zeta+_k - mt)^T + diag(s^2) with s^2 from q, walk
 *     and dt[s+1] as in phase a of hode_ukf_step; m- = mt, minus 0.5 s_j^2 on the states under the log link.  These are the step's m-
 *     and P- bit for bit.  pred_mean = m-, pred_cov = P-.
 *  c. Cross covariance.  C = sum wc_k (zeta_k - mean_f[s])(zeta+_k - mt)^T (the images about their pre-drift mean).
 *  d. Gain.  G = C (P-)^-1 through L = the column Cholesky factor of P- as in phase b of hode_ukf_step, zero columns included.  Row i:
 *     forward, p ascending, w_p = (C_ip - sum_{c<p} L_pc w_c) / L_pp; backward, p descending, g_p = (w_p - sum_{c>p} L_cp g_c)
 *     / L_pp, c ascending; a zero column p gives w_p = g_p = 0: a coordinate the filter holds exactly takes nothing from the
 *     future and gives nothing.  gain = G.
 *  e. Recursion (per patient, s = S - 2 .. 0).  delta = ms_{s+1} - m-, D = Ps_{s+1} - P-; ms_s[i] = mean_f[s][i] + sum_j G_ij
 *     delta_j; T_ik = sum_j G_ij D_jk, U_ij = sum_k T_ik G_jk; Ps_s[i][j] = 0.5 ((P_s[i][j] + U_ij) + (P_s[j][i] + U_ji)) with
 *     P_s = cov_f[s].  At the terminal step ms, Ps are mean_f, cov_f bit for bit.
 *  f. Natural-space moments (per step).  The points of (ms, Ps) as in phase d of hode_ukf_step, mapped with g^-1; moments [0..5] =
 *     sum wm_k x_k, [6..11] = sum wc_k (x_k - mean)^2 of the six states: at the terminal step the step's stats [4..15] bit for bit.
 *
 * Lost patients: a patient's terminal step is its last alive one; every later step is NaN in mean_s, cov_s and moments, and so
 * is every pair into a dead step in gain, pred_mean and pred_cov; a patient dead at step 0 is NaN throughout.  The other
 * patients are untouched.
 *
 * There are no atomics and every sum runs in a fixed order: the same call gives the same bits, and an item's bits depend neither
 * on B nor on its row.
 *
 * HODE_EINVAL (nothing launched): S < 1, B < 1, link not 0 or 1, a mode value outside 0..2, gamma not finite or not positive, a
 * non-finite wm0, wc0 or wi, a NULL among mode, the inputs, mean_s, cov_s, moments (and, with S > 1, gain, pred_mean, pred_cov),
 * an output that is an input or another output.  HODE_EUNSUPPORTED: never.
 * ===================================================================================================== */
int hode_ukf_smooth_f32(void *stream, int S, int B, int link, const int32_t *mode, double gamma, double wm0, double wc0, double wi,
                        const float *history, const float *ode_history, const float *propagated, const double *mean_f,
                        const double *cov_f, const int32_t *alive, const double *q, const double *walk, const double *dt,
                        double *mean_s, double *cov_s, double *gain, double *pred_mean, double *pred_cov, double *moments);
int hode_ukf_smooth_f64(void *stream, int S, int B, int link, const int32_t *mode, double gamma, double wm0, double wc0, double wi,
                        const double *history, const double *ode_history, const double *propagated, const double *mean_f,
                        const double *cov_f, const int32_t *alive, const double *q, const double *walk, const double *dt,
                        double *mean_s, double *cov_s, double *gain, double *pred_mean, double *pred_cov, double *moments);

#ifdef __cplusplus
}
#endif
#endif /* HODE_UKF_SMOOTH_H */

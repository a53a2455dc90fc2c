// hode_capi.hip -- extern "C" entry points of libhode.so (declared in include/hode.h).
// Plain pointers and sizes only; argument validation happens here, on the host, BEFORE any
// launch: a kernel is never started on shapes it was not compiled for.
#include "hode_kernels.h"
#include <math.h>
#include <string.h>

using namespace hode;

namespace {

inline bool mode_ok(int mode, const void *p) { return mode == 0 || (p != nullptr && (mode == 1 || mode == 2)); }

template <typename R>
int solve_fwd(void *stream, int B, int T, const R *x0, const R *t, int t_batched, const R *meal, int meal_mode,
              const R *tvns, int tvns_mode, const R *gd, int gd_mode, const R *ode_p, const R *nn_p, int n_sets,
              int H, int L, int method, double rtol, double atol, int max_steps, R *y, int32_t *status,
              int32_t *nsteps, int32_t *nfev, void *tape)
{
    if (B == 0 && T >= 1) return HODE_OK;                     // an empty batch is valid (empty tensors have null data)
    if (B < 0 || T < 1 || !x0 || !t || !ode_p || !nn_p || !y || !status) return HODE_EINVAL;
    if (!mode_ok(meal_mode, meal) || !mode_ok(tvns_mode, tvns) || !mode_ok(gd_mode, gd)) return HODE_EINVAL;
    if (n_sets < 1 || (B % n_sets) != 0 || max_steps < 1) return HODE_EINVAL;
    if (method != HODE_METHOD_DP54 && method != HODE_METHOD_RK4) return HODE_EINVAL;
    if (!(rtol >= 0) || !(atol >= 0) || (method == HODE_METHOD_DP54 && rtol == 0 && atol == 0)) return HODE_EINVAL;
    if (H < 1 || H > HODE_MAX_HIDDEN || layers_of(L) < 1 || layers_of(L) > HODE_MAX_LAYERS || act_of(L) > HODE_ACT_LEAKY_RELU || (L >> 17) != 0)
        return HODE_EUNSUPPORTED;
    const bool nn_shared = (L & HODE_LAYERS_NN_SHARED) != 0;   // one network for every set of constants (forward only)
    if (nn_shared && tape) return HODE_EUNSUPPORTED;          // (the adjoint writes one gradient row per parameter set)
    L &= 0xffff;
    if (B == 0) return HODE_OK;
    SolveArgs<R> a;
    a.B = B; a.T = T; a.t_batched = t_batched ? 1 : 0;
    a.meal_mode = meal_mode; a.tvns_mode = tvns_mode; a.gd_mode = gd_mode;
    a.n_sets = n_sets; a.H = H; a.P = nn_param_count(H, L); a.max_steps = max_steps;
    a.x0 = x0; a.t = t; a.meal = meal; a.tvns = tvns; a.gd = gd; a.ode_p = ode_p; a.nn_p = nn_p;
    a.rtol = (R)rtol; a.atol = (R)atol;
    a.y = y; a.status = status; a.nsteps = nsteps; a.nfev = nfev;
    a.tape = (R *)tape;
    a.tape_seg = tape ? (int32_t *)((char *)tape + tape_seg_offset(B, max_steps, sizeof(R))) : nullptr;
    a.tape_stage = tape ? (R *)((char *)tape + tape_stage_offset(B, max_steps, sizeof(R))) : nullptr;
    a.L = layers_of(L);
    a.act = act_of(L);
    a.nn_stride = nn_shared ? 0 : a.P;
    if (!tuned_shape(H, L)) return launch_solve_fwd_generic<R>((hipStream_t)stream, a, method);
    return launch_solve_fwd<R>((hipStream_t)stream, a, layers_of(L), method);
}

template <typename R>
int rhs_fwd(void *stream, int B, const R *x, const R *t, const R *meal, const R *tvns, const R *gd, const R *ode_p,
            const R *nn_p, int H, int L, R *out)
{
    if (B == 0) return HODE_OK;
    if (B < 0 || !x || !ode_p || !nn_p || !out) return HODE_EINVAL;
    if (H < 1 || H > HODE_MAX_HIDDEN || layers_of(L) < 1 || layers_of(L) > HODE_MAX_LAYERS || act_of(L) > HODE_ACT_LEAKY_RELU || (L >> 16) != 0)
        return HODE_EUNSUPPORTED;
    if (B == 0) return HODE_OK;
    RhsArgs<R> a{};
    a.B = B; a.H = H; a.P = nn_param_count(H, L);
    a.x = x; a.t = t; a.meal = meal; a.tvns = tvns; a.gd = gd; a.ode_p = ode_p; a.nn_p = nn_p; a.out = out;
    a.act = act_of(L);
    if (!tuned_shape(H, L)) return launch_rhs_fwd_generic<R>((hipStream_t)stream, a, layers_of(L));
    return launch_rhs_fwd<R>((hipStream_t)stream, a, layers_of(L));
}

template <typename R>
int solve_bwd(void *stream, int B, int T, const R *t, int t_batched, const R *meal, int meal_mode, const R *tvns,
              int tvns_mode, const R *gd, int gd_mode, const R *ode_p, const R *nn_p, int n_sets, int H, int L,
              int method, int max_steps, const int32_t *nsteps, const int32_t *status, void *tape, const R *gy,
              R *gx0, R *gnn, R *gode, R *gmeal = nullptr, R *gtvns = nullptr, R *ggd = nullptr)
{
    // a gradient is only defined for an input that is there (mode 1 or 2)
    if ((gmeal && meal_mode == 0) || (gtvns && tvns_mode == 0) || (ggd && gd_mode == 0)) return HODE_EINVAL;
    if (B == 0 && T >= 1) return HODE_OK;
    if (B < 0 || T < 1 || !t || !ode_p || !nn_p || !nsteps || !status || !tape || !gy || !gx0) return HODE_EINVAL;
    if (!mode_ok(meal_mode, meal) || !mode_ok(tvns_mode, tvns) || !mode_ok(gd_mode, gd)) return HODE_EINVAL;
    if (n_sets < 1 || (B % n_sets) != 0 || max_steps < 1) return HODE_EINVAL;
    if (method != HODE_METHOD_DP54 && method != HODE_METHOD_RK4) return HODE_EINVAL;
    if (H < 1 || H > HODE_MAX_HIDDEN || layers_of(L) < 1 || layers_of(L) > HODE_MAX_LAYERS || act_of(L) > HODE_ACT_LEAKY_RELU || (L >> 16) != 0)
        return HODE_EUNSUPPORTED;
    if (B == 0) return HODE_OK;
    AdjArgs<R> a;
    a.B = B; a.T = T; a.t_batched = t_batched ? 1 : 0;
    a.meal_mode = meal_mode; a.tvns_mode = tvns_mode; a.gd_mode = gd_mode;
    a.n_sets = n_sets; a.H = H; a.P = nn_param_count(H, L); a.max_steps = max_steps;
    a.t = t; a.meal = meal; a.tvns = tvns; a.gd = gd; a.ode_p = ode_p; a.nn_p = nn_p;
    a.nsteps = nsteps; a.status = status;
    a.tape = (const R *)tape;
    a.tape_seg = (const int32_t *)((const char *)tape + tape_seg_offset(B, max_steps, sizeof(R)));
    a.tape_stage = (const R *)((const char *)tape + tape_stage_offset(B, max_steps, sizeof(R)));
    a.gy = gy; a.gx0 = gx0; a.gnn = gnn; a.gode = gode;
    a.tape_delta = has_delta_tape(sizeof(R), H, L) ? (R *)((char *)tape + tape_delta_offset(B, max_steps, sizeof(R), H, L)) : nullptr;
    a.partials = (tuned_shape(H, L) || sizeof(R) == 4) ? (R *)((char *)tape + tape_partials_offset(B, max_steps, sizeof(R), H, L)) : nullptr;
    a.partial_rows = adj_partial_rows(B);
    a.act = act_of(L);
    if (gmeal || gtvns || ggd) {
        // input gradients: kernels of their own (include/hode.h); without them every call takes the path it took before
        AdjInArgs<R> ai;
        static_cast<AdjArgs<R> &>(ai) = a;
        ai.gmeal = gmeal; ai.gtvns = gtvns; ai.ggd = ggd;
        if (!tuned_shape(H, L)) return launch_solve_bwd_generic_gin<R>((hipStream_t)stream, ai, layers_of(L), method);
        return launch_solve_bwd_inputs<R>((hipStream_t)stream, ai, layers_of(L), method);
    }
    if (!tuned_shape(H, L)) return launch_solve_bwd_generic<R>((hipStream_t)stream, a, layers_of(L), method);
    return launch_solve_bwd<R>((hipStream_t)stream, a, layers_of(L), method);
}

// tangent-linear solve (hode_solve_jvp_*): host checks first -- directions, modes, shapes -- then one launch
// ANY (hode_solve_jvp_any_*): every shape the forward can tape; otherwise the tuned shapes only, the documented envelope of K6
template <typename R, bool ANY = false>
int solve_jvp(void *stream, int B, int T, const R *t, int t_batched, const R *meal, int meal_mode, const R *tvns, int tvns_mode,
              const R *gd, int gd_mode, const R *ode_p, const R *nn_p, int n_sets, int H, int L, int method, int max_steps,
              const int32_t *nsteps, const int32_t *status, const void *tape, int K, const R *v_ode, const R *v_x0, R *dy)
{
    if (K < 1 || (!v_ode && !v_x0)) return HODE_EINVAL;
    if (B == 0 && T >= 1) return HODE_OK;
    if (B < 0 || T < 1 || !t || !ode_p || !nn_p || !nsteps || !status || !tape || !dy) return HODE_EINVAL;
    if (!mode_ok(meal_mode, meal) || !mode_ok(tvns_mode, tvns) || !mode_ok(gd_mode, gd)) return HODE_EINVAL;
    if (n_sets < 1 || (B % n_sets) != 0 || max_steps < 1) return HODE_EINVAL;
    if (method != HODE_METHOD_DP54 && method != HODE_METHOD_RK4) return HODE_EINVAL;
    // tuned shapes only (H <= 64, L <= 4, ReLU, one network per parameter set): the physics-on configurations
    if (H < 1 || layers_of(L) < 1 || (L >> 16) != 0 || (!ANY && !tuned_shape(H, L))) return HODE_EUNSUPPORTED;
    if (H > HODE_MAX_HIDDEN || layers_of(L) > HODE_MAX_LAYERS || act_of(L) > HODE_ACT_LEAKY_RELU) return HODE_EUNSUPPORTED;
    JvpArgs<R> a;
    a.B = B; a.T = T; a.t_batched = t_batched ? 1 : 0; a.gd_mode = gd_mode;
    a.n_sets = n_sets; a.H = H; a.P = nn_param_count(H, L); a.max_steps = max_steps; a.K = K;
    a.t = t; a.ode_p = ode_p; a.nn_p = nn_p;
    a.nsteps = nsteps; a.status = status;
    a.tape = (const R *)tape;
    a.tape_seg = (const int32_t *)((const char *)tape + tape_seg_offset(B, max_steps, sizeof(R)));
    a.tape_stage = (const R *)((const char *)tape + tape_stage_offset(B, max_steps, sizeof(R)));
    a.v_ode = v_ode; a.v_x0 = v_x0; a.dy = dy;
    if (!tuned_shape(H, L)) return launch_solve_jvp_generic<R>((hipStream_t)stream, a, layers_of(L), act_of(L), method);
    return launch_solve_jvp<R>((hipStream_t)stream, a, layers_of(L), method);
}

template <typename R>
int rhs_bwd(void *stream, int B, const R *x, const R *t, const R *meal, const R *tvns, const R *gd, const R *ode_p,
            const R *nn_p, int H, int L, const R *gout, R *gx, R *gt, R *gnn, R *gode, R *gmeal = nullptr, R *gtvns = nullptr,
            R *ggd = nullptr)
{
    if ((gmeal && !meal) || (gtvns && !tvns) || (ggd && !gd)) return HODE_EINVAL;
    if (B == 0) return HODE_OK;
    if (B < 0 || !x || !ode_p || !nn_p || !gout || !gx) return HODE_EINVAL;
    if (H < 1 || H > HODE_MAX_HIDDEN || layers_of(L) < 1 || layers_of(L) > HODE_MAX_LAYERS || act_of(L) > HODE_ACT_LEAKY_RELU || (L >> 16) != 0)
        return HODE_EUNSUPPORTED;
    if (B == 0) return HODE_OK;
    RhsArgs<R> a{};
    a.B = B; a.H = H; a.P = nn_param_count(H, L);
    a.x = x; a.t = t; a.meal = meal; a.tvns = tvns; a.gd = gd; a.ode_p = ode_p; a.nn_p = nn_p;
    a.gout = gout; a.gx = gx; a.gt = gt; a.gnn = gnn; a.gode = gode;
    a.act = act_of(L);
    a.gmeal = gmeal; a.gtvns = gtvns; a.ggd = ggd;
    if (!tuned_shape(H, L)) return launch_rhs_bwd_generic<R>((hipStream_t)stream, a, layers_of(L));
    return launch_rhs_bwd<R>((hipStream_t)stream, a, layers_of(L));
}

// ---- MCMC (hode_hmc.hip): sizes and pointers checked here, before any launch
inline bool chains_ok(int C, int D, int ld) { return C >= 1 && D >= 1 && ld >= D && (int64_t)C * ld <= ((int64_t)1 << 40); }

template <typename R> int mse_sets(void *stream, int n_sets, int64_t len, const R *y, const R *obs, R scale, double *loss_sum, R *gy)
{
    if (n_sets < 0 || len < 0) return HODE_EINVAL;
    if (n_sets == 0 || len == 0) return HODE_OK;
    if (!y || !obs || !loss_sum) return HODE_EINVAL;
    return launch_mse_sets<R>((hipStream_t)stream, n_sets, len, y, obs, scale, loss_sum, gy);
}

template <typename R> int obs_nll_sets(void *stream, int n_sets, int64_t len, const R *y, const R *obs, const uint8_t *mask, int mode, int flags,
                                       const double *w, const double *a, const double *b, const double *n, double *sse, double *loss_sum, R *gy)
{
    if (n_sets < 0 || len < 0 || (mode != HODE_OBS_FIXED && mode != HODE_OBS_MARGINAL) || flags < 0 || flags > HODE_OBS_FROM_SSE)
        return HODE_EINVAL;
    if (mode == HODE_OBS_FIXED ? !w : (!a || !b || !n)) return HODE_EINVAL;
    for (int k = 0; k < 6; ++k) {
        if (mode == HODE_OBS_FIXED ? !(w[k] > 0.0) : (!(a[k] > 0.0) || !(b[k] > 0.0) || !(n[k] >= 0.0))) return HODE_EINVAL;
    }
    if (n_sets == 0 || len == 0) return HODE_OK;
    if (!y || !obs || !sse) return HODE_EINVAL;
    ObsArgs<R> o{};
    o.n_sets = n_sets; o.mode = mode; o.flags = flags; o.len = len; o.y = y; o.obs = obs; o.mask = mask;
    o.w = w; o.a = a; o.b = b; o.n = n; o.sse = sse; o.loss_sum = loss_sum; o.gy = gy;
    return launch_obs_nll_sets<R>((hipStream_t)stream, o);
}

template <typename R> int hmc_refresh(void *stream, int C, int D, int ld, uint64_t seed, uint32_t iter, double jitter, const R *minv,
                                      const double *log_eps, const R *z, const R *g, const double *U, R *p, R *z0, R *g0, double *U0,
                                      double *ke0, double *eps, int32_t *failed)
{
    if (!chains_ok(C, D, ld) || !(jitter >= 0.0 && jitter < 1.0)) return HODE_EINVAL;
    if (!minv || !log_eps || !z || !g || !U || !p || !z0 || !g0 || !U0 || !ke0 || !eps || !failed) return HODE_EINVAL;
    HmcRefreshArgs<R> a{C, D, ld, seed, iter, jitter, minv, log_eps, z, g, U, p, z0, g0, U0, ke0, eps, failed};
    return launch_hmc_refresh<R>((hipStream_t)stream, a);
}

template <typename R> int hmc_leapfrog(void *stream, int C, int D, int ld, int flags, double kick, const double *eps, const R *minv,
                                       R *z, R *p, R *g, const R *gnn, const R *gode, int P, const double *loss_sum, double lik_scale,
                                       const int32_t *status, int n_traj, double *U, double *ke, int32_t *failed, uint32_t ode_mask,
                                       const double *mu, const double *sd, int sample_nn, R *nn_p, R *ode_p)
{
    if (!chains_ok(C, D, ld) || (flags & ~31) || (ode_mask >> 17)) return HODE_EINVAL;
    const int n_ode = __builtin_popcount(ode_mask);
    if (P < 0 || (sample_nn && P < 1) || D != n_ode + (sample_nn ? P : 0) || (status && n_traj < 1)) return HODE_EINVAL;
    if (!eps || !minv || !z || !p || !g) return HODE_EINVAL;
    if (n_ode && (!mu || !sd)) return HODE_EINVAL;
    if ((flags & HODE_HMC_ASSEMBLE) && (!U || !failed || (sample_nn && gode && !gnn))) return HODE_EINVAL;
    if ((flags & HODE_HMC_KE) && !ke) return HODE_EINVAL;
    if ((flags & (HODE_HMC_DRIFT | HODE_HMC_PARAMS)) && ((n_ode && !ode_p) || (sample_nn && !nn_p))) return HODE_EINVAL;
    HmcLeapfrogArgs<R> a;
    a.C = C; a.D = D; a.ld = ld; a.flags = flags; a.P = P; a.n_traj = n_traj; a.n_ode = n_ode; a.sample_nn = sample_nn ? 1 : 0;
    a.kick = kick; a.lik_scale = lik_scale; a.ode_mask = ode_mask; a.eps = eps; a.minv = minv; a.z = z; a.p = p; a.g = g;
    a.gnn = gnn; a.gode = gode; a.loss_sum = loss_sum; a.status = status; a.U = U; a.ke = ke; a.failed = failed; a.mu = mu;
    a.sd = sd; a.nn_p = nn_p; a.ode_p = ode_p;
    return launch_hmc_leapfrog<R>((hipStream_t)stream, a);
}

template <typename R> int hmc_accept(void *stream, int C, int D, int ld, int mode, uint64_t seed, uint32_t iter, double target_accept,
                                     R *z, const R *z0, R *g, const R *g0, double *U, const double *U0, const double *ke0,
                                     const double *ke, const int32_t *failed, double *log_eps, double *da, int32_t *search, int n_ode,
                                     const double *mu, const double *sd, R *draws, double *stats, int n_slots, int slot)
{
    if (!chains_ok(C, D, ld) || mode < HODE_HMC_SAMPLE || mode > HODE_HMC_DA_FINISH || n_ode < 0 || n_ode > 17 || n_ode > D)
        return HODE_EINVAL;
    if (!(target_accept > 0.0 && target_accept < 1.0)) return HODE_EINVAL;
    if (!z || !z0 || !g || !g0 || !U || !U0 || !ke0 || !ke || !failed || !log_eps || !da || !search) return HODE_EINVAL;
    if (n_ode && (!mu || !sd)) return HODE_EINVAL;
    if (slot >= 0 && (slot >= n_slots || !stats)) return HODE_EINVAL;
    HmcAcceptArgs<R> a;
    a.C = C; a.D = D; a.ld = ld; a.mode = mode; a.n_ode = n_ode; a.n_slots = n_slots; a.slot = slot < 0 ? -1 : slot;
    a.seed = seed; a.iter = iter; a.delta = target_accept; a.z = z; a.z0 = z0; a.g = g; a.g0 = g0; a.U = U; a.U0 = U0; a.ke0 = ke0;
    a.ke = ke; a.failed = failed; a.log_eps = log_eps; a.da = da; a.search = search; a.mu = mu; a.sd = sd; a.draws = draws;
    a.stats = stats;
    return launch_hmc_accept<R>((hipStream_t)stream, a);
}

template <typename R> int hmc_welford(void *stream, int C, int D, int ld, int flags, const R *z, double *wf, R *minv)
{
    if (!chains_ok(C, D, ld) || flags < 1 || flags > 3 || !wf) return HODE_EINVAL;
    if (((flags & HODE_HMC_WELFORD_ACCUM) && !z) || ((flags & HODE_HMC_WELFORD_FINISH) && !minv)) return HODE_EINVAL;
    return launch_hmc_welford<R>((hipStream_t)stream, C, D, ld, flags, z, wf, minv);
}

// ---- population model (hode_population.hip)
inline bool pop_ok(int A, int B, int K, int ld, uint32_t ode_mask)
{
    return A >= 0 && B >= 1 && K >= 1 && K <= 17 && !(ode_mask >> 17) && __builtin_popcount(ode_mask) == K && ld >= (int64_t)K * (B + 2) &&
           (int64_t)A * ld <= ((int64_t)1 << 40) && (int64_t)A * B <= ((int64_t)1 << 36);
}

template <typename R> int pop_params(void *stream, int A, int B, int K, int ld, const R *coords, uint32_t ode_mask, const double *mu0,
                                     const double *sd0, const double *tau0, double tau_log_sd, const R *ode_base, R *ode_p)
{
    if (!pop_ok(A, B, K, ld, ode_mask)) return HODE_EINVAL;
    if (A == 0) return HODE_OK;
    if (!coords || !mu0 || !sd0 || !tau0 || !ode_base || !ode_p) return HODE_EINVAL;
    return launch_pop_params<R>((hipStream_t)stream, A, B, K, ld, coords, ode_mask, mu0, sd0, tau0, tau_log_sd, ode_base, ode_p);
}

template <typename R> int pop_grad(void *stream, int A, int B, int K, int ld, const R *coords, const R *gode, uint32_t ode_mask,
                                   const double *sd0, const double *tau0, double tau_log_sd, R *glik)
{
    if (!pop_ok(A, B, K, ld, ode_mask)) return HODE_EINVAL;
    if (A == 0) return HODE_OK;
    if (!coords || !gode || !sd0 || !tau0 || !glik) return HODE_EINVAL;
    return launch_pop_grad<R>((hipStream_t)stream, A, B, K, ld, coords, gode, ode_mask, sd0, tau0, tau_log_sd, glik);
}

// ---- initial-state model (hode_x0.hip)
inline bool x0_ok(int A, int B, int n_lat, int ld, int off, uint32_t lat_mask, int link, int K, uint32_t ode_mask, bool with_ode)
{
    if (A < 1 || B < 1 || n_lat < 1 || n_lat > 6 || (lat_mask >> 6) || __builtin_popcount(lat_mask) != n_lat) return false;
    if (K < 0 || K > 17 || (ode_mask >> 17) || __builtin_popcount(ode_mask) != K || (link != 0 && link != 1)) return false;
    if (off < 0 || (with_ode && off < K) || ld < off + (int64_t)B * n_lat) return false;
    return (int64_t)A * ld <= ((int64_t)1 << 40) && (int64_t)A * B <= ((int64_t)1 << 36) && B <= (1 << 21);   // (tiles in grid.y)
}

template <typename R> int x0_params(void *stream, int A, int B, int n_lat, int ld, int off, const R *coords, uint32_t lat_mask, int link,
                                    const double *m, const double *s, const R *x0_base, R *x0_out, int K, uint32_t ode_mask,
                                    const double *mu, const double *sd, const R *ode_base, R *ode_p)
{
    if (!x0_ok(A, B, n_lat, ld, off, lat_mask, link, K, ode_mask, ode_p != nullptr)) return HODE_EINVAL;
    if (!coords || !m || !s || !x0_base || !x0_out) return HODE_EINVAL;
    if (ode_p && (!ode_base || (K > 0 && (!mu || !sd)))) return HODE_EINVAL;
    return launch_x0_params<R>((hipStream_t)stream, A, B, n_lat, ld, off, coords, lat_mask, link, m, s, x0_base, x0_out, ode_mask, mu, sd,
                               ode_base, ode_p);
}

template <typename R> int x0_grad(void *stream, int A, int B, int n_lat, int ld, int off, const R *coords, uint32_t lat_mask, int link,
                                  const double *m, const double *s, const R *gx0, int K, uint32_t ode_mask, const double *sd, const R *gode,
                                  R *glik)
{
    if (!x0_ok(A, B, n_lat, ld, off, lat_mask, link, K, ode_mask, gode != nullptr)) return HODE_EINVAL;
    if (!coords || !m || !s || !gx0 || !glik) return HODE_EINVAL;
    if (gode && K > 0 && !sd) return HODE_EINVAL;
    return launch_x0_grad<R>((hipStream_t)stream, A, B, n_lat, ld, off, coords, lat_mask, link, m, s, gx0, K, ode_mask, sd, gode, glik);
}

// ---- No-U-Turn sampling (hode_nuts.hip)
template <typename R> int nuts_begin(void *stream, int C, int D, int ld, const R *z, const R *p, const R *g, const double *U, const double *U0,
                                     const double *ke0, R *tree, double *dst, int32_t *ist)
{
    if (!chains_ok(C, D, ld)) return HODE_EINVAL;
    if (!z || !p || !g || !U || !U0 || !ke0 || !tree || !dst || !ist) return HODE_EINVAL;
    return launch_nuts_begin<R>((hipStream_t)stream, C, D, ld, z, p, g, U, U0, ke0, tree, dst, ist);
}

template <typename R> int nuts_pre(void *stream, int C, int D, int ld, uint64_t seed, uint32_t iter, const double *eps, const R *minv,
                                   R *tree, int32_t *ist, const int32_t *rank, uint32_t ode_mask, const double *mu, const double *sd,
                                   int sample_nn, int P, R *nn_p, R *ode_p)
{
    if (!chains_ok(C, D, ld) || (ode_mask >> 17)) return HODE_EINVAL;
    const int n_ode = __builtin_popcount(ode_mask);
    if (P < 0 || (sample_nn && P < 1) || D != n_ode + (sample_nn ? P : 0)) return HODE_EINVAL;
    if (!eps || !minv || !tree || !ist || !rank) return HODE_EINVAL;
    if (n_ode && ode_p && (!mu || !sd)) return HODE_EINVAL;
    NutsPreArgs<R> a;
    a.C = C; a.D = D; a.ld = ld; a.n_ode = n_ode; a.sample_nn = sample_nn ? 1 : 0; a.P = P; a.seed = seed; a.iter = iter;
    a.ode_mask = ode_mask; a.eps = eps; a.minv = minv; a.tree = tree; a.ist = ist; a.rank = rank; a.mu = mu; a.sd = sd;
    a.nn_p = nn_p; a.ode_p = ode_p;
    return launch_nuts_pre<R>((hipStream_t)stream, a);
}

template <typename R> int nuts_post(void *stream, int C, int D, int ld, int max_depth, uint64_t seed, uint32_t iter, const double *eps,
                                    const R *minv, R *tree, R *ckpt, double *dst, int32_t *ist, const int32_t *rank, const R *gnn,
                                    const R *gode, int P, const double *loss_sum, double lik_scale, const int32_t *status, int n_traj,
                                    uint32_t ode_mask, const double *sd, int sample_nn)
{
    if (!chains_ok(C, D, ld) || max_depth < 1 || max_depth > HODE_NUTS_MAX_DEPTH || (ode_mask >> 17)) return HODE_EINVAL;
    const int n_ode = __builtin_popcount(ode_mask);
    if (P < 0 || (sample_nn && P < 1) || D != n_ode + (sample_nn ? P : 0) || (status && n_traj < 1)) return HODE_EINVAL;
    if (!eps || !minv || !tree || !ckpt || !dst || !ist || !rank) return HODE_EINVAL;
    if ((n_ode && gode && !sd) || (sample_nn && gode && !gnn)) return HODE_EINVAL;
    NutsPostArgs<R> a;
    a.C = C; a.D = D; a.ld = ld; a.max_depth = max_depth; a.n_ode = n_ode; a.P = P; a.n_traj = n_traj; a.vec = false; a.seed = seed;
    a.iter = iter; a.ode_mask = ode_mask; a.lik_scale = lik_scale; a.eps = eps; a.minv = minv; a.tree = tree; a.ckpt = ckpt;
    a.dst = dst; a.ist = ist; a.rank = rank; a.gnn = gnn; a.gode = gode; a.loss_sum = loss_sum; a.status = status; a.sd = sd;
    return launch_nuts_post<R>((hipStream_t)stream, a);
}

template <typename R> int nuts_finish(void *stream, int C, int D, int ld, int adapt, double target_accept, R *z, R *g, double *U,
                                      const R *tree, const double *dst, const int32_t *ist, double *log_eps, double *da, int n_ode,
                                      const double *mu, const double *sd, R *draws, double *stats, int n_slots, int slot)
{
    if (!chains_ok(C, D, ld) || n_ode < 0 || n_ode > 17 || n_ode > D || (adapt != 0 && adapt != 1)) return HODE_EINVAL;
    if (!(target_accept > 0.0 && target_accept < 1.0)) return HODE_EINVAL;
    if (!z || !g || !U || !tree || !dst || !ist || !log_eps || !da) return HODE_EINVAL;
    if (n_ode && (!mu || !sd)) return HODE_EINVAL;
    if (slot >= 0 && (slot >= n_slots || !stats)) return HODE_EINVAL;
    NutsFinishArgs<R> a;
    a.C = C; a.D = D; a.ld = ld; a.adapt = adapt; a.n_ode = n_ode; a.n_slots = n_slots; a.slot = slot < 0 ? -1 : slot;
    a.delta = target_accept; a.z = z; a.g = g; a.U = U; a.tree = tree; a.dst = dst; a.ist = ist; a.log_eps = log_eps; a.da = da;
    a.mu = mu; a.sd = sd; a.draws = draws; a.stats = stats;
    return launch_nuts_finish<R>((hipStream_t)stream, a);
}

}  // namespace

extern "C" {

const char *hode_version(void) { return "hode 0.3.0 (gfx950; wave-per-trajectory DP5(4) + wave-specialised adjoint; MLP up to 8 x 128)"; }

int hode_nn_param_count(int H, int L) { return (H < 1 || layers_of(L) < 1) ? HODE_EINVAL : nn_param_count(H, L); }

size_t hode_tape_bytes_hl(int B, int max_steps, int elem_size, int H, int L)
{
    if (B < 0 || max_steps < 0 || (elem_size != 4 && elem_size != 8) || H < 1 || H > HODE_MAX_HIDDEN || layers_of(L) < 1 ||
        layers_of(L) > HODE_MAX_LAYERS || act_of(L) > HODE_ACT_LEAKY_RELU || (L >> 16) != 0)
        return 0;
    return tape_total_bytes(B, max_steps, (size_t)elem_size, H, L);
}
size_t hode_tape_bytes(int B, int max_steps, int elem_size, int L) { return hode_tape_bytes_hl(B, max_steps, elem_size, 64, L); }

int hode_rhs_fwd_f32(void *stream, int B, const float *x, const float *t, const float *meal, const float *tvns,
                     const float *gd, const float *ode_p, const float *nn_p, int H, int L, float *out)
{
    return rhs_fwd<float>(stream, B, x, t, meal, tvns, gd, ode_p, nn_p, H, L, out);
}
int hode_rhs_fwd_f64(void *stream, int B, const double *x, const double *t, const double *meal, const double *tvns,
                     const double *gd, const double *ode_p, const double *nn_p, int H, int L, double *out)
{
    return rhs_fwd<double>(stream, B, x, t, meal, tvns, gd, ode_p, nn_p, H, L, out);
}

int hode_solve_fwd_f32(void *stream, int B, int T, const float *x0, const float *t, int t_batched, const float *meal,
                       int meal_mode, const float *tvns, int tvns_mode, const float *gd, int gd_mode,
                       const float *ode_p, const float *nn_p, int n_sets, int H, int L, int method, double rtol,
                       double atol, int max_steps, float *y, int32_t *status, int32_t *nsteps, int32_t *nfev, void *tape)
{
    return solve_fwd<float>(stream, B, T, x0, t, t_batched, meal, meal_mode, tvns, tvns_mode, gd, gd_mode, ode_p, nn_p,
                            n_sets, H, L, method, rtol, atol, max_steps, y, status, nsteps, nfev, tape);
}
int hode_solve_fwd_f64(void *stream, int B, int T, const double *x0, const double *t, int t_batched, const double *meal,
                       int meal_mode, const double *tvns, int tvns_mode, const double *gd, int gd_mode,
                       const double *ode_p, const double *nn_p, int n_sets, int H, int L, int method, double rtol,
                       double atol, int max_steps, double *y, int32_t *status, int32_t *nsteps, int32_t *nfev, void *tape)
{
    return solve_fwd<double>(stream, B, T, x0, t, t_batched, meal, meal_mode, tvns, tvns_mode, gd, gd_mode, ode_p, nn_p,
                             n_sets, H, L, method, rtol, atol, max_steps, y, status, nsteps, nfev, tape);
}

int hode_rhs_bwd_f32(void *stream, int B, const float *x, const float *t, const float *meal, const float *tvns,
                     const float *gd, const float *ode_p, const float *nn_p, int H, int L, const float *gout, float *gx,
                     float *gt, float *gnn, float *gode)
{
    return rhs_bwd<float>(stream, B, x, t, meal, tvns, gd, ode_p, nn_p, H, L, gout, gx, gt, gnn, gode);
}
int hode_rhs_bwd_f64(void *stream, int B, const double *x, const double *t, const double *meal, const double *tvns,
                     const double *gd, const double *ode_p, const double *nn_p, int H, int L, const double *gout,
                     double *gx, double *gt, double *gnn, double *gode)
{
    return rhs_bwd<double>(stream, B, x, t, meal, tvns, gd, ode_p, nn_p, H, L, gout, gx, gt, gnn, gode);
}

int hode_solve_bwd_f32(void *stream, int B, int T, const float *t, int t_batched, const float *meal, int meal_mode,
                       const float *tvns, int tvns_mode, const float *gd, int gd_mode, const float *ode_p,
                       const float *nn_p, int n_sets, int H, int L, int method, int max_steps, const int32_t *nsteps,
                       const int32_t *status, void *tape, const float *gy, float *gx0, float *gnn, float *gode)
{
    return solve_bwd<float>(stream, B, T, t, t_batched, meal, meal_mode, tvns, tvns_mode, gd, gd_mode, ode_p, nn_p,
                            n_sets, H, L, method, max_steps, nsteps, status, tape, gy, gx0, gnn, gode);
}
int hode_solve_bwd_f64(void *stream, int B, int T, const double *t, int t_batched, const double *meal, int meal_mode,
                       const double *tvns, int tvns_mode, const double *gd, int gd_mode, const double *ode_p,
                       const double *nn_p, int n_sets, int H, int L, int method, int max_steps, const int32_t *nsteps,
                       const int32_t *status, void *tape, const double *gy, double *gx0, double *gnn, double *gode)
{
    return solve_bwd<double>(stream, B, T, t, t_batched, meal, meal_mode, tvns, tvns_mode, gd, gd_mode, ode_p, nn_p,
                             n_sets, H, L, method, max_steps, nsteps, status, tape, gy, gx0, gnn, gode);
}

int hode_rhs_bwd_inputs_f32(void *stream, int B, const float *x, const float *t, const float *meal, const float *tvns,
                            const float *gd, const float *ode_p, const float *nn_p, int H, int L, const float *gout, float *gx,
                            float *gt, float *gnn, float *gode, float *gmeal, float *gtvns, float *ggd)
{
    return rhs_bwd<float>(stream, B, x, t, meal, tvns, gd, ode_p, nn_p, H, L, gout, gx, gt, gnn, gode, gmeal, gtvns, ggd);
}
int hode_rhs_bwd_inputs_f64(void *stream, int B, const double *x, const double *t, const double *meal, const double *tvns,
                            const double *gd, const double *ode_p, const double *nn_p, int H, int L, const double *gout,
                            double *gx, double *gt, double *gnn, double *gode, double *gmeal, double *gtvns, double *ggd)
{
    return rhs_bwd<double>(stream, B, x, t, meal, tvns, gd, ode_p, nn_p, H, L, gout, gx, gt, gnn, gode, gmeal, gtvns, ggd);
}

int hode_solve_bwd_inputs_f32(void *stream, int B, int T, const float *t, int t_batched, const float *meal, int meal_mode,
                              const float *tvns, int tvns_mode, const float *gd, int gd_mode, const float *ode_p,
                              const float *nn_p, int n_sets, int H, int L, int method, int max_steps, const int32_t *nsteps,
                              const int32_t *status, void *tape, const float *gy, float *gx0, float *gnn, float *gode,
                              float *gmeal, float *gtvns, float *ggd)
{
    return solve_bwd<float>(stream, B, T, t, t_batched, meal, meal_mode, tvns, tvns_mode, gd, gd_mode, ode_p, nn_p,
                            n_sets, H, L, method, max_steps, nsteps, status, tape, gy, gx0, gnn, gode, gmeal, gtvns, ggd);
}
int hode_solve_bwd_inputs_f64(void *stream, int B, int T, const double *t, int t_batched, const double *meal, int meal_mode,
                              const double *tvns, int tvns_mode, const double *gd, int gd_mode, const double *ode_p,
                              const double *nn_p, int n_sets, int H, int L, int method, int max_steps, const int32_t *nsteps,
                              const int32_t *status, void *tape, const double *gy, double *gx0, double *gnn, double *gode,
                              double *gmeal, double *gtvns, double *ggd)
{
    return solve_bwd<double>(stream, B, T, t, t_batched, meal, meal_mode, tvns, tvns_mode, gd, gd_mode, ode_p, nn_p,
                             n_sets, H, L, method, max_steps, nsteps, status, tape, gy, gx0, gnn, gode, gmeal, gtvns, ggd);
}

int hode_solve_jvp_f32(void *stream, int B, int T, const float *t, int t_batched, const float *meal, int meal_mode,
                       const float *tvns, int tvns_mode, const float *gd, int gd_mode, const float *ode_p,
                       const float *nn_p, int n_sets, int H, int L, int method, int max_steps, const int32_t *nsteps,
                       const int32_t *status, const void *tape, int K, const float *v_ode, const float *v_x0, float *dy)
{
    return solve_jvp<float>(stream, B, T, t, t_batched, meal, meal_mode, tvns, tvns_mode, gd, gd_mode, ode_p, nn_p,
                            n_sets, H, L, method, max_steps, nsteps, status, tape, K, v_ode, v_x0, dy);
}
int hode_solve_jvp_f64(void *stream, int B, int T, const double *t, int t_batched, const double *meal, int meal_mode,
                       const double *tvns, int tvns_mode, const double *gd, int gd_mode, const double *ode_p,
                       const double *nn_p, int n_sets, int H, int L, int method, int max_steps, const int32_t *nsteps,
                       const int32_t *status, const void *tape, int K, const double *v_ode, const double *v_x0, double *dy)
{
    return solve_jvp<double>(stream, B, T, t, t_batched, meal, meal_mode, tvns, tvns_mode, gd, gd_mode, ode_p, nn_p,
                             n_sets, H, L, method, max_steps, nsteps, status, tape, K, v_ode, v_x0, dy);
}

int hode_solve_jvp_any_f32(void *stream, int B, int T, const float *t, int t_batched, const float *meal, int meal_mode,
                           const float *tvns, int tvns_mode, const float *gd, int gd_mode, const float *ode_p,
                           const float *nn_p, int n_sets, int H, int L, int method, int max_steps, const int32_t *nsteps,
                           const int32_t *status, const void *tape, int K, const float *v_ode, const float *v_x0, float *dy)
{
    return solve_jvp<float, true>(stream, B, T, t, t_batched, meal, meal_mode, tvns, tvns_mode, gd, gd_mode, ode_p, nn_p,
                                  n_sets, H, L, method, max_steps, nsteps, status, tape, K, v_ode, v_x0, dy);
}
int hode_solve_jvp_any_f64(void *stream, int B, int T, const double *t, int t_batched, const double *meal, int meal_mode,
                           const double *tvns, int tvns_mode, const double *gd, int gd_mode, const double *ode_p,
                           const double *nn_p, int n_sets, int H, int L, int method, int max_steps, const int32_t *nsteps,
                           const int32_t *status, const void *tape, int K, const double *v_ode, const double *v_x0, double *dy)
{
    return solve_jvp<double, true>(stream, B, T, t, t_batched, meal, meal_mode, tvns, tvns_mode, gd, gd_mode, ode_p, nn_p,
                                   n_sets, H, L, method, max_steps, nsteps, status, tape, K, v_ode, v_x0, dy);
}

int hode_adam_step_f32(void *stream, int64_t n, float *p, const float *g, float *m, float *v, float lr, float beta1,
                       float beta2, float eps, int step, float max_norm, float grad_scale, float weight_decay,
                       void *scratch)
{
    if (n < 0 || !p || !g || !m || !v || !scratch || step < 1) return HODE_EINVAL;
    return launch_adam((hipStream_t)stream, n, p, g, m, v, lr, beta1, beta2, eps, step, max_norm, grad_scale,
                       weight_decay, scratch);
}

int hode_mse_fwd_bwd_f32(void *stream, int64_t n, const float *y, const float *obs, float scale, double *loss_sum,
                         float *gy)
{
    if (n < 0 || !y || !obs || !loss_sum) return HODE_EINVAL;
    return launch_mse((hipStream_t)stream, n, y, obs, scale, loss_sum, gy);
}

int hode_selftest_xlane(void *stream, int32_t *out)
{
    if (!out) return HODE_EINVAL;
    return launch_selftest((hipStream_t)stream, out);
}

// ---- data side -----------------------------------------------------------------------------------------------
int hode_4gi_default_params(int patient_type, double *par)
{
    if (!par || (patient_type != HODE_4GI_T2DM && patient_type != HODE_4GI_HV)) return HODE_EINVAL;
    const bool hv = patient_type == HODE_4GI_HV;
    // data/generate4GI.py:15-64, in the order of HODE_4GI_NPAR
    const double v[HODE_4GI_NPAR] = {hv ? 5.36 : 1.72, hv ? 0.072 : 0.0256, 26.5, 9.33, 8.56, 73.2, 6.09, exp(-0.159),
                                     16.0, exp(7.97), exp(4.91), 453.2, 64.6, 86.8, 9.21, 49.4, 22.8, 2.46, exp(2.37),
                                     exp(3.29), 1.79, 6.73, exp(4.59), 0.0102, 0.0343, 0.00329};
    for (int i = 0; i < HODE_4GI_NPAR; ++i) par[i] = v[i];
    return HODE_OK;
}

static int fourgi_params(int patient_type, const double *par_host, FourGIPar *out)
{
    double v[HODE_4GI_NPAR];
    if (patient_type != HODE_4GI_T2DM && patient_type != HODE_4GI_HV) return HODE_EINVAL;
    if (par_host)
        for (int i = 0; i < HODE_4GI_NPAR; ++i) v[i] = par_host[i];
    else
        hode_4gi_default_params(patient_type, v);
    memcpy(out, v, sizeof v);
    return HODE_OK;
}

int hode_4gi_generate_f64(void *stream, int B, int T, double interval_min, int patient_type, const double *par_host,
                          const double *bsl, int n_meals, const double *meal_time, const double *meal_size,
                          int meals_per_subject, const double *z, double noise_cv, int64_t subject0, double rtol,
                          double atol, int max_steps, double *table, int32_t *status)
{
    if (B < 0 || T < 1 || n_meals < 0 || max_steps < 1) return HODE_EINVAL;
    if (!(interval_min > 0.0) || !(rtol > 0.0) || !(atol >= 0.0)) return HODE_EINVAL;
    if (B == 0) return HODE_OK;
    if (!bsl || !table || (n_meals > 0 && (!meal_time || !meal_size))) return HODE_EINVAL;
    GenArgs a{};
    if (int rc = fourgi_params(patient_type, par_host, &a.par)) return rc;
    a.B = B; a.T = T; a.hv = patient_type == HODE_4GI_HV; a.n_meals = n_meals; a.meals_per_subject = meals_per_subject != 0;
    a.max_steps = max_steps; a.subject0 = subject0; a.interval_min = interval_min; a.rtol = rtol; a.atol = atol;
    a.noise_cv = noise_cv; a.bsl = bsl; a.meal_time = meal_time; a.meal_size = meal_size; a.z = z; a.table = table;
    a.status = status;
    return launch_4gi_generate((hipStream_t)stream, a);
}

int hode_4gi_rhs_f64(void *stream, int B, int patient_type, const double *par_host, const double *bsl, const double *y,
                     const double *meal, double *d)
{
    if (B < 0) return HODE_EINVAL;
    if (B == 0) return HODE_OK;
    if (!bsl || !y || !meal || !d) return HODE_EINVAL;
    FourGIPar p;
    if (int rc = fourgi_params(patient_type, par_host, &p)) return rc;
    return launch_4gi_rhs((hipStream_t)stream, B, patient_type == HODE_4GI_HV, p, bsl, y, meal, d);
}

int hode_4gi_windows_f32(void *stream, const double *table, int ncols, int col_time, double time_div, int col_glucose,
                         int col_insulin, int col_glucagon, int col_glp1, int col_ge, int col_ffa, int col_meal,
                         int col_tvns, const int64_t *row0, int64_t N, int64_t S, int normalize, float *states,
                         float *meal, float *tvns, float *time, double *mean_std, void *scratch)
{
    if (N < 0 || S < 1 || ncols < 1 || !mean_std || !(time_div != 0.0)) return HODE_EINVAL;
    if (normalize < HODE_4GI_NORM_NONE || normalize > HODE_4GI_NORM_GIVEN) return HODE_EINVAL;
    const int need[5] = {col_time, col_glucose, col_insulin, col_glucagon, col_glp1};
    for (int c : need)
        if (c < 0 || c >= ncols) return HODE_EINVAL;
    const int opt[4] = {col_ge, col_ffa, col_meal, col_tvns};
    for (int c : opt)
        if (c < -1 || c >= ncols) return HODE_EINVAL;
    if (N > 0 && (!table || !row0 || !states || !meal || !tvns || !time || !scratch)) return HODE_EINVAL;
    WinArgs a{};
    a.table = table; a.ncols = ncols; a.col_time = col_time; a.col_meal = col_meal; a.col_tvns = col_tvns;
    a.col_state[0] = col_glucose; a.col_state[1] = col_insulin; a.col_state[2] = col_glucagon; a.col_state[3] = col_glp1;
    a.col_state[4] = col_ge; a.col_state[5] = col_ffa;
    a.time_div = time_div; a.row0 = row0; a.N = N; a.S = S; a.states = states; a.meal = meal; a.tvns = tvns; a.time = time;
    return launch_4gi_windows((hipStream_t)stream, a, normalize, mean_std, scratch);
}

int hode_4gi_window_moments_f64(void *stream, const double *table, int ncols, int col_glucose, int col_insulin,
                                int col_glucagon, int col_glp1, int col_ge, int col_ffa, const int64_t *row0, int64_t N,
                                int64_t S, double *moments, void *scratch)
{
    if (N < 0 || S < 1 || ncols < 1 || !moments) return HODE_EINVAL;
    const int need[4] = {col_glucose, col_insulin, col_glucagon, col_glp1};
    for (int c : need)
        if (c < 0 || c >= ncols) return HODE_EINVAL;
    if (col_ge < -1 || col_ge >= ncols || col_ffa < -1 || col_ffa >= ncols) return HODE_EINVAL;
    if (N > 0 && (!table || !row0 || !scratch)) return HODE_EINVAL;
    WinArgs a{};
    a.table = table; a.ncols = ncols; a.col_time = 0; a.col_meal = -1; a.col_tvns = -1;
    a.col_state[0] = col_glucose; a.col_state[1] = col_insulin; a.col_state[2] = col_glucagon; a.col_state[3] = col_glp1;
    a.col_state[4] = col_ge; a.col_state[5] = col_ffa;
    a.time_div = 1.0; a.row0 = row0; a.N = N; a.S = S;
    return launch_4gi_window_moments((hipStream_t)stream, a, moments, scratch);
}

// ---- MCMC
#define HODE_HMC_ABI(SFX, R)                                                                                                             \
    int hode_mse_sets_##SFX(void *stream, int n_sets, int64_t len, const R *y, const R *obs, R scale, double *loss_sum, R *gy)         \
    {                                                                                                                                  \
        return mse_sets<R>(stream, n_sets, len, y, obs, scale, loss_sum, gy);                                                         \
    }                                                                                                                                  \
    int hode_hmc_refresh_##SFX(void *stream, int C, int D, int ld, uint64_t seed, uint32_t iter, double jitter, const R *minv,         \
                               const double *log_eps, const R *z, const R *g, const double *U, R *p, R *z0, R *g0, double *U0,        \
                               double *ke0, double *eps, int32_t *failed)                                                             \
    {                                                                                                                                  \
        return hmc_refresh<R>(stream, C, D, ld, seed, iter, jitter, minv, log_eps, z, g, U, p, z0, g0, U0, ke0, eps, failed);         \
    }                                                                                                                                  \
    int hode_hmc_leapfrog_##SFX(void *stream, int C, int D, int ld, int flags, double kick, const double *eps, const R *minv, R *z,    \
                                R *p, R *g, const R *gnn, const R *gode, int P, const double *loss_sum, double lik_scale,             \
                                const int32_t *status, int n_traj, double *U, double *ke, int32_t *failed, uint32_t ode_mask,         \
                                const double *mu, const double *sd, int sample_nn, R *nn_p, R *ode_p)                                 \
    {                                                                                                                                  \
        return hmc_leapfrog<R>(stream, C, D, ld, flags, kick, eps, minv, z, p, g, gnn, gode, P, loss_sum, lik_scale, status, n_traj,  \
                               U, ke, failed, ode_mask, mu, sd, sample_nn, nn_p, ode_p);                                              \
    }                                                                                                                                  \
    int hode_hmc_accept_##SFX(void *stream, int C, int D, int ld, int mode, uint64_t seed, uint32_t iter, double target_accept, R *z,  \
                              const R *z0, R *g, const R *g0, double *U, const double *U0, const double *ke0, const double *ke,        \
                              const int32_t *failed, double *log_eps, double *da, int32_t *search, int n_ode, const double *mu,       \
                              const double *sd, R *draws, double *stats, int n_slots, int slot)                                       \
    {                                                                                                                                  \
        return hmc_accept<R>(stream, C, D, ld, mode, seed, iter, target_accept, z, z0, g, g0, U, U0, ke0, ke, failed, log_eps, da,    \
                             search, n_ode, mu, sd, draws, stats, n_slots, slot);                                                     \
    }                                                                                                                                  \
    int hode_hmc_welford_##SFX(void *stream, int C, int D, int ld, int flags, const R *z, double *wf, R *minv)                        \
    {                                                                                                                                  \
        return hmc_welford<R>(stream, C, D, ld, flags, z, wf, minv);                                                                  \
    }
#define HODE_OBS_ABI(SFX, R)                                                                                                             \
    int hode_obs_nll_sets_##SFX(void *stream, int n_sets, int64_t len, const R *y, const R *obs, const uint8_t *mask, int mode,        \
                                int flags, const double *w, const double *a, const double *b, const double *n, double *sse,           \
                                double *loss_sum, R *gy)                                                                              \
    {                                                                                                                                  \
        return obs_nll_sets<R>(stream, n_sets, len, y, obs, mask, mode, flags, w, a, b, n, sse, loss_sum, gy);                       \
    }
HODE_OBS_ABI(f32, float)
HODE_OBS_ABI(f64, double)

HODE_HMC_ABI(f32, float)
HODE_HMC_ABI(f64, double)

#define HODE_POP_ABI(SFX, R)                                                                                                             \
    int hode_pop_params_##SFX(void *stream, int A, int B, int K, int ld, const R *coords, uint32_t ode_mask, const double *mu0,       \
                              const double *sd0, const double *tau0, double tau_log_sd, const R *ode_base, R *ode_p)                  \
    {                                                                                                                                  \
        return pop_params<R>(stream, A, B, K, ld, coords, ode_mask, mu0, sd0, tau0, tau_log_sd, ode_base, ode_p);                     \
    }                                                                                                                                  \
    int hode_pop_grad_##SFX(void *stream, int A, int B, int K, int ld, const R *coords, const R *gode, uint32_t ode_mask,             \
                            const double *sd0, const double *tau0, double tau_log_sd, R *glik)                                        \
    {                                                                                                                                  \
        return pop_grad<R>(stream, A, B, K, ld, coords, gode, ode_mask, sd0, tau0, tau_log_sd, glik);                                 \
    }
HODE_POP_ABI(f32, float)
HODE_POP_ABI(f64, double)

#define HODE_X0_ABI(SFX, R)                                                                                                              \
    int hode_x0_params_##SFX(void *stream, int A, int B, int n_lat, int ld, int off, const R *coords, uint32_t lat_mask, int link,     \
                             const double *m, const double *s, const R *x0_base, R *x0_out, int K, uint32_t ode_mask,                  \
                             const double *mu, const double *sd, const R *ode_base, R *ode_p)                                         \
    {                                                                                                                                  \
        return x0_params<R>(stream, A, B, n_lat, ld, off, coords, lat_mask, link, m, s, x0_base, x0_out, K, ode_mask, mu, sd,         \
                            ode_base, ode_p);                                                                                          \
    }                                                                                                                                  \
    int hode_x0_grad_##SFX(void *stream, int A, int B, int n_lat, int ld, int off, const R *coords, uint32_t lat_mask, int link,       \
                           const double *m, const double *s, const R *gx0, int K, uint32_t ode_mask, const double *sd, const R *gode,  \
                           R *glik)                                                                                                    \
    {                                                                                                                                  \
        return x0_grad<R>(stream, A, B, n_lat, ld, off, coords, lat_mask, link, m, s, gx0, K, ode_mask, sd, gode, glik);              \
    }
HODE_X0_ABI(f32, float)
HODE_X0_ABI(f64, double)

#define HODE_NUTS_ABI(SFX, R)                                                                                                            \
    int hode_nuts_begin_##SFX(void *stream, int C, int D, int ld, const R *z, const R *p, const R *g, const double *U,                \
                              const double *U0, const double *ke0, R *tree, double *dst, int32_t *ist)                                \
    {                                                                                                                                  \
        return nuts_begin<R>(stream, C, D, ld, z, p, g, U, U0, ke0, tree, dst, ist);                                                  \
    }                                                                                                                                  \
    int hode_nuts_pre_##SFX(void *stream, int C, int D, int ld, uint64_t seed, uint32_t iter, const double *eps, const R *minv,       \
                            R *tree, int32_t *ist, const int32_t *rank, uint32_t ode_mask, const double *mu, const double *sd,        \
                            int sample_nn, int P, R *nn_p, R *ode_p)                                                                  \
    {                                                                                                                                  \
        return nuts_pre<R>(stream, C, D, ld, seed, iter, eps, minv, tree, ist, rank, ode_mask, mu, sd, sample_nn, P, nn_p, ode_p);    \
    }                                                                                                                                  \
    int hode_nuts_post_##SFX(void *stream, int C, int D, int ld, int max_depth, uint64_t seed, uint32_t iter, const double *eps,      \
                             const R *minv, R *tree, R *ckpt, double *dst, int32_t *ist, const int32_t *rank, const R *gnn,           \
                             const R *gode, int P, const double *loss_sum, double lik_scale, const int32_t *status, int n_traj,      \
                             uint32_t ode_mask, const double *sd, int sample_nn)                                                      \
    {                                                                                                                                  \
        return nuts_post<R>(stream, C, D, ld, max_depth, seed, iter, eps, minv, tree, ckpt, dst, ist, rank, gnn, gode, P, loss_sum,  \
                            lik_scale, status, n_traj, ode_mask, sd, sample_nn);                                                      \
    }                                                                                                                                  \
    int hode_nuts_finish_##SFX(void *stream, int C, int D, int ld, int adapt, double target_accept, R *z, R *g, double *U,           \
                               const R *tree, const double *dst, const int32_t *ist, double *log_eps, double *da, int n_ode,          \
                               const double *mu, const double *sd, R *draws, double *stats, int n_slots, int slot)                    \
    {                                                                                                                                  \
        return nuts_finish<R>(stream, C, D, ld, adapt, target_accept, z, g, U, tree, dst, ist, log_eps, da, n_ode, mu, sd, draws,    \
                              stats, n_slots, slot);                                                                                  \
    }
HODE_NUTS_ABI(f32, float)
HODE_NUTS_ABI(f64, double)

int hode_nuts_compact(void *stream, int C, const int32_t *ist, int32_t *rank, int32_t *count)
{
    if (C < 1 || !ist || !rank || !count) return HODE_EINVAL;
    return launch_nuts_compact((hipStream_t)stream, C, ist, rank, count);
}

}  // extern "C"

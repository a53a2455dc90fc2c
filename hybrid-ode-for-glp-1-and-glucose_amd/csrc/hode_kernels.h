// hode_kernels.h -- host-visible argument blocks and launchers shared by the .hip files and the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "../../include/hode.h"

namespace hode {

template <typename R> struct SolveArgs {
    int B, T, t_batched, meal_mode, tvns_mode, gd_mode, n_sets, H, P, max_steps;
    const R *x0, *t, *meal, *tvns, *gd, *ode_p, *nn_p;
    R rtol, atol;
    R *y;
    int32_t *status, *nsteps, *nfev;
    R *tape;            // [B][max_steps][8] = {t, h, t0, 1/(t1-t0), v0, v1-v0, d0, d1-d0}: the step + the constants of its grid interval
    int32_t *tape_seg;  // [B][max_steps] grid interval of each accepted step (| kSegClosed)
    R *tape_stage;      // [B][max_steps][6 stages][tape_slot_elems]: layer activations + stage state of every accepted step
    int L;              // hidden layers (plain count)
    int act;            // HODE_ACT_* (generic kernels; the tuned ones are ReLU)
    int nn_stride;      // reals between the networks of consecutive parameter sets: P, or 0 for one shared network (HODE_LAYERS_NN_SHARED)
};

template <typename R> struct AdjArgs {
    int B, T, t_batched, meal_mode, tvns_mode, gd_mode, n_sets, H, P, max_steps;
    const R *t, *meal, *tvns, *gd, *ode_p, *nn_p;
    const int32_t *nsteps, *status;
    const R *tape;
    const int32_t *tape_seg;
    const R *tape_stage;
    const R *gy;
    R *gx0, *gnn, *gode;
    R *tape_delta;      // fp32 tuned shapes: [B][max_steps][6][delta_slot_elems] scratch of the split adjoint (part of the tape)
    R *partials;        // tuned shapes: [adj_partial_rows(B)][adj_partial_rowlen(P)] per-workgroup gradient sums (tail of the tape)
    int partial_rows;
    int act;            // HODE_ACT_* (generic kernels)
};
// AdjArgs + the input gradients (hode_solve_bwd_inputs_*): NULL, or [B] / [B,T] by the input's mode (1 / 2); WRITTEN, not
// accumulated.  Only the input-gradient kernels take it: every other adjoint kernel keeps its AdjArgs argument block.
template <typename R> struct AdjInArgs : AdjArgs<R> {
    R *gmeal, *gtvns, *ggd;
};
// the argument block of an adjoint kernel template with a GIN flag (solve_bwd_kernel, solve_bwd_generic_kernel), and the gradient
// row of input q (0 meal, 1 tVNS, 2 GD) in either block
template <typename R, bool GIN> using AdjArgsT = std::conditional_t<GIN, AdjInArgs<R>, AdjArgs<R>>;
template <typename R> __device__ __forceinline__ R *gin_row(const AdjArgs<R> &, int) { return nullptr; }
template <typename R> __device__ __forceinline__ R *gin_row(const AdjInArgs<R> &a, int q) { return (q == 0) ? a.gmeal : (q == 1) ? a.gtvns : a.ggd; }

// tangent-linear pass over the tape (hode_solve_jvp.hip).  The external inputs are not arguments: the tape holds what the
// stages used (activations, stage state, the step's interval constants); gd_mode selects the Hill-term instantiation.
template <typename R> struct JvpArgs {
    int B, T, t_batched, gd_mode, n_sets, H, P, max_steps, K;
    const R *t, *ode_p, *nn_p;
    const int32_t *nsteps, *status;
    const R *tape;
    const int32_t *tape_seg;
    const R *tape_stage;
    const R *v_ode, *v_x0;  // [n_sets][K][17] / [B][K][6], either may be NULL
    R *dy;                  // [B][K][T][6]
};

template <typename R> struct RhsArgs {
    int B, H, P;
    const R *x, *t, *meal, *tvns, *gd, *ode_p, *nn_p;
    R *out;                 // fwd
    const R *gout;          // bwd
    R *gx, *gt, *gnn, *gode;
    int act;                // HODE_ACT_* (generic kernels)
    R *gmeal, *gtvns, *ggd; // bwd, input gradients [B] (hode_rhs_bwd_inputs_*): written; NULL = not wanted
};

template <typename R> int launch_solve_fwd(hipStream_t s, const SolveArgs<R> &a, int L, int method);
#ifdef HODE_LAB
// Experiment kernels (csrc/lab/): compiled into hode/lab/libhode_lab.so only (make lab).  The product
// library libhode.so is built without HODE_LAB: none of these kernels, no environment-variable dispatch on the call path.
int launch_solve_fwd_wg(hipStream_t s, const SolveArgs<float> &a, int L, int method);   // lab/hode_solve_fwd_wg.hip (fp32, L = 2..4)
int launch_solve_fwd_quad(hipStream_t s, const SolveArgs<float> &a, int L, int method); // lab/hode_solve_fwd_quad.hip (fp32, L = 2..4)
int launch_solve_fwd_rows(hipStream_t s, const SolveArgs<float> &a, int L, int method); // lab/hode_solve_fwd_rows.hip (fp32, L = 2..4)
#endif
template <typename R> int launch_solve_bwd(hipStream_t s, const AdjArgs<R> &a, int L, int method);
// the same with input gradients (solve_bwd_kernel, GIN instantiations; tuned shapes, every dtype)
template <typename R> int launch_solve_bwd_inputs(hipStream_t s, const AdjInArgs<R> &a, int L, int method);
// wave-specialised fp32 adjoint (hode_solve_bwd_ws.hip; L = 2..4, needs the partial rows); HODE_EUNSUPPORTED -> solve_bwd_kernel
int launch_solve_bwd_ws(hipStream_t s, const AdjArgs<float> &a, int L, int method, int cus);
// second pass of the gradient reduction: rows of a.partials added in workgroup order (hode_solve_bwd.hip)
void launch_adj_reduce(hipStream_t s, const float *partials, int rowlen, int blocks_per_set, int n_sets, int P, float *gnn, float *gode);
// tangent-linear solve (hode_solve_jvp.hip; tuned shapes, every dtype)
template <typename R> int launch_solve_jvp(hipStream_t s, const JvpArgs<R> &a, int L, int method);
// the same for generic networks (hode_generic_jvp.hip): one trajectory and a tile of directions per eight-wave team
template <typename R> int launch_solve_jvp_generic(hipStream_t s, const JvpArgs<R> &a, int L, int act, int method);
template <typename R> int launch_rhs_fwd(hipStream_t s, const RhsArgs<R> &a, int L);
template <typename R> int launch_rhs_bwd(hipStream_t s, const RhsArgs<R> &a, int L);
// generic network path: H <= 128, L <= 8, weights streamed from L2.  Forward (hode_generic.hip):
template <typename R> int launch_solve_fwd_generic(hipStream_t s, const SolveArgs<R> &a, int method);
template <typename R> int launch_rhs_fwd_generic(hipStream_t s, const RhsArgs<R> &a, int L);
// adjoint and RHS backward (hode_generic_bwd.hip)
template <typename R> int launch_solve_bwd_generic(hipStream_t s, const AdjArgs<R> &a, int L, int method);
template <typename R> int launch_rhs_bwd_generic(hipStream_t s, const RhsArgs<R> &a, int L);
// tb = 2 / 4 / 8 trajectories per eight-wave team (hode_generic_bwd_multi.hip; fp32, L - 1 <= 4, gradient rows: launch_solve_bwd_generic
// decides when)
int launch_solve_bwd_generic_multi(hipStream_t s, const AdjArgs<float> &a, int L, int method, int tb);
// the same with input gradients (hode_generic_gin.hip; launch_*_generic route requests there): one-trajectory teams for every batch
template <typename R> int launch_solve_bwd_generic_gin(hipStream_t s, const AdjInArgs<R> &a, int L, int method);
template <typename R> int launch_rhs_bwd_generic_gin(hipStream_t s, const RhsArgs<R> &a, int L);
// shapes the tuned (register-resident) kernels are compiled for; everything else up to HODE_MAX_* takes the generic path
// The `L` argument of the C ABI carries the number of hidden layers in bits 0..7 and the activation (HODE_ACT_*) in bits 8..15.
inline int layers_of(int L) { return L & 0xff; }
inline int act_of(int L) { return (L >> 8) & 0xff; }
// (ReLU only: every other activation takes the generic kernels whatever the shape)
inline bool tuned_shape(int H, int L) { return act_of(L) == HODE_ACT_RELU && H <= 64 && layers_of(L) <= 4; }
// reals of one network's flat parameter vector: W1[H][9], b1 | (L - 1) x (W[H][H], b) | Wout[6][H], bout
__host__ __device__ inline int nn_param_count(int H, int L) { L &= 0xff; return 9 * H + H + (L - 1) * (H * H + H) + 6 * H + 6; }   // (L may carry an activation code in bits 8..15)
int launch_adam(hipStream_t s, int64_t n, float *p, const float *g, float *m, float *v, float lr, float b1,
                float b2, float eps, int step, float max_norm, float grad_scale, float wd, void *scratch);
int launch_mse(hipStream_t s, int64_t n, const float *y, const float *obs, float scale, double *loss, float *gy);
int launch_selftest(hipStream_t s, int32_t *out);

// ---- MCMC (hode_hmc.hip): the per-chain passes of multi-chain HMC; chains [C][ld] row-major, see include/hode.h
template <typename R> int launch_mse_sets(hipStream_t s, int n_sets, int64_t len, const R *y, const R *obs, R scale, double *loss_sum, R *gy);
// the observation model (hode_obs.hip); w / a / b / n are HOST arrays of six
template <typename R> struct ObsArgs {
    int n_sets, mode, flags;
    int64_t len;
    const R *y, *obs;
    const uint8_t *mask;
    const double *w, *a, *b, *n;
    double *sse, *loss_sum;
    R *gy;
};
template <typename R> int launch_obs_nll_sets(hipStream_t s, const ObsArgs<R> &a);
template <typename R> struct HmcRefreshArgs {
    int C, D, ld;
    uint64_t seed;
    uint32_t iter;
    double jitter;
    const R *minv;
    const double *log_eps;
    const R *z, *g;
    const double *U;
    R *p, *z0, *g0;
    double *U0, *ke0, *eps;
    int32_t *failed;
};
template <typename R> struct HmcLeapfrogArgs {
    int C, D, ld, flags, P, n_traj, n_ode, sample_nn;
    double kick, lik_scale;
    uint32_t ode_mask;
    const double *eps;
    const R *minv;
    R *z, *p, *g;
    const R *gnn, *gode;
    const double *loss_sum;
    const int32_t *status;
    double *U, *ke;
    int32_t *failed;
    const double *mu, *sd;
    R *nn_p, *ode_p;
};
template <typename R> struct HmcAcceptArgs {
    int C, D, ld, mode, n_ode, n_slots, slot;
    uint64_t seed;
    uint32_t iter;
    double delta;
    R *z;
    const R *z0;
    R *g;
    const R *g0;
    double *U;
    const double *U0, *ke0, *ke;
    const int32_t *failed;
    double *log_eps, *da;
    int32_t *search;
    const double *mu, *sd;
    R *draws;
    double *stats;
};
template <typename R> int launch_hmc_refresh(hipStream_t s, const HmcRefreshArgs<R> &a);
template <typename R> int launch_hmc_leapfrog(hipStream_t s, const HmcLeapfrogArgs<R> &a);
template <typename R> int launch_hmc_accept(hipStream_t s, const HmcAcceptArgs<R> &a);
template <typename R> int launch_hmc_welford(hipStream_t s, int C, int D, int ld, int flags, const R *z, double *wf, R *minv);

// ---- population model (hode_population.hip): chain coordinates [A][ld] <-> per-(row, patient) constants [A * B][17], see include/hode.h
template <typename R> int launch_pop_params(hipStream_t s, int A, int B, int K, int ld, const R *coords, uint32_t ode_mask, const double *mu0,
                                            const double *sd0, const double *tau0, double tau_log_sd, const R *ode_base, R *ode_p);
template <typename R> int launch_pop_grad(hipStream_t s, int A, int B, int K, int ld, const R *coords, const R *gode, uint32_t ode_mask,
                                          const double *sd0, const double *tau0, double tau_log_sd, R *glik);

// ---- initial-state model (hode_x0.hip): chain coordinates [A][ld] <-> per-(row, patient) initial states [A * B][6], see include/hode.h
template <typename R> int launch_x0_params(hipStream_t s, int A, int B, int n_lat, int ld, int off, const R *coords, uint32_t lat_mask,
                                           int link, const double *m, const double *sd_x, const R *x0_base, R *x0_out, uint32_t ode_mask,
                                           const double *mu, const double *sd, const R *ode_base, R *ode_p);
template <typename R> int launch_x0_grad(hipStream_t s, int A, int B, int n_lat, int ld, int off, const R *coords, uint32_t lat_mask,
                                         int link, const double *m, const double *sd_x, const R *gx0, int K, uint32_t ode_mask,
                                         const double *sd, const R *gode, R *glik);

// ---- MCMC (hode_nuts.hip): the per-chain passes of multi-chain No-U-Turn sampling; tree [HODE_NUTS_ROWS][C][ld], see include/hode.h
template <typename R> struct NutsPreArgs {
    int C, D, ld, n_ode, sample_nn, P;
    uint64_t seed;
    uint32_t iter, ode_mask;
    const double *eps;
    const R *minv;
    R *tree;
    int32_t *ist;
    const int32_t *rank;
    const double *mu, *sd;
    R *nn_p, *ode_p;
};
template <typename R> struct NutsPostArgs {
    int C, D, ld, max_depth, n_ode, P, n_traj;
    bool vec;
    uint64_t seed;
    uint32_t iter, ode_mask;
    double lik_scale;
    const double *eps;
    const R *minv;
    R *tree, *ckpt;
    double *dst;
    int32_t *ist;
    const int32_t *rank;
    const R *gnn, *gode;
    const double *loss_sum;
    const int32_t *status;
    const double *sd;
};
template <typename R> struct NutsFinishArgs {
    int C, D, ld, adapt, n_ode, n_slots, slot;
    double delta;
    R *z, *g;
    double *U;
    const R *tree;
    const double *dst;
    const int32_t *ist;
    double *log_eps, *da;
    const double *mu, *sd;
    R *draws;
    double *stats;
};
template <typename R> int launch_nuts_begin(hipStream_t s, int C, int D, int ld, const R *z, const R *p, const R *g, const double *U,
                                            const double *U0, const double *ke0, R *tree, double *dst, int32_t *ist);
template <typename R> int launch_nuts_pre(hipStream_t s, const NutsPreArgs<R> &a);
template <typename R> int launch_nuts_post(hipStream_t s, NutsPostArgs<R> a);
int launch_nuts_compact(hipStream_t s, int C, const int32_t *ist, int32_t *rank, int32_t *count);
template <typename R> int launch_nuts_finish(hipStream_t s, const NutsFinishArgs<R> &a);

// ---- data side (hode_datagen.hip) ----------------------------------------------------------------------------
// 4GI model parameters, in the order of include/hode.h (HODE_4GI_NPAR)
struct FourGIPar {
    double CLglc, CLglci, Qglc, VCglc, VPglc, CLins, VCins, Ke0ins, VCglp, VM_GLP, KM_GLP, CLglg, VCglg, CLgip, VCgip,
        Qgip, VPgip, GLCINS_S, EMAX_1, EC50_1, HILL_1, EMAX_4, EC50_4, FDGLP, FDGIP, FDGLG;
};
static_assert(sizeof(FourGIPar) == HODE_4GI_NPAR * sizeof(double), "parameter block layout");

struct GenArgs {
    int B, T, hv, n_meals, meals_per_subject, max_steps;
    int64_t subject0;
    double interval_min, rtol, atol, noise_cv;
    const double *bsl, *meal_time, *meal_size, *z;
    double *table;      // [B*T][9]
    int32_t *status;
    FourGIPar par;
};

struct WinArgs {
    const double *table;
    int ncols, col_time, col_meal, col_tvns;
    int col_state[6];   // glucose, insulin, glucagon, glp1, ge, ffa  (-1 = absent)
    double time_div;
    const int64_t *row0;  // [N] first table row of every window
    int64_t N, S;
    float *states, *meal, *tvns, *time;
};

int launch_4gi_generate(hipStream_t s, const GenArgs &a);
int launch_4gi_rhs(hipStream_t s, int B, int hv, const FourGIPar &p, const double *bsl, const double *y, const double *meal,
                   double *d);
int launch_4gi_windows(hipStream_t s, const WinArgs &a, int normalize, double *mean_std, void *scratch);
int launch_4gi_window_moments(hipStream_t s, const WinArgs &a, double *moments, void *scratch);

// interval index of an accepted step on the tape: bit 30 set = the step ended exactly on the grid point closing its interval
constexpr int kSegClosed = 1 << 30;

// tape = entries | interval indices | (256-byte aligned) stage tape
inline size_t tape_seg_offset(int B, int max_steps, size_t elem) { return (size_t)B * max_steps * 8 * elem; }
inline size_t tape_stage_offset(int B, int max_steps, size_t elem)
{
    size_t o = tape_seg_offset(B, max_steps, elem) + (size_t)B * max_steps * sizeof(int32_t);
    return (o + 255) & ~(size_t)255;
}
// reals per stage record: h_1..h_L (tuned path: L rows of 64; generic path: 2 L rows, two hidden units per lane) + 8 for the
// stage state
inline size_t tape_slot_elems(int H, int L) { return (size_t)(tuned_shape(H, L) ? layers_of(L) : 2 * layers_of(L)) * 64 + 8; }
// The split adjoint of the tuned fp32 path (lab/hode_solve_bwd_split.hip; lab library only, HODE_BWD=split) hands the layer
// cotangents of every stage from its propagation kernel to its accumulation kernel through HBM: delta_1..delta_L (L rows of
// 64) + {kb[6], t, tVNS} in 8 reals per stage, in a region of the tape behind the stage tape (the tape is the adjoint's
// workspace: nothing is allocated inside the library).  In the product library, and for other dtypes / shapes, there is no
// such region.
inline size_t delta_slot_elems(int L) { return (size_t)L * 64 + 8; }
#ifdef HODE_LAB
bool split_adjoint_enabled();       // HODE_BWD=split (hode_solve_bwd.hip); the default is the fused one-kernel adjoint
#else
constexpr bool split_adjoint_enabled() { return false; }
#endif
inline bool has_delta_tape(size_t elem, int H, int L) { return elem == 4 && tuned_shape(H, L) && layers_of(L) >= 2 && split_adjoint_enabled(); }
inline size_t tape_delta_offset(int B, int max_steps, size_t elem, int H, int L)
{
    size_t o = tape_stage_offset(B, max_steps, elem) + (size_t)B * max_steps * 6 * tape_slot_elems(H, L) * elem;
    return (o + 255) & ~(size_t)255;
}
// Gradient partials of the tuned adjoint: every workgroup writes ONE row [ dL/d nn_p (P) | dL/d ode_p (17) | pad ] and a second,
// fixed-order pass adds the rows into gnn / gode -- no floating-point atomics, so a training step is bit-reproducible run to
// run (the reference's CPU training is deterministic; fp32 atomics from 256 workgroups are not).  The rows live in the tail of
// the tape, the adjoint's workspace (nothing is allocated inside the library): at most kAdjPartialRows of them, never more
// than there are trajectories (a launch has at most one workgroup per trajectory).
constexpr int kAdjPartialRows = 1024;
__host__ __device__ inline int adj_partial_rows(int B) { return B < kAdjPartialRows ? B : kAdjPartialRows; }
__host__ __device__ inline size_t adj_partial_rowlen(int P) { return (size_t)(P + 17 + 63) / 64 * 64; }
inline size_t tape_partials_offset(int B, int max_steps, size_t elem, int H, int L)
{
    size_t o = tape_delta_offset(B, max_steps, elem, H, L);
    if (has_delta_tape(elem, H, L)) o += (size_t)B * max_steps * 6 * delta_slot_elems(L) * elem;
    return (o + 255) & ~(size_t)255;
}
inline size_t tape_total_bytes(int B, int max_steps, size_t elem, int H, int L)
{
    const size_t o = tape_partials_offset(B, max_steps, elem, H, L);
    // (generic shapes: the fp32 team kernels write gradient rows as well since round 4; fp64 and networks with more than four hidden
    //  matrices keep the coalesced atomics of hode_generic_vjp.h)
    if (!tuned_shape(H, L) && elem != 4) return o;
    return o + (size_t)adj_partial_rows(B) * adj_partial_rowlen(nn_param_count(H, L)) * elem;
}
#ifdef HODE_LAB
int launch_solve_bwd_split(hipStream_t s, const AdjArgs<float> &a, int L, int method);   // lab/hode_solve_bwd_split.hip (fp32, tuned shapes)
#endif

}  // namespace hode

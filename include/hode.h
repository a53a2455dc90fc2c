/*
 * hode.h -- C ABI of libhode.so: batched hybrid-ODE (6-state GLP-1/glucose RHS + MLP residual)
 * integration and adjoint on AMD MI355X (gfx950).
 *
 * This is the drop-in boundary for ONE path of OliverDOU776/Hybrid-ODE-for-GLP-1-and-Glucose.
 * The reference has no FFI of its own (pure Python): each entry point
 * below names the reference Python it replaces.  Citations are relative to the reference root.
 *
 * Conventions
 *   - every pointer is DEVICE memory owned by the caller, contiguous row-major, 16-byte aligned
 *     where noted; nothing is allocated, freed or kept by the callee;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); all work is enqueued
 *     on it, nothing synchronises, so calls may be captured into a hipGraph;
 *   - return value: 0 ok, HODE_EINVAL bad argument, HODE_EUNSUPPORTED shape outside the
 *     kernels' compiled range, HODE_ELAUNCH HIP launch error.  Integration failures are NEVER
 *     a return code: they are per-trajectory values in `status[B]`
 *     (reference: models/hybrid_ode_nn.py:243-256 logs a warning and zero-fills);
 *   - flat MLP parameter vector `nn_p` = PyTorch parameters() order of NNResidual.network
 *     (models/nn_residual.py:59-78):  W1[H,9] b1[H] (W[H,H] b[H])x(L-1) Wout[6,H] bout[6];
 *   - `ode_p[17]` = ODECore buffers in registration order (models/ode_core.py:44-71):
 *     a_GI k_I rho G_b I_b E_max EC_50 Glu_b V_max K_m k_L k_GE0 IGD_50 g p_7 p_8 p_9;
 *   - input "mode" of meal / tvns / gd (models/hybrid_ode_nn.py:217-231):
 *     0 absent (=0), 1 constant per patient [B], 2 time-varying on the grid [B,T] (lerp);
 *   - parameter sets: the B trajectories are n_sets equal contiguous groups, group s uses
 *     ode_p + 17*s and nn_p + P*s (n_sets = 1: one shared set; >1: VI samples / Sobol sets,
 *     inference/vi.py:88-100, plots/plot_all.py:171-196).  B % n_sets must be 0.
 */
#ifndef HODE_H
#define HODE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HODE_OK 0
#define HODE_EINVAL (-1)
#define HODE_EUNSUPPORTED (-2)
#define HODE_ELAUNCH (-3)

/* integrator (hybrid_ode_nn.py:174-181 maps names to SciPy; 'rk45' == DP5(4)) */
#define HODE_METHOD_DP54 0 /* adaptive Dormand-Prince 5(4), grid points are step boundaries */
#define HODE_METHOD_RK4 1  /* classic RK4, one step per grid interval (BASELINE config 1)   */

/* per-trajectory status */
#define HODE_ST_OK 0
#define HODE_ST_MAXSTEPS 1  /* accepted-step budget (max_steps) exhausted */
#define HODE_ST_UNDERFLOW 2 /* step size below 10 ulp(t) (scipy rk.py:128-129) */
#define HODE_ST_NONFINITE 3 /* state became non-finite */

/* Network envelope.  NNResidual (models/nn_residual.py:28-98) builds 9 -> H x L -> 6 for any H, L; the reference's configs
 * use 64 x 4 (default, 4gi_*, mimic_clinical) and 128 x 5 (configs/ablation_no_physics.yaml:11-12).
 *   H <= 64 and L <= 4   tuned kernels: all weights register-resident, one hidden unit per wavefront lane;
 *   otherwise            generic kernels (two hidden units per lane, weights streamed from L2, gradients by coalesced
 *                        atomics), same results contract, sized for the batches such shapes are trained with.
 * Activation: ReLU in the tuned kernels; tanh / elu / leaky_relu(0.1) through the generic kernels (HODE_LAYERS below).  Dropout
 * (also offered by NNResidual, never passed by HybridODENN, models/hybrid_ode_nn.py:57-58) is a training-time random mask with
 * no meaning inside an ODE right-hand side that is evaluated six times per step: the host class raises NotImplementedError for
 * it instead of silently computing something else. */
/* Activation codes.  The `L` argument of every entry point is HODE_LAYERS(hidden layers, activation): layers in bits 0..7, the
 * code in bits 8..15 -- a plain layer count means ReLU, which is all HybridODENN ever builds.  tanh / elu (alpha 1) /
 * leaky_relu (0.1) of NNResidual (models/nn_residual.py:50-56) are reached by replacing `model.nn_residual`; they run through
 * the generic kernels whatever the shape. */
#define HODE_ACT_RELU 0
#define HODE_ACT_TANH 1
#define HODE_ACT_ELU 2
#define HODE_ACT_LEAKY_RELU 3
#define HODE_LAYERS(L, act) (((L) & 0xff) | ((act) << 8))
/* hode_solve_fwd_* only: OR into `L` when nn_p holds ONE network shared by all n_sets sets of mechanistic constants (ode_p stays
 * [n_sets][17]).  The Sobol study of plots/plot_all.py:139-196 integrates 16 384 constant sets through one trained network: shared,
 * the launch reads 54 KB of weights instead of 885 MB of copies. */
#define HODE_LAYERS_NN_SHARED (1 << 16)
#define HODE_MAX_HIDDEN 128
#define HODE_MAX_LAYERS 8
#define HODE_TUNED_HIDDEN 64 /* envelope of the register-resident kernels */
#define HODE_TUNED_LAYERS 4

const char *hode_version(void);

/* number of MLP parameters for (H hidden, L hidden layers); 13510 for (64,4), 68102 for (128,5) */
int hode_nn_param_count(int H, int L);

/* bytes of the tape the solve writes for the adjoint: per accepted step {t, h, t0, 1/(t1-t0), v0, v1-v0, d0, d1-d0}
 * (the step and the constants of its grid interval: time, tVNS and gastric-distension inputs), the grid
 * interval (bit 30 set when the step ended exactly on the grid point closing that interval), and the "stage tape" -- the
 * MLP activations and stage state of every Runge-Kutta stage (tuned path 6 x (L x 64 + 8) reals per step, generic path
 * 6 x (2L x 64 + 8)), so that the adjoint never re-runs the forward.  This is a memory-for-compute trade sized for
 * 288 GB of HBM: 6.3 KB per step in fp32 for (64,4), i.e. 1.9 MB per trajectory at max_steps = 300.  Tuned shapes: + the
 * adjoint's gradient rows, min(B, 1024) x (P + 17 reals, padded to a multiple of 64).
 * hode_tape_bytes(.., L) == hode_tape_bytes_hl(.., 64, L). */
size_t hode_tape_bytes_hl(int B, int max_steps, int elem_size /* 4 or 8 */, int H, int L);
size_t hode_tape_bytes(int B, int max_steps, int elem_size /* 4 or 8 */, int L);

/* ---- K1: RHS forward.  Replaces HybridODENN.ode_residual (models/hybrid_ode_nn.py:108-134)
 *      = ODECore.forward (models/ode_core.py:81-166) + NNResidual.forward
 *      (models/nn_residual.py:100-151).  t/meal/tvns/gd: [B] or NULL.  out[B,6].            */
int hode_rhs_fwd_f32(void *stream, int B, const float *x, const float *t, const float *meal,
                     const float *tvns, const float *gd, const float *ode_p, const float *nn_p,
                     int H, int L, float *out);
int hode_rhs_fwd_f64(void *stream, int B, const double *x, const double *t, const double *meal,
                     const double *tvns, const double *gd, const double *ode_p, const double *nn_p,
                     int H, int L, double *out);

/* ---- K5: RHS backward (VJP).  Replaces torch autograd over ode_residual in the physics loss
 *      (models/hybrid_ode_nn.py:318-330).  gout[B,6] -> gx[B,6] (written), gt[B] (written, may
 *      be NULL), gnn[P] and gode[17] (ACCUMULATED with atomics: zero them first; may be NULL). */
int hode_rhs_bwd_f32(void *stream, int B, const float *x, const float *t, const float *meal,
                     const float *tvns, const float *gd, const float *ode_p, const float *nn_p,
                     int H, int L, const float *gout, float *gx, float *gt, float *gnn, float *gode);
int hode_rhs_bwd_f64(void *stream, int B, const double *x, const double *t, const double *meal,
                     const double *tvns, const double *gd, const double *ode_p, const double *nn_p,
                     int H, int L, const double *gout, double *gx, double *gt, double *gnn, double *gode);

/* ---- K2+K3: forward solve.  Replaces HybridODENN.forward (models/hybrid_ode_nn.py:136-261):
 *      the per-patient scipy.integrate.solve_ivp loop (:184-256) incl. input interpolation
 *      (:210-231) and the RK45 stepper (scipy/integrate/_ivp/rk.py:14-72,111-176).
 *      t: [T] (t_batched=0) or [B,T] (t_batched=1).  y[B,T,6] written (rows after a failure
 *      are zero).  status/nsteps/nfev: int32[B] (nsteps/nfev may be NULL).
 *      tape: NULL, or hode_tape_bytes_hl(B,max_steps,sizeof(real),H,L) bytes (256-byte aligned) that
 *      receive the accepted steps and their stage activations (needed by hode_solve_bwd_*).     */
int hode_solve_fwd_f32(void *stream, int B, int T, const float *x0, const float *t, int t_batched,
                       const float *meal, int meal_mode, const float *tvns, int tvns_mode,
                       const float *gd, int gd_mode, const float *ode_p, const float *nn_p,
                       int n_sets, int H, int L, int method, double rtol, double atol,
                       int max_steps, float *y, int32_t *status, int32_t *nsteps, int32_t *nfev,
                       void *tape);
int hode_solve_fwd_f64(void *stream, int B, int T, const double *x0, const double *t, int t_batched,
                       const double *meal, int meal_mode, const double *tvns, int tvns_mode,
                       const double *gd, int gd_mode, const double *ode_p, const double *nn_p,
                       int n_sets, int H, int L, int method, double rtol, double atol,
                       int max_steps, double *y, int32_t *status, int32_t *nsteps, int32_t *nfev,
                       void *tape);

/* ---- K4: reverse-time discrete adjoint of the solve above (no reference counterpart: the
 *      reference detaches the solve; north_star requires it).
 *      gy[B,T,6] = dLoss/dy  ->  gx0[B,6] (written), gnn[n_sets,P] and gode[n_sets,17]
 *      (ACCUMULATED: added to what is there -- zero them first; either may be NULL).  Tuned shapes (H <= 64, L <= 4): no
 *      floating-point atomics -- every workgroup writes one gradient row into the tail of the tape and a second, fixed-order
 *      pass adds the rows: the same call gives the same bits (the reference's CPU training is deterministic).  Generic shapes:
 *      coalesced atomics, reproducible to rounding only.  tape: the buffer the forward filled.  It is not const: the adjoint
 *      uses its tail (the gradient rows) as scratch -- and its LDS-DMA reads whole 256-byte rows: up to 224 bytes beyond the last stage
 *      record and up to 224 beyond a step entry, i.e. into the regions that FOLLOW them inside the same buffer (never beyond
 *      hode_tape_bytes_hl() bytes: the gradient rows, at least 256 bytes, close the buffer) --; what the forward recorded stays intact, the same tape may be walked
 *      again.
 *      nsteps[b], status[b]: what the forward returned for this tape.  The adjoint walks min(nsteps[b], max_steps) steps:
 *      a count larger than the tape it is handed (the caller merged the bookkeeping of a re-integration with a larger
 *      budget, say) is CLAMPED SILENTLY -- never an out-of-bounds read, but then the gradient is that of the truncated
 *      trajectory; pass the nsteps of the forward call that filled THIS tape.  A trajectory with status != 0 contributes the
 *      cotangents of the rows it still wrote (rows after the failure are zero in y and their gy is ignored); a non-finite
 *      step is never on the tape (status 3 trajectories end BEFORE the step that blew up).                  */
int hode_solve_bwd_f32(void *stream, int B, int T, const float *t, int t_batched,
                       const float *meal, int meal_mode, const float *tvns, int tvns_mode,
                       const float *gd, int gd_mode, const float *ode_p, const float *nn_p,
                       int n_sets, int H, int L, int method, int max_steps, const int32_t *nsteps,
                       const int32_t *status, void *tape, const float *gy, float *gx0,
                       float *gnn, float *gode);
int hode_solve_bwd_f64(void *stream, int B, int T, const double *t, int t_batched,
                       const double *meal, int meal_mode, const double *tvns, int tvns_mode,
                       const double *gd, int gd_mode, const double *ode_p, const double *nn_p,
                       int n_sets, int H, int L, int method, int max_steps, const int32_t *nsteps,
                       const int32_t *status, void *tape, const double *gy, double *gx0,
                       double *gnn, double *gode);

/* ---- K4 / K5 with input gradients: the derivatives with respect to the external inputs meal, tVNS and GD as well.  The
 *      exact derivative of what the kernels compute: d f_G / d meal = 1; tVNS enters only the MLP (input column 8 of W1); GD
 *      enters only k_GE = k_GE0 (1 - GD^g / (IGD_50^g + GD^g)) in dG (zero derivative at GD <= 0).  Step sizes are constants, as
 *      for every other gradient of the adjoint.
 *      Every gradient pointer is NULL (not wanted) or, for an input of mode 1, [B], for mode 2, [B,T]; a non-NULL pointer for an
 *      input of mode 0 (absent / NULL) is HODE_EINVAL.  Input gradients are WRITTEN, not accumulated (like gx0 / gx).
 *      Solve (hode_solve_bwd_inputs_*): on grid interval k an accepted step evaluates its stages at u(t_s) = u_k + a_s (u_{k+1} - u_k),
 *      a_s = (t_s - t_k) / (t_{k+1} - t_k); with c_s the stage's input cotangent,
 *        mode 2:  g[b,k] += (1 - a_s) c_s,  g[b,k+1] += a_s c_s   over every stage of every taped step on interval k;
 *        mode 1:  g[b] = sum of c_s over every stage of every taped step.
 *      A grid row that bounds no taped step (rows after a failure, rows inside a run of repeated grid times) is 0.  Each row
 *      belongs to one trajectory: no atomics, the same call gives the same bits.  gx0 / gnn / gode are those of
 *      hode_solve_bwd_*: fp64 gx0 the same bits, fp64 gnn / gode the same bits on the tuned shapes (on generic shapes they are summed
 *      with atomics, equal to rounding as between any two calls); fp32: the request takes the one-role adjoint kernels (the
 *      wave-specialised and the multi-trajectory kernels have no input gradients), equal to rounding.
 *      RHS (hode_rhs_bwd_inputs_*): gmeal / gtvns / ggd [B] = (d out[s,:] / d input[s]) . gout[s,:]; the other arguments are
 *      those of hode_rhs_bwd_*.                                                                                          */
int hode_solve_bwd_inputs_f32(void *stream, int B, int T, const float *t, int t_batched,
                              const float *meal, int meal_mode, const float *tvns, int tvns_mode,
                              const float *gd, int gd_mode, const float *ode_p, const float *nn_p,
                              int n_sets, int H, int L, int method, int max_steps, const int32_t *nsteps,
                              const int32_t *status, void *tape, const float *gy, float *gx0,
                              float *gnn, float *gode, float *gmeal, float *gtvns, float *ggd);
int hode_solve_bwd_inputs_f64(void *stream, int B, int T, const double *t, int t_batched,
                              const double *meal, int meal_mode, const double *tvns, int tvns_mode,
                              const double *gd, int gd_mode, const double *ode_p, const double *nn_p,
                              int n_sets, int H, int L, int method, int max_steps, const int32_t *nsteps,
                              const int32_t *status, void *tape, const double *gy, double *gx0,
                              double *gnn, double *gode, double *gmeal, double *gtvns, double *ggd);
/* ---- K6: tangent-linear (forward-mode) solve over the tape of the forward -- the sensitivities of a trajectory with respect to
 *      a few directions (the reference has no sensitivities; per-patient calibration needs them.  CPU restatement:
 *      hode_oracle_solve_jvp_f32 / _f64, oracle/hode_oracle_impl.h, to which tests/test_jvp_enum_gpu.py holds this kernel).
 *      For K directions per trajectory
 *        dy[b,k,:,:] = (d y_b / d ode_p) v_ode[set(b),k,:] + (d y_b / d x0_b) v_x0[b,k,:]
 *      v_ode [n_sets][K][17] and v_x0 [B][K][6]: either may be NULL (that part is 0), not both; dy [B][K][T][6] is WRITTEN.
 *      The exact derivative of the discrete scheme the forward ran: the taped accepted steps with their step sizes held
 *      constant, the same tableau and grid breaks; ReLU' = (taped activation > 0); GD enters through k_GE (zero derivative of the
 *      Hill term's constants at GD <= 0, as in the adjoint).  The arguments up to `tape` are those of hode_solve_bwd_* for the
 *      same tape, which is READ ONLY here: the same tape may be walked again by this call or by the adjoint.
 *      Rows follow y exactly: row 0 = v_x0; a grid row is the tangent at the end of the step that closes its interval; a
 *      repeated grid time copies the row before it; rows after a failure (status 1-3) are 0, as in y.  Non-finite tangents are
 *      returned as computed; status is the forward's.
 *      Duality: this pass and hode_solve_bwd_* differentiate the same discrete map, so for any gy
 *        <gy, dy>  ==  <gx0, v_x0> + <gode, v_ode>       to rounding (gx0, gode of hode_solve_bwd_* with the same gy).
 *      One trajectory per wavefront, no atomics: the same call gives the same bits, and a K-direction call gives the bits of K
 *      one-direction calls.  Any K >= 1 (tiled internally).
 *      Envelope: the tuned shapes (H <= 64, L <= 4, ReLU), fp32 and fp64, both methods, every input mode, batched or shared
 *      grids.  HODE_EUNSUPPORTED for larger or non-ReLU networks and for HODE_LAYERS_NN_SHARED; HODE_EINVAL for K < 1, no
 *      direction, or the argument rules of hode_solve_bwd_* -- all checked before any launch.                              */
int hode_solve_jvp_f32(void *stream, int B, int T, const float *t, int t_batched,
                       const float *meal, int meal_mode, const float *tvns, int tvns_mode,
                       const float *gd, int gd_mode, const float *ode_p, const float *nn_p,
                       int n_sets, int H, int L, int method, int max_steps, const int32_t *nsteps,
                       const int32_t *status, const void *tape, int K, const float *v_ode,
                       const float *v_x0, float *dy);
int hode_solve_jvp_f64(void *stream, int B, int T, const double *t, int t_batched,
                       const double *meal, int meal_mode, const double *tvns, int tvns_mode,
                       const double *gd, int gd_mode, const double *ode_p, const double *nn_p,
                       int n_sets, int H, int L, int method, int max_steps, const int32_t *nsteps,
                       const int32_t *status, const void *tape, int K, const double *v_ode,
                       const double *v_x0, double *dy);
/*      The same pass for EVERY network hode_solve_fwd_* can tape: argument list, semantics, rows and duality as above.
 *      Envelope: 1 <= H <= HODE_MAX_HIDDEN (128), 1 <= L <= HODE_MAX_LAYERS (8), HODE_ACT_RELU / TANH / ELU / LEAKY_RELU in bits
 *      8..15 of L, fp32 and fp64, both methods, every input mode, batched or shared grids, n_sets >= 1.  The tuned shapes take
 *      the kernel of hode_solve_jvp_* (the same bits); every other shape takes a kernel of its own (hode_generic_jvp.hip: one
 *      trajectory and a tile of directions per eight-wave team, act' from the taped post-activation values, no atomics), with
 *      the same contracts: the same call gives the same bits, a K-direction call gives the bits of K one-direction calls, and a
 *      trajectory's tangent does not depend on the rest of the batch.
 *      HODE_EUNSUPPORTED for H > 128, L > 8, an unknown activation code and HODE_LAYERS_NN_SHARED; HODE_EINVAL as above, and a
 *      bad argument outranks an unsupported shape -- all checked before any launch.                                          */
int hode_solve_jvp_any_f32(void *stream, int B, int T, const float *t, int t_batched,
                           const float *meal, int meal_mode, const float *tvns, int tvns_mode,
                           const float *gd, int gd_mode, const float *ode_p, const float *nn_p,
                           int n_sets, int H, int L, int method, int max_steps, const int32_t *nsteps,
                           const int32_t *status, const void *tape, int K, const float *v_ode,
                           const float *v_x0, float *dy);
int hode_solve_jvp_any_f64(void *stream, int B, int T, const double *t, int t_batched,
                           const double *meal, int meal_mode, const double *tvns, int tvns_mode,
                           const double *gd, int gd_mode, const double *ode_p, const double *nn_p,
                           int n_sets, int H, int L, int method, int max_steps, const int32_t *nsteps,
                           const int32_t *status, const void *tape, int K, const double *v_ode,
                           const double *v_x0, double *dy);
int hode_rhs_bwd_inputs_f32(void *stream, int B, const float *x, const float *t, const float *meal,
                            const float *tvns, const float *gd, const float *ode_p, const float *nn_p,
                            int H, int L, const float *gout, float *gx, float *gt, float *gnn, float *gode,
                            float *gmeal, float *gtvns, float *ggd);
int hode_rhs_bwd_inputs_f64(void *stream, int B, const double *x, const double *t, const double *meal,
                            const double *tvns, const double *gd, const double *ode_p, const double *nn_p,
                            int H, int L, const double *gout, double *gx, double *gt, double *gnn, double *gode,
                            double *gmeal, double *gtvns, double *ggd);

/* ---- K6: fused global-norm clip + Adam.  Replaces clip_grad_norm_(...,5.0) + torch.optim.Adam
 *      .step() (train/train_hybrid.py:255-261, 438-441).  g is first multiplied by grad_scale
 *      (e.g. 1/world_size after an all-reduce(sum)); max_norm <= 0 disables clipping.
 *      scratch: >= 8 bytes of device memory (holds the squared norm), zeroed by the call.       */
int hode_adam_step_f32(void *stream, int64_t n, float *p, const float *g, float *m, float *v,
                       float lr, float beta1, float beta2, float eps, int step, float max_norm,
                       float grad_scale, float weight_decay, void *scratch);

/* ---- loss helper: sum((y - obs)^2) and dLoss/dy = 2*scale*(y-obs) in one pass
 *      (models/hybrid_ode_nn.py:294 F.mse_loss).  loss_sum: double[1], ACCUMULATED.            */
int hode_mse_fwd_bwd_f32(void *stream, int64_t n, const float *y, const float *obs, float scale,
                         double *loss_sum, float *gy);

/* ---- self test of the cross-lane primitives (DPP / permlane swaps); out: int32[64*8].        */
int hode_selftest_xlane(void *stream, int32_t *out);

/* =====================================================================================================
 * Data side: the cohort generator and the dataset windows, on the device.
 * ===================================================================================================== */
#define HODE_4GI_NPAR 26       /* CLglc CLglci Qglc VCglc VPglc CLins VCins Ke0ins VCglp VM_GLP KM_GLP CLglg VCglg
                                  CLgip VCgip Qgip VPgip GLCINS_S EMAX_1 EC50_1 HILL_1 EMAX_4 EC50_4 FDGLP FDGIP FDGLG */
#define HODE_4GI_T2DM 0
#define HODE_4GI_HV 1
#define HODE_4GI_TABLE_COLS 9  /* subject_id time_hours time_minutes glucose_mmol_L insulin_pmol_L glp1_pmol_L
                                  glucagon_pmol_L gip_pmol_L meal_indicator  (data/generate4GI.py:246-257) */
#define HODE_4GI_SCRATCH_BYTES 98304
#define HODE_4GI_NORM_NONE 0   /* mean 0 / std 1 */
#define HODE_4GI_NORM_LOCAL 1  /* statistics of the windows passed in this call */
#define HODE_4GI_NORM_GIVEN 2  /* mean_std[12] is an INPUT (statistics combined over the shards of a multi-GPU dataset) */

/* the reference's parameter set (data/generate4GI.py:15-64) for a patient type -> par[HODE_4GI_NPAR] (HOST memory) */
int hode_4gi_default_params(int patient_type, double *par_host);

/* ---- K7: 4GI cohort generator.  Replaces FourGIModel.simulate (data/generate4GI.py:159-212: one scipy odeint call
 *      per subject per grid interval) and the table assembly of generate_dataset (:221-271) for B subjects at once.
 *      One subject per wavefront lane, fp64, DP5(4) at (rtol, atol) inside every grid interval.
 *      T grid points at k*interval_min minutes; bsl[B,5] = the subject's baselines (glucose, insulin, GLP-1, glucagon,
 *      GIP); meals: meal_time/meal_size [n_meals] shared by all subjects (meals_per_subject = 0) or [B,n_meals];
 *      par_host: HOST pointer to HODE_4GI_NPAR doubles or NULL (= hode_4gi_default_params(patient_type));
 *      z[T,5,B]: standard-normal draws for the measurement noise (biomarker order glucose, insulin, glp1, glucagon,
 *      gip; subject index fastest so that a wavefront reads contiguous memory) or NULL / noise_cv = 0 for the clean
 *      solution;
 *      table[B*T, 9] written, subject ids start at subject0; status[B] (may be NULL) as in hode_solve_fwd.          */
int hode_4gi_generate_f64(void *stream, int B, int T, double interval_min, int patient_type, const double *par_host,
                          const double *bsl, int n_meals, const double *meal_time, const double *meal_size,
                          int meals_per_subject, const double *z, double noise_cv, int64_t subject0, double rtol,
                          double atol, int max_steps, double *table, int32_t *status);

/* 4GI right-hand side alone (FourGIModel.model_equations, data/generate4GI.py:73-157): y[B,8], meal[B] -> d[B,8] */
int hode_4gi_rhs_f64(void *stream, int B, int patient_type, const double *par_host, const double *bsl, const double *y,
                     const double *meal, double *d);

/* ---- K8: sliding windows + z-scoring.  Replaces GlucoseDataset.__init__/__getitem__ (train/train_hybrid.py:43-155).
 *      table[rows, ncols] fp64 row-major; col_* = column indices (col_ge / col_ffa / col_meal / col_tvns may be -1:
 *      0, 1, 0, 0 as in :76-91); time = table[:, col_time] / time_div (60 for time_minutes, :93-94);
 *      row0[N] (device int64) = first table row of every window (subject by subject, start += stride, :105-121);
 *      normalize = HODE_4GI_NORM_LOCAL: mean/std over ALL window rows (overlaps counted as often as they occur, population std
 *      + 1e-6; :124-127), HODE_4GI_NORM_NONE: mean 0 / std 1, HODE_4GI_NORM_GIVEN: as found in mean_std.  Written: states[N,S,6] fp32 (observations; initial_state = [:,0]),
 *      meal[N,S], tvns[N,S], time[N,S] fp32, mean_std[12] fp64 (6 means, 6 stds).
 *      scratch: HODE_4GI_SCRATCH_BYTES of device memory.  Deterministic (no atomics).                              */
int hode_4gi_windows_f32(void *stream, const double *table, int ncols, int col_time, double time_div, int col_glucose,
                         int col_insulin, int col_glucagon, int col_glp1, int col_ge, int col_ffa, int col_meal,
                         int col_tvns, const int64_t *row0, int64_t N, int64_t S, int normalize, float *states,
                         float *meal, float *tvns, float *time, double *mean_std, void *scratch);

/* Mergeable statistics of the windows of ONE shard: moments[13] = {count, mean[6], M2[6]} (M2 = sum of squared
 * deviations from the shard mean).  A dataset sharded over GPUs all-gathers these 13 doubles, merges them in rank
 * order (Chan et al.: M2 = M2a + M2b + d^2 na nb / n), sets std = sqrt(M2/n) + 1e-6 and calls hode_4gi_windows_f32
 * with HODE_4GI_NORM_GIVEN, so every rank normalises with the statistics of the whole dataset. */
int hode_4gi_window_moments_f64(void *stream, const double *table, int ncols, int col_glucose, int col_insulin,
                                int col_glucagon, int col_glp1, int col_ge, int col_ffa, const int64_t *row0, int64_t N,
                                int64_t S, double *moments, void *scratch);

/* =====================================================================================================
 * MCMC: the per-chain passes of multi-chain Hamiltonian Monte Carlo (inference/hmc.py, run_hmc).  Replaces the
 * random-walk placeholder of the reference's inference/mcmc.py:17-173 (run_nuts).
 *
 * The driver evaluates U(z) = scale * sum (y - obs)^2 + |z|^2 / 2 for C chains at once: the forward solve and the adjoint
 * (hode_solve_fwd_* / hode_solve_bwd_*) run with n_sets = C, hode_mse_sets_* gives every chain its own sum and cotangent.
 * Everything else a sampling iteration does to the chains' state is these kernels.
 *   - pointers: DEVICE memory, except where noted; `stream` as everywhere in this header; HODE_EINVAL for a bad size or a
 *     NULL that is not allowed, checked on the host before any launch;
 *   - chains: C rows of `ld` reals (ld >= D), row c at offset c * ld: z (position), p (momentum), g (grad U), z0 / g0 (the
 *     trajectory's start); minv[ld] = the diagonal of M^-1, shared by all chains.  ld % 4 == 0 and 16-byte aligned rows let
 *     every lane move four coordinates per 16-byte access; the padding (D <= d < ld) must hold 0 in z and 1 in minv;
 *   - coordinates of z (prior-standardised): d < n_ode = popcount(ode_mask) are the sampled mechanistic constants in ascending
 *     ODE-index order (bit k of ode_mask = ode_p[k]), theta = mu[d] + sd[d] z[d] (mu, sd: fp64 [n_ode], the Gaussian priors);
 *     then, with sample_nn, the P MLP weights in nn_p order, theta = z (prior N(0, 1)).  D = n_ode + (sample_nn ? P : 0);
 *   - per-chain scalars are fp64 [C]: U, U0, ke, ke0 (energies), eps (this trajectory's step), log_eps (the adapted one);
 *     failed: int32 [C];
 *   - random numbers: Philox4x32-10, key (seed bits 0..31, chain), counter (coordinate / 4, stream, iter, seed bits 32..63):
 *     a chain's draws do not depend on C or on the launch geometry;
 *   - no floating-point atomics: every chain sum is taken in a fixed order, the same call gives the same bits.
 * ===================================================================================================== */
#define HODE_HMC_ASSEMBLE 1 /* leapfrog flags: g = likelihood gradient (gnn, gode) + z; U = lik_scale * loss_sum + |z|^2 / 2;
                               failed |= any status != 0 of the chain's n_traj trajectories */
#define HODE_HMC_KICK 2     /* p -= kick * eps * g */
#define HODE_HMC_DRIFT 4    /* z += eps * minv * p, then write the sampled entries of nn_p / ode_p (natural coordinates) */
#define HODE_HMC_KE 8       /* ke = p^T minv p / 2 (after the kick) */
#define HODE_HMC_PARAMS 16  /* write the sampled entries of nn_p / ode_p from z without moving */
#define HODE_HMC_SAMPLE 0     /* accept modes: Metropolis test, restore (z0, g0, U0) on reject */
#define HODE_HMC_ADAPT 1      /*   the same + one dual-averaging update of log_eps (gamma 0.05, t0 10, kappa 0.75) */
#define HODE_HMC_SEARCH 2     /*   one trial of the initial step-size search (double / halve to one-step acceptance 0.8); always restores */
#define HODE_HMC_DA_RESTART 3 /*   restart dual averaging: mu = log(10 eps), clear the search state */
#define HODE_HMC_DA_FINISH 4  /*   log_eps = the averaged log step (end of warm-up) */
#define HODE_HMC_WELFORD_ACCUM 1  /* welford flags: add z of every chain, chains in order */
#define HODE_HMC_WELFORD_FINISH 2 /* minv = n/(n+5) var + 1e-3 * 5/(n+5) (Stan), then reset the accumulators */

/* ---- per-set sum of squares and cotangent.  y[n_sets][len] (set s = one chain's trajectories), obs[len] ONE copy shared by
 *      every set (obs index = element index modulo len); loss_sum: double[n_sets], ACCUMULATED (a set split over several calls
 *      sums to its whole); gy[n_sets][len] = 2 * scale * (y - obs) (may be NULL).  Unaligned pointers and any len are fine. */
int hode_mse_sets_f32(void *stream, int n_sets, int64_t len, const float *y, const float *obs, float scale,
                      double *loss_sum, float *gy);
int hode_mse_sets_f64(void *stream, int n_sets, int64_t len, const double *y, const double *obs, double scale,
                      double *loss_sum, double *gy);

/* ---- Observation model (inference/observation.py): the negative log-likelihood of incomplete data with per-state noise, and
 *      its cotangent, per parameter set.  y[n_sets][len] and obs[len] as for hode_mse_sets_*; len = n_traj * T * 6, element i
 *      belongs to state i % 6.  Entry i is OBSERVED when obs[i] is finite and, with a mask (uint8[len], NULL = finiteness
 *      only), mask[i] != 0; an unobserved entry may hold anything (NaN included): it adds exactly 0 to every sum and gets gy = 0.
 *      With S_k = the sum of (y - obs)^2 over the observed entries of state k:
 *        HODE_OBS_FIXED     nll = sum_k w[k] S_k / 2 (w[k] = 1 / sigma_k^2),            gy = w[k] (y - obs);
 *        HODE_OBS_MARGINAL  sigma_k^2 ~ InvGamma(a[k], b[k]) integrated out, n[k] = the number of observed entries of state k
 *                           in the WHOLE set: nll = sum_{n[k] > 0} (a[k] + n[k]/2) log(b[k] + S_k/2),
 *                           gy = (a[k] + n[k]/2) / (b[k] + S_k/2) (y - obs); a state with n[k] = 0 adds 0 and gets gy = 0.
 *      w, a, b, n: HOST double[6] (w: fixed mode, the other three NULL; a, b, n: marginal mode, w NULL).
 *      sse: double[n_sets][6], the S_k, ACCUMULATED like loss_sum of hode_mse_sets; loss_sum: double[n_sets], nll ACCUMULATED
 *      (may be NULL); gy[n_sets][len] (may be NULL).  A non-finite y at an observed entry makes sse and loss_sum non-finite.
 *      flags: 0 = everything in one launch (sums added to sse, then nll and gy from the totals: zero sse before a whole set);
 *      for a set cut into pieces, HODE_OBS_SUMS_ONLY adds the piece's sums to sse and touches nothing else, and
 *      HODE_OBS_FROM_SSE takes sse as finished: nll (add it with ONE piece of the set, NULL for the others) and the piece's gy.
 *      In fixed mode flags = 0 per piece is enough: its nll is that of the call's own sums.  One workgroup per set, sums reduced
 *      in a fixed order: the same call gives the same bits, and 0 equals SUMS_ONLY then FROM_SSE bit for bit on a whole set.
 *      Unaligned pointers and any len are fine. */
#define HODE_OBS_FIXED 0
#define HODE_OBS_MARGINAL 1
#define HODE_OBS_SUMS_ONLY 1
#define HODE_OBS_FROM_SSE 2
int hode_obs_nll_sets_f32(void *stream, int n_sets, int64_t len, const float *y, const float *obs, const uint8_t *mask, int mode,
                          int flags, const double *w, const double *a, const double *b, const double *n, double *sse,
                          double *loss_sum, float *gy);
int hode_obs_nll_sets_f64(void *stream, int n_sets, int64_t len, const double *y, const double *obs, const uint8_t *mask, int mode,
                          int flags, const double *w, const double *a, const double *b, const double *n, double *sse,
                          double *loss_sum, double *gy);

/* ---- trajectory start: p = M^{1/2} xi (xi ~ N(0, 1), stream `iter`), ke0 = p^T minv p / 2, z0 = z, g0 = g, U0 = U,
 *      eps = exp(log_eps) * (1 + jitter * (2u - 1)) (u uniform, same stream), failed = 0. */
int hode_hmc_refresh_f32(void *stream, int C, int D, int ld, uint64_t seed, uint32_t iter, double jitter, const float *minv,
                         const double *log_eps, const float *z, const float *g, const double *U, float *p, float *z0,
                         float *g0, double *U0, double *ke0, double *eps, int32_t *failed);
int hode_hmc_refresh_f64(void *stream, int C, int D, int ld, uint64_t seed, uint32_t iter, double jitter, const double *minv,
                         const double *log_eps, const double *z, const double *g, const double *U, double *p, double *z0,
                         double *g0, double *U0, double *ke0, double *eps, int32_t *failed);

/* ---- one leapfrog pass (HODE_HMC_* flags, applied in the order assemble, kick, ke, drift, params).  gnn[C][P] / gode[C][17]:
 *      the adjoint's per-set gradients of scale * sum (y - obs)^2 (NULL: no likelihood term), loss_sum[C] its value (NULL: 0);
 *      status[C][n_traj]: the solve's (NULL: none); nn_p[C][P] / ode_p[C][17]: the parameters of the next solve, only the sampled
 *      entries are written.  A NULL that a set flag needs is HODE_EINVAL. */
int hode_hmc_leapfrog_f32(void *stream, int C, int D, int ld, int flags, double kick, const double *eps, const float *minv,
                          float *z, float *p, float *g, const float *gnn, const float *gode, int P, const double *loss_sum,
                          double lik_scale, const int32_t *status, int n_traj, double *U, double *ke, int32_t *failed,
                          uint32_t ode_mask, const double *mu, const double *sd, int sample_nn, float *nn_p, float *ode_p);
int hode_hmc_leapfrog_f64(void *stream, int C, int D, int ld, int flags, double kick, const double *eps, const double *minv,
                          double *z, double *p, double *g, const double *gnn, const double *gode, int P, const double *loss_sum,
                          double lik_scale, const int32_t *status, int n_traj, double *U, double *ke, int32_t *failed,
                          uint32_t ode_mask, const double *mu, const double *sd, int sample_nn, double *nn_p, double *ode_p);

/* ---- end of a trajectory (mode HODE_HMC_*).  H = U + ke; divergent = failed, H1 not finite or H1 - H0 > 1000 (accept
 *      probability 0); a rejected proposal restores z, g, U from z0, g0, U0.  da: fp64 [C][4] dual-averaging state {mu, log eps
 *      bar, H bar, t}; search: int32 [C][2] {direction, done}.  slot >= 0 (sample modes) stores the kept state:
 *      draws[C][n_slots][D] in natural coordinates (may be NULL), stats[C][n_slots][4] = {accept probability, log posterior
 *      (-U, up to a constant), divergent, failed solve}. */
int hode_hmc_accept_f32(void *stream, int C, int D, int ld, int mode, uint64_t seed, uint32_t iter, double target_accept,
                        float *z, const float *z0, float *g, const float *g0, double *U, const double *U0, const double *ke0,
                        const double *ke, const int32_t *failed, double *log_eps, double *da, int32_t *search, int n_ode,
                        const double *mu, const double *sd, float *draws, double *stats, int n_slots, int slot);
int hode_hmc_accept_f64(void *stream, int C, int D, int ld, int mode, uint64_t seed, uint32_t iter, double target_accept,
                        double *z, const double *z0, double *g, const double *g0, double *U, const double *U0, const double *ke0,
                        const double *ke, const int32_t *failed, double *log_eps, double *da, int32_t *search, int n_ode,
                        const double *mu, const double *sd, double *draws, double *stats, int n_slots, int slot);

/* ---- pooled cross-chain variance of every coordinate (the diagonal mass matrix of a slow warm-up window).
 *      wf: fp64 [3][D] = {count, mean, M2} per coordinate, zero it before the first window. */
int hode_hmc_welford_f32(void *stream, int C, int D, int ld, int flags, const float *z, double *wf, float *minv);
int hode_hmc_welford_f64(void *stream, int C, int D, int ld, int flags, const double *z, double *wf, double *minv);

/* ---- No-U-Turn sampling (inference/nuts.py, run_nuts): multinomial NUTS with the generalised U-turn criterion, every
 *      chain's tree built one leaf per global step.  An iteration is hode_hmc_refresh, hode_nuts_begin, hode_nuts_compact,
 *      then, while the count of active chains A > 0: hode_nuts_pre, the solve + hode_mse_sets + adjoint of the A active
 *      chains' parameter sets, hode_nuts_post, hode_nuts_compact; then hode_nuts_finish.  Chains, coordinates, mu / sd and
 *      minv as for the HMC passes above.
 *   - tree: [HODE_NUTS_ROWS][C][ld] reals, rows {frontier z, p, g; left edge z, p, g; right edge z, p, g; proposal z, g;
 *     subtree proposal z, g; rho; rho_sub}; ckpt: [C][max_depth][2][ld] reals (the open U-turn blocks' first p# and the
 *     momentum sum before it); dst: fp64 [C][8] {H0, log_w, log_w_sub, sum_acc, U of the proposal, U of the subtree
 *     proposal}; ist: int32 [C][8] {j, leaf in the subtree, n_leaf, active, divergent, failed, direction, tree_depth};
 *   - rank: int32 [C], the chain's slot in the compacted solve (hode_nuts_compact: active chains numbered 0..A-1 in chain
 *     order, -1 for the others); count: int32 [1], A;
 *   - random numbers: Philox streams 4 (direction of doubling j, group j), 5 (multinomial choice of leaf n, group n) and 6
 *     (merge of subtree j, group j) of the chain and `iter`: independent of C and of the slot. */
#define HODE_NUTS_ROWS 15
#define HODE_NUTS_MAX_DEPTH 30

/* tree set-up after hode_hmc_refresh: edges and frontier = (z, p, g), proposal = (z, g, U), rho = p, H0 = U0 + ke0, log_w = 0,
 * j = n_leaf = 0, every chain active. */
int hode_nuts_begin_f32(void *stream, int C, int D, int ld, const float *z, const float *p, const float *g, const double *U,
                        const double *U0, const double *ke0, float *tree, double *dst, int32_t *ist);
int hode_nuts_begin_f64(void *stream, int C, int D, int ld, const double *z, const double *p, const double *g, const double *U,
                        const double *U0, const double *ke0, double *tree, double *dst, int32_t *ist);

/* start of a leaf of every active chain: at a doubling's first leaf its direction v (stream 4) and frontier = the edge on side
 * v; then p -= v eps/2 g, z += v eps minv p at the frontier, and the sampled entries of nn_p[rank][P] / ode_p[rank][17] (NULL:
 * not written) from z. */
int hode_nuts_pre_f32(void *stream, int C, int D, int ld, uint64_t seed, uint32_t iter, const double *eps, const float *minv,
                      float *tree, int32_t *ist, const int32_t *rank, uint32_t ode_mask, const double *mu, const double *sd,
                      int sample_nn, int P, float *nn_p, float *ode_p);
int hode_nuts_pre_f64(void *stream, int C, int D, int ld, uint64_t seed, uint32_t iter, const double *eps, const double *minv,
                      double *tree, int32_t *ist, const int32_t *rank, uint32_t ode_mask, const double *mu, const double *sd,
                      int sample_nn, int P, double *nn_p, double *ode_p);

/* end of a leaf of every active chain: grad U and U from slot rank[c] of gnn[A][P] / gode[A][17] / loss_sum[A] / status[A][n_traj]
 * (as hode_hmc_leapfrog's HODE_HMC_ASSEMBLE; NULL: no likelihood term), p -= v eps/2 g, H = U + ke; then divergence (failed
 * solve, H not finite, H - H0 > 1000), the accept statistic, the multinomial choice inside the subtree (stream 5), rho_sub,
 * the U-turn checks of the aligned blocks that end here, and, when the subtree is complete, the biased progressive choice
 * (stream 6), the merge and the U-turn check of the whole tree.  A divergence, a U-turn or j = max_depth ends the chain's tree. */
int hode_nuts_post_f32(void *stream, int C, int D, int ld, int max_depth, uint64_t seed, uint32_t iter, const double *eps,
                       const float *minv, float *tree, float *ckpt, double *dst, int32_t *ist, const int32_t *rank,
                       const float *gnn, const float *gode, int P, const double *loss_sum, double lik_scale,
                       const int32_t *status, int n_traj, uint32_t ode_mask, const double *sd, int sample_nn);
int hode_nuts_post_f64(void *stream, int C, int D, int ld, int max_depth, uint64_t seed, uint32_t iter, const double *eps,
                       const double *minv, double *tree, double *ckpt, double *dst, int32_t *ist, const int32_t *rank,
                       const double *gnn, const double *gode, int P, const double *loss_sum, double lik_scale,
                       const int32_t *status, int n_traj, uint32_t ode_mask, const double *sd, int sample_nn);

/* active flags -> rank[C] and count[0] = A (one workgroup, chains in order). */
int hode_nuts_compact(void *stream, int C, const int32_t *ist, int32_t *rank, int32_t *count);

/* end of an iteration: (z, g, U) = the tree's proposal; accept statistic = sum_acc / n_leaf; adapt = 1: one dual-averaging
 * update of log_eps with it (da as for hode_hmc_accept); slot >= 0 stores draws[C][n_slots][D] (natural coordinates, may be
 * NULL) and stats[C][n_slots][6] = {accept statistic, log posterior (-U), divergent, failed solve, tree_depth, n_leapfrog}. */
int hode_nuts_finish_f32(void *stream, int C, int D, int ld, int adapt, double target_accept, float *z, float *g, double *U,
                         const float *tree, const double *dst, const int32_t *ist, double *log_eps, double *da, int n_ode,
                         const double *mu, const double *sd, float *draws, double *stats, int n_slots, int slot);
int hode_nuts_finish_f64(void *stream, int C, int D, int ld, int adapt, double target_accept, double *z, double *g, double *U,
                         const double *tree, const double *dst, const int32_t *ist, double *log_eps, double *da, int n_ode,
                         const double *mu, const double *sd, double *draws, double *stats, int n_slots, int slot);

/* ---- Population model (inference/population.py, run_population): a reparameterisation layer between the samplers' chain
 *      coordinates and the solve's per-set constants.  K sampled constants (the set bits of ode_mask, ascending), B patients.
 *      A row of coords [A][ld] (ld >= D = K (B + 2), DEVICE) holds, each with an N(0, 1) prior,
 *          [ m_0..m_{K-1} | s_0..s_{K-1} | z_{0,0}..z_{0,K-1} | ... | z_{B-1,0}..z_{B-1,K-1} ]
 *      and means
 *          mu_pop_k = mu0_k + sd0_k m_k,   tau_k = tau0_k exp(tau_log_sd s_k),   theta_{b,k} = mu_pop_k + tau_k z_{b,k}.
 *      mu0, sd0, tau0: fp64 [K], DEVICE.  Everything is computed in double and rounded once.
 *   - pop_params: ode_p[A * B][17], set a * B + b = patient b of row a; ALL 17 entries are written, the unsampled ones from
 *     ode_base[17].
 *   - pop_grad: the transpose.  With G_{b,k} = gode[a * B + b][ODE index of k] (the adjoint's per-set gradient):
 *          glik[a][k] = sd0_k sum_b G_{b,k},  glik[a][K + k] = tau_log_sd tau_k sum_b G_{b,k} z_{b,k},
 *          glik[a][2 K + b K + k] = tau_k G_{b,k};  entries D..ld-1 are written as 0.
 *     One workgroup per row, lane t sums the patients t, t + 256, ... in ascending order in fp64, then the fixed order of the
 *     chain reductions above; no floating-point atomics: the same call gives the same bits, and a row's result depends neither
 *     on A nor on the row's index.
 *   A == 0: HODE_OK, nothing launched.  HODE_EINVAL: K < 1, K > 17, popcount(ode_mask) != K, B < 1, ld < K (B + 2), a NULL. */
int hode_pop_params_f32(void *stream, int A, int B, int K, int ld, const float *coords, uint32_t ode_mask, const double *mu0,
                        const double *sd0, const double *tau0, double tau_log_sd, const float *ode_base, float *ode_p);
int hode_pop_params_f64(void *stream, int A, int B, int K, int ld, const double *coords, uint32_t ode_mask, const double *mu0,
                        const double *sd0, const double *tau0, double tau_log_sd, const double *ode_base, double *ode_p);
int hode_pop_grad_f32(void *stream, int A, int B, int K, int ld, const float *coords, const float *gode, uint32_t ode_mask,
                      const double *sd0, const double *tau0, double tau_log_sd, float *glik);
int hode_pop_grad_f64(void *stream, int A, int B, int K, int ld, const double *coords, const double *gode, uint32_t ode_mask,
                      const double *sd0, const double *tau0, double tau_log_sd, double *glik);

/* ---- Initial-state model (inference/initial_state.py; run_hmc / run_nuts / run_population with initial_state=...): a
 *      reparameterisation layer between the samplers' chain coordinates and the solve's per-trajectory initial states.  B
 *      patients, n_lat latent states (the set bits of lat_mask over the six states, ascending).  A row of coords [A][ld]
 *      (DEVICE) holds from column `off` the B n_lat values w_{b,i} (patient-major, ld >= off + B n_lat), each with an N(0, 1)
 *      prior.  m, s: fp64 [B][6], DEVICE; only the latent entries are read.  Everything is computed in double and rounded once.
 *   - x0_params: x0_out[(a B + b) 6 + j] = m_{b,j} + s_{b,j} w_{b,rank(j)} (link 0) or m_{b,j} exp(s_{b,j} w_{b,rank(j)})
 *     (link 1) for latent j, and x0_base[b 6 + j], copied exactly, otherwise.  With ode_p != NULL also the global constants of
 *     the row, ode_p[a][17]: mu_k + sd_k coords[a ld + k] for the K set bits of ode_mask (ascending ODE index; mu, sd fp64 [K],
 *     off >= K), ode_base[17] elsewhere.
 *   - x0_grad: the transpose.  glik[a ld + off + b n_lat + i] = gx0[(a B + b) 6 + j] s_{b,j} (link 0) or
 *     gx0[..] s_{b,j} x0_{b,j} (link 1, x0 recomputed in double from coords); with gode != NULL (the adjoint's per-row gradient
 *     [A][17]) glik[a ld + k] = sd_k gode[a 17 + idx_k].  Values are written, not accumulated, and no other entry of glik is
 *     touched (the pad, and the columns another layer owns: the pair composes with pop_params / pop_grad).
 *   One lane per entry, no sums, no atomics: the same call gives the same bits.
 *   HODE_EINVAL, nothing launched: A, B or n_lat < 1, n_lat > 6, popcount(lat_mask) != n_lat, K != popcount(ode_mask), K > 17,
 *   link not 0 or 1, off < 0, off < K with ode_p / gode, ld < off + B n_lat, a NULL among the required pointers (coords, m, s,
 *   x0_base, x0_out / gx0, glik; with ode_p: ode_base and, for K > 0, mu, sd; with gode and K > 0: sd). */
int hode_x0_params_f32(void *stream, int A, int B, int n_lat, int ld, int off, const float *coords, uint32_t lat_mask, int link,
                       const double *m, const double *s, const float *x0_base, float *x0_out, int K, uint32_t ode_mask,
                       const double *mu, const double *sd, const float *ode_base, float *ode_p);
int hode_x0_params_f64(void *stream, int A, int B, int n_lat, int ld, int off, const double *coords, uint32_t lat_mask, int link,
                       const double *m, const double *s, const double *x0_base, double *x0_out, int K, uint32_t ode_mask,
                       const double *mu, const double *sd, const double *ode_base, double *ode_p);
int hode_x0_grad_f32(void *stream, int A, int B, int n_lat, int ld, int off, const float *coords, uint32_t lat_mask, int link,
                     const double *m, const double *s, const float *gx0, int K, uint32_t ode_mask, const double *sd,
                     const float *gode, float *glik);
int hode_x0_grad_f64(void *stream, int A, int B, int n_lat, int ld, int off, const double *coords, uint32_t lat_mask, int link,
                     const double *m, const double *s, const double *gx0, int K, uint32_t ode_mask, const double *sd,
                     const double *gode, double *glik);

/* =====================================================================================================
 * Sobol indices (inference/sobol.py, sobol_indices / sobol_study): the analysis half of the sensitivity study of the
 * reference's plots/plot_all.py:139-224, i.e. what SALib.analyze.sobol.analyze computes from the model outputs of a
 * Saltelli design, for M output columns at once.
 *
 * Input.  Y holds N * nb rows, nb = 2 D + 2 with second_order and D + 2 without; row i * nb + b is block b of base sample i,
 * the blocks in SALib's order A, AB_1..AB_D, [BA_1..BA_D,] B.  Element (row, m) is Y[row * ldy + m], ldy >= M: trajectories
 * y[S][T][6] go in as they are with M = ldy = 6 T.  DEVICE memory, any alignment, any ldy.
 *
 * Estimators, per column m.  z = (Y - mean) / std with mean and std (ddof 0) over all N * nb rows of the column;
 * V = the ddof-0 variance of the 2 N values A u B;
 *   S1_j  = mean_i(B_i (AB_ij - A_i)) / V
 *   ST_j  = mean_i((A_i - AB_ij)^2) / (2 V)
 *   S2_jk = mean_i(BA_ij AB_ik - A_i B_i) / V - S1_j - S1_k    for j < k; every other entry of S2 is NaN.
 * Confidence: resample r < R draws indices rho_r(q), q < N, and applies the same formulas to A[rho], AB[rho], BA[rho], B[rho]
 * (V again from the resampled A u B); *_conf = conf_z * the ddof-1 standard deviation of the R resampled estimates, NaN for
 * R < 2.  rho_r(q) = (word * N) >> 32 with word = element q & 3 of the Philox4x32-10 block of counter (q >> 2, 7, r,
 * seed bits 32..63) and key (seed bits 0..31, 0): stream tag 7 of the samplers' generator.  All columns share rho; it depends
 * on (seed, r, q, N) only.
 *
 * Outputs (DEVICE, fp64): S1, ST [M][D]; S2 [M][D][D] (read only with second_order); S1_conf, ST_conf, S2_conf the same shapes
 * (all may be NULL when R == 0); variance [M] = the ddof-0 variance of the raw column over all rows (may be NULL).
 * A column whose raw values are all equal, or that holds a non-finite value, gets NaN in every index and conf and variance 0
 * or NaN; its neighbours are not disturbed.
 *
 * Arithmetic: inputs converted to fp64 on load, every sum fp64 in a fixed order, no floating-point atomics.  One workgroup
 * per column; the column is staged in LDS when it fits and gathered from global memory when not, with the same bits either
 * way.  The same call gives the same bits, and a call on M columns gives the bits of M one-column calls.
 *
 * HODE_EINVAL: N, D or M < 1, ldy < M, R < 0, a NULL among Y, S1, ST, S2 NULL with second_order, a NULL conf with R > 0 whose
 * index array is given.  HODE_EUNSUPPORTED: D > HODE_SOBOL_MAX_D.
 * ===================================================================================================== */
#define HODE_SOBOL_MAX_D 32
int hode_sobol_indices_f32(void *stream, int N, int D, int M, const float *Y, int64_t ldy, int second_order, int R, uint64_t seed,
                           double conf_z, double *S1, double *ST, double *S2, double *S1_conf, double *ST_conf, double *S2_conf,
                           double *variance);
int hode_sobol_indices_f64(void *stream, int N, int D, int M, const double *Y, int64_t ldy, int second_order, int R, uint64_t seed,
                           double conf_z, double *S1, double *ST, double *S2, double *S1_conf, double *ST_conf, double *S2_conf,
                           double *variance);

/* =====================================================================================================
 * Posterior-predictive summaries (inference/predictive.py, eval/evaluate.py): what the reference's eval/evaluate.py
 * computes from a stack of predictive draws -- mean(0), std(0), RMSE / MAE, the calibration scores -- without the stack.
 *
 * An ENTRY is one element i < N of a [n_traj][T][6] block, N = n_traj * T * 6; its state is i % 6.  Entry i is OBSERVED as
 * in hode_obs_nll_sets_*: obs[i] finite and, with a mask (uint8[N], NULL = finiteness only), mask[i] != 0; no arithmetic
 * touches the obs value of an unobserved entry.
 *
 * The running state of the entries, DEVICE memory the caller owns, N elements each:
 *   n      int32   draws folded so far
 *   mean   double  running mean
 *   m2     double  running sum of squared deviations from the mean
 *   pit    double  sum over the folded draws of the predictive CDF at the observation
 *   lmax   double  running maximum of the streaming log-sum-exp of log N(obs | y, sigma_k^2)
 *   lsum   double  running sum of the same: sum_s exp(lp_s - lmax)
 * A fresh state is all zero except lmax = -infinity.
 *
 * hode_pred_fold_* folds n_draws more draws y[n_draws][N] into the state, ONE AT A TIME IN DRAW ORDER, per entry:
 *   skip the draw when status[s][i / row_len] != 0 (status: int32[n_draws][N / row_len], NULL = all fine; rows of y after a
 *   failed solve are zero and must not be averaged in) or when y is not finite; else
 *     n += 1;  d = y - mean;  mean += d / n;  m2 += d * (y - mean)                                     (Welford)
 *   and, for an observed entry,
 *     with sigma (double[n_draws][6], DEVICE; NULL = no observation noise) and sigma[s][k] > 0:
 *       z = (obs - y) / sigma;  pit += Phi(z);  lp = -z^2 / 2 - log sigma - log(2 pi) / 2;
 *       lp > lmax ?  (lsum = lsum * exp(lmax - lp) + 1, lmax = lp)  :  lsum += exp(lp - lmax)
 *     else  pit += 1 if y < obs, 1/2 if y == obs, 0 otherwise;  lmax, lsum stay.
 *   obs NULL: nothing is observed, and pit, lmax, lsum are not written at all.
 * Each update is computed in fp64 without contraction and does not depend on where a call begins or ends, and the state is
 * fp64 in memory as in registers: folding S draws in one call and folding the same draws in ANY split into consecutive calls
 * give bit-identical state.  A lane owns one entry (no reduction, no atomics): the same call gives the same bits.
 * Unaligned pointers and any N are fine (a wave reads 64 consecutive reals of a draw).
 * HODE_EINVAL: n_draws < 0, N < 6 or N % 6 != 0, a NULL state pointer, y NULL with n_draws > 0, a mask without obs, with
 * status a row_len that is no multiple of 6 or does not divide N.  n_draws == 0 is a no-op.
 *
 * hode_pred_score_* reads a finished state and writes, in the working precision,
 *   out_mean = mean (NaN where n == 0),  out_sd = sqrt(m2 / (n - 1) + extra_var[k]) (NaN where n < 2),
 *   out_pit = pit / n (NaN where n < 2 or the entry is unobserved)
 * -- extra_var: HOST double[6] (NULL = 0), the mean over the draws of sigma_k^2 (law of total variance) -- and
 * table: double[6][K], K = HODE_PRED_FIXED_COLS + 2 * n_bins, per-state sums over the OBSERVED entries, with e = mean - obs,
 * u = |e| / (sd + 1e-6), everything from the fp64 state:
 *   over n >= 1:   0 count   1 sum e^2   2 sum |e|   3 sum obs   4 sum obs^2
 *   over n >= 2:   5 count   6 sum sd   7 sum u
 *                  8 sum of the 95 % interval score: (hi - lo) + (2 / 0.05) ((lo - obs)+ + (obs - hi)+), lo, hi = mean -+ 1.96 sd
 *                  9..12 counts of lo <= obs <= hi at 50 / 80 / 90 / 95 % (z = 0.6744897501960817, 1.2815515655446004,
 *                        1.6448536269514722, 1.96; inclusive bounds)
 *                  13 sum of the Gaussian CRPS  sd (w (2 Phi(w) - 1) + 2 phi(w) - 1 / sqrt(pi)), w = (obs - mean) / sd (|e| at sd = 0)
 *                  14 sum of the log pointwise predictive density lmax + log(lsum / n) over the entries with lsum > 0,  15 their count
 *                  16 .. 16 + n_bins - 1            counts of u <= thr[j]   (thr: HOST double[n_bins])
 *                  16 + n_bins .. 16 + 2 n_bins - 1 PIT histogram: counts of min(floor(n_bins pit / n), n_bins - 1) == j
 * Reduction in a fixed order: lane sums, block sums (a butterfly inside each wave, then the four wave sums in order), one
 * partial row per workgroup in work (DEVICE double[HODE_PRED_SCORE_BLOCKS * 6 * K], scratch space), then one pass that adds
 * the rows in index order; the two histograms are integer counts.  The same call gives the same bits.  Unaligned pointers
 * and any N are fine (16-byte accesses, twelve entries per lane, when N % 4 == 0 and every pointer allows them).
 * HODE_EINVAL: N < 6 or N % 6 != 0, n_bins outside 1..HODE_PRED_MAX_BINS, a NULL among the state, thr, the outputs, table
 * and work, a mask without obs.  obs NULL: nothing is observed (an all-zero table).
 * ===================================================================================================== */
#define HODE_PRED_MAX_BINS 32
#define HODE_PRED_FIXED_COLS 16
#define HODE_PRED_SCORE_BLOCKS 128
int hode_pred_fold_f32(void *stream, int n_draws, int64_t N, const float *y, const float *obs, const uint8_t *mask, const double *sigma,
                       const int32_t *status, int64_t row_len, int32_t *n, double *mean, double *m2, double *pit, double *lmax,
                       double *lsum);
int hode_pred_fold_f64(void *stream, int n_draws, int64_t N, const double *y, const double *obs, const uint8_t *mask, const double *sigma,
                       const int32_t *status, int64_t row_len, int32_t *n, double *mean, double *m2, double *pit, double *lmax,
                       double *lsum);
int hode_pred_score_f32(void *stream, int64_t N, const int32_t *n, const double *mean, const double *m2, const double *pit,
                        const double *lmax, const double *lsum, const float *obs, const uint8_t *mask, const double *extra_var,
                        const double *thr, int n_bins, float *out_mean, float *out_sd, float *out_pit, double *table, double *work);
int hode_pred_score_f64(void *stream, int64_t N, const int32_t *n, const double *mean, const double *m2, const double *pit,
                        const double *lmax, const double *lsum, const double *obs, const uint8_t *mask, const double *extra_var,
                        const double *thr, int n_bins, double *out_mean, double *out_sd, double *out_pit, double *table, double *work);

/* =====================================================================================================
 * Posterior bands: exact tail quantiles across the draws (inference/predictive.py `quantiles=`, HMCResult.summary): what the
 * reference's np.percentile(draws, 2.5 / 97.5, axis=0) and posterior_summary compute from the stack of draws, without the
 * stack.  The quantile q of n values is interpolated between order statistics floor(q (n - 1)) and the next one, so only the
 * K = floor(min(q, 1 - q) (n - 1)) + 2 smallest (q <= 1/2) or largest values of an entry matter.
 *
 * The tail state of N entries (ANY N >= 1: an entry is one element of y, no state index is used), DEVICE memory the caller
 * owns, R the working precision:
 *   cnt   int32[N]   draws taken so far
 *   lo    R[K][N]    the min(cnt, K) smallest values taken, slot j of entry i at j * N + i
 *   hi    R[K][N]    the min(cnt, K) largest values taken, the same layout
 * A fresh state is cnt = 0; lo and hi need no initialisation.  The order of the values inside a buffer is the library's
 * business (lo is a binary max-heap, hi a min-heap: slot 0 is the largest of lo and the smallest of hi).
 *
 * hode_pred_tails_* takes n_draws more draws y[n_draws][N], ONE AT A TIME IN DRAW ORDER, per entry, with the skip rules of
 * hode_pred_fold_*: the draw is skipped when status[s][i / row_len] != 0 (status: int32[n_draws][N / row_len], NULL = all
 * fine) or when y is not finite; else, while cnt < K, y enters both buffers, and after that it replaces the largest of lo
 * when y < it and the smallest of hi when it < y; cnt += 1.  Values are copied and compared with <, never computed with.
 * A draw is a pure update of the state in memory: any split of the draws into consecutive calls leaves bit-identical state,
 * and any permutation of the draws leaves the same multiset in each buffer (+0.0 and -0.0 compare equal: which of the two
 * is kept may depend on the order).  A lane owns one entry (no reduction, no atomics); a value that enters a buffer costs
 * O(log K) loads and stores, any other its load and two compares.  K is a run-time argument without a cap.
 * HODE_EINVAL: n_draws < 0, N < 1, K < 1, a NULL state pointer, y NULL with n_draws > 0, with status a row_len < 1 or one
 * that does not divide N.  n_draws == 0 is a no-op without a launch.
 *
 * hode_pred_quantiles_* reads a tail state and writes out[n_levels][N] (R) for levels (HOST double[n_levels], strictly
 * inside (0, 1), ascending, n_levels in 1..HODE_PRED_MAX_LEVELS): numpy's default "linear" quantile.  With n = cnt[i]:
 *   h = q (double)(n - 1);  j = floor(h);  g = h - j;  out = a + (b - a) g
 * a, b the order statistics j and min(j + 1, n - 1) (ascending, from 0), read from lo when q <= 1/2 and from hi otherwise, in
 * fp64 without contraction, rounded once to R.  out is NaN where n == 0 and where a needed order statistic is not in the
 * buffer: with n > K, j + 1 >= K for q <= 1/2 and n - 1 - j >= K for q > 1/2.
 * The call SORTS lo and hi in place (lo largest first, hi smallest first).  A sorted buffer is still a valid heap, so
 * hode_pred_tails_* may go on folding into the state afterwards; that is why lo and hi are not const here.
 * band_table: DEVICE double[6][HODE_PRED_BAND_COLS] or NULL.  It needs N % 6 == 0 (the state of entry i is i % 6), obs, work
 * (DEVICE double[HODE_PRED_SCORE_BLOCKS * 6 * HODE_PRED_BAND_COLS], scratch space) and levels[0] < 1/2 < levels[n_levels - 1].
 * With lo = out[0][i], hi = out[n_levels - 1][i] as written (R) and alpha = 1 - (levels[n_levels - 1] - levels[0]), per
 * state over the OBSERVED entries (obs, mask as above) with n >= 2 and both bounds finite:
 *   0 count   1 sum (hi - lo)   2 count of lo <= obs <= hi (inclusive)
 *   3 sum of the interval score (hi - lo) + (2 / alpha) ((lo - obs)+ + (obs - hi)+)
 * reduced in the fixed order of hode_pred_score_*: the same call gives the same bits.
 * HODE_EINVAL: N < 1, K < 1, a NULL among cnt, lo, hi, levels and out, n_levels outside its range, a level outside (0, 1)
 * or not above its predecessor, a mask without obs, a band_table without what it needs.
 * ===================================================================================================== */
#define HODE_PRED_MAX_LEVELS 16
#define HODE_PRED_BAND_COLS 4
int hode_pred_tails_f32(void *stream, int n_draws, int64_t N, const float *y, const int32_t *status, int64_t row_len, int K, int32_t *cnt,
                        float *lo, float *hi);
int hode_pred_tails_f64(void *stream, int n_draws, int64_t N, const double *y, const int32_t *status, int64_t row_len, int K, int32_t *cnt,
                        double *lo, double *hi);
int hode_pred_quantiles_f32(void *stream, int64_t N, int K, const int32_t *cnt, float *lo, float *hi, int n_levels, const double *levels,
                            float *out, const float *obs, const uint8_t *mask, double *band_table, double *work);
int hode_pred_quantiles_f64(void *stream, int64_t N, int K, const int32_t *cnt, double *lo, double *hi, int n_levels, const double *levels,
                            double *out, const double *obs, const uint8_t *mask, double *band_table, double *work);

/* =====================================================================================================
 * Model comparison: PSIS-LOO and WAIC folded across the draws (inference/predictive.py `loo=`, inference.compare): what
 * arviz.loo / arviz.waic / arviz.compare compute from the [draws][N] block of pointwise log likelihoods, without the block
 * (Vehtari, Gelman & Gabry 2017; Vehtari, Simpson, Gelman, Yao & Gabry 2024; Zhang & Stephens 2009).
 *
 * For an OBSERVED entry i (obs, mask as above; N % 6 == 0, the state of entry i is i % 6) and a draw s that pred_fold would
 * take (status zero, y finite) with sigma[s][k] > 0, the pointwise log likelihood is pred_fold's lp,
 *   z = (obs - y) / sigma;  l = -z^2 / 2 - log sigma - log(2 pi) / 2,
 * and r = -l is the log importance ratio of leaving the observation out.  Pareto smoothing needs the M + 1 largest r of an
 * entry and sums over the rest, M = ceil(min(n / 5, 3 sqrt(n / r_eff))).
 *
 * The LOO state of the entries, DEVICE memory the caller owns:
 *   cnt          int32[N]      draws that produced an l
 *   lmean, lm2   double[N]     Welford's mean and sum of squared deviations of l (WAIC)
 *   pmax, psum   double[N]     streaming log-sum-exp of l: sum_s exp(l_s) = exp(pmax) psum (lppd; it does not read pred_fold's)
 *   top          double[K][N]  the min(cnt, K) largest r, slot j of entry i at j * N + i (a binary min-heap: slot 0 is the least)
 *   rmax, rsum   double[N]     streaming log-sum-exp of every r that is not in top
 * A fresh state is all zero except pmax = rmax = -infinity; top needs no initialisation.
 *
 * hode_pred_loo_fold_* takes n_draws more draws y[n_draws][N], ONE AT A TIME IN DRAW ORDER, per entry:
 *   d = l - lmean;  lmean += d / (cnt + 1);  lm2 += d * (l - lmean);
 *   l > pmax ?  (psum = psum * exp(pmax - l) + 1, pmax = l)  :  psum += exp(l - pmax);
 *   while cnt < K, r enters top; afterwards, when the least of top is < r, r replaces it and the replaced value is added to
 *   {rmax, rsum} as l was to {pmax, psum}; otherwise r itself is added;  cnt += 1.
 * Every r is therefore in exactly one of top and {rmax, rsum}: no subtraction forms the sum of the non-tail ratios.  All of
 * it is fp64 without contraction and a draw is a pure update of the state in memory: any split of the draws into consecutive
 * calls leaves bit-identical state; a permutation of the draws leaves the same multiset in top and the four running sums equal
 * to rounding.  A lane owns one entry (no reduction, no atomics).  K is a run-time argument without a cap.
 * HODE_EINVAL: n_draws < 0, N < 6 or N % 6 != 0, K < 2, a NULL state pointer, obs or sigma NULL (without observation noise
 * there is no likelihood; hence a mask without obs is refused too), y NULL with n_draws > 0, with status a row_len that is no
 * multiple of 6 or does not divide N.  n_draws == 0 is a no-op without a launch.
 *
 * hode_pred_loo_finish_* reads a state and writes, per entry in the working precision R, elpd_loo, pareto_k, elpd_waic, p_waic
 * and lppd.  With n = cnt[i], h = min(n, K) and r_eff (a HOST scalar in (0, 1], the relative efficiency of the draws; 1 for
 * independent draws), all five are NaN when n < 2 or M + 1 > h (the state was sized for fewer draws; unobserved entries
 * have n = 0).  Otherwise:
 *   shift     c = the largest r;  x = r - c;  x_cut = max(x of the (M + 1)-th largest, log(DBL_MIN));  e_cut = exp(x_cut)
 *   tail      the held values with x > x_cut (strictly: ties with the cut are not tail), t of them, ascending, j = 1..t
 *   fit       t <= 4: k = +infinity, nothing is smoothed.  Else on a_j = exp(x_j) - e_cut:
 *               m = 30 + floor(sqrt(t));  b_q = (1 - sqrt(m / (q - 1/2))) / (3 a_[floor(t / 4 + 1/2)]) + 1 / a_t,  q = 1..m
 *               k_q = mean_j log1p(-b_q a_j);  L_q = t (log(-b_q / k_q) - k_q - 1);  w_q = 1 / sum_p exp(L_p - L_q)
 *               b = sum w_q b_q / sum w_q over the q with w_q >= 10 * 2^-52
 *               k = mean_j log1p(-b a_j);  sigma = -k / b;  k <- (t k + 5) / (t + 10)
 *   smooth    when k is finite and sigma > 0, the j-th smallest tail value becomes
 *               x~_j = min(log(a~_j + e_cut), 0),  a~_j = sigma expm1(-k log1p(-p_j)) / k  (-sigma log1p(-p_j) when |k| < 2^-52),
 *               p_j = (j - 1/2) / t;  otherwise x~_j = x_j
 *   estimate  elpd_loo = LSE({log(n - t) - c} u {x~_j - r_j}) - LSE({rmax + log rsum - c} u {x of the held non-tail values} u {x~_j})
 *             (in log space: (n - t) exp(-c) underflows for heavy tails);  pareto_k = k
 *   lppd = pmax + log(psum / n);  p_waic = lm2 / (n - 1);  elpd_waic = lppd - p_waic
 * The call SORTS top in place (ascending; a sorted buffer is still a valid heap, so folding may go on afterwards: that is
 * why top is not const here).
 * fit: DEVICE double[rows][N], scratch space, rows = (K - 1) + 30 + floor(sqrt(K - 1)): the a_j / x~_j and the L_q of every
 * entry, slot-major like top.
 * table: DEVICE double[6][HODE_PRED_LOO_COLS], per-state sums over the scored entries (those whose outputs are not NaN by the
 * rule above), from the fp64 values before they are rounded to R, with p_loo = lppd - elpd_loo:
 *   0 count   1 sum elpd_loo   2 sum elpd_loo^2   3 sum p_loo   4 sum elpd_waic   5 sum elpd_waic^2   6 sum p_waic   7 sum lppd
 *   8..11 counts of k <= 0.5, 0.5 < k <= 0.7, 0.7 < k <= 1, k > 1 (+infinity included)   12 count of p_waic > 0.4
 * reduced in the fixed order of hode_pred_score_* (work: DEVICE double[HODE_PRED_SCORE_BLOCKS * 6 * HODE_PRED_LOO_COLS],
 * scratch space): the same call gives the same bits.
 * HODE_EINVAL: N < 6 or N % 6 != 0, K < 2, r_eff outside (0, 1] or NaN, a NULL among the state, the outputs, table, fit
 * and work.
 * ===================================================================================================== */
#define HODE_PRED_LOO_COLS 13
int hode_pred_loo_fold_f32(void *stream, int n_draws, int64_t N, const float *y, const float *obs, const uint8_t *mask, const double *sigma,
                           const int32_t *status, int64_t row_len, int K, int32_t *cnt, double *lmean, double *lm2, double *pmax,
                           double *psum, double *top, double *rmax, double *rsum);
int hode_pred_loo_fold_f64(void *stream, int n_draws, int64_t N, const double *y, const double *obs, const uint8_t *mask, const double *sigma,
                           const int32_t *status, int64_t row_len, int K, int32_t *cnt, double *lmean, double *lm2, double *pmax,
                           double *psum, double *top, double *rmax, double *rsum);
int hode_pred_loo_finish_f32(void *stream, int64_t N, int K, double r_eff, const int32_t *cnt, const double *lmean, const double *lm2,
                             const double *pmax, const double *psum, double *top, const double *rmax, const double *rsum, float *elpd_loo,
                             float *pareto_k, float *elpd_waic, float *p_waic, float *lppd, double *table, double *fit, double *work);
int hode_pred_loo_finish_f64(void *stream, int64_t N, int K, double r_eff, const int32_t *cnt, const double *lmean, const double *lm2,
                             const double *pmax, const double *psum, double *top, const double *rmax, const double *rsum, double *elpd_loo,
                             double *pareto_k, double *elpd_waic, double *p_waic, double *lppd, double *table, double *fit, double *work);

/* =====================================================================================================
 * Particle filter (inference/filter.py, run_filter): one step of a bootstrap particle filter per patient -- process noise,
 * the weight update under the observation model, normalisation, effective sample size (ESS), systematic resampling and the
 * gather -- i.e. everything between two forward solves of the B * N particle trajectories.
 *
 * Layout.  Patient-major: particle i of patient b is row b * N + i, 1 <= N <= HODE_PF_MAX_PARTICLES.  One workgroup of 256
 * lanes per patient; the patient's N cumulative weights (fp64) live in LDS, 32 KB at the maximum.
 *
 * Arguments (DEVICE unless noted): B, N, step, seed, id0, link, ess_frac, n_aux on the host; patient b draws from the Philox
 * key id0 + b (the samplers' generator: key = (seed bits 0..31, id0 + b), counter = (group, tag, step, seed bits 32..63));
 * x_in [B*N][6] the solve's output row at this time; status [B*N] int32 or NULL; obs [B][6]; mask [B][6] uint8 or NULL;
 * sigma [6], q [6], dt [B] fp64; lw [B*N] fp64 IN/OUT, the unnormalised log-weights; x_out [B*N][6]; anc [B*N] int32;
 * stats [B][HODE_PF_COLS] fp64; aux_in / aux_out [B*N][n_aux], 0 <= n_aux <= HODE_PF_MAX_AUX, a payload that is gathered
 * with the particle (run_filter carries each particle's 17 mechanistic constants in it; both NULL with n_aux == 0).
 *
 * Everything below is computed in fp64 and rounded once on store.
 *  a. Noise.  For state j with s = q_j sqrt(dt_b) > 0: xi = element j & 3 of the four normals (Box-Muller, as the samplers')
 *     of the block (group 2 i + (j >> 2), tag 8, step); link HODE_PF_LINK_ADD: x += s xi; HODE_PF_LINK_LOG:
 *     x *= exp(s xi - s^2 / 2).  With s == 0 the state is copied exactly.
 *  b. Weight.  lw_i += sum_j seen_j [-((obs_j - x_ij) / sigma_j)^2 / 2 - log sigma_j - log(2 pi) / 2]; seen_j: obs_j finite and,
 *     with a mask, the mask byte set (no arithmetic touches an unseen obs_j).  A particle with status != 0, a non-finite state,
 *     or lw = -inf (or NaN) on entry gets lw = -inf: it is dead and stays dead.
 *  c. Normalise.  m = max lw, w_i = exp(lw_i - m), c_k = sum_{i <= k} w_i.  stats: [0] the log-evidence increment
 *     m + log c_{N-1} - (m_in + log c_in), the _in values being the same quantities of the log-weights on entry;
 *     [1] ESS = (sum w)^2 / sum w^2; [3] particles alive; [4..9] the weighted mean of each state; [10..15] the weighted variance
 *     of each state about that mean.  No particle alive: increment -inf, ESS 0, mean and variance NaN, x_out = x after (a),
 *     anc = identity, lw stays -inf.
 *  d. Resample iff ESS < ess_frac * N; stats[2] = 1 then, else 0.  Systematic: one u in (0, 1) per patient and step (word x of
 *     the block (group 0, tag 9, step)), anc_i = min{k : c_k >= (i + u) / N * c_{N-1}}, never a dead particle; then lw = 0 in
 *     every slot.  Otherwise anc = identity and lw is kept.
 *  e. Gather.  x_out[i] = x[anc_i] after (a), aux_out[i] = aux_in[anc_i].  x_out may not alias x_in, aux_out not aux_in.
 *
 * Reductions run in a fixed order and there are no floating-point atomics: the same call gives the same bits, and a patient's
 * result depends on its key id0 + b only, not on B or on its row.  c_k comes from a parallel scan: against a sequential sum,
 * anc can differ only where a pointer falls within the summation error of a boundary c_k.
 *
 * HODE_EINVAL (nothing launched): B < 1, N < 1, n_aux outside 0..HODE_PF_MAX_AUX, link not 0 or 1, ess_frac outside [0, 1] or
 * NaN, a NULL among x_in, obs, sigma, q, dt, lw, x_out, anc, stats (and, with n_aux > 0, aux_in, aux_out), x_out == x_in,
 * aux_out == aux_in.  HODE_EUNSUPPORTED: N > HODE_PF_MAX_PARTICLES (a bad argument outranks it).
 * ===================================================================================================== */
#define HODE_PF_MAX_PARTICLES 4096
#define HODE_PF_MAX_AUX 17
#define HODE_PF_COLS 16
#define HODE_PF_LINK_ADD 0
#define HODE_PF_LINK_LOG 1
int hode_pf_step_f32(void *stream, int B, int N, uint32_t step, uint64_t seed, uint32_t id0, const float *x_in, const int32_t *status,
                     const float *obs, const uint8_t *mask, const double *sigma, const double *q, const double *dt, int link,
                     double ess_frac, double *lw, float *x_out, int32_t *anc, double *stats, int n_aux, const float *aux_in,
                     float *aux_out);
int hode_pf_step_f64(void *stream, int B, int N, uint32_t step, uint64_t seed, uint32_t id0, const double *x_in, const int32_t *status,
                     const double *obs, const uint8_t *mask, const double *sigma, const double *q, const double *dt, int link,
                     double ess_frac, double *lw, double *x_out, int32_t *anc, double *stats, int n_aux, const double *aux_in,
                     double *aux_out);

/* =====================================================================================================
 * Particle smoother (inference/filter.py, FilterResult.smooth): backward-simulation smoothing (forward filtering, backward
 * simulation) over a stored particle filter -- M trajectories per patient, each drawn from the joint smoothing distribution
 * that the filter's particles carry, in one launch for the whole backward pass.
 *
 * Arguments (DEVICE unless noted): B, N, M, S, seed, id0, link on the host.  hist [S][B][N][6]: the particles after each of the
 * S filter steps (run_filter's history); lwh [S][B][N] fp64: their log-weights as hode_pf_step left them (unnormalised, 0 after
 * a resampling, -inf for a dead particle); pred [S][B][N][6]: pred[s][b][i] is the x_in row of step s, i.e. the state that slot
 * i of step s - 1 was carried to by the segment solve, before the noise (pred[0] is not read; a failed solve's row is NaN);
 * q [6] fp64 the process noise; dt [S][B] fp64 the dt of every step (dt[0] is not read); link as in hode_pf_step.
 * Outputs: idx [S][B][M] int32, paths [S][B][M][6].
 *
 * Patient b draws from the Philox key id0 + b.  For trajectory m = 0..M-1, all in fp64 on the stored values, a * b + c being two
 * roundings:
 *  Last step.   l_i = lwh[S-1][i]; k_{S-1} is drawn as below with step number S - 1.
 *  Steps s = S-2 .. 0.  With x~ = hist[s+1][k_{s+1}], sg_j = q_j * sqrt(dt[s+1][b]), r_j = 1 / sg_j and p = pred[s+1][i]:
 *     l_i = lwh[s][i] + T,  T = the sum over j = 0..5 (from 0, in order) of tau_j,
 *       sg_j > 0:       tau_j = -0.5 * (z * z);  additive link z = (x~_j - p_j) * r_j;
 *                       log link z = (log x~_j - (log p_j - 0.5 * (sg_j * sg_j))) * r_j
 *                       (which is (log x~_j - log p_j + sg_j^2 / 2) / sg_j; the candidate's bracket is formed once);
 *       otherwise:      the transition is a point mass: tau_j = 0 if p_j == x~_j exactly (as stored values), else -inf.
 *     A non-finite l_i counts as -inf: a NaN pred row, a dead particle, the logarithm of a non-positive number.  Terms that
 *     are the same for every i are dropped.
 *  Draw.  mx = max_i l_i, w_i = exp(l_i - mx) (0 for -inf), c_k = the SEQUENTIAL running sum of w over i = 0..k,
 *     u = u01(word x of the block (group m, tag 10, step s)), k_s = min{k : c_k >= u * c_{N-1}}, moved back to the nearest k
 *     with w_k > 0 (hode_pf_step's rule; on a sequential sum the minimum already has w_k > 0).  No candidate alive:
 *     idx = -1 and paths = NaN for this step and every earlier one of that trajectory.
 *  Outputs.  idx[s][b][m] = k_s, paths[s][b][m] = hist[s][b][k_s].
 *
 * The same call gives the same bits, and a trajectory's bits depend on (seed, id0 + b, m) and the patient's stored data only:
 * not on M, on B or on how the launch is cut.  The kernel computes both instantiations in fp64 (there is no fp32 pair loop).
 *
 * HODE_EINVAL (nothing launched): B, N, M or S < 1, link not 0 or 1, a NULL pointer.  HODE_EUNSUPPORTED:
 * N > HODE_PF_MAX_PARTICLES (a bad argument outranks it), or B * ceil(M / 256) >= 2^31; M itself is not bounded.
 * ===================================================================================================== */
int hode_pf_smooth_f32(void *stream, int B, int N, int M, int S, uint64_t seed, uint32_t id0, const float *hist, const double *lwh,
                       const float *pred, const double *q, const double *dt, int link, int32_t *idx, float *paths);
int hode_pf_smooth_f64(void *stream, int B, int N, int M, int S, uint64_t seed, uint32_t id0, const double *hist, const double *lwh,
                       const double *pred, const double *q, const double *dt, int link, int32_t *idx, double *paths);

/* =====================================================================================================
 * Particle filter: parameter move (inference/filter.py, run_filter(learn=...)): Liu & West's kernel shrinkage and / or a random
 * walk on chosen columns of the payload rows, so that a filter whose particles carry their own constants learns them online
 * instead of collapsing onto the rows it started with.  Launched after hode_pf_step_*: it reads the log-weights the step left
 * and moves, in place, the aux rows the step gathered.
 *
 * Arguments (DEVICE unless noted): B, N, step, seed, id0, n_aux, shrink on the host.  lw [B*N] fp64, read only; aux [B*N][n_aux],
 * 1 <= n_aux <= HODE_PF_MAX_AUX, IN/OUT; mode [n_aux] int32: HODE_PF_MOVE_CARRIED (0) the column is carried, HODE_PF_MOVE_IDENTITY
 * (1) it is selected with phi = theta, HODE_PF_MOVE_LOG (2) selected with phi = log theta (any other value: carried); walk [n_aux]
 * fp64, a standard deviation per sqrt(time) in link space (only its square is used); dt [B] fp64; shrink = a in [0, 1];
 * pstats [B][2 * n_aux] fp64.  Layout and launch as hode_pf_step_*: one workgroup of 256 lanes per patient, the patient's N
 * weights (fp64) in LDS.
 *
 * For patient b, everything in fp64, a * b + c being two roundings, every sum over the particles in the order of the step
 * kernel's sums (lane t adds its particles t, t + 256, ... in order from 0.0; a butterfly inside each wave of 64; then
 * (wave 0 + wave 1) + (wave 2 + wave 3)):
 *  Counting.  Particle i counts iff lw_i > -inf (false for NaN) and, for every selected column k, (double) aux[i][k] is finite
 *     and, under the log link, > 0 -- judged on the rows as they came in.  m = the maximum of lw over the particles that count;
 *     w_i = exp(lw_i - m), sw = sum w.  No particle counts (or m = +inf, of which no weights can be formed): pstats[b] is NaN
 *     in all 2 * n_aux entries and nothing is moved.
 *  Moments, per selected column k.  phi_i = (double) aux[i][k] or its log; mean = (sum w_i * phi_i) / sw;
 *     var = (sum w_i * (d_i * d_i)) / sw with d_i = phi_i - mean.  pstats[b][2k] = mean, pstats[b][2k + 1] = var: the cloud
 *     before the move.  A carried column has NaN in both.
 *  Move, per selected column k unless a == 1 and walk_k == 0 (then the column keeps its bits):
 *     sd = sqrt((1 - a * a) * var + (walk_k * walk_k) * dt_b);
 *     eps = element k & 3 of the four normals (Box-Muller, as the samplers') of the block (group 5 i + (k >> 2), tag 11, step);
 *     phi' = (mean + a * (phi_i - mean)) + sd * eps;  aux[i][k] = (R) phi' or (R) exp(phi'), rounded once.
 *     Rows that do not count and carried columns keep their bits.
 * With a = (3 delta - 1) / (2 delta) and walk = 0 this is Liu & West's (2001) shrinkage for the discount delta: it keeps the
 * weighted mean and variance of the cloud in expectation.  a = 1 with walk > 0 is a random walk.
 *
 * A draw is keyed by what is drawn -- (seed, id0 + b, step, particle, column) -- and depends neither on which other columns
 * are selected nor on B or the launch.  The same call gives the same bits, and a patient's bits depend on its key id0 + b only.
 *
 * HODE_EINVAL (nothing launched): B < 1, N < 1, n_aux outside 1..HODE_PF_MAX_AUX, shrink outside [0, 1] or NaN, a NULL among
 * lw, aux, mode, walk, dt, pstats.  HODE_EUNSUPPORTED: N > HODE_PF_MAX_PARTICLES (a bad argument outranks it).  mode and walk
 * live on the device and are not validated here: the caller does.
 * ===================================================================================================== */
#define HODE_PF_MOVE_CARRIED 0
#define HODE_PF_MOVE_IDENTITY 1
#define HODE_PF_MOVE_LOG 2
int hode_pf_params_f32(void *stream, int B, int N, uint32_t step, uint64_t seed, uint32_t id0, const double *lw, int n_aux, float *aux,
                       const int32_t *mode, const double *walk, const double *dt, double shrink, double *pstats);
int hode_pf_params_f64(void *stream, int B, int N, uint32_t step, uint64_t seed, uint32_t id0, const double *lw, int n_aux, double *aux,
                       const int32_t *mode, const double *walk, const double *dt, double shrink, double *pstats);

/* =====================================================================================================
 * Unscented Kalman filter (inference/ukf.py, run_ukf): one step of a sigma-point Kalman filter per patient -- the unscented
 * mean and covariance of the propagated points, the redraw, the measurement update under the observation model and the points
 * for the next solve -- i.e. everything between two forward solves of the B * K sigma-point trajectories.  Deterministic: there
 * is no seed.
 *
 * Sizes and layout.  P = the number of non-zero entries of mode [17] (0 <= P <= 17), n = 6 + P, K = 2 n + 1 (13 <= K <= 47).
 * Coordinates 0..5 are the states, 6..n-1 the learned columns of the ode_p row in ascending column order.  Patient-major:
 * sigma point k of patient b is row b * K + k.  One wave of 64 lanes per patient, four patients per workgroup of 256 lanes; a
 * patient's working set (fp64) lives in LDS, 2.8 KB at n = 6 and 21.3 KB at n = 23, sized by n at launch.
 *
 * Arguments (DEVICE unless noted): B, predict (0 / 1), link (HODE_PF_LINK_ADD / _LOG, for the states) on the host;
 * mode [17] int32 on the HOST, the hode_pf_params encoding (HODE_PF_MOVE_CARRIED 0, _IDENTITY 1, _LOG 2): the ABI validates it
 * and sizes the launch from it, and the kernel receives the columns by value -- there is no device copy that could disagree;
 * gamma, wm0, wc0, wi fp64 on the host: the spread and the weights of the unscented transform (centre point wm0 / wc0 for
 * the mean / the covariance, every other point wi for both); x_in [B*K][6] the solve's output rows; status [B*K] int32 or NULL;
 * aux_in [B*K][17] the ode_p row every sigma point was solved with; obs [B][6]; mask [B][6] uint8 or NULL; sigma [6], q [6],
 * walk [17] fp64 (observation noise, process noise of the states, random-walk sd of the learned constants per sqrt(time));
 * dt [B] fp64; alive [B] int32 IN/OUT (0 = the patient is lost); mean [B][n], cov [B][n][n] fp64, read only when predict == 0,
 * always written; x_out [B*K][6], aux_out [B*K][17] the sigma points and their ode_p rows for the next solve;
 * stats [B][HODE_UKF_COLS] fp64.
 *
 * Everything below is computed in fp64 and rounded once on store; a * b + c is two roundings; every sum over the points k runs
 * from 0.0 over k = 0, 1, .. in order with the weight multiplied first (acc += w_k * term).  g is the state link (log or
 * identity), phi_c the link of learned column c.
 *  a. Predict (predict == 1).  zeta_k = (g(x_in[k]), phi(aux_in[k][cols])); m- = sum wm_k zeta_k;
 *     P- = sum wc_k (zeta_k - m-)(zeta_k - m-)^T + diag(s^2), s_j^2 = (q_j q_j) dt_b for a state and (walk_c walk_c) dt_b for a
 *     learned column; then, under the log link, m-_j -= 0.5 s_j^2 for every state j (the drift that keeps the mean: exactly
 *     hode_pf_step's state model).  The patient is lost if a row has status != 0, or a state or a learned value that is not
 *     finite, or not positive under a log link.  With predict == 0, (m-, P-) are read from mean, cov; status, dt, q and walk are
 *     not read, x_in only to copy a lost patient's rows, and row b * K of aux_in supplies the carried columns.
 *  b. Redraw.  L = the lower Cholesky factor of P-, column by column without pivoting: pivot_j = P-_jj - sum_{k<j} L_jk^2,
 *     L_jj = sqrt(pivot_j), L_ij = (P-_ij - sum_{k<j} L_ik L_jk) / L_jj.  A pivot <= n 2^-52 |P-_jj| gives a zero column (so a
 *     coordinate with zero spread stays exact, and an all-zero covariance gives K equal points); a non-finite pivot loses the
 *     patient.  chi_0 = m-, chi_i = m- + gamma L[:, i-1], chi_{n+i} = m- - gamma L[:, i-1], i = 1..n.
 *  c. Update.  J = the seen states: obs_j finite and, with a mask, the mask byte set (no arithmetic touches an unseen obs_j);
 *     d = |J|.  Y_k = g^-1(chi_k) on J; yh = sum wm_k Y_k; S = sum wc_k (Y_k - yh)(Y_k - yh)^T + diag(sigma_J sigma_J);
 *     C = sum wc_k (chi_k - m-)(Y_k - yh)^T; r = obs_J - yh.  Through the Cholesky factor L_S of S (plain: a pivot that is not
 *     positive and finite loses the patient): z = L_S^-1 r, W = C L_S^-T (forward substitution, row by row), which makes the gain
 *     K_g = W L_S^-1; m = m- + W z (= m- + K_g r); P = P- - W W^T (= P- - K_g S K_g^T), symmetrised as 0.5 (P_ij + P_ji);
 *     NIS = z^T z (= r^T S^-1 r); log det S = 2 sum log L_S,aa; increment = -0.5 ((NIS + log det S) + d log 2 pi).
 *     With d == 0 the increment is exactly 0, NIS is 0 and m = m-, P = P- bit for bit.
 *  d. Emit.  New points from (m, P) as in (b); x_out[k] = g^-1(state part); aux_out[k] = row b * K of aux_in with the learned
 *     columns replaced by phi^-1(parameter part); mean = m, cov = P.  A non-finite pivot or a non-finite emitted value loses
 *     the patient.  x_out may not alias x_in, aux_out may not alias aux_in.
 *  e. stats: [0] the evidence increment, [1] NIS, [2] d, [3] alive after the step (1 / 0), [4..9] the unscented mean of the
 *     natural-space states of the emitted points, sum wm_k x_k, [10..15] their variance, sum wc_k (x_k - mean)^2 (both on the
 *     fp64 values, before the rounding of the store).
 *
 * A lost patient (alive == 0 on entry, or lost in a..d): alive = 0; stats[0] = -inf, [2] = d, [3] = 0, the rest NaN; mean and
 * cov NaN; x_out = x_in and aux_out = aux_in copied (hode_pf_step's rule for a dead patient).  It stays lost; the other
 * patients are untouched.
 *
 * There are no atomics and every sum runs in a fixed order: the same call gives the same bits, and a patient's bits depend
 * neither on B nor on its row.
 *
 * HODE_EINVAL (nothing launched): B < 1, predict not 0 or 1, link not 0 or 1, a mode value outside 0..2, gamma not finite or
 * not positive, a non-finite wm0, wc0 or wi, a NULL among mode, x_in, aux_in, obs, sigma, q, walk, dt, alive, mean, cov, x_out,
 * aux_out, stats, x_out == x_in, aux_out == aux_in.  HODE_EUNSUPPORTED: never (n <= 23 always holds).
 * ===================================================================================================== */
#define HODE_UKF_COLS 16
int hode_ukf_step_f32(void *stream, int B, int predict, int link, const int32_t *mode, double gamma, double wm0, double wc0, double wi,
                      const float *x_in, const int32_t *status, const float *aux_in, const float *obs, const uint8_t *mask,
                      const double *sigma, const double *q, const double *walk, const double *dt, int32_t *alive, double *mean,
                      double *cov, float *x_out, float *aux_out, double *stats);
int hode_ukf_step_f64(void *stream, int B, int predict, int link, const int32_t *mode, double gamma, double wm0, double wc0, double wi,
                      const double *x_in, const int32_t *status, const double *aux_in, const double *obs, const uint8_t *mask,
                      const double *sigma, const double *q, const double *walk, const double *dt, int32_t *alive, double *mean,
                      double *cov, double *x_out, double *aux_out, double *stats);

#ifdef __cplusplus
}
#endif
#endif /* HODE_H */

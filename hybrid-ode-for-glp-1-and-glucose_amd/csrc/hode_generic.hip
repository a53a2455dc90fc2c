// hode_generic.hip -- the GENERIC network path: K1 / K2+K3 / K4 / K5 for every MLP shape outside the tuned envelope,
// up to hidden width 128 and 8 hidden layers (reference configs/ablation_no_physics.yaml:11-12 trains nn_hidden 128,
// nn_layers 5; models/nn_residual.py:28-98 builds any width / depth).
//
// The tuned kernels (hode_solve_fwd.hip, hode_solve_bwd_ws.hip) keep a 4 x 64 network in registers: 211 weight registers
// per lane, gradient accumulators in registers, matrices compiled in as template parameters.  A 5 x 128 network has
// 67 k parameters (270 KB): it fits neither the register file of a wave nor the 160 KB of LDS.  So here
//   * depth is a run-time loop, every lane owns TWO hidden units (j and j + 64) in the "natural" layout of a layer's activations,
//     and the stage tape records 2 L rows of 64 + the state in 8 reals per stage;
//   * K1 / K5 (one evaluation per sample) and one-wave solves walk the matrices in their PyTorch layout, h_k by v_readlane
//     (rhs_stream / rhs_vjp_stream), parameter gradients through coalesced global atomics;
//   * the SOLVE kernels give every trajectory a TEAM of 4 / 8 waves (one workgroup) -- a trajectory of such a network is one long
//     chain of dependent evaluations, and the batches these shapes are trained on (32 windows) would leave the chip empty:
//       forward  rhs_rows: hidden layers split by output rows, activations through LDS, one barrier per layer, the wave's rows
//                register-resident for small batches, streamed from L2 (16-byte loads) for large ones;
//       adjoint  rhs_vjp_stream with TeamAccT: the wave's rows of W^T delta as partial sums (LDS exchange), ALL parameter gradients
//                in registers (compile-time indexed), one flush per workgroup and parameter set;
//     the edge parameters (first / output matrix, biases) come from an LDS image (EdgeImage).
// DESIGN.md section 4.6 has the measurements that led here.  The integrator, controller, tape format and state layout are those
// of the tuned path (hode_solve_body.h); CPU restatement: oracle/hode_oracle_impl.h (HODE_MAXH 128, HODE_MAXL 8).
//
// The path by file:
//   hode_generic_net.h          the network as the kernels see it: parameter layout, edge image, act_bwd, the skewed LDS vector
//   hode_generic_rhs.h          the forward right-hand side: rhs_stream, rhs_rows, RhsStream, RhsMulti
//   hode_generic.hip            (this file) the FORWARD kernels: K1, K2 + K3, and the batch-size rule that picks among them
//   hode_generic_vjp.h          the reverse right-hand side (rhs_vjp_stream, TeamAccT) and the kernel templates of K5 and the
//                               one-trajectory K4, with the input gradients as a template flag
//   hode_generic_bwd.hip        their production instantiations and the adjoint's launch rule
//   hode_generic_bwd_multi.hip  K4 with several trajectories per team
//   hode_generic_gin.hip        the input-gradient instantiations of K4 and K5
//   hode_generic_jvp.hip        K6, the tangent-linear pass
#include "hode_generic_rhs.h"

namespace hode {

// ------------------------------------------------------------------------------------------ K1
template <typename R>
__global__ __launch_bounds__(256) void rhs_fwd_generic_kernel(const RhsArgs<R> a, int L)
{
    const int lane = threadIdx.x & 63;
    const int wave = first_lane((int)(threadIdx.x >> 6));
    const StreamNet<R> n{a.nn_p, a.H, L, a.act};
    OdeP<R> o;
    ode_load(o, a.ode_p);
    for (int s = blockIdx.x * 4 + wave; s < a.B; s += gridDim.x * 4) {
        const R Y = (lane < 6) ? a.x[(size_t)s * 6 + lane] : R(0);
        const R gde = a.gd ? gd_effect(o, a.gd[s]) : R(0);
        const R F = rhs_stream<R>(n, EdgeFromParams<R>{n}, o, a.t ? a.t[s] : R(0), Y, a.meal ? a.meal[s] : R(0), a.tvns ? a.tvns[s] : R(0), gde, lane, nullptr);
        if (lane < 6) a.out[(size_t)s * 6 + lane] = F;
    }
}

template <typename R> int launch_rhs_fwd_generic(hipStream_t s, const RhsArgs<R> &a, int L)
{
    int blocks = (a.B + 3) / 4;
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) return HODE_OK;
    hipLaunchKernelGGL((rhs_fwd_generic_kernel<R>), dim3(blocks), dim3(256), 0, s, a, L);
    return hipGetLastError() == hipSuccess ? HODE_OK : HODE_ELAUNCH;
}

// ------------------------------------------------------------------------------------------ K2 + K3
// A team of NW waves per trajectory.  Every wave runs the integration (solve_one) on identical data -- identical step-size
// decisions, identical control flow -- and the team splits the rows of the hidden matrices inside the right-hand side (rhs_rows).
// The waves of a team write the same y / tape values to the same addresses (benign: identical bits); the stage records are written
// by the first wave only.
// (second launch bound = waves per SIMD the register allocation must leave room for: 4 for the streaming kernels -- at 130 VGPRs, three
//  waves per SIMD, the 1 024 x 61 forward of 5 x 128 took 7.3 ms instead of 5.5 -- and 2 with register-resident weights; fp64 unbounded)
template <typename R, int METHOD, bool TAPE, bool GD, int NW, int CC, int NB>
__global__ __launch_bounds__(64 * NW, (sizeof(R) == 8) ? 1 : (NB > 0 ? 2 : 4)) void solve_fwd_generic_kernel(const SolveArgs<R> a)
{
    __shared__ R rows[8 * kWave];
    __shared__ R cvec[8];
    __shared__ R ybuf[NW * (kWave + 8)];
    __shared__ R xch[(NW * 2 * kWave > 2 * kHbStride) ? NW * 2 * kWave : 2 * kHbStride];   // column split: partial sums; row split: hb[2][128]
    const int lane = threadIdx.x & 63;
    const int part = first_lane((int)(threadIdx.x >> 6));
    const int b = blockIdx.x;
    const int set = b / (a.B / a.n_sets);
    for (int i = threadIdx.x; i < 2 * kHbStride; i += 64 * NW) xch[i] = R(0);      // rhs_rows: zero beyond H, for good
    tableau_rows_store<R>(rows, METHOD, threadIdx.x, 64 * NW);
    if (threadIdx.x < 8) cvec[threadIdx.x] = (R)kTableau[METHOD].c[threadIdx.x];
    OdeP<R> o;
    ode_load(o, a.ode_p + 17 * set);
    __shared__ R edge_img[kEdgeImageMax];                // the edge parameters of this trajectory's set (EdgeImage)
    const StreamNet<R> net{a.nn_p + (size_t)set * a.nn_stride, a.H, a.L, a.act};
    EdgeImage<R>::fill(edge_img, net, threadIdx.x, 64 * NW);
    __syncthreads();
    RhsStream<R, NW, EdgeImage<R>, CC, NB> rhs{net, EdgeImage<R>{edge_img, a.H, a.L}, o, lane, part, xch, {}};
    rows_preload<R, NW, CC, NB>(rhs.rw, net, lane, part);
    solve_one<R, METHOD, TAPE, GD>(a, b, rhs, o, rows, cvec, ybuf + part * (kWave + 8), lane);
}

// TB trajectories per eight-wave workgroup (RhsMulti).  Launched for fp32, at most kGenAccMats hidden matrices, whole parameter sets
// per workgroup (per_set % TB == 0).
template <int METHOD, bool TAPE, bool GD, int TB, int CC, int NB>
__global__ __launch_bounds__(512, 2) void solve_fwd_generic_multi_kernel(const SolveArgs<float> a)
{
    constexpr int NW = 8;
    __shared__ float rows[8 * kWave];
    __shared__ float cvec[8];
    __shared__ float ybuf[NW * (kWave + 8)];
    __shared__ float hbm[TB * 3 * kHbStride];
    __shared__ float edge_img[kEdgeImageMax];
    __shared__ int done_cnt;
    const int lane = threadIdx.x & 63;
    const int part = first_lane((int)(threadIdx.x >> 6));
    const int b = blockIdx.x * TB + part % TB;
    const int set = (blockIdx.x * TB) / (a.B / a.n_sets);
    for (int i = threadIdx.x; i < TB * 3 * kHbStride; i += 64 * NW) hbm[i] = 0.f;
    tableau_rows_store<float>(rows, METHOD, threadIdx.x, 64 * NW);
    if (threadIdx.x < 8) cvec[threadIdx.x] = (float)kTableau[METHOD].c[threadIdx.x];
    if (threadIdx.x == 0) done_cnt = 0;
    OdeP<float> o;
    ode_load(o, a.ode_p + 17 * set);
    const StreamNet<float> net{a.nn_p + (size_t)set * a.nn_stride, a.H, a.L, a.act};
    EdgeImage<float>::fill(edge_img, net, threadIdx.x, 64 * NW);
    __syncthreads();
    RhsMulti<TB, CC, NB> rhs{net, EdgeImage<float>{edge_img, a.H, a.L}, o, lane, part, hbm, {}};
    rows_preload<float, NW, CC, NB>(rhs.rw, net, lane, part);
    if (b < a.B) solve_one<float, METHOD, TAPE, GD>(a, b, rhs, o, rows, cvec, ybuf + part * (kWave + 8), lane);
    // serve the other trajectories' rounds until every wave of the team is here
    if (lane == 0) atomicAdd(&done_cnt, 1);
    for (;;) {
        __syncthreads();                                    // = the first barrier of a round
        if (*(volatile int *)&done_cnt == NW) break;        // (nobody is integrating any more: every wave reads NW in the same round)
        rhs.layers(nullptr);
    }
}

template <int METHOD, int TB, int CC, int NB> static int launch_fwd_generic_multi(hipStream_t s, const SolveArgs<float> &a)
{
    const bool tape = a.tape != nullptr, gd = a.gd_mode != 0;
    const dim3 grid((a.B + TB - 1) / TB), block(512);
    if (tape) {
        if (gd) hipLaunchKernelGGL((solve_fwd_generic_multi_kernel<METHOD, true, true, TB, CC, NB>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((solve_fwd_generic_multi_kernel<METHOD, true, false, TB, CC, NB>), grid, block, 0, s, a);
    } else {
        if (gd) hipLaunchKernelGGL((solve_fwd_generic_multi_kernel<METHOD, false, true, TB, CC, NB>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((solve_fwd_generic_multi_kernel<METHOD, false, false, TB, CC, NB>), grid, block, 0, s, a);
    }
    return hipGetLastError() == hipSuccess ? HODE_OK : HODE_ELAUNCH;
}

template <typename R, int METHOD, int NW, int CC = 16, int NB = 0> static int launch_fwd_generic_t(hipStream_t s, const SolveArgs<R> &a)
{
    const bool tape = a.tape != nullptr, gd = a.gd_mode != 0;
    const dim3 grid(a.B), block(64 * NW);
    if (tape) {
        if (gd) hipLaunchKernelGGL((solve_fwd_generic_kernel<R, METHOD, true, true, NW, CC, NB>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((solve_fwd_generic_kernel<R, METHOD, true, false, NW, CC, NB>), grid, block, 0, s, a);
    } else {
        if (gd) hipLaunchKernelGGL((solve_fwd_generic_kernel<R, METHOD, false, true, NW, CC, NB>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((solve_fwd_generic_kernel<R, METHOD, false, false, NW, CC, NB>), grid, block, 0, s, a);
    }
    return hipGetLastError() == hipSuccess ? HODE_OK : HODE_ELAUNCH;
}
template <typename R, int METHOD> static int launch_fwd_generic_m(hipStream_t s, const SolveArgs<R> &a)
{
    // Teams of waves per trajectory, hidden layers split by rows (rhs_rows).  fp32 with at most kGenAccMats hidden matrices and a
    // batch of one or two trajectories per CU: eight waves with their rows of every matrix in registers (one workgroup per CU).
    // Larger batches, fp64, deeper networks: four waves (eight up to 256 trajectories) streaming the weights from L2.
    // Measured, 5 x 128 / 5 x 64, T = 61, forward (ms): B = 32: 1.56 / 0.98 (round-3 column split: 4.7 / 1.9); 256: 1.59 / 1.00;
    // 512: 3.10 resident against 3.57 streamed / 1.97 against 1.71; 1 024: 6.2 against 5.5 / 3.9 against 2.2 (one wave per
    // trajectory, the policy until now: 10.6 / 4.9); 4 096: 24.6 against 22.0 / 15.4 against 7.8.
    const bool narrow = a.H <= 64;
    if constexpr (sizeof(R) == 4) {
        // up to one trajectory per CU's team: one trajectory per team.  Above: several per team, rows still register-resident -- the
        // fewest per team (2, 4, 8) that put the batch on the chip in ONE round of 256 teams (768 trajectories as 384 teams of two: 4.0 +
        // 8.0 ms; as 192 teams of four: 2.9 + 5.1); whole parameter sets per workgroup
        if (a.L >= 2 && a.L - 1 <= kGenAccMats && a.B > 256) {
            const int per_set = a.B / a.n_sets;
            if (a.B <= 512 && per_set % 2 == 0)
                return narrow ? launch_fwd_generic_multi<METHOD, 2, 8, 1>(s, a) : launch_fwd_generic_multi<METHOD, 2, 16, 2>(s, a);
            if (a.B <= 1024 && per_set % 4 == 0)
                return narrow ? launch_fwd_generic_multi<METHOD, 4, 8, 1>(s, a) : launch_fwd_generic_multi<METHOD, 4, 16, 2>(s, a);
            if (per_set % 8 == 0)
                return narrow ? launch_fwd_generic_multi<METHOD, 8, 8, 1>(s, a) : launch_fwd_generic_multi<METHOD, 8, 16, 2>(s, a);
            if (per_set % 4 == 0)
                return narrow ? launch_fwd_generic_multi<METHOD, 4, 8, 1>(s, a) : launch_fwd_generic_multi<METHOD, 4, 16, 2>(s, a);
            if (per_set % 2 == 0)
                return narrow ? launch_fwd_generic_multi<METHOD, 2, 8, 1>(s, a) : launch_fwd_generic_multi<METHOD, 2, 16, 2>(s, a);
        }
        if (a.L >= 2 && a.L - 1 <= kGenAccMats && a.B <= (narrow ? 256 : 512))
            return narrow ? launch_fwd_generic_t<R, METHOD, 8, 8, 1>(s, a) : launch_fwd_generic_t<R, METHOD, 8, 16, 2>(s, a);
    }
    if (a.B <= 256) return narrow ? launch_fwd_generic_t<R, METHOD, 8, 8, 0>(s, a) : launch_fwd_generic_t<R, METHOD, 8, 16, 0>(s, a);
    return narrow ? launch_fwd_generic_t<R, METHOD, 4, 8, 0>(s, a) : launch_fwd_generic_t<R, METHOD, 4, 16, 0>(s, a);
}
template <typename R> int launch_solve_fwd_generic(hipStream_t s, const SolveArgs<R> &a, int method)
{
    return method == HODE_METHOD_DP54 ? launch_fwd_generic_m<R, HODE_METHOD_DP54>(s, a) : launch_fwd_generic_m<R, HODE_METHOD_RK4>(s, a);
}

template int launch_rhs_fwd_generic<float>(hipStream_t, const RhsArgs<float> &, int);
template int launch_rhs_fwd_generic<double>(hipStream_t, const RhsArgs<double> &, int);
template int launch_solve_fwd_generic<float>(hipStream_t, const SolveArgs<float> &, int);
template int launch_solve_fwd_generic<double>(hipStream_t, const SolveArgs<double> &, int);

}  // namespace hode

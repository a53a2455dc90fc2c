// hode_solve_fwd.hip -- K2+K3: batched forward integration, one trajectory per wavefront, ALL weights in registers.
//
// Replaces HybridODENN.forward (reference models/hybrid_ode_nn.py:136-261).  The integration itself is
// hode_solve_body.h (solve_one).  This kernel -- one wave per workgroup, 211 weight registers, 2 waves per SIMD -- is the
// production kernel for fp32 and fp64.  Three experiment kernels that reach 4 waves per SIMD and measured SLOWER (DESIGN.md
// section 6.2) live in csrc/lab/ and are compiled into the lab library only.
#include "hode_solve_body.h"
#include <cstdlib>

namespace hode {

// MULTI: launches of MANY SHORT trajectories of ONE parameter set (the two-point solves of the physics loss: 81 920 per 4 096-patient
// step, a dozen evaluations each) hand every wave `chunk` consecutive trajectories, so that the 54 KB of weights are gathered from L2
// once per wave and not once per trajectory (half of such a launch's time).  A separate instantiation: the loop is kept out of the
// kernels every other launch runs.
// PACE: every wave sets its issue priority from the share of its own work that is left (pace_prio, hode_solve_body.h), so that the two
// waves of a SIMD reach the end of the launch together.  The product library always paces; the lab library and experiment builds can
// switch it off for A/B runs (fwd_pace() below, -DHODE_FWD_NOPACE).
// ROT: how many of a hidden layer's 15 rotations a kernel fetches through LDS instead of DPP (mlp_hidden_blk_lds, hode_mlp.h: K, and
// LEAN = its form that lands two of them in v9 / v11); 0 = mlp_hidden_blk.  A compile-time choice per instantiation, by the registers
// it has (hipcc -Rpass-analysis=kernel-resource-usage; no instantiation may gain scratch or lose occupancy over K = 0):
//   three hidden matrices (NL = 4): 256 registers, none to spare.  The lean K = 8 costs 8 and fits where K = 0 left that many: DP5(4)
//     without tape, Hill term or the MULTI loop (the benchmark kernel), and RK4 unless it tapes AND carries the Hill term; the others
//     keep K = 0 (the taping DP5(4) goes 0 -> 16 B of scratch with K = 4 already)
//   two (NL = 3): <= 217 registers at K = 12, every instantiation takes it
//   one (NL = 2): three to four waves per SIMD, a regime the microbenchmark did not cover, and RK4 + tape + Hill term would drop from four
//     waves to three: K = 0
// Experiment builds (tools/build_variant.sh) force one form on every fp32 instantiation with a hidden matrix:
// -DHODE_FWD_LDS_ROT=<0|4|8|12> [-DHODE_FWD_LDS_ROT_LEAN=1, with 8].
template <typename R, int NL, int METHOD, bool TAPE, bool GD, bool MULTI> struct FwdRot {
#ifdef HODE_FWD_LDS_ROT
    static constexpr int K = (sizeof(R) == 4 && NL >= 2) ? HODE_FWD_LDS_ROT : 0;
#ifdef HODE_FWD_LDS_ROT_LEAN
    static constexpr bool LEAN = K > 0 && HODE_FWD_LDS_ROT_LEAN;
#else
    static constexpr bool LEAN = false;
#endif
#else
    static constexpr bool kRoom4 = METHOD == HODE_METHOD_DP54 ? (!TAPE && !GD && !MULTI) : !(TAPE && GD);
    static constexpr int K = sizeof(R) != 4 ? 0 : NL == 3 ? 12 : (NL == 4 && kRoom4) ? 8 : 0;
    static constexpr bool LEAN = K == 8;
#endif
};

template <typename R, int NL, int METHOD, int LB, bool TAPE, bool GD, bool MULTI, bool PACE>
__global__ __launch_bounds__(64, LB) void solve_fwd_kernel(const SolveArgs<R> a, const int chunk)
{
    HODE_WL(0);
    using Rot = FwdRot<R, NL, METHOD, TAPE, GD, MULTI>;
    __shared__ R rows[8 * kWave];             // tableau coefficient rows (hode_tableau.h)
    __shared__ R cvec[8];                     // tableau nodes c[s] as reals
    __shared__ R ybuf[kWave + 8];             // output staging: rows of 6 reals are gathered into 256-byte stores
    const int lane = threadIdx.x;
    const int b0 = MULTI ? blockIdx.x * chunk : blockIdx.x;                 // one wave == one trajectory (MULTI: one after the other)
    const int set = b0 / (a.B / a.n_sets);

    tableau_rows_store<R>(rows, METHOD, lane, 64);
    if (lane < 8) cvec[lane] = (R)kTableau[METHOD].c[lane];
    std::conditional_t<(Rot::K > 0), MlpRegsRot<NL, Rot::K, Rot::LEAN>, MlpRegs<R, NL>> W;
    if constexpr (Rot::K > 0) {
        __shared__ float rotbuf[kRotBufElems];    // the hidden layers' rotation operands (this wave's: one wave per workgroup)
        W.rot = rot_lane_addr((unsigned)(size_t)(__attribute__((address_space(3))) float *)rotbuf, lane);
    }
    mlp_load<R, NL>(W, a.nn_p + (size_t)set * a.nn_stride, a.H, lane);
    OdeP<R> o;
    ode_load(o, a.ode_p + 17 * set);
    __syncthreads();
    HODE_WL(1);
    const RhsRegs<R, NL, decltype(W)> rhs{W, o, lane};
    if constexpr (MULTI) {
        const int b1 = (b0 + chunk < a.B) ? b0 + chunk : a.B;
        const int per = a.T - 1;              // grid intervals of one trajectory; the pace is taken over the whole chunk
#pragma unroll 1
        for (int b = b0; b < b1; ++b) solve_one<R, METHOD, TAPE, GD, PACE>(a, b, rhs, o, rows, cvec, ybuf, lane, (b1 - 1 - b) * per, (b1 - b0) * per);
    } else {
        solve_one<R, METHOD, TAPE, GD, PACE>(a, b0, rhs, o, rows, cvec, ybuf, lane);
    }
    HODE_WL_EXIT();
}

#ifdef HODE_LAB
static bool fwd_pace();
#endif

template <typename R, int NL, int METHOD, bool TAPE, bool GD, bool PACE = true>
static void launch_one(hipStream_t s, const SolveArgs<R> &a)
{
#if defined(HODE_LAB) || defined(HODE_FWD_NOPACE)
    if constexpr (PACE) {
#ifdef HODE_LAB
        if (!fwd_pace())
#endif
            return launch_one<R, NL, METHOD, TAPE, GD, false>(s, a);
    }
#endif
    // waves per SIMD the register budget allows: 211 weight registers for 3 hidden matrices -> 2; fewer layers -> more
    constexpr int LB = (sizeof(R) == 4) ? (NL >= 3 ? 2 : (NL == 2 ? 3 : 4)) : 1;
    if constexpr (!TAPE && !GD && METHOD == HODE_METHOD_DP54 && sizeof(R) == 4) {
        // grid points <= 4, one parameter set, more trajectories than four rounds of the chip's 2 048 wave slots: see the kernel
        // (the benchmark batch as ONE round of 2 048 waves with two trajectories each was measured too: 3.10 against 3.01 ms)
        if (a.T <= 4 && a.n_sets == 1 && a.B > 8192) {
            const int chunk = (a.B + 8191) / 8192;
            hipLaunchKernelGGL((solve_fwd_kernel<R, NL, METHOD, LB, TAPE, GD, true, PACE>), dim3((a.B + chunk - 1) / chunk), dim3(64), 0, s, a, chunk);
            return;
        }
    }
    hipLaunchKernelGGL((solve_fwd_kernel<R, NL, METHOD, LB, TAPE, GD, false, PACE>), dim3(a.B), dim3(64), 0, s, a, 1);
}

template <typename R, int NL>
static int launch_nl(hipStream_t s, const SolveArgs<R> &a, int method)
{
    const bool tape = a.tape != nullptr, gd = a.gd_mode != 0;
    if (method == HODE_METHOD_DP54) {
        if (tape) { if (gd) launch_one<R, NL, HODE_METHOD_DP54, true, true>(s, a); else launch_one<R, NL, HODE_METHOD_DP54, true, false>(s, a); }
        else { if (gd) launch_one<R, NL, HODE_METHOD_DP54, false, true>(s, a); else launch_one<R, NL, HODE_METHOD_DP54, false, false>(s, a); }
    } else {
        if (tape) { if (gd) launch_one<R, NL, HODE_METHOD_RK4, true, true>(s, a); else launch_one<R, NL, HODE_METHOD_RK4, true, false>(s, a); }
        else { if (gd) launch_one<R, NL, HODE_METHOD_RK4, false, true>(s, a); else launch_one<R, NL, HODE_METHOD_RK4, false, false>(s, a); }
    }
    return hipGetLastError() == hipSuccess ? HODE_OK : HODE_ELAUNCH;
}

#ifdef HODE_LAB
// Lab library only (make lab -> hode/lab/libhode_lab.so).  HODE_FWD=wg: the LDS-image workgroup kernel
// (lab/hode_solve_fwd_wg.hip); HODE_FWD=quad: four trajectories per four waves with column-split weights
// (lab/hode_solve_fwd_quad.hip); HODE_FWD=rows: four trajectories per four waves, weights split by output rows over the waves
// and by input blocks over the 16-lane rows (lab/hode_solve_fwd_rows.hip); anything else: this file's kernel
static char fwd_mode()
{
    static const char v = [] {
        const char *e = getenv("HODE_FWD");
        if (e == nullptr) return '\0';
        return (e[0] == 'r' && e[1] == 'o') ? 'R' : e[0];
    }();
    return v;
}
// HODE_FWD_PACE=off: the register kernels without the priority pacing (A/B timings; tests/test_fwd_pacing_gpu.py compares the bits)
static bool fwd_pace()
{
    static const bool v = [] {
        const char *e = getenv("HODE_FWD_PACE");
        return !(e != nullptr && (e[0] == '0' || (e[0] == 'o' && e[1] == 'f')));
    }();
    return v;
}
#endif

template <typename R> int launch_solve_fwd(hipStream_t s, const SolveArgs<R> &a, int L, int method)
{
#ifdef HODE_LAB
    if constexpr (sizeof(R) == 4) {
        if (L >= 2 && L <= 4 && fwd_mode() == 'w') return launch_solve_fwd_wg(s, a, L, method);
        if (L >= 2 && L <= 4 && fwd_mode() == 'q') return launch_solve_fwd_quad(s, a, L, method);
        if (L >= 2 && L <= 4 && fwd_mode() == 'R') return launch_solve_fwd_rows(s, a, L, method);
    }
#endif
    switch (L) {
    case 1: return launch_nl<R, 1>(s, a, method);
    case 2: return launch_nl<R, 2>(s, a, method);
    case 3: return launch_nl<R, 3>(s, a, method);
    case 4: return launch_nl<R, 4>(s, a, method);
    }
    return HODE_EUNSUPPORTED;
}

template int launch_solve_fwd<float>(hipStream_t, const SolveArgs<float> &, int, int);
template int launch_solve_fwd<double>(hipStream_t, const SolveArgs<double> &, int, int);

}  // namespace hode

#ifdef HODE_FWD_TRACE
// experiment build only: the stamps of hode_rhs_eval.h's g_ft (this translation unit's copy: the forward kernels are instantiated here)
extern "C" int hode_lab_fwd_trace(unsigned long long *dst, int n_words, unsigned *count)
{
    if (hipMemcpyFromSymbol(count, HIP_SYMBOL(hode::g_ft_n), sizeof(unsigned)) != hipSuccess) return -1;
    return hipMemcpyFromSymbol(dst, HIP_SYMBOL(hode::g_ft), sizeof(unsigned long long) * (size_t)n_words) == hipSuccess ? 0 : -1;
}
// the wave-lifetime records of the last forward launch: n_waves <= kWlWaves records of 8 words (hode_rhs_eval.h, g_wl)
extern "C" int hode_lab_fwd_lifetimes(unsigned long long *dst, int n_waves)
{
    if (n_waves < 0 || n_waves > hode::kWlWaves) return -1;
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    return hipMemcpyFromSymbol(dst, HIP_SYMBOL(hode::g_wl), sizeof(unsigned long long) * 8 * (size_t)n_waves) == hipSuccess ? 0 : -1;
}
#endif

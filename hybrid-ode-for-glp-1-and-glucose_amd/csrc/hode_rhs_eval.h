// hode_rhs_eval.h -- the right-hand side f(t, x, u) = mechanistic part + residual network of ONE evaluation by one wave: the 17
// ODE constants, the state broadcasts, mech_eval, rhs_eval, and the shader-clock stamps of the HODE_FWD_TRACE experiment build.
// Used by: hode_solve_body.h (every forward solve), hode_rhs.hip, hode_solve_jvp.hip, hode_adjoint.h (OdeP; the adjoints re-evaluate
// nothing), hode_generic_rhs.h.
#pragma once
#include "hode_mlp.h"

namespace hode {

// ------------------------------------------------------------------------------------------
// The 17 mechanistic constants (models/ode_core.py:44-71), wave-uniform (scalar loads).
template <typename R> struct OdeP {
    R a_GI, k_I, rho, G_b, I_b, E_max, EC_50, Glu_b, V_max, K_m, k_L, k_GE0, IGD_50, g, p_7, p_8, p_9;
};
template <typename R> __device__ __forceinline__ void ode_load(OdeP<R> &o, const R *__restrict__ p)
{
    o.a_GI = p[0]; o.k_I = p[1]; o.rho = p[2]; o.G_b = p[3]; o.I_b = p[4]; o.E_max = p[5];
    o.EC_50 = p[6]; o.Glu_b = p[7]; o.V_max = p[8]; o.K_m = p[9]; o.k_L = p[10]; o.k_GE0 = p[11];
    o.IGD_50 = p[12]; o.g = p[13]; o.p_7 = p[14]; o.p_8 = p[15]; o.p_9 = p[16];
}

// gastric-distension Hill term (models/ode_core.py:139-140); only evaluated when a GD input exists
template <typename R> __device__ __forceinline__ R gd_effect(const OdeP<R> &o, R gd)
{
    R u = rpow(gd, o.g), v = rpow(o.IGD_50, o.g);
    return u / (v + u);
}

// x_K of the replicated state layout on every lane.  fp32: a DPP row broadcast into a VGPR (lane K of each 16-lane row holds
// x_K) instead of a v_readlane into an SGPR: the mechanistic terms combine the state with the 17 ODE constants, which live
// in SGPRs, and a VALU instruction reads at most one SGPR -- every (state, constant) pair cost a v_mov_b32 before.
template <int K> __device__ __forceinline__ float state_bcast(float Y)
{
    return i2f(__builtin_amdgcn_update_dpp(0, f2i(Y), 0x150 + K, 0xF, 0xF, true));       // row_newbcast:K (every lane written)
}
template <int K> __device__ __forceinline__ double state_bcast(double Y) { return lane_bcast(Y, K); }
// acc + x_K * w with the broadcast folded into the FMA (fp32: v_fmac_f32_dpp row_newbcast:K) -- for a component only one
// instruction reads.  Y must be two wait states old (it is the stage state, computed well before the RHS starts).
template <int K> __device__ __forceinline__ float fmac_state(float acc, float Y, float w);
#define HODE_FMAC_STATE(K)                                                                                              \
    template <> __device__ __forceinline__ float fmac_state<K>(float acc, float Y, float w)                             \
    {                                                                                                                   \
        asm("v_fmac_f32_dpp %0, %1, %2 row_newbcast:" #K " row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(Y), "v"(w));   \
        return acc;                                                                                                     \
    }
HODE_FMAC_STATE(0) HODE_FMAC_STATE(1) HODE_FMAC_STATE(2) HODE_FMAC_STATE(3) HODE_FMAC_STATE(4) HODE_FMAC_STATE(5)
#undef HODE_FMAC_STATE
template <int K> __device__ __forceinline__ double fmac_state(double acc, double Y, double w) { return rfma(w, lane_bcast(Y, K), acc); }
// x_K as the factor of ONE product, x_K * v: a broadcast value (the generic path, fp64), or the replicated state itself with the
// broadcast folded into the multiplication (fp32: v_mul_f32_dpp row_newbcast:K; Y two wait states old, as for fmac_state)
template <typename R> struct StateVal {
    R x;
    __device__ __forceinline__ R times(R v) const { return x * v; }
};
template <int K> struct StateDpp {
    float Y;
    __device__ __forceinline__ float times(float v) const
    {
        static_assert(K == 5, "row_newbcast:5 is the one the right-hand side folds");
        float out;
        asm("v_mul_f32_dpp %0, %1, %2 row_newbcast:5 row_mask:0xf bank_mask:0xf" : "=v"(out) : "v"(Y), "v"(v));
        return out;
    }
};

// KK with the eight lanes of stage slot s (lanes 8 s .. 8 s + 7) replaced by F.  fp32: the lane mask 0xff << 8 s is scalar
// arithmetic and feeds v_cndmask_b32 as an SGPR pair -- (lane >> 3) == s costs a shift and a compare on the vector ALU in
// every stage.  s must be wave-uniform.
__device__ __forceinline__ float stage_put(float KK, float F, int s)
{
    const unsigned long long m = 0xffull << (8 * s);
    float out;
    asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(out) : "v"(KK), "v"(F), "s"(m));
    return out;
}
__device__ __forceinline__ double stage_put(double KK, double F, int s) { return ((int)(threadIdx.x & 63) >> 3) == s ? F : KK; }

// sel ? term : other, with `term` (a wave-uniform value every lane can compute) evaluated on ALL lanes first.  Left alone,
// hipcc sinks the arithmetic of each term of a select chain into an exec-masked region of the lanes that keep it: the same
// VALU instructions plus a v_cmp / s_and_saveexec / s_cbranch_execz round trip per term (measured: 4 % of the forward solve).
template <typename R> __device__ __forceinline__ R keep_term(bool sel, R term, R other)
{
    asm volatile("" : "+v"(term));
    return sel ? term : other;
}

// ------------------------------------------------------------------------------------------
// Mechanistic part (models/ode_core.py:124-153), evaluated redundantly on every lane from the broadcast state; the lane
// keeps the component of its slot c8 = lane & 7 (GE, slot 4, has no dynamics; slots 6, 7 are padding).
// FFA is the factor of one product only: a StateVal, or a StateDpp<5> that reads it out of the replicated state in that product.
// PACK (fp32): the independent pairs of the terms as packed adds and products -- (u, d1) = (G, GLP1) + (-G_b, EC_50),
// (v, w) = (I, Glu) + (-I_b, -Glu_b), (q2, q1) = (G, GLP1) * (rcp d2, rcp d1) -- three instructions for six.  Each half rounds exactly
// like the scalar instruction, and a - b == a + (-b) bit for bit: the kernels stay comparable whichever form they take.
template <typename R, bool PACK = false, typename FS>
__device__ __forceinline__ R mech_eval(const OdeP<R> &o, R G, R I, R Glu, R GLP1, const FS &FFA, R meal, R gde, int c8)
{
    // Every product / sum is written out (fused where one rounding is saved) and contraction is off: the bits do not depend
    // on which kernel this is inlined into (the forward variants are compared bit for bit, tests/test_hip_parity.py).
#pragma clang fp contract(off)
    R v, w, dI, dGlu, dGLP1;
    if constexpr (PACK) {
        static_assert(sizeof(R) == 4, "packed fp32 instructions");
        const f2_t A = {G, GLP1}, B = {I, Glu};
        const f2_t ud = A + f2_t{-o.G_b, o.EC_50}, vw = B + f2_t{-o.I_b, -o.Glu_b};
        v = vw.x, w = vw.y;
        const f2_t rr = {__builtin_amdgcn_rcpf(o.K_m + G), __builtin_amdgcn_rcpf(ud.y)};
        const f2_t qq = A * rr;                                                    // (G / (K_m + G), GLP1 / (EC_50 + GLP1))
        const R Pi = rfma(o.rho, GLP1, R(1));
        dI = rfma(Pi * o.a_GI, ud.x, -(o.k_I * v));
        dGlu = -(o.E_max * qq.y) * w;
        dGLP1 = rfma(o.V_max, qq.x, -(o.k_L * GLP1));
    } else {
        const R u = G - o.G_b;
        v = I - o.I_b, w = Glu - o.Glu_b;
        const R Pi = rfma(o.rho, GLP1, R(1));
        dI = rfma(Pi * o.a_GI, u, -(o.k_I * v));                                   // ode_core.py:124-125
        dGlu = -(o.E_max * rdiv(GLP1, o.EC_50 + GLP1)) * w;                        // :129-130
        dGLP1 = rfma(o.V_max, rdiv(G, o.K_m + G), -(o.k_L * GLP1));                // :134-135
    }
    const R k_GE = o.k_GE0 * (R(1) - gde);                                         // :139-140
    R dFFA = FFA.times(rfma(o.p_9, G, rfma(-o.p_8, I, -o.p_7)));                   // :144  (-p7 - p8 I + p9 G) F
    R dG = rfma(-k_GE, G, rfma(R(0.005), w, rfma(R(-0.01), v, meal)));             // :148-150
    R r = keep_term(c8 == 0, dG, R(0));
    r = keep_term(c8 == 1, dI, r);
    r = keep_term(c8 == 2, dGlu, r);
    r = keep_term(c8 == 3, dGLP1, r);
    r = keep_term(c8 == 5, dFFA, r);
    return r;
}
template <typename R> __device__ __forceinline__ R mech_eval(const OdeP<R> &o, R G, R I, R Glu, R GLP1, R FFA, R meal, R gde, int c8)
{
    return mech_eval<R, false>(o, G, I, Glu, GLP1, StateVal<R>{FFA}, meal, gde, c8);
}

// ------------------------------------------------------------------------------------------
// RHS  f(t, x, u) = ODECore + NNResidual  (models/hybrid_ode_nn.py:108-134)
//   Y   lane-distributed state: lane l holds x_{l&7} (replicated over the eight 8-lane groups;
//       fp32 reads lane k of EVERY 16-lane row for x_k, fp64 lane k of the wave)
//   returns the derivative in the same replicated layout (component slots 6,7 hold 0)
//   W   weights holder: MlpRegs (everything in VGPRs) or, in the lab library, MlpLds (lab/hode_lab_layers.h)
#ifdef HODE_FWD_TRACE
// experiment build only (tools/build_variant.sh fwdtrace -DHODE_FWD_TRACE=<workgroup>; tools/fwd_trace.py): shader-clock stamps of ONE
// wave at six points of every right-hand side it evaluates -- entry | mechanistic terms | first layer | hidden layers 1..3 | return --, in a ring of 4 096 records
static __device__ unsigned long long g_ft[4096 * 8];
static __device__ unsigned g_ft_n;
#define HODE_FT(i, v) if (ft_on) asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(ft[i]), "+v"(v))
// ... and the LIFETIME of every wave of a forward launch (tools/fwd_trace.py --lifetimes), one record of 8 words per workgroup:
//   0 entry | 1 after the weight prologue | 2, 3, 4 grid index T/4, T/2, 3T/4 | 5 exit        (s_memtime, shader clock of the wave's XCC)
//   6 HW_REG_HW_ID (wave slot, SIMD, CU, SH, SE) | HW_REG_XCC_ID << 32
//   7 blockIdx.x | low word of s_memrealtime at exit << 32 (100 MHz, ONE counter for the chip: the XCCs' shader clocks are not aligned)
// written by lane 0 with vector stores; launches of more than kWlWaves workgroups record the first kWlWaves
constexpr int kWlWaves = 8192;
static __device__ unsigned long long g_wl[kWlWaves * 8];
__device__ __forceinline__ void wl_put(int i, unsigned long long v)
{
    if ((threadIdx.x & 63) == 0 && threadIdx.x < 64 && blockIdx.x < (unsigned)kWlWaves) g_wl[(size_t)blockIdx.x * 8 + i] = v;
}
__device__ __forceinline__ unsigned long long wl_clock()
{
    unsigned long long c;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(c));
    return c;
}
__device__ __forceinline__ void wl_stamp(int i) { wl_put(i, wl_clock()); }
__device__ __forceinline__ void wl_exit()
{
    unsigned hw, xcc;
    unsigned long long rt;
    wl_stamp(5);
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)\n\ts_getreg_b32 %1, hwreg(HW_REG_XCC_ID)\n\ts_memrealtime %2\n\ts_waitcnt lgkmcnt(0)"
                 : "=s"(hw), "=s"(xcc), "=s"(rt));
    wl_put(6, (unsigned long long)hw | ((unsigned long long)xcc << 32));
    wl_put(7, (unsigned long long)blockIdx.x | (rt << 32));
}
#define HODE_WL(i) wl_stamp(i)
#define HODE_WL_EXIT() wl_exit()
#define HODE_WL_GRID(k, T) do { if ((k) == (T) / 4) wl_stamp(2); else if ((k) == (T) / 2) wl_stamp(3); else if ((k) == 3 * (T) / 4) wl_stamp(4); } while (0)
#else
#define HODE_FT(i, v)
#define HODE_WL(i)
#define HODE_WL_EXIT()
#define HODE_WL_GRID(k, T)
#endif
// weight holders whose kernel takes the packed form of the mechanistic terms (the forward solve kernels choose per instantiation)
template <typename T, typename = void> struct packs_mech { static constexpr bool value = false; };
template <typename T> struct packs_mech<T, decltype((void)T::kPackMech)> { static constexpr bool value = T::kPackMech; };
template <typename R, int NL, bool KEEP, typename WT, typename ACTS = MlpActs<R, NL>>
__device__ __forceinline__ R rhs_eval(const WT &W, const OdeP<R> &o, R t, R Y, R meal, R tvns,
                                      R gde /* Hill term, 0 without GD */, int lane, ACTS *acts)
{
#ifdef HODE_FWD_TRACE
    const bool ft_on = sizeof(R) == 4 && NL == 4 && blockIdx.x == HODE_FWD_TRACE;
    unsigned long long ft[8] = {};
#endif
    HODE_FT(0, Y);
    const R G = state_bcast<0>(Y), I = state_bcast<1>(Y), Glu = state_bcast<2>(Y), GLP1 = state_bcast<3>(Y);
    const int c8 = lane & 7;
    // FFA has two readers, both products: fp32 folds its broadcast into each of them (as GE's into its one)
    constexpr bool kFoldFFA = sizeof(R) == 4;
    [[maybe_unused]] R FFA = R(0);
    if constexpr (!kFoldFFA) FFA = state_bcast<5>(Y);
    R mech;
    if constexpr (kFoldFFA) mech = mech_eval<R, packs_mech<WT>::value>(o, G, I, Glu, GLP1, StateDpp<5>{Y}, meal, gde, c8);
    else mech = mech_eval(o, G, I, Glu, GLP1, FFA, meal, gde, c8);
    HODE_FT(6, mech);
    // ---- MLP (models/nn_residual.py:138-147): input row [t, G, I, Glu, GLP1, GE, FFA, glp1:=GLP1, tvns]
    R h = W.b[0];
    h = rfma(W.w1[0], t, h);
    h = rfma(W.w1[1], G, h);
    h = rfma(W.w1[2], I, h);
    h = rfma(W.w1[3], Glu, h);
    h = rfma(W.w1g, GLP1, h);                    // columns 4 and 7 (both GLP1), folded by the loaders
    h = fmac_state<4>(h, Y, W.w1[5]);            // GE: only the first layer reads it
    if constexpr (kFoldFFA) h = fmac_state<5>(h, Y, W.w1[6]);
    else h = rfma(W.w1[6], FFA, h);
    h = rfma(W.w1[8], tvns, h);
    h = rmax0(h);
    HODE_FT(1, h);
    if constexpr (KEEP) acts->put(0, h);
#pragma unroll
    for (int l = 0; l < NL - 1; ++l) {
        if constexpr (applies_relu<WT>::value) h = W.hidden_relu(l, h);
        else h = rmax0(W.hidden(l, h));
        HODE_FT(2 + l, h);
        if constexpr (KEEP) acts->put(l + 1, h);
    }
    if constexpr (sizeof(R) == 4) {
        // out_rot leaves Wout h + bout on the lanes of slot c8 < 6 and exact zeros on slots 6, 7 (zero weights, zero bias);
        // the mechanistic select chain ends in zero there as well: no final select
        R res = mech + out_rot(W.w5r, W.b5, h);
        HODE_FT(5, res);
#ifdef HODE_FWD_TRACE
        if (ft_on && lane == 0) {
            // slot = a hash of the entry time (an evaluation takes > 2 000 cycles: consecutive ones fall into different slots); a counter
            // in memory would put a load round trip between every two evaluations of the wave that is being measured
            const unsigned n = (unsigned)(ft[0] >> 10);
            for (int i = 0; i < 8; ++i) g_ft[(n & 4095) * 8 + i] = ft[i];
        }
#endif
        return res;
    }
    R nn;
    {
        R p[6];
#pragma unroll
        for (int q = 0; q < 6; ++q) p[q] = W.w5[q] * h;
        nn = wave_reduce6_to_lanes(p, lane);
    }
    return (c8 < 6) ? (mech + nn + W.b5) : R(0);
}

}  // namespace hode

// hode_mlp.h -- the residual network of the tuned path (H <= 64, 1..4 hidden layers) in registers: the weight holders and their
// loaders, the hidden layer (fp32: one asm statement in row-block order, with or without rotations through LDS; fp64: readlane),
// the output layer in rotating order, and where a layer's activations go.
// Used by: hode_rhs_eval.h (and through it every kernel that evaluates the right-hand side), hode_solve_fwd.hip (MlpRegsRot),
// hode_solve_jvp.hip, hode_solve_bwd_ws.hip (blk_rows_finish, f2_t), hode_adjoint.h (MlpActs).
#pragma once
#include "hode_xlane.h"
#include <type_traits>

namespace hode {

// ------------------------------------------------------------------------------------------
// MLP parameters of ONE parameter set, register-resident.  NL = number of hidden layers (1..4).
// Activations: lane j = hidden unit j of every layer.  H < 64 is zero-padded (relu(0) = 0 keeps it exact).
__device__ __forceinline__ double mlp_hidden(const double (&w)[64], double bias, double h);
typedef float f2_t __attribute__((ext_vector_type(2)));       // an even-aligned VGPR pair: operand of the packed fp32 instructions
template <bool RELU> __device__ __forceinline__ float mlp_hidden_blk(const f2_t (&wp)[32], float bias, float h);
__device__ __forceinline__ double mlp_hidden_relu(const double (&w)[64], double bias, double h);
template <typename R, int NL> struct MlpRegs {
    R w1[9];                          // W1[j][0..8]
    R w1g;                            // W1[j][4] + W1[j][7]: the weight of GLP1, which the input row holds twice
    R b[NL];                          // b_l[j]
    // fp64: W_l[j][0..63], l = 2..NL.  fp32: the row-block order of mlp_hidden_blk as the register PAIRS its packed FMAs take --
    // wh[l][2 n] = (w0_n, w2_n), wh[l][2 n + 1] = (w1_n, w3_n) -- filled pair by pair in mlp_load (gathered into single registers first
    // and paired up afterwards, hipcc shuffled the 192 weights through 456 B of scratch per lane: 240 MB of HBM traffic per launch)
    using HW = std::conditional_t<sizeof(R) == 4, f2_t, R>;
    HW wh[(NL > 1) ? NL - 1 : 1][sizeof(R) == 4 ? kMaxH / 2 : kMaxH];
    R w5[6];                          // Wout[o][j]
    R w5r[8];                         // fp32: Wout[lane & 7] in rotating order (out_rot_fill); unused in fp64
    R b5;                             // lane l: bout[l & 7] (0 for slots 6,7)
    // pre-activation of hidden layer l + 2 (l is a compile-time constant at every call site: unrolled layer loop)
    __device__ __forceinline__ R hidden(int l, R h) const
    {
        if constexpr (sizeof(R) == 4) return mlp_hidden_blk<false>(wh[l], b[l + 1], h);
        else return mlp_hidden(wh[l], b[l + 1], h);
    }
    // fp32: the ReLU is the last instruction of the layer's asm statement (hidden_relu); applied to the asm's result from
    // outside it costs two instructions -- hipcc canonicalises a value it did not compute itself before a max
    static constexpr bool kHiddenRelu = sizeof(R) == 4;
    __device__ __forceinline__ R hidden_relu(int l, R h) const
    {
        if constexpr (sizeof(R) == 4) return mlp_hidden_blk<true>(wh[l], b[l + 1], h);
        else return mlp_hidden_relu(wh[l], b[l + 1], h);
    }
};
// weight holders whose hidden_relu(l, h) returns the POST-activation of hidden layer l + 2
template <typename T, typename = void> struct applies_relu { static constexpr bool value = false; };
template <typename T> struct applies_relu<T, decltype((void)T::kHiddenRelu)> { static constexpr bool value = T::kHiddenRelu; };

// Load one parameter set into registers: every lane gathers its weights straight from L2 in the lane-dependent rotated order (the
// hidden layers below; a coalesced load + LDS permutation measured the same, profiles/r04_fwd_sizes_staged.log, and cost 8.3 KB of LDS
// per wave).
// Output layer in rotating order (fp32): lane (r, i) = lane 16 r + i keeps, for output o = i & 7,
//     w5r[n] = Wout[o][16 r + ((i - n) & 15)]   n = 0..7        (zero for o >= 6)
// so that sum_n row_ror:n(h) * w5r[n] -- 8 FMAs on the activation vector in its natural layout -- is one half of the lane's
// row-r part of output o; lane i + 8 of the same row (same output) holds the other half (its eight sources are the other
// eight lanes), a row_ror:8 add joins them, and an all-reduce over the four rows (2 swaps + 2 adds) leaves out_o on every lane
// with i & 7 == o: the replicated layout of the state.  15 vector instructions instead of the 35 of six products +
// wave_reduce6_to_lanes, for two more weight registers.
template <typename WT> __device__ __forceinline__ void out_rot_fill(WT &W, const float *__restrict__ pout, int H, int lane)
{
    const int i = lane & 15, r = lane >> 4, o = lane & 7;
#pragma unroll
    for (int n = 0; n < 8; ++n) {
        const int k = 16 * r + ((i - n) & 15);
        const bool ok = o < 6 && k < H;
        W.w5r[n] = ok ? pout[(ok ? o : 0) * H + (ok ? k : 0)] : 0.f;
    }
}
template <typename WT> __device__ __forceinline__ void out_rot_fill(WT &, const double *__restrict__, int, int) {}

template <typename R, int NL>
__device__ __forceinline__ void mlp_load(MlpRegs<R, NL> &W, const R *__restrict__ p, int H, int lane)
{
    // branch-free: out-of-range lanes / columns read a clamped (valid) address and are zeroed
    const R live = (lane < H) ? R(1) : R(0);
    const int j = (lane < H) ? lane : H - 1;
#pragma unroll
    for (int i = 0; i < 9; ++i) W.w1[i] = live * p[j * 9 + i];
    W.w1g = W.w1[4] + W.w1[7];        // input row = [t, G, I, Glu, GLP1, GE, FFA, GLP1, tvns]: the two GLP1 columns act as one
    p += 9 * H;
    W.b[0] = live * p[j];
    p += H;
#pragma unroll
    for (int l = 0; l < NL - 1; ++l) {
        const R *row = p + (size_t)j * H;
        if constexpr (sizeof(R) == 4) {
            // row-block order (mlp_hidden_blk): lane (r, i) = lane 16 r + i keeps, for w = 0..3 and n = 0..15,
            //     weight (w, n) = W_l[16 w + i][16 r + ((i - n) & 15)]    -> half (w >> 1) of the pair wh[l][2 n + (w & 1)]
            // gathered straight from L2 (192 dword loads per lane and trajectory, ~0.5 % of a 241-point solve)
            (void)row;
            const int i = lane & 15, r = lane >> 4;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const int u = 16 * w + i;
#pragma unroll
                for (int n = 0; n < 16; ++n) {
                    const int c = 16 * r + ((i - n) & 15);
                    const bool ok = u < H && c < H;
                    const R v = ok ? p[(size_t)(ok ? u : 0) * H + (ok ? c : 0)] : R(0);
                    if (w >> 1) W.wh[l][2 * n + (w & 1)].y = v;
                    else W.wh[l][2 * n + (w & 1)].x = v;
                }
            }
        } else {
            if (H == kMaxH) {
                const double2 *r2 = reinterpret_cast<const double2 *>(row);
#pragma unroll
                for (int k = 0; k < kMaxH / 2; ++k) {
                    double2 v = r2[k];
                    W.wh[l][2 * k + 0] = v.x; W.wh[l][2 * k + 1] = v.y;
                }
            } else {
#pragma unroll
                for (int k = 0; k < kMaxH; ++k) W.wh[l][k] = ((k < H) ? live : R(0)) * row[(k < H) ? k : H - 1];
            }
        }
        p += (size_t)H * H;
        W.b[l + 1] = live * p[j];
        p += H;
    }
#pragma unroll
    for (int o = 0; o < 6; ++o) W.w5[o] = live * p[o * H + j];
    out_rot_fill(W, p, H, lane);
    p += 6 * H;
    W.b5 = ((lane & 7) < 6) ? p[((lane & 7) < 6) ? (lane & 7) : 0] : R(0);   // replicated per 8-lane group
    if constexpr (sizeof(R) == 4) W.b5 = (lane < 8) ? W.b5 : R(0);            // fp32: enters out_rot once, before the row sums
}

// ------------------------------------------------------------------------------------------
// One 64x64 hidden layer: out_j = b_j + sum_k W[j][k] h_k, lane j owns row j, h_k lives in lane k.
// The four accumulators of a row-block product -- pairs (a0, a2), (a1, a3) -- summed over the four 16-lane rows and transposed
// (row t <- unit 16 t + i): two v_permlane16_swap, ONE packed add, one v_permlane32_swap, one add.
// (q0 + q1) + (q2 + q3): the order every fp32 kernel of this library uses.  Every swap reads data at least two instructions old.
// On allocator-chosen pairs (the adjoint's W^T products, hode_solve_bwd_ws.hip); mlp_hidden_blk below has the same finish on named
// registers inside its own statement.  (The four accumulators as four 32-bit operands, two swaps and two plain adds: no faster.)
__device__ __forceinline__ float blk_rows_finish(f2_t a02, f2_t a13)
{
    asm("s_nop 1\n\t"                          /* (hipcc may have just COPIED an accumulator) */
        "v_permlane16_swap_b32 %[a2], %[a3]\n\t" /* a2 = [u2.q0 u3.q0 u2.q2 u3.q2]   a3 = [u2.q1 u3.q1 u2.q3 u3.q3] */
        "v_permlane16_swap_b32 %[a0], %[a1]"      /* a0 = [u0.q0 u1.q0 u0.q2 u1.q2]   a1 = [u0.q1 u1.q1 u0.q3 u1.q3]  (three states behind the s_nop's subjects) */
        : [a0] "+v"(a02.x), [a2] "+v"(a02.y), [a1] "+v"(a13.x), [a3] "+v"(a13.y));
    asm("v_pk_add_f32 %0, %0, %1" : "+v"(a02) : "v"(a13));     // rows: u0 / u2 q0+q1, u1 / u3 q0+q1, q2+q3, q2+q3
    float a0 = a02.x, a2 = a02.y;
    asm("s_nop 1\n\tv_permlane32_swap_b32 %[a0], %[a2]\n\tv_add_f32 %[a0], %[a0], %[a2]" : [a0] "+v"(a0), [a2] "+v"(a2));
    return a0;
}

// ---- one hidden layer WITHOUT row replication (fp32, register kernel) ---------------------------------------------------------
// Lane (r, i) = lane 16 r + i keeps w[16 w + n] = W[16 w + i][16 r + ((i - n) & 15)]: accumulator a_w of the lane is the part
// of unit 16 w + i that comes from the lane's OWN 16-lane row of the activation vector, so h in its natural layout (unit per
// lane) is the DPP operand as it is.  The four accumulators are then added over the rows AND transposed -- row t <- unit
// 16 t + i -- by two v_permlane16_swap, one v_permlane32_swap and three adds (the trick of hode_solve_fwd_rows.hip inside
// one wave):   72 vector instructions per layer instead of the 75 of the row-replicated form (lab/hode_lab_layers.h), no copies, h back in the natural layout.
// The bias (natural layout: b[16 t + i] on lane (t, i)) is added behind the reduction: (q0 + q1) + (q2 + q3) + b -- the order
// every fp32 forward kernel of this library uses, so that they stay comparable bit for bit.
// Hazards: h is a VALU result (the previous layer's v_max): four plain multiplications stand before the first DPP read; every
// v_permlane*_swap reads accumulators at least two instructions old (the s_nops where nothing else fits).
// Instruction selection (round 3): per rotation n ONE v_mov_b32_dpp materialises row_ror:n(h) and TWO v_pk_fma_f32 update the
// accumulator pairs (a0, a1), (a2, a3) from the weight pairs (w0_n, w1_n), (w2_n, w3_n), both halves taking the low half of the
// moved operand (op_sel_hi:[1,0,1]) -- 47 instructions per layer instead of 64 v_fmac_f32_dpp, 12.3 against 14.7 SIMD cycles per
// rotation at two waves per SIMD (tools/ubench/inst_cost_ubench.hip: k_step_pk2 / k_step_dpp4).  Same products, same order per
// accumulator, one rounding per FMA: bit-identical to the DPP form.
// A rotation's move and its FMAs stand in ONE asm statement.  The moved operand has to be named as a 32-bit register for the
// v_mov_b32_dpp and as a 64-bit pair for the packed FMAs, which an allocator-chosen operand cannot be; as two statements (the
// layout of rounds 3-4) hipcc put its boundary pad -- one s_nop behind a statement whose output the next instruction reads --
// between every move and its FMAs: 245 of the 457 s_nops of the 1 904-instruction DP5(4) step, a quarter of a lone wave's issue
// slots.  Naming a fixed pair such as v[0:1] and declaring it CLOBBERED had been tried: hipcc then spills whatever lived there and
// reloads it, with a full vmcnt wait, inside the stage loop of the taping kernel.  A fixed register as an early-clobber OUTPUT is a
// def the allocator plans around: no fp32 instantiation of the forward, JVP, RHS or adjoint kernels gained scratch, two lost theirs.
// Measured (profiles/fwd_asm_merge_ab.log, four alternating pairs on one MI355X): step block 1 904 -> 1 569 instructions, s_nop
// 457 -> 123, vector instructions 1 438 -> 1 437; benchmark launch 2.724 -> 2.655 ms (-2.6 %), taping forward 3.21 -> 3.06 ms (-4.6 %).
// So the pads were NOT free issue slots of the SIMD's other wave -- and removing 17.6 % of a wave's instructions bought 2.6 %: the
// vector pipe of a SIMD with two resident waves is what binds, the pads cost where a wave runs alone or both waves stall.
template <bool RELU> __device__ __forceinline__ float mlp_hidden_blk(const f2_t (&wp)[kMaxH / 2], float bias, float h)
{
    // accumulator pairs (a0, a2) and (a1, a3): after the two 16-lane swaps the sums a0 + a1 and a2 + a3 are ONE packed add
    f2_t a02, a13;
    // h is a FRESH vector result (the previous layer's v_max) and a DPP read needs two wait states behind its producer.  By source
    // order alone that is not safe: a DPP move depends on h only, and when the moves were statements of their own hipcc scheduled
    // some in front of the rotation-0 products in some instantiations (RK4 x three layers x tape): stale lanes, trajectories off by
    // 1e-1, silently (found by tools/soak_tuned.py, checked by tools/dpp_hazard_check.py).  Now every DPP read of h is INSIDE a
    // string, behind at least two instructions of that string that are not DPP reads -- whatever hipcc puts in front of a statement
    // (a copy of h into its register, say) is two wait states old by then.
    // The accumulators live in v[4:7] BY NAME (constraint {v[..]} on every statement of the layer, so that the register
    // allocator keeps them there from the first product to the last swap): the finish can then swap HALVES of the pairs and add
    // the PAIRS -- 2 swaps + 1 packed add.  With allocator-chosen pairs the halves are separate operands, and hipcc wrapped the
    // swaps of two layers out of three in a copy out of a pair and back (5 instructions; tools/fwd_valu.py).  Kernels that hold
    // the weights in registers run at two waves per SIMD (256 registers), so v4..255 exist wherever this function is used.
    // The moved operand of a rotation is v8 BY NAME as well: the 32-bit v_mov_b32_dpp writes v8 and the packed FMAs read the pair
    // v[8:9], of which op_sel_hi:[1,0,1] selects the low half twice -- v9 is read and never used, whatever lives there.  The layer's
    // input sits in v[10:11], so that one register is the 32-bit source of the moves (v10) and the pair of the rotation-0 products.
    // A statement takes 30 operands, so the layer is two: rotations 0..7 + the move of rotation 8, then the FMAs of rotation 8,
    // rotations 9..15 and the finish.  The second statement so opens with two plain FMAs, not with a DPP read of v10 (hipcc did
    // reload v10 right in front of it in rhs_bwd_kernel<float, 4>); the one boundary pad of the layer falls between that move and
    // its FMAs.
    f2_t hh;
    float lo;
    hh.x = h;
#define HODE_BK_MOV(n) "v_mov_b32_dpp v8, v10 row_ror:" #n " row_mask:0xf bank_mask:0xf\n\t"
#define HODE_BK_FMA(n)                                                                                                         \
    "v_pk_fma_f32 v[4:5], %[wa" #n "], v[8:9], v[4:5] op_sel_hi:[1,0,1]\n\t"                                                    \
    "v_pk_fma_f32 v[6:7], %[wb" #n "], v[8:9], v[6:7] op_sel_hi:[1,0,1]\n\t"
#define HODE_BK_STEP(n) HODE_BK_MOV(n) HODE_BK_FMA(n)
#define HODE_BK_W(n) [wa##n] "v"(wp[2 * n]), [wb##n] "v"(wp[2 * n + 1])
    // (no pad opens the layer: the two products are the two wait states between whatever wrote v10 and its first DPP read.  The
    //  s_nop 1 that stood here until the stage trim, DESIGN.md section 4.2, was worth 1.4 % of the benchmark launch in the LDS form)
    asm("v_pk_mul_f32 v[4:5], %[wa0], v[10:11] op_sel_hi:[1,0]\n\t"
        "v_pk_mul_f32 v[6:7], %[wb0], v[10:11] op_sel_hi:[1,0]\n\t"
        HODE_BK_STEP(1) HODE_BK_STEP(2) HODE_BK_STEP(3) HODE_BK_STEP(4) HODE_BK_STEP(5) HODE_BK_STEP(6) HODE_BK_STEP(7) HODE_BK_MOV(8)
        : "=&{v[4:5]}"(a02), "=&{v[6:7]}"(a13), "=&{v8}"(lo)
        : "{v[10:11]}"(hh), HODE_BK_W(0), HODE_BK_W(1), HODE_BK_W(2), HODE_BK_W(3), HODE_BK_W(4), HODE_BK_W(5), HODE_BK_W(6),
          HODE_BK_W(7));
    // a02 = v4 (a0), v5 (a2); a13 = v6 (a1), v7 (a3).  Same sums as blk_rows_finish: (q0 + q1) + (q2 + q3) + b.  Pads: a lane swap
    // reads its operands through the cross-lane path, two wait states behind the VALU that wrote them -- v7 (the last FMA) and
    // v[4:5] (the packed add); the second 16-lane swap reads v4 / v6, which are older, and a plain VALU reads a swap's result at once.
#define HODE_BK_TAIL(RELU_TAIL)                                                                                                \
    asm(HODE_BK_FMA(8) HODE_BK_STEP(9) HODE_BK_STEP(10) HODE_BK_STEP(11) HODE_BK_STEP(12) HODE_BK_STEP(13) HODE_BK_STEP(14)   \
        HODE_BK_STEP(15)                                                                                                       \
        "s_nop 1\n\t"                                                                                                          \
        "v_permlane16_swap_b32 v5, v7\n\t"   /* a2 = [u2.q0 u3.q0 u2.q2 u3.q2]   a3 = [u2.q1 u3.q1 u2.q3 u3.q3] */             \
        "v_permlane16_swap_b32 v4, v6\n\t"   /* a0 = [u0.q0 u1.q0 u0.q2 u1.q2]   a1 = [u0.q1 u1.q1 u0.q3 u1.q3] */             \
        "v_pk_add_f32 v[4:5], v[4:5], v[6:7]\n\t"     /* rows: u0 / u2 q0+q1, u1 / u3 q0+q1, q2+q3, q2+q3 */                   \
        "s_nop 1\n\t"                                                                                                          \
        "v_permlane32_swap_b32 v4, v5\n\t"                                                                                     \
        "v_add_f32 v4, v4, v5\n\t"                                                                                             \
        "v_add_f32 v4, v4, %[bias]" RELU_TAIL                                                                                  \
        : "+{v[4:5]}"(a02), "+{v[6:7]}"(a13), "+{v8}"(lo)                                                                      \
        : "{v[10:11]}"(hh), [bias] "v"(bias), HODE_BK_W(8), HODE_BK_W(9), HODE_BK_W(10), HODE_BK_W(11), HODE_BK_W(12),         \
          HODE_BK_W(13), HODE_BK_W(14), HODE_BK_W(15))
    if constexpr (RELU) HODE_BK_TAIL("\n\tv_max_f32 v4, 0, v4");
    else HODE_BK_TAIL("");
#undef HODE_BK_TAIL
#undef HODE_BK_W
#undef HODE_BK_STEP
#undef HODE_BK_FMA
#undef HODE_BK_MOV
    return a02.x;
}
// ---- the same layer with its LAST K rotations fetched through LDS (forward solve kernels only) --------------------------------
// The 15 v_mov_b32_dpp of mlp_hidden_blk are copies on the pipe that binds the forward kernel.  Here the wave writes the layer's
// input to a private LDS buffer of 4 rows x 48 dwords (kRotBufElems; row r holds its 16 activations twice, at entries j and
// j + 16: ONE ds_write2_b32) and fetches the moved operands of rotations 16 - K .. 15 at the layer's START, two per
// ds_read2_b32 into an aligned register pair: lane (r, i) reads rotation n at entry i + 16 - n of row r, immediate offsets on
// the one per-lane address `rot` (rot_lane_addr).  Rotations 0 .. 15 - K stay DPP and hide the round trip; one
// s_waitcnt lgkmcnt(0); then the packed FMAs of rotation n take the pair's low half (op_sel_hi:[1,0,1], as with v[8:9]) and
// those of n + 1 its high half (op_sel:[0,1,0] op_sel_hi:[1,1,1]).  Same products, same weight pairs, same order per
// accumulator, same finish: the bits of mlp_hidden_blk.
// Row stride 48: inside each 32-lane group rows 0/1 and 2/3 fall on disjoint halves of the 32 banks -- no conflict, write or read.
// The wait is lgkmcnt(0): the scalar look-ahead loads of UniformInput share the counter and return out of order (they were
// issued an interval earlier).  It stands at the END of the first statement, so every fetched pair is complete before hipcc
// sees it as a value it may copy; DS operations of one wave execute in order, so nothing stands between the write and the
// reads, and the buffer is private to the wave (one wave per workgroup): no barrier.
// Registers: K / 2 pairs and the address, live through the layer.  LEAN (K = 8) lands the first two LDS rotations in v9 and
// v11 instead -- the high halves of the moved-operand pair and of the input pair, which the DPP part never selects -- by two
// ds_read_b32 (the LDS cycles of one ds_read2_b32): K = 8 for 8 registers, not 9, which is what the benchmark kernel has.
// Which instantiation takes which K: FwdRot, hode_solve_fwd.hip.
// Measured (tools/ubench/fwd_lds_rot_ubench.hip, profiles/fwd_lds_rot_ubench.log): chain form, cycles per layer and SIMD,
// K = 0 / 4 / 8 / lean 8 / 12: 285.7 / 287.5 / 282.1 / 279.3 / 271.4 at two waves per SIMD, 425.5 / 445.2 / 442.7 / 446.2 / 430.0 at
// one -- a wave that has its SIMD to itself pays for the round trip; a pair fetched a second time behind its first use (fewer registers) loses at
// both.  In the kernels (profiles/fwd_lds_rot_ab.log): benchmark launch 2.618 -> 2.547 ms (-2.7 %) with the lean K = 8, three
// layers 2.04 -> 1.96 ms with K = 12; launches of at most one wave per SIMD (B <= 1 024) +3.4 .. +4.5 %.
constexpr int kRotBufElems = 4 * 48;
// byte address of entry i of row r in the wave's buffer at LDS byte offset `base`
__device__ __forceinline__ unsigned rot_lane_addr(unsigned base, int lane) { return base + 4u * (48 * (lane >> 4) + (lane & 15)); }
template <bool RELU, int K, bool LEAN = false>
__device__ __forceinline__ float mlp_hidden_blk_lds(const f2_t (&wp)[kMaxH / 2], float bias, float h, unsigned rot)
{
    static_assert(K == 4 || K == 8 || K == 12, "K rotations through LDS: 4, 8 or 12 (0 is mlp_hidden_blk)");
    static_assert(!LEAN || K == 8, "the lean form exists for K = 8");
    f2_t a02, a13, hh;
    float lo;
    hh.x = h;
#define HODE_BL_MOV(n) "v_mov_b32_dpp v8, v10 row_ror:" #n " row_mask:0xf bank_mask:0xf\n\t"
#define HODE_BL_FMA(n)                                                                                                         \
    "v_pk_fma_f32 v[4:5], %[wa" #n "], v[8:9], v[4:5] op_sel_hi:[1,0,1]\n\t"                                                    \
    "v_pk_fma_f32 v[6:7], %[wb" #n "], v[8:9], v[6:7] op_sel_hi:[1,0,1]\n\t"
#define HODE_BL_STEP(n) HODE_BL_MOV(n) HODE_BL_FMA(n)
    // rotation n from the low half of the fetched pair q, rotation m = n + 1 from its high half
#define HODE_BL_LDS2(n, m, q)                                                                                                  \
    "v_pk_fma_f32 v[4:5], %[wa" #n "], %[" #q "], v[4:5] op_sel_hi:[1,0,1]\n\t"                                                 \
    "v_pk_fma_f32 v[6:7], %[wb" #n "], %[" #q "], v[6:7] op_sel_hi:[1,0,1]\n\t"                                                 \
    "v_pk_fma_f32 v[4:5], %[wa" #m "], %[" #q "], v[4:5] op_sel:[0,1,0] op_sel_hi:[1,1,1]\n\t"                                  \
    "v_pk_fma_f32 v[6:7], %[wb" #m "], %[" #q "], v[6:7] op_sel:[0,1,0] op_sel_hi:[1,1,1]\n\t"
#define HODE_BL_WR "ds_write2_b32 %[ad], v10, v10 offset1:16\n\t"
#define HODE_BL_RD(q, o0, o1) "ds_read2_b32 %[" #q "], %[ad] offset0:" #o0 " offset1:" #o1 "\n\t"
#define HODE_BL_WAIT "s_waitcnt lgkmcnt(0)\n\t"
    // (two plain products stand between the layer's producer and the first DPP read of v10, as in mlp_hidden_blk)
#define HODE_BL_HEAD                                                                                                           \
    "v_pk_mul_f32 v[4:5], %[wa0], v[10:11] op_sel_hi:[1,0]\n\t"                                                                \
    "v_pk_mul_f32 v[6:7], %[wb0], v[10:11] op_sel_hi:[1,0]\n\t"
#define HODE_BL_FINISH                                                                                                         \
    "s_nop 1\n\t"                                                                                                              \
    "v_permlane16_swap_b32 v5, v7\n\t"                                                                                         \
    "v_permlane16_swap_b32 v4, v6\n\t"                                                                                         \
    "v_pk_add_f32 v[4:5], v[4:5], v[6:7]\n\t"                                                                                  \
    "s_nop 1\n\t"                                                                                                              \
    "v_permlane32_swap_b32 v4, v5\n\t"                                                                                         \
    "v_add_f32 v4, v4, v5\n\t"
    // The finish's LAST instruction writes v10 and the function returns the low half of the input pair, a read-write operand of the
    // tail statement: the result stands where the next layer's {v[10:11]} takes its input -- no v_mov_b64 v[10:11], v[4:5] and no
    // boundary pad between two layers (12 + 12 per DP5(4) step).  Here only: the same in mlp_hidden_blk put 12 B of scratch into
    // rhs_bwd_kernel<float, 4>.
#define HODE_BL_END_RELU "v_add_f32 v4, v4, %[bias]\n\tv_max_f32 v10, 0, v4"
#define HODE_BL_END_LIN "v_add_f32 v10, v4, %[bias]"
#define HODE_BL_W(n) [wa##n] "v"(wp[2 * n]), [wb##n] "v"(wp[2 * n + 1])
#define HODE_BL_OUT1 "=&{v[4:5]}"(a02), "=&{v[6:7]}"(a13), "=&{v8}"(lo)
#define HODE_BL_IO2 "+{v[4:5]}"(a02), "+{v[6:7]}"(a13), "+{v8}"(lo), "+{v[10:11]}"(hh)
#define HODE_BL_IN1 "{v[10:11]}"(hh), [ad] "v"(rot)
#define HODE_BL_IN2 [bias] "v"(bias)
#define HODE_BL_Q(q) [q] "=&v"(q)
#define HODE_BL_QI(q) [q] "v"(q)
    // one rotation from the HIGH half of the named pair p (v[8:9] or v[10:11]: the lean form fetches into v9 and v11)
#define HODE_BL_HI(n, p)                                                                                                       \
    "v_pk_fma_f32 v[4:5], %[wa" #n "], " p ", v[4:5] op_sel:[0,1,0] op_sel_hi:[1,1,1]\n\t"                                      \
    "v_pk_fma_f32 v[6:7], %[wb" #n "], " p ", v[6:7] op_sel:[0,1,0] op_sel_hi:[1,1,1]\n\t"
    if constexpr (LEAN) {
        // The first two LDS rotations land in v9 and v11, the high halves of the moved-operand pair and of the input pair that no
        // instruction of the DPP part uses (both forms read their low halves only): two rotations for ONE more register (v9; v11
        // is the input pair's own), each by a ds_read_b32 -- 2 + 2 LDS cycles, what one ds_read2_b32 costs.
        f2_t lo2, q0, q1, q2;
        asm(HODE_BL_WR "ds_read_b32 v9, %[ad] offset:32\n\tds_read_b32 v11, %[ad] offset:28\n\t" HODE_BL_RD(q0, 6, 5) HODE_BL_RD(q1, 4, 3)
            HODE_BL_RD(q2, 2, 1) HODE_BL_HEAD HODE_BL_STEP(1) HODE_BL_STEP(2) HODE_BL_STEP(3) HODE_BL_STEP(4) HODE_BL_STEP(5) HODE_BL_STEP(6)
            HODE_BL_STEP(7) HODE_BL_WAIT
            : "=&{v[4:5]}"(a02), "=&{v[6:7]}"(a13), "=&{v[8:9]}"(lo2), "+{v[10:11]}"(hh), HODE_BL_Q(q0), HODE_BL_Q(q1), HODE_BL_Q(q2)
            : [ad] "v"(rot), HODE_BL_W(0), HODE_BL_W(1), HODE_BL_W(2), HODE_BL_W(3), HODE_BL_W(4), HODE_BL_W(5), HODE_BL_W(6), HODE_BL_W(7));
#define HODE_BL_TAIL(RELU_TAIL)                                                                                                \
        asm(HODE_BL_HI(8, "v[8:9]") HODE_BL_HI(9, "v[10:11]") HODE_BL_LDS2(10, 11, q0) HODE_BL_LDS2(12, 13, q1) HODE_BL_LDS2(14, 15, q2) \
            HODE_BL_FINISH RELU_TAIL                                                                                        \
            : "+{v[4:5]}"(a02), "+{v[6:7]}"(a13), "+{v[10:11]}"(hh)                                                         \
            : "{v[8:9]}"(lo2), [bias] "v"(bias), HODE_BL_QI(q0), HODE_BL_QI(q1), HODE_BL_QI(q2), HODE_BL_W(8),      \
              HODE_BL_W(9), HODE_BL_W(10), HODE_BL_W(11), HODE_BL_W(12), HODE_BL_W(13), HODE_BL_W(14), HODE_BL_W(15))
        if constexpr (RELU) HODE_BL_TAIL(HODE_BL_END_RELU);
        else HODE_BL_TAIL(HODE_BL_END_LIN);
#undef HODE_BL_TAIL
    } else if constexpr (K == 4) {
        f2_t q0, q1;
        asm(HODE_BL_WR HODE_BL_RD(q0, 4, 3) HODE_BL_RD(q1, 2, 1) HODE_BL_HEAD
            HODE_BL_STEP(1) HODE_BL_STEP(2) HODE_BL_STEP(3) HODE_BL_STEP(4) HODE_BL_STEP(5) HODE_BL_STEP(6) HODE_BL_STEP(7) HODE_BL_STEP(8)
            HODE_BL_STEP(9) HODE_BL_STEP(10) HODE_BL_MOV(11) HODE_BL_WAIT
            : HODE_BL_OUT1, HODE_BL_Q(q0), HODE_BL_Q(q1)
            : HODE_BL_IN1, HODE_BL_W(0), HODE_BL_W(1), HODE_BL_W(2), HODE_BL_W(3), HODE_BL_W(4), HODE_BL_W(5), HODE_BL_W(6), HODE_BL_W(7),
              HODE_BL_W(8), HODE_BL_W(9), HODE_BL_W(10));
#define HODE_BL_TAIL(RELU_TAIL)                                                                                                \
        asm(HODE_BL_FMA(11) HODE_BL_LDS2(12, 13, q0) HODE_BL_LDS2(14, 15, q1) HODE_BL_FINISH RELU_TAIL                         \
            : HODE_BL_IO2                                                                                                      \
            : HODE_BL_IN2, HODE_BL_QI(q0), HODE_BL_QI(q1), HODE_BL_W(11), HODE_BL_W(12), HODE_BL_W(13), HODE_BL_W(14), HODE_BL_W(15))
        if constexpr (RELU) HODE_BL_TAIL(HODE_BL_END_RELU);
        else HODE_BL_TAIL(HODE_BL_END_LIN);
#undef HODE_BL_TAIL
    } else if constexpr (K == 8) {
        f2_t q0, q1, q2, q3;
        asm(HODE_BL_WR HODE_BL_RD(q0, 8, 7) HODE_BL_RD(q1, 6, 5) HODE_BL_RD(q2, 4, 3) HODE_BL_RD(q3, 2, 1) HODE_BL_HEAD
            HODE_BL_STEP(1) HODE_BL_STEP(2) HODE_BL_STEP(3) HODE_BL_STEP(4) HODE_BL_STEP(5) HODE_BL_STEP(6) HODE_BL_STEP(7) HODE_BL_WAIT
            : HODE_BL_OUT1, HODE_BL_Q(q0), HODE_BL_Q(q1), HODE_BL_Q(q2), HODE_BL_Q(q3)
            : HODE_BL_IN1, HODE_BL_W(0), HODE_BL_W(1), HODE_BL_W(2), HODE_BL_W(3), HODE_BL_W(4), HODE_BL_W(5), HODE_BL_W(6), HODE_BL_W(7));
#define HODE_BL_TAIL(RELU_TAIL)                                                                                                \
        asm(HODE_BL_LDS2(8, 9, q0) HODE_BL_LDS2(10, 11, q1) HODE_BL_LDS2(12, 13, q2) HODE_BL_LDS2(14, 15, q3) HODE_BL_FINISH RELU_TAIL \
            : HODE_BL_IO2                                                                                                      \
            : HODE_BL_IN2, HODE_BL_QI(q0), HODE_BL_QI(q1), HODE_BL_QI(q2), HODE_BL_QI(q3), HODE_BL_W(8), HODE_BL_W(9), HODE_BL_W(10),  \
              HODE_BL_W(11), HODE_BL_W(12), HODE_BL_W(13), HODE_BL_W(14), HODE_BL_W(15))
        if constexpr (RELU) HODE_BL_TAIL(HODE_BL_END_RELU);
        else HODE_BL_TAIL(HODE_BL_END_LIN);
#undef HODE_BL_TAIL
    } else {
        f2_t q0, q1, q2, q3, q4, q5;
        asm(HODE_BL_WR HODE_BL_RD(q0, 12, 11) HODE_BL_RD(q1, 10, 9) HODE_BL_RD(q2, 8, 7) HODE_BL_RD(q3, 6, 5) HODE_BL_RD(q4, 4, 3)
            HODE_BL_RD(q5, 2, 1) HODE_BL_HEAD HODE_BL_STEP(1) HODE_BL_STEP(2) HODE_BL_STEP(3) HODE_BL_WAIT
            HODE_BL_LDS2(4, 5, q0) HODE_BL_LDS2(6, 7, q1)
            : HODE_BL_OUT1, HODE_BL_Q(q0), HODE_BL_Q(q1), HODE_BL_Q(q2), HODE_BL_Q(q3), HODE_BL_Q(q4), HODE_BL_Q(q5)
            : HODE_BL_IN1, HODE_BL_W(0), HODE_BL_W(1), HODE_BL_W(2), HODE_BL_W(3), HODE_BL_W(4), HODE_BL_W(5), HODE_BL_W(6), HODE_BL_W(7));
#define HODE_BL_TAIL(RELU_TAIL)                                                                                                \
        asm(HODE_BL_LDS2(8, 9, q2) HODE_BL_LDS2(10, 11, q3) HODE_BL_LDS2(12, 13, q4) HODE_BL_LDS2(14, 15, q5) HODE_BL_FINISH RELU_TAIL \
            : HODE_BL_IO2                                                                                                      \
            : HODE_BL_IN2, HODE_BL_QI(q2), HODE_BL_QI(q3), HODE_BL_QI(q4), HODE_BL_QI(q5), HODE_BL_W(8), HODE_BL_W(9), HODE_BL_W(10),  \
              HODE_BL_W(11), HODE_BL_W(12), HODE_BL_W(13), HODE_BL_W(14), HODE_BL_W(15))
        if constexpr (RELU) HODE_BL_TAIL(HODE_BL_END_RELU);
        else HODE_BL_TAIL(HODE_BL_END_LIN);
#undef HODE_BL_TAIL
    }
#undef HODE_BL_HI
#undef HODE_BL_QI
#undef HODE_BL_Q
#undef HODE_BL_IN2
#undef HODE_BL_IN1
#undef HODE_BL_IO2
#undef HODE_BL_OUT1
#undef HODE_BL_W
#undef HODE_BL_FINISH
#undef HODE_BL_END_RELU
#undef HODE_BL_END_LIN
#undef HODE_BL_HEAD
#undef HODE_BL_WAIT
#undef HODE_BL_RD
#undef HODE_BL_WR
#undef HODE_BL_LDS2
#undef HODE_BL_STEP
#undef HODE_BL_FMA
#undef HODE_BL_MOV
    return hh.x;
}
// The forward solve kernels' weight holder: MlpRegs whose hidden layers take the hybrid form (mlp_load and RhsRegs see an MlpRegs)
template <int NL, int K, bool LEAN = false> struct MlpRegsRot : MlpRegs<float, NL> {
    // the kernels that had the registers for this layer have the aligned pairs of the packed mechanistic terms too (mech_eval<R, PACK>,
    // hode_rhs_eval.h); the K = 0 instantiations do not: the taping DP5(4) kernel answers the packed form with 12 B of scratch
    static constexpr bool kPackMech = true;
    unsigned rot;                     // rot_lane_addr of the wave's buffer
    __device__ __forceinline__ float hidden(int l, float h) const { return mlp_hidden_blk_lds<false, K, LEAN>(this->wh[l], this->b[l + 1], h, rot); }
    __device__ __forceinline__ float hidden_relu(int l, float h) const { return mlp_hidden_blk_lds<true, K, LEAN>(this->wh[l], this->b[l + 1], h, rot); }
};
// ---- fp64 (parity runs): natural weight order, v_readlane broadcast (no 64-bit DPP FMA) ------------------------------------------
__device__ __forceinline__ double mlp_hidden_relu(const double (&w)[kMaxH], double bias, double h)
{
    const double v = mlp_hidden(w, bias, h);
    return v > 0.0 ? v : 0.0;
}
__device__ __forceinline__ double mlp_hidden(const double (&w)[kMaxH], double bias, double h)
{
    double acc0 = bias, acc1 = 0.0;
#pragma unroll
    for (int k = 0; k < kMaxH; k += 2) {
        acc0 = rfma(w[k], lane_bcast(h, k), acc0);
        acc1 = rfma(w[k + 1], lane_bcast(h, k + 1), acc1);
    }
    return acc0 + acc1;
}

// Activations kept by the backward pass: h[l] = relu output of hidden layer l+1 on lane j.
template <typename R, int NL> struct MlpActs {
    R h[NL];
    __device__ __forceinline__ void put(int l, R v) { h[l] = v; }
};
// ... or written straight to the stage record (row l of 64 reals) the moment a layer is done: the forward solve with a tape
// has no register to hold four rows until the end of the evaluation
template <typename R> struct ActsToRecord {
    R *__restrict__ dst;                  // record + lane
    __device__ __forceinline__ void put(int l, R v) { dst[l * kWave] = v; }
};

// the output layer of out_rot_fill: 1 v_mul + 7 v_fmac_f32_dpp on h (natural layout; the s_nop gives the DPP read of h its
// second wait state after the v_max that produced it), the row_ror:8 add of the two half sums, the all-reduce over the rows.
// (The partner row (lane ^ 16) through ds_swizzle_b32 instead of the copy + v_permlane16_swap saves two vector instructions per
// right-hand side and measured 1.5 % slower: its latency sits on the stage's dependent chain)
__device__ __forceinline__ float out_rot(const float (&w)[8], float b5m, float h)
{
    float a, t;
#define HODE_OR(n) "v_fmac_f32_dpp %[a], %[h], %[w" #n "] row_ror:" #n " row_mask:0xf bank_mask:0xf\n\t"
    asm("v_fma_f32 %[a], %[h], %[w0], %[b]\n\t"     // b = bout[o] on lanes 0..7 only: it passes the reductions once
        "s_nop 0\n\t"
        HODE_OR(1) HODE_OR(2) HODE_OR(3) HODE_OR(4) HODE_OR(5) HODE_OR(6) HODE_OR(7)
        "s_nop 1\n\t"
        "v_add_f32_dpp %[a], %[a], %[a] row_ror:8 row_mask:0xf bank_mask:0xf\n\t"
        "v_mov_b32 %[t], %[a]\n\t"
        "s_nop 1\n\t"
        "v_permlane16_swap_b32 %[a], %[t]\n\t"       // a = [r0 r0 r2 r2], t = [r1 r1 r3 r3]
        "v_add_f32 %[a], %[a], %[t]\n\t"             // [r0+r1 x2, r2+r3 x2]
        "v_mov_b32 %[t], %[a]\n\t"
        "s_nop 1\n\t"
        "v_permlane32_swap_b32 %[a], %[t]\n\t"       // a = [r0+r1 x4], t = [r2+r3 x4]
        "v_add_f32 %[a], %[a], %[t]"
        : [a] "=&v"(a), [t] "=&v"(t)
        : [h] "v"(h), [b] "v"(b5m), [w0] "v"(w[0]), [w1] "v"(w[1]), [w2] "v"(w[2]), [w3] "v"(w[3]), [w4] "v"(w[4]), [w5] "v"(w[5]),
          [w6] "v"(w[6]), [w7] "v"(w[7]));
#undef HODE_OR
    return a;
}

}  // namespace hode

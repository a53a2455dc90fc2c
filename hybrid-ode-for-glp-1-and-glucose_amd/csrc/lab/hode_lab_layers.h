// lab/hode_lab_layers.h -- device code that only the lab library instantiates: the edge-parameter loader of
// the lab forward kernels, and the layer forms on ROW-REPLICATED activations -- the 64-FMA hidden layer as one asm statement, the
// workgroup-shared LDS image of the hidden matrices, the fp32 outer-product accumulation one instruction at a time, and the
// transposed matrices in registers.
// Used by: lab/hode_solve_fwd_{wg,quad,rows}.hip (mlp_load_edges; wg: MlpLds), lab/hode_solve_bwd_split.hip (WtRegs,
// mlp_outer_step), and hode_adjoint.h when it is compiled with -DHODE_LAB (hode_solve_bwd.hip's WTREG instantiations,
// HODE_BWD_WT=regs).
#pragma once
#include "../hode_mlp.h"

namespace hode {

// first / last layer weights and all biases ("edge" parameters) of one parameter set -> registers of lane j, for the
// weight holders of the lab forward kernels that keep their hidden matrices elsewhere (mlp_load, hode_mlp.h, loads an MlpRegs whole)
template <typename R, int NL, typename WT>
__device__ __forceinline__ void mlp_load_edges(WT &W, const R *__restrict__ p, int H, int lane)
{
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

// One 64x64 hidden layer on replicated rows: out_j = b_j + sum_k W[j][k] h_k, lane j owns row j, h_k lives in lane k.
//        The four 16-lane rows of h are first replicated to every row (1 v_permlane16_swap +
//        2 v_permlane32_swap), then each FMA takes its activation through a DPP row_ror:n operand
//        (lane i reads lane (i-n)&15 of its row): 64 v_fmac_f32_dpp + ~8 instead of 64 v_readlane +
//        32 v_pk_fma.  Four independent accumulators.
// ---- one hidden layer as ONE asm statement (fp32, weights in registers) ----------------------------------------------------
// Written as 64 separate asm statements hipcc's hazard recognizer puts an s_nop between any two of them that touch the same
// register (it assumes an opaque asm may have the dst_sel forwarding hazard and does not count other asm statements as wait
// states): one s_nop per four FMAs, ~50 per right-hand side.  As one statement the layer is 75 instructions instead of 94
// (measured: neutral for the forward, -1 % for forward-with-tape and adjoint -- at two waves per SIMD an s_nop of one wave is
// an issue slot of the other):
//     v_mov + s_nop 1 + v_permlane16_swap, 2 v_mov + s_nop 0 + 2 v_permlane32_swap     rows of h replicated (rows_replicate)
//     v_fma + 3 v_mul                                                                  rotation 0, bias folded in
//     60 v_fmac_f32_dpp                                                                rotations 1..15
//     3 v_add                                                                          (a0 + a1) + (a2 + a3)
// Hazards (the compiler pads nothing inside an asm): a VALU result needs 2 wait states before a v_permlane*_swap reads it
// (the s_nops, as hipcc emits them for the builtins) and before a DPP operand reads it (the four rotation-0 instructions
// stand between the swaps and the first DPP read); accumulators and weights are ordinary interlocked operands.
#define HODE_MV_ROW(n) \
    "v_fmac_f32_dpp %[a0], %[r0], %[w0_" #n "] row_ror:" #n " row_mask:0xf bank_mask:0xf\n\t" \
    "v_fmac_f32_dpp %[a1], %[r1], %[w1_" #n "] row_ror:" #n " row_mask:0xf bank_mask:0xf\n\t" \
    "v_fmac_f32_dpp %[a2], %[r2], %[w2_" #n "] row_ror:" #n " row_mask:0xf bank_mask:0xf\n\t" \
    "v_fmac_f32_dpp %[a3], %[r3], %[w3_" #n "] row_ror:" #n " row_mask:0xf bank_mask:0xf\n\t"
#define HODE_MV_ROWS_1_15 \
    HODE_MV_ROW(1) HODE_MV_ROW(2) HODE_MV_ROW(3) HODE_MV_ROW(4) HODE_MV_ROW(5) HODE_MV_ROW(6) HODE_MV_ROW(7) HODE_MV_ROW(8) \
    HODE_MV_ROW(9) HODE_MV_ROW(10) HODE_MV_ROW(11) HODE_MV_ROW(12) HODE_MV_ROW(13) HODE_MV_ROW(14) HODE_MV_ROW(15)
#define HODE_MV_W(n) [w0_##n] "v"(w[n]), [w1_##n] "v"(w[16 + n]), [w2_##n] "v"(w[32 + n]), [w3_##n] "v"(w[48 + n])
#define HODE_MV_WEIGHTS \
    HODE_MV_W(0), HODE_MV_W(1), HODE_MV_W(2), HODE_MV_W(3), HODE_MV_W(4), HODE_MV_W(5), HODE_MV_W(6), HODE_MV_W(7), HODE_MV_W(8), \
    HODE_MV_W(9), HODE_MV_W(10), HODE_MV_W(11), HODE_MV_W(12), HODE_MV_W(13), HODE_MV_W(14), HODE_MV_W(15)
// bias + sum_k W[j][k] h_k with w[16 q + n] on lane j = W[j][16 q + ((j - n) & 15)]
__device__ __forceinline__ float mlp_hidden(const float (&w)[kMaxH], float bias, float h)
{
    float r0 = h, r1, r2, r3, a0, a1, a2, a3;
    asm("v_mov_b32 %[r1], %[r0]\n\t"
        "s_nop 1\n\t"
        "v_permlane16_swap_b32 %[r0], %[r1]\n\t" /* r0 = [h0 h0 h2 h2]   r1 = [h1 h1 h3 h3]   (16-lane rows of h) */
        "v_mov_b32 %[r2], %[r0]\n\t"
        "v_mov_b32 %[r3], %[r1]\n\t"
        "s_nop 0\n\t"
        "v_permlane32_swap_b32 %[r0], %[r2]\n\t" /* r0 = h0 x 4, r2 = h2 x 4 */
        "v_permlane32_swap_b32 %[r1], %[r3]\n\t" /* r1 = h1 x 4, r3 = h3 x 4 */
        "v_mul_f32 %[a0], %[r0], %[w0_0]\n\t"
        "v_mul_f32 %[a1], %[r1], %[w1_0]\n\t"
        "v_mul_f32 %[a2], %[r2], %[w2_0]\n\t"
        "v_mul_f32 %[a3], %[r3], %[w3_0]\n\t"
        HODE_MV_ROWS_1_15
        "v_add_f32 %[a0], %[a0], %[a1]\n\t"
        "v_add_f32 %[a2], %[a2], %[a3]\n\t"
        "v_add_f32 %[a0], %[a0], %[a2]\n\t"
        "v_add_f32 %[a0], %[a0], %[bias]"
        : [r0] "+v"(r0), [r1] "=&v"(r1), [r2] "=&v"(r2), [r3] "=&v"(r3), [a0] "=&v"(a0), [a1] "=&v"(a1), [a2] "=&v"(a2),
          [a3] "=&v"(a3)
        : [bias] "v"(bias), HODE_MV_WEIGHTS);
    return a0;
}
// acc[q] += sum_n row_ror:n(R[q]) * w[16 q + n], n ascending within each accumulator; R[] must be two wait states old
__device__ __forceinline__ void rot_matvec64(const float (&w)[kMaxH], const float (&R)[4], float (&acc)[4])
{
    asm("v_fmac_f32 %[a0], %[r0], %[w0_0]\n\tv_fmac_f32 %[a1], %[r1], %[w1_0]\n\t"
        "v_fmac_f32 %[a2], %[r2], %[w2_0]\n\tv_fmac_f32 %[a3], %[r3], %[w3_0]\n\t"
        HODE_MV_ROWS_1_15
        : [a0] "+v"(acc[0]), [a1] "+v"(acc[1]), [a2] "+v"(acc[2]), [a3] "+v"(acc[3])
        : [r0] "v"(R[0]), [r1] "v"(R[1]), [r2] "v"(R[2]), [r3] "v"(R[3]), HODE_MV_WEIGHTS);
}
#undef HODE_MV_ROW
#undef HODE_MV_ROWS_1_15
#undef HODE_MV_W
#undef HODE_MV_WEIGHTS

// ---- hidden matrices in a workgroup-shared LDS image (forward solve, fp32) ---------------------------------------
// 211 weight registers per wave cap the register-resident forward kernel at 2 waves per SIMD, where the ~200 plain
// (2-cycle) VALU instructions of the per-RHS fixed part cannot overlap: one wave issues at most one VALU per 4 cycles.
// The image keeps the SAME rotating-operand order, four weights per 16-byte word:
//     img[l][n][lane j] = { W_l[j][16 q + ((j - n) & 15)] : q = 0..3 }          (n = 0..15)
// i.e. exactly the operands of FMA group n of mlp_hidden_step, so the arithmetic (and its order) is bit-identical to the
// register kernel; a layer is 16 conflict-free ds_read_b128 + 64 v_fmac_f32_dpp.  NREG of the NL-1 matrices may still be
// copied to registers (fewer LDS reads, fewer waves): the LDS pipe moves 256 B/clk per CU, four SIMDs of DPP FMAs
// fed from LDS alone would ask for 244 B/clk.
constexpr int kImgVec = 16 * kWave;                     // float4 words per hidden matrix
__device__ __forceinline__ void wimg_store(float *__restrict__ img, const float *__restrict__ nn_p, int H, int NLm1, int tid,
                                           int nthreads)
{
    const float *Wl = nn_p + 9 * H + H;
    for (int l = 0; l < NLm1; ++l) {
        for (int i = tid; i < kMaxH * kMaxH; i += nthreads) {
            const int q = i & 3, j = (i >> 2) & 63, n = i >> 8;
            const int col = 16 * q + ((j - n) & 15);
            img[(size_t)l * kMaxH * kMaxH + i] = (j < H && col < H) ? Wl[(size_t)j * H + col] : 0.f;
        }
        Wl += (size_t)H * H + H;
    }
}
template <int N>
__device__ __forceinline__ void mlp_hidden_lds_step(const float4 *__restrict__ img, int lane, const float (&R)[4], float (&acc)[4])
{
    const float4 w = img[N * kWave + lane];
    acc[0] = fmac_ror<N>(acc[0], R[0], w.x);
    acc[1] = fmac_ror<N>(acc[1], R[1], w.y);
    acc[2] = fmac_ror<N>(acc[2], R[2], w.z);
    acc[3] = fmac_ror<N>(acc[3], R[3], w.w);
    if constexpr (N < 15) mlp_hidden_lds_step<N + 1>(img, lane, R, acc);
}
__device__ __forceinline__ float mlp_hidden_lds(const float4 *__restrict__ img, int lane, float bias, float h)
{
    float R[4];
    rows_replicate(h, R);
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    mlp_hidden_lds_step<0>(img, lane, R, acc);
    return ((acc[0] + acc[1]) + (acc[2] + acc[3])) + bias;      // bias last: the order of every fp32 forward kernel
}
template <int NL, int NREG> struct MlpLds {
    static_assert(NREG >= 0 && NREG <= ((NL > 1) ? NL - 1 : 0), "NREG counts hidden matrices");
    float w1[9];
    float w1g;
    float b[NL];
    float w5[6];
    float w5r[8];
    float b5;
    float whr[(NREG > 0) ? NREG : 1][kMaxH];      // the first NREG hidden matrices, register-resident
    const float4 *img;                            // all NL-1 matrices (LDS)
    int lane;
    __device__ __forceinline__ void load_regs()
    {
#pragma unroll
        for (int l = 0; l < NREG; ++l)
#pragma unroll
            for (int n = 0; n < 16; ++n) {
                const float4 w = img[(l * 16 + n) * kWave + lane];
                whr[l][n] = w.x; whr[l][16 + n] = w.y; whr[l][32 + n] = w.z; whr[l][48 + n] = w.w;
            }
    }
    __device__ __forceinline__ float hidden(int l, float h) const
    {
        if (l < NREG) return mlp_hidden(whr[(l < NREG) ? l : 0], b[l + 1], h);
        return mlp_hidden_lds(img + (size_t)l * kImgVec, lane, b[l + 1], h);
    }
};

// dW[j][k] += d_j * h_k in the register order of the weights (rotated)
template <int N> __device__ __forceinline__ void mlp_outer_step(float (&gw)[kMaxH], float d, const float (&R)[4])
{
    gw[0 * 16 + N] = fmac_ror<N>(gw[0 * 16 + N], R[0], d);
    gw[1 * 16 + N] = fmac_ror<N>(gw[1 * 16 + N], R[1], d);
    gw[2 * 16 + N] = fmac_ror<N>(gw[2 * 16 + N], R[2], d);
    gw[3 * 16 + N] = fmac_ror<N>(gw[3 * 16 + N], R[3], d);
    if constexpr (N < 15) mlp_outer_step<N + 1>(gw, d, R);
}
__device__ __forceinline__ void mlp_outer_acc(float (&gw)[kMaxH], float d, float hin)
{
    float R[4];
    rows_replicate(hin, R);
    mlp_outer_step<0>(gw, d, R);
}

// The transposed hidden matrices of the adjoint's delta propagation in 64 more registers per matrix, in the same rotating-operand
// order as the LDS image of hode_adjoint.h (WtLds): 1 wave/SIMD, no memory wait inside the 64-FMA loop; fp32 only
template <int NL> struct WtRegs {
    float w[(NL > 1) ? NL - 1 : 1][kMaxH];     // w[l][16q+n] on lane k = W_l[16q + ((k - n) & 15)][k]
    __device__ __forceinline__ void load(const float *__restrict__ nn_p, int H, int lane)
    {
        const float *Wl = nn_p + 9 * H + H;
#pragma unroll
        for (int l = 0; l < NL - 1; ++l) {
#pragma unroll
            for (int r = 0; r < kMaxH; ++r) {
                const int j = (r & 48) | ((lane - r) & 15);
                const bool in = (j < H) && (lane < H);
                w[l][r] = in ? Wl[(size_t)(in ? j : 0) * H + (in ? lane : 0)] : 0.f;
            }
            Wl += (size_t)H * H + H;
        }
    }
    __device__ __forceinline__ float mul(int l, int lane, float d) const
    {
        (void)lane;
        float Rr[4];
        rows_replicate(d, Rr);
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        // l is a compile-time constant at every call site (unrolled layer loop)
        rot_matvec64(w[l], Rr, acc);
        return (acc[0] + acc[1]) + (acc[2] + acc[3]);
    }
};

}  // namespace hode

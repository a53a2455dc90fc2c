// hode_adjoint.h -- backward (VJP) building blocks of the tuned path: the transposed-matrix LDS image and its products, one hidden
// layer backward, the edge-parameter policies and flushes, mech_vjp, input_vjp, rhs_vjp.
// Used by: hode_solve_bwd.hip (K4 adjoint, K5 RHS backward), hode_solve_bwd_ws.hip, hode_generic_vjp.h and
// hode_generic_bwd_multi.hip (mech_vjp, input_vjp), lab/hode_solve_bwd_split.hip.  No forward kernel includes it.
#pragma once
#include "hode_rhs_eval.h"
#ifdef HODE_LAB
#include "lab/hode_lab_layers.h"     // WtRegs and the fp32 mlp_outer_acc that layer_bwd reaches with it (HODE_BWD_WT=regs)
#endif

namespace hode {

// The fp32 gradient accumulators of a hidden matrix use the "rotating operand" order of fmac_ror (hode_xlane.h): register
// r = 16q + n of lane j holds dW_l[j][16q + ((j - n) & 15)], so that the activation can be fetched with a DPP row_ror:n operand of
// the FMA itself instead of a v_readlane per element.  fp64 keeps the natural order (readlane path).
template <typename R> __device__ __forceinline__ int wcol(int r, int lane)
{
    if constexpr (sizeof(R) == 4) return (r & 48) | ((lane - r) & 15);
    else return r;
}

// dW[j][k] += d_j * h_k in the register order of the accumulators.  fp64 form; the fp32 form one instruction at a time is
// lab/hode_lab_layers.h (the product kernels interleave it with the W^T product: layer_bwd_group)
__device__ __forceinline__ void mlp_outer_acc(double (&gw)[kMaxH], double d, double hin)
{
#pragma unroll
    for (int k = 0; k < kMaxH; ++k) gw[k] = rfma(d, lane_bcast(hin, k), gw[k]);
}

// LDS image of the TRANSPOSED hidden matrices in "rotating operand" order (shared by a workgroup):
//   wt[l][r >> 2][k][r & 3] = W_l[ (r & 48) | ((k - r) & 15) ][k]        r = 16q + n, k = lane
// so that delta_{l-1}[k] = sum_j W_l[j][k] delta_l[j] becomes, on lane k,
//   sum_r  row_ror:n( rows-replicated delta_l )[k] * wt[l][r][k]
// i.e. 64 v_fmac_f32_dpp fed by 16 conflict-free 16-byte LDS reads per layer (fp32).  The fp64
// instantiation (parity runs) uses the same image with v_readlane broadcasts.
template <typename R>
__device__ __forceinline__ void wt_rot_store(R *__restrict__ wt, const R *__restrict__ nn_p, int H, int NLm1, int tid,
                                             int nthreads)
{
    const R *Wl = nn_p + 9 * H + H;
    for (int l = 0; l < NLm1; ++l) {
        for (int i = tid; i < kMaxH * kMaxH; i += nthreads) {
            const int r = ((i >> 8) << 2) | (i & 3), k = (i >> 2) & 63;
            const int j = (r & 48) | ((k - r) & 15);
            wt[(size_t)l * kMaxH * kMaxH + i] = (j < H && k < H) ? Wl[(size_t)j * H + k] : R(0);
        }
        Wl += (size_t)H * H + H;
    }
}

template <typename R> struct alignas(sizeof(R) * 4) Vec4 { R v[4]; };

// delta_prev = W^T delta for one hidden layer from the LDS image above
template <int RR> __device__ __forceinline__ void wt_mul_step(const Vec4<float> *__restrict__ wt4, int lane, const float (&Rr)[4],
                                                              float (&acc)[4])
{
    const Vec4<float> w = wt4[RR * kMaxH + lane];
    constexpr int q = RR >> 2, n0 = (RR & 3) * 4;
    acc[0] = fmac_ror<n0 + 0>(acc[0], Rr[q], w.v[0]);
    acc[1] = fmac_ror<n0 + 1>(acc[1], Rr[q], w.v[1]);
    acc[2] = fmac_ror<n0 + 2>(acc[2], Rr[q], w.v[2]);
    acc[3] = fmac_ror<n0 + 3>(acc[3], Rr[q], w.v[3]);
    if constexpr ((RR & 3) == 3) __builtin_amdgcn_sched_barrier(0);     // keep at most 4 LDS reads hoisted
    if constexpr (RR < 15) wt_mul_step<RR + 1>(wt4, lane, Rr, acc);
}
__device__ __forceinline__ float wt_mul(const float *__restrict__ wt, int lane, float d)
{
    float Rr[4];
    rows_replicate(d, Rr);
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    wt_mul_step<0>(reinterpret_cast<const Vec4<float> *>(wt), lane, Rr, acc);
    return (acc[0] + acc[1]) + (acc[2] + acc[3]);
}
__device__ __forceinline__ double wt_mul(const double *__restrict__ wt, int lane, double d)
{
    const Vec4<double> *wt4 = reinterpret_cast<const Vec4<double> *>(wt);
    double acc0 = 0.0, acc1 = 0.0;
#pragma unroll 2
    for (int rr = 0; rr < kMaxH / 4; ++rr) {
        const Vec4<double> w = wt4[rr * kMaxH + lane];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int r = 4 * rr + c;
            const int j = (r & 48) | ((lane - r) & 15);            // the lane whose delta this entry multiplies
            const double dj = __shfl(d, j);
            if (c & 1) acc1 = rfma(w.v[c], dj, acc1); else acc0 = rfma(w.v[c], dj, acc0);
        }
    }
    return acc0 + acc1;
}

// Where the transposed hidden matrices live for the delta propagation:
//   WtLds  : the LDS image above (2 waves/SIMD fit, every group of 4 reads is an LDS-latency wait)
//   WtRegs : 64 more registers per hidden matrix in the same rotating-operand order (1 wave/SIMD,
//            no memory wait inside the 64-FMA loop); fp32 only.  Lab library only (lab/hode_lab_layers.h, HODE_BWD_WT=regs):
//            the product kernels name it in a conditional_t and never take it
template <typename R> struct WtLds {
    const R *wt;
    __device__ __forceinline__ R mul(int l, int lane, R d) const { return wt_mul(wt + (size_t)l * kMaxH * kMaxH, lane, d); }
};
#ifndef HODE_LAB
template <int NL> struct WtRegs;
#endif

// One hidden layer of the backward pass: gw += d (x) hin  and  returns W^T d.
// Generic form: the two products one after the other.
template <typename R, typename Wt>
__device__ __forceinline__ R layer_bwd(R (&gw)[kMaxH], const Wt &wt, int l, int lane, R d, R hin, const R *__restrict__ hrow = nullptr)
{
    (void)hrow;
    mlp_outer_acc(gw, d, hin);
    return wt.mul(l, lane, d);
}
// fp32 + LDS-resident transposed matrix: the outer-product FMAs (which need no memory) are interleaved
// with the W^T product so that each group of four 16-byte LDS reads has 16 independent FMAs between its
// issue and its first use -- the LDS latency hides behind work of the same wave.
template <int G>
__device__ __forceinline__ void layer_bwd_group(float (&gw)[kMaxH], const Vec4<float> *__restrict__ wt4, int lane, float d,
                                                const float (&Rh)[4], const float (&Rd)[4], float (&acc)[4])
{
    const Vec4<float> w0 = wt4[(4 * G + 0) * kMaxH + lane], w1 = wt4[(4 * G + 1) * kMaxH + lane],
                      w2 = wt4[(4 * G + 2) * kMaxH + lane], w3 = wt4[(4 * G + 3) * kMaxH + lane];
    __builtin_amdgcn_sched_barrier(0);          // reads are issued HERE, the 16 outer-product FMAs below cover their latency
    constexpr int n = 4 * G;
    gw[0 * 16 + n + 0] = fmac_ror<n + 0>(gw[0 * 16 + n + 0], Rh[0], d);
    gw[1 * 16 + n + 0] = fmac_ror<n + 0>(gw[1 * 16 + n + 0], Rh[1], d);
    gw[2 * 16 + n + 0] = fmac_ror<n + 0>(gw[2 * 16 + n + 0], Rh[2], d);
    gw[3 * 16 + n + 0] = fmac_ror<n + 0>(gw[3 * 16 + n + 0], Rh[3], d);
    gw[0 * 16 + n + 1] = fmac_ror<n + 1>(gw[0 * 16 + n + 1], Rh[0], d);
    gw[1 * 16 + n + 1] = fmac_ror<n + 1>(gw[1 * 16 + n + 1], Rh[1], d);
    gw[2 * 16 + n + 1] = fmac_ror<n + 1>(gw[2 * 16 + n + 1], Rh[2], d);
    gw[3 * 16 + n + 1] = fmac_ror<n + 1>(gw[3 * 16 + n + 1], Rh[3], d);
    gw[0 * 16 + n + 2] = fmac_ror<n + 2>(gw[0 * 16 + n + 2], Rh[0], d);
    gw[1 * 16 + n + 2] = fmac_ror<n + 2>(gw[1 * 16 + n + 2], Rh[1], d);
    gw[2 * 16 + n + 2] = fmac_ror<n + 2>(gw[2 * 16 + n + 2], Rh[2], d);
    gw[3 * 16 + n + 2] = fmac_ror<n + 2>(gw[3 * 16 + n + 2], Rh[3], d);
    gw[0 * 16 + n + 3] = fmac_ror<n + 3>(gw[0 * 16 + n + 3], Rh[0], d);
    gw[1 * 16 + n + 3] = fmac_ror<n + 3>(gw[1 * 16 + n + 3], Rh[1], d);
    gw[2 * 16 + n + 3] = fmac_ror<n + 3>(gw[2 * 16 + n + 3], Rh[2], d);
    gw[3 * 16 + n + 3] = fmac_ror<n + 3>(gw[3 * 16 + n + 3], Rh[3], d);
    __builtin_amdgcn_sched_barrier(0);          // (hipcc otherwise hoists the dependent FMAs right behind the reads;
                                                //  a two-deep pipeline of groups was tried: 32 more live registers spill)
    // rows 4G..4G+3 of the image: r = 16 G + 4 i + c  ->  q = G, n = 4 i + c.  ONE asm statement: between separate
    // statements that share an accumulator hipcc inserts an s_nop (see mlp_hidden, lab/hode_lab_layers.h)
    static_assert(G >= 0 && G < 4, "four groups of sixteen rotations");
    if constexpr (G == 0) {
        // the first group starts the four sums with products: no zero-initialised accumulators (four v_mov_b32 per layer)
        asm("v_mul_f32 %[a0], %[r], %[w0]\n\t"
            "v_mul_f32_dpp %[a1], %[r], %[w1] row_ror:1 row_mask:0xf bank_mask:0xf\n\t"
            "v_mul_f32_dpp %[a2], %[r], %[w2] row_ror:2 row_mask:0xf bank_mask:0xf\n\t"
            "v_mul_f32_dpp %[a3], %[r], %[w3] row_ror:3 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f32_dpp %[a0], %[r], %[w4] row_ror:4 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f32_dpp %[a1], %[r], %[w5] row_ror:5 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f32_dpp %[a2], %[r], %[w6] row_ror:6 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f32_dpp %[a3], %[r], %[w7] row_ror:7 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f32_dpp %[a0], %[r], %[w8] row_ror:8 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f32_dpp %[a1], %[r], %[w9] row_ror:9 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f32_dpp %[a2], %[r], %[w10] row_ror:10 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f32_dpp %[a3], %[r], %[w11] row_ror:11 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f32_dpp %[a0], %[r], %[w12] row_ror:12 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f32_dpp %[a1], %[r], %[w13] row_ror:13 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f32_dpp %[a2], %[r], %[w14] row_ror:14 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f32_dpp %[a3], %[r], %[w15] row_ror:15 row_mask:0xf bank_mask:0xf"
            : [a0] "=&v"(acc[0]), [a1] "=&v"(acc[1]), [a2] "=&v"(acc[2]), [a3] "=&v"(acc[3])
        : [r] "v"(Rd[G]), [w0] "v"(w0.v[0]), [w1] "v"(w0.v[1]), [w2] "v"(w0.v[2]), [w3] "v"(w0.v[3]), [w4] "v"(w1.v[0]),
          [w5] "v"(w1.v[1]), [w6] "v"(w1.v[2]), [w7] "v"(w1.v[3]), [w8] "v"(w2.v[0]), [w9] "v"(w2.v[1]), [w10] "v"(w2.v[2]),
          [w11] "v"(w2.v[3]), [w12] "v"(w3.v[0]), [w13] "v"(w3.v[1]), [w14] "v"(w3.v[2]), [w15] "v"(w3.v[3]));
    } else {
    asm("v_fmac_f32 %[a0], %[r], %[w0]\n\t"
        "v_fmac_f32_dpp %[a1], %[r], %[w1] row_ror:1 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f32_dpp %[a2], %[r], %[w2] row_ror:2 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f32_dpp %[a3], %[r], %[w3] row_ror:3 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f32_dpp %[a0], %[r], %[w4] row_ror:4 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f32_dpp %[a1], %[r], %[w5] row_ror:5 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f32_dpp %[a2], %[r], %[w6] row_ror:6 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f32_dpp %[a3], %[r], %[w7] row_ror:7 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f32_dpp %[a0], %[r], %[w8] row_ror:8 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f32_dpp %[a1], %[r], %[w9] row_ror:9 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f32_dpp %[a2], %[r], %[w10] row_ror:10 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f32_dpp %[a3], %[r], %[w11] row_ror:11 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f32_dpp %[a0], %[r], %[w12] row_ror:12 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f32_dpp %[a1], %[r], %[w13] row_ror:13 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f32_dpp %[a2], %[r], %[w14] row_ror:14 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f32_dpp %[a3], %[r], %[w15] row_ror:15 row_mask:0xf bank_mask:0xf"
        : [a0] "+v"(acc[0]), [a1] "+v"(acc[1]), [a2] "+v"(acc[2]), [a3] "+v"(acc[3])
        : [r] "v"(Rd[G]), [w0] "v"(w0.v[0]), [w1] "v"(w0.v[1]), [w2] "v"(w0.v[2]), [w3] "v"(w0.v[3]), [w4] "v"(w1.v[0]),
          [w5] "v"(w1.v[1]), [w6] "v"(w1.v[2]), [w7] "v"(w1.v[3]), [w8] "v"(w2.v[0]), [w9] "v"(w2.v[1]), [w10] "v"(w2.v[2]),
          [w11] "v"(w2.v[3]), [w12] "v"(w3.v[0]), [w13] "v"(w3.v[1]), [w14] "v"(w3.v[2]), [w15] "v"(w3.v[3]));
    }
    __builtin_amdgcn_sched_barrier(0);
}
// hrow != nullptr: the 64 activations h_in[0..63] also sit in LDS (the stage record the DMA delivered): their four 16-lane
// rows are read back replicated -- four conflict-free broadcast reads -- instead of being replicated through
// v_permlane swaps (3 swaps + 3 copies of VALU time per layer)
__device__ __forceinline__ float layer_bwd(float (&gw)[kMaxH], const WtLds<float> &wt, int l, int lane, float d, float hin,
                                           const float *__restrict__ hrow = nullptr)
{
    const Vec4<float> *wt4 = reinterpret_cast<const Vec4<float> *>(wt.wt + (size_t)l * kMaxH * kMaxH);
    float Rh[4], Rd[4];
    if (hrow != nullptr) {
        const int p16 = lane & 15;
        Rh[0] = hrow[p16]; Rh[1] = hrow[16 + p16]; Rh[2] = hrow[32 + p16]; Rh[3] = hrow[48 + p16];
        // the DPP reads of Rh[] in the asm FMAs need no wait states after an LDS return (not a VALU write), but keep the
        // compiler from sinking the loads below the asm block boundary
        asm volatile("" : "+v"(Rh[0]), "+v"(Rh[1]), "+v"(Rh[2]), "+v"(Rh[3]));
    } else {
        rows_replicate(hin, Rh);
    }
    rows_replicate(d, Rd);
    float acc[4];                                   // started by group 0
    __builtin_amdgcn_sched_barrier(0);
    layer_bwd_group<0>(gw, wt4, lane, d, Rh, Rd, acc);
    layer_bwd_group<1>(gw, wt4, lane, d, Rh, Rd, acc);
    layer_bwd_group<2>(gw, wt4, lane, d, Rh, Rd, acc);
    layer_bwd_group<3>(gw, wt4, lane, d, Rh, Rd, acc);
    return (acc[0] + acc[1]) + (acc[2] + acc[3]);
}

// ------------------------------------------------------------------------------------------
// First/last-layer weights and their gradient accumulators ("edge" parameters: W1[.,9], b_1..b_NL,
// Wout[6,.], bout) behind a small policy, so that the adjoint kernel can keep them in LDS and spend
// its registers on the 3 x 64 hidden-matrix accumulators:
//   EdgeRegs : everything in VGPRs (K5, fp64 parity builds)
//   EdgeLds  : weights in a workgroup-shared LDS table, accumulators in a wave-private LDS table
//              (read-modify-write; the table is private to the wave, so no atomics are needed)
// slots: 0..8 W1 columns, 9..9+NL-1 hidden biases, then 6 Wout rows, then bout (lane o < 6).
template <int NL> struct EdgeSlots { static constexpr int w1 = 0, b = 9, w5 = 9 + NL, b5 = 15 + NL, count = 16 + NL; };

template <typename R, int NL> struct EdgeRegs {
    R w[EdgeSlots<NL>::count];
    R gacc[EdgeSlots<NL>::count];
    __device__ __forceinline__ R W(int slot) const { return w[slot]; }
    __device__ __forceinline__ void add(int slot, R v) { gacc[slot] += v; }
    __device__ __forceinline__ void fma(int slot, R a, R b) { gacc[slot] = rfma(a, b, gacc[slot]); }
    __device__ __forceinline__ R G(int slot) const { return gacc[slot]; }
    // gacc[slot] += v[slot] for the first N slots
    template <int N> __device__ __forceinline__ void add_all(const R (&v)[EdgeSlots<NL>::count])
    {
#pragma unroll
        for (int i = 0; i < N; ++i) gacc[i] += v[i];
    }
};
template <typename R, int NL> struct EdgeLds {
    const R *w;      // [slots][64] shared by the workgroup
    R *gacc;         // [slots][64] private to the wave
    int lane;
    __device__ __forceinline__ R W(int slot) const { return w[slot * kWave + lane]; }
    // wave-private table: a plain read-modify-write is safe and runs at the full LDS rate
    // (ds_add_f32 serialises per lane: measured 2.5x slower for the whole kernel)
    __device__ __forceinline__ void add(int slot, R v) { gacc[slot * kWave + lane] += v; }
    __device__ __forceinline__ void fma(int slot, R a, R b) { gacc[slot * kWave + lane] = rfma(a, b, gacc[slot * kWave + lane]); }
    __device__ __forceinline__ R G(int slot) const { return gacc[slot * kWave + lane]; }
    // all reads first (one LDS wait instead of one per slot), then the adds, then all writes
    template <int N> __device__ __forceinline__ void add_all(const R (&v)[EdgeSlots<NL>::count])
    {
        R cur[N];
#pragma unroll
        for (int i = 0; i < N; ++i) cur[i] = gacc[i * kWave + lane];
#pragma unroll
        for (int i = 0; i < N; ++i) gacc[i * kWave + lane] = cur[i] + v[i];
    }
};
// edge weights of one parameter set into a [slots][64] table (weights only; accumulators start at 0)
template <typename R, int NL>
__device__ __forceinline__ void edge_table_store(R *__restrict__ tab, const R *__restrict__ p, int H, int tid, int nthreads)
{
    using S = EdgeSlots<NL>;
    const R *pout = p + 9 * H + H + (size_t)(NL - 1) * ((size_t)H * H + H);
    for (int i = tid; i < S::count * kWave; i += nthreads) {
        const int slot = i >> 6, j = i & 63;
        R v = R(0);
        if (j < H) {
            if (slot < S::b) v = p[j * 9 + slot];
            else if (slot >= S::w5 && slot < S::b5) v = pout[(slot - S::w5) * H + j];
        }
        tab[i] = v;            // bias slots hold no weight the VJP needs
    }
}
// flush the edge accumulators into the flat gradient vector
template <typename R, int NL, typename Edge>
__device__ __forceinline__ void edge_flush(const Edge &e, R *__restrict__ gp, int H, int lane)
{
    using S = EdgeSlots<NL>;
    const bool live = lane < H;
    if (live) {
#pragma unroll
        for (int i = 0; i < 9; ++i) atomic_add(gp + lane * 9 + i, e.G(S::w1 + i));
        atomic_add(gp + 9 * H + lane, e.G(S::b + 0));
    }
    R *q = gp + 9 * H + H;
#pragma unroll
    for (int l = 1; l < NL; ++l) {
        q += (size_t)H * H;
        if (live) atomic_add(q + lane, e.G(S::b + l));
        q += H;
    }
    if (live) {
#pragma unroll
        for (int o = 0; o < 6; ++o) atomic_add(q + o * H + lane, e.G(S::w5 + o));
    }
    if (lane < 6) atomic_add(q + 6 * H + lane, e.G(S::b5));
}
// hidden-matrix accumulators only
template <typename R, int NL>
__device__ __forceinline__ void hidden_flush(const R (&wh)[(NL > 1) ? NL - 1 : 1][kMaxH], R *__restrict__ gp, int H, int lane)
{
    const bool live = lane < H;
    R *q = gp + 9 * H + H;
#pragma unroll
    for (int l = 0; l < NL - 1; ++l) {
        if (live) {
#pragma unroll
            for (int k = 0; k < kMaxH; ++k) {
                const int c = wcol<R>(k, lane);            // register k of lane j is column c (rotated order in fp32)
                if (c < H) atomic_add(q + (size_t)lane * H + c, wh[l][k]);
            }
        }
        q += (size_t)H * H + H;
    }
}

// J_mech^T kb (analytic Jacobian of models/ode_core.py:124-153) in the replicated layout; GODE: also d f / d(ode constant p) . kb
// for the 17 constants, accumulated LANE-DISTRIBUTED: lane p < 17 of the single register `go` holds the running sum for
// constant p (17 separate uniform accumulators cost 16 more VGPRs, which the adjoint kernel does not have).
template <typename R, bool GODE>
__device__ __forceinline__ R mech_vjp(const OdeP<R> &o, R G, R I, R Glu, R GLP1, R FFA, R lG, R lI, R lGlu, R lGLP, R lF, R gde,
                                      R gd_in, bool use_gd, int lane, R &go)
{
    const R Pi = R(1) + o.rho * GLP1;
    const R den1 = o.EC_50 + GLP1, den2 = o.K_m + G;
    const R k_GE = o.k_GE0 * (R(1) - gde);
    const R r1 = rdiv(R(1), den1), r2 = rdiv(R(1), den2);
    const R oG = -k_GE * lG + Pi * o.a_GI * lI + o.V_max * o.K_m * r2 * r2 * lGLP + o.p_9 * FFA * lF;
    const R oI = R(-0.01) * lG - o.k_I * lI - o.p_8 * FFA * lF;
    const R oGlu = R(0.005) * lG - o.E_max * GLP1 * r1 * lGlu;
    const R oGLP = o.rho * o.a_GI * (G - o.G_b) * lI - o.E_max * o.EC_50 * r1 * r1 * (Glu - o.Glu_b) * lGlu - o.k_L * lGLP;
    const R oF = (-o.p_7 - o.p_8 * I + o.p_9 * G) * lF;
    const int c8 = lane & 7;
    // (select chains that keep hipcc from sinking the terms into exec-masked regions -- keep_term as in mech_eval, or
    //  v_cndmask_b32 with literal lane masks -- were tried here: the adjoint kernel, at its register limit, answers with
    //  60-90 B of scratch instead of 28-36 and reloads inside the stage loop)
    const R mech = (c8 == 0) ? oG : (c8 == 1) ? oI : (c8 == 2) ? oGlu : (c8 == 3) ? oGLP : (c8 == 5) ? oF : R(0);
    if constexpr (GODE) {
        R c[17];
        c[0] = lI * Pi * (G - o.G_b);
        c[1] = -lI * (I - o.I_b);
        c[2] = lI * GLP1 * o.a_GI * (G - o.G_b);
        c[3] = -lI * Pi * o.a_GI;
        c[4] = lI * o.k_I + lG * R(0.01);
        c[5] = -lGlu * GLP1 * r1 * (Glu - o.Glu_b);
        c[6] = lGlu * o.E_max * GLP1 * r1 * r1 * (Glu - o.Glu_b);
        c[7] = lGlu * o.E_max * GLP1 * r1 - lG * R(0.005);
        c[8] = lGLP * G * r2;
        c[9] = -lGLP * o.V_max * G * r2 * r2;
        c[10] = -lGLP * GLP1;
        c[11] = -lG * G * (R(1) - gde);
        c[12] = R(0);
        c[13] = R(0);
        if (use_gd && gd_in > R(0)) {
            const R u = rpow(gd_in, o.g), v = rpow(o.IGD_50, o.g), s2 = (v + u) * (v + u);
            c[12] = lG * o.k_GE0 * G * (-u * o.g * rpow(o.IGD_50, o.g - R(1)) / s2);
            c[13] = lG * o.k_GE0 * G * (u * v * (rlog(gd_in) - rlog(o.IGD_50)) / s2);
        }
        c[14] = -lF * FFA;
        c[15] = -lF * I * FFA;
        c[16] = lF * G * FFA;
        R sel = R(0);
#pragma unroll
        for (int p = 0; p < 17; ++p) sel = (lane == p) ? c[p] : sel;
        go += sel;
    }
    return mech;
}

// VJP of rhs_eval.  kb = cotangent of f (replicated layout); returns the cotangent of the state in the
// same layout and accumulates parameter gradients.  acts = activations of this evaluation (from
// rhs_eval<KEEP> or from the stage tape).  Needs only the first/last layer weights in registers;
// the hidden matrices come transposed from LDS (wt).   GODE: also d/d(ode constants) (wave-uniform values).
//   Y     the stage state in the replicated layout (lane l holds x_{l&7}; from the compact stage record / the input batch)
//   acts  h_1 .. h_NL of this evaluation.  (Recomputing h_1 here from (t, x, tvns) -- 9 FMAs instead of a 256-byte tape row
//         per stage -- was built and measured: it costs the adjoint kernel its last registers, 80 B of scratch with
//         reloads inside the stage loop, whose vmcnt waits serialise behind the record DMA: 8.1 -> 12.5 ms.)
// GIN: the cotangent kb pulled back to the three external inputs of one evaluation, in the input-gradient layout -- lanes 2q and
// 2q + 1 receive input q (0 meal, 1 tVNS, 2 GD), every other lane GD's value (a wave-uniform select, no lane test for them):
//   meal  enters dG additively (models/ode_core.py:148-150):  d f / d meal = lG;
//   tVNS  enters the MLP only, as input 8 of the first layer:  ctv = sum_j W1[j][8] delta1_j  (the caller's wave_allsum);
//   GD    enters k_GE = k_GE0 (1 - gde(GD)) only (:139-140):    lG k_GE0 G gde'(GD),  gde' = g u v / (GD (v + u)^2),
//         u = GD^g, v = IGD_50^g; zero for GD <= 0 (the derivative the ODE-constant gradient of IGD_50 / g also takes there).
template <typename R>
__device__ __forceinline__ R input_vjp(const OdeP<R> &o, R G, R lG, R ctv, R gd_in, bool use_gd, int lane)
{
    R cg = R(0);
    if (use_gd && gd_in > R(0)) {
        const R u = rpow(gd_in, o.g), v = rpow(o.IGD_50, o.g);
        cg = lG * o.k_GE0 * G * rdiv(o.g * u * v, gd_in * ((v + u) * (v + u)));
    }
    const int q = lane >> 1;
    return (q == 0) ? lG : (q == 1) ? ctv : cg;
}

// GIN: *gin_out = input_vjp(...) of this evaluation (see above).
template <typename R, int NL, bool GODE, bool GT, bool GIN = false, typename Edge, typename Wt>
__device__ __forceinline__ R rhs_vjp(Edge &e, R (&gwh)[(NL > 1) ? NL - 1 : 1][kMaxH], const Wt &wt,
                                     const OdeP<R> &o, R t, R Y, R tvns, R gde, R gd_in, bool use_gd, int lane,
                                     const MlpActs<R, NL> &acts, R kb, R &go, R *gt_out, const R *__restrict__ hrows = nullptr,
                                     R *gin_out = nullptr)
{
    // hrows: LDS copy of the record rows h_1 .. h_NL ([NL][64]) or nullptr
    using S = EdgeSlots<NL>;
    // increments of the edge-parameter gradients are collected and applied in ONE batch at the end
    R inc[S::count];
    const R G = lane_bcast(Y, 0), I = lane_bcast(Y, 1), Glu = lane_bcast(Y, 2), GLP1 = lane_bcast(Y, 3),
            GE = lane_bcast(Y, 4), FFA = lane_bcast(Y, 5);
    // h_1 exactly as rhs_eval computes it (same operation order)
    const R h1 = acts.h[0];
    const R lG = lane_bcast(kb, 0), lI = lane_bcast(kb, 1), lGlu = lane_bcast(kb, 2), lGLP = lane_bcast(kb, 3),
            lGE = lane_bcast(kb, 4), lF = lane_bcast(kb, 5);
    const int c8 = lane & 7;
    const R mech = mech_vjp<R, GODE>(o, G, I, Glu, GLP1, FFA, lG, lI, lGlu, lGLP, lF, gde, gd_in, use_gd, lane, go);
    // ---- MLP backward
    const R hl = (NL > 1) ? acts.h[NL - 1] : h1;
    // fetch the six output-layer weights in one batch (LDS policy: six reads in flight, one wait)
    const R w50 = e.W(S::w5 + 0), w51 = e.W(S::w5 + 1), w52 = e.W(S::w5 + 2), w53 = e.W(S::w5 + 3),
            w54 = e.W(S::w5 + 4), w55 = e.W(S::w5 + 5);
    R d = w50 * lG;
    d = rfma(w51, lI, d);
    d = rfma(w52, lGlu, d);
    d = rfma(w53, lGLP, d);
    d = rfma(w54, lGE, d);
    d = rfma(w55, lF, d);
    inc[S::b5] = kb;                             // lane o < 6 holds d bout[o] (other groups hold copies)
    inc[S::w5 + 0] = lG * hl;
    inc[S::w5 + 1] = lI * hl;
    inc[S::w5 + 2] = lGlu * hl;
    inc[S::w5 + 3] = lGLP * hl;
    inc[S::w5 + 4] = lGE * hl;
    inc[S::w5 + 5] = lF * hl;
    d = (hl > R(0)) ? d : R(0);
#pragma unroll
    for (int l = NL - 1; l >= 1; --l) {           // hidden matrix l-1 maps acts.h[l-1] -> acts.h[l]
        const R hin = (l > 1) ? acts.h[l - 1] : h1;
        inc[S::b + l] = d;
        const R dp = layer_bwd(gwh[l - 1], wt, l - 1, lane, d, hin, hrows ? hrows + (l - 1) * kWave : nullptr);   // dW_l += d (x) h_{l-1};  dp = W_l^T d
        d = (hin > R(0)) ? dp : R(0);
    }
    inc[S::b + 0] = d;
    inc[S::w1 + 0] = d * t;
    inc[S::w1 + 1] = d * G;
    inc[S::w1 + 2] = d * I;
    inc[S::w1 + 3] = d * Glu;
    inc[S::w1 + 4] = d * GLP1;
    inc[S::w1 + 5] = d * GE;
    inc[S::w1 + 6] = d * FFA;
    inc[S::w1 + 7] = d * GLP1;
    inc[S::w1 + 8] = d * tvns;
    e.template add_all<S::count>(inc);
    const R w11 = e.W(S::w1 + 1), w12 = e.W(S::w1 + 2), w13 = e.W(S::w1 + 3), w14 = e.W(S::w1 + 4), w15 = e.W(S::w1 + 5),
            w16 = e.W(S::w1 + 6), w17 = e.W(S::w1 + 7);
    R p[6];
    p[0] = w11 * d;
    p[1] = w12 * d;
    p[2] = w13 * d;
    p[3] = (w14 + w17) * d;                       // GLP1 feeds inputs 4 and 7
    p[4] = w15 * d;
    p[5] = w16 * d;
    const R nn = wave_reduce6_to_lanes(p, lane);
    if constexpr (GT) *gt_out = wave_allsum(e.W(S::w1 + 0) * d);
    if constexpr (GIN) *gin_out = input_vjp(o, G, lG, wave_allsum(e.W(S::w1 + 8) * d), gd_in, use_gd, lane);
    return (c8 < 6) ? (mech + nn) : R(0);
}

}  // namespace hode

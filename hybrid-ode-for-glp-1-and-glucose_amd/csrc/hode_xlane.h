// hode_xlane.h -- wave-level primitives of every kernel (gfx950 / CDNA4 only): bit casts, lane broadcasts, DPP moves, the cross-lane
// sums, the rotating-operand FMA, the per-dtype math wrappers (r*) and atomic_add.
// Used by: every other device header (hode_tableau.h, hode_mlp.h, hode_rhs_eval.h, hode_adjoint.h, hode_generic_net.h,
// lab/hode_lab_layers.h), hode_optim.hip, and hode_rhs.hip's self test.
//
// Execution model used throughout: ONE TRAJECTORY PER WAVEFRONT, ONE HIDDEN UNIT PER LANE.
//   * the hidden weight matrices live in VGPRs, 64 registers per matrix and lane (loaded once per trajectory, register-
//     resident for all ~1440 RHS evaluations); activations are kept one unit per lane;
//   * a 64x64 layer is 64 FMAs per lane; the activation of lane k reaches lane j as the DPP row_ror:n operand of the FMA
//     itself ("rotating operand") -- no v_readlane per element, no LDS round trip, no barrier.  fp32 forward kernels: lane
//     16 r + i keeps W[16 w + i][16 r + ((i - n) & 15)] and reduces four row-partial accumulators with a 3-swap transpose
//     (mlp_hidden_blk); the adjoint and the LDS-image experiment replicate the 16-lane rows first (rows_replicate);
//   * the 6-vector state is replicated per 8-lane group (lane l holds component l & 7) and the
//     Runge-Kutta stage derivatives are packed into ONE VGPR (lanes 8s..8s+7 = stage s), so a stage
//     combination is one multiply by a per-lane coefficient row + a 7-instruction cross-lane sum;
//   * step-size control is per trajectory == per wave: accept/reject is a wave-uniform branch,
//     there is no lane divergence and no cross-trajectory coupling.
// MFMA is deliberately not used (north_star): every layer is a matrix-VECTOR product per
// trajectory.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hode {

constexpr int kWave = 64;
constexpr int kMaxH = 64;

// ------------------------------------------------------------------------------------------
// bit casts
__device__ __forceinline__ int f2i(float v) { return __builtin_bit_cast(int, v); }
__device__ __forceinline__ float i2f(int v) { return __builtin_bit_cast(float, v); }

// ------------------------------------------------------------------------------------------
// lane broadcast: value of lane k (k wave-uniform) to every lane, via SGPR
__device__ __forceinline__ float lane_bcast(float v, int k)
{
    return i2f(__builtin_amdgcn_readlane(f2i(v), k));
}
__device__ __forceinline__ double lane_bcast(double v, int k)
{
    uint64_t u = __builtin_bit_cast(uint64_t, v);
    uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)u, k);
    uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(u >> 32), k);
    return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ float first_lane(float v) { return i2f(__builtin_amdgcn_readfirstlane(f2i(v))); }
__device__ __forceinline__ double first_lane(double v)
{
    uint64_t u = __builtin_bit_cast(uint64_t, v);
    uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)u);
    uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(u >> 32));
    return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ int first_lane(int v) { return __builtin_amdgcn_readfirstlane(v); }

// ------------------------------------------------------------------------------------------
// DPP moves.  CTRL: quad_perm 0x00-0xFF, row_shl:n 0x100+n, row_shr:n 0x110+n, row_ror:n 0x120+n
template <int CTRL, int BANK, bool BOUND>
__device__ __forceinline__ float dpp_mov(float old, float v)
{
    return i2f(__builtin_amdgcn_update_dpp(f2i(old), f2i(v), CTRL, 0xF, BANK, BOUND));
}
template <int CTRL, int BANK, bool BOUND>
__device__ __forceinline__ double dpp_mov(double old, double v)
{
    uint64_t o = __builtin_bit_cast(uint64_t, old), u = __builtin_bit_cast(uint64_t, v);
    uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp((int)(uint32_t)o, (int)(uint32_t)u, CTRL, 0xF, BANK, BOUND);
    uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp((int)(uint32_t)(o >> 32), (int)(uint32_t)(u >> 32), CTRL, 0xF, BANK, BOUND);
    return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}

// value of lane (l ^ 1), (l ^ 2), (l ^ 4), (l ^ 8)
template <typename R> __device__ __forceinline__ R xlane_xor1(R v) { return dpp_mov<0xB1, 0xF, true>(v, v); }  // quad_perm [1,0,3,2]
template <typename R> __device__ __forceinline__ R xlane_xor2(R v) { return dpp_mov<0x4E, 0xF, true>(v, v); }  // quad_perm [2,3,0,1]
template <typename R> __device__ __forceinline__ R xlane_xor4(R v)
{
    R t = dpp_mov<0x104, 0x5, false>(v, v);   // row_shl:4 into banks 0,2  (lane i <- i+4)
    return dpp_mov<0x114, 0xA, false>(t, v);  // row_shr:4 into banks 1,3  (lane i <- i-4)
}
template <typename R> __device__ __forceinline__ R xlane_xor8(R v) { return dpp_mov<0x128, 0xF, true>(v, v); }  // row_ror:8
// value of lane (l ^ 7) within each 8-lane half row (row_half_mirror).  For a value that is already uniform over the quads
// -- a sum after the xor1 / xor2 exchanges -- this IS the other quad's value, in one DPP operand instead of the two masked
// moves + copy of xlane_xor4.
template <typename R> __device__ __forceinline__ R xlane_hmirror(R v) { return dpp_mov<0x141, 0xF, true>(v, v); }

// v(l) + v(l ^ 16) and v(l) + v(l ^ 32) on every lane: gfx950 v_permlane16_swap / v_permlane32_swap
__device__ __forceinline__ float allsum_x16(float v)
{
    auto r = __builtin_amdgcn_permlane16_swap((unsigned)f2i(v), (unsigned)f2i(v), false, false);
    return i2f((int)r[0]) + i2f((int)r[1]);
}
__device__ __forceinline__ float allsum_x32(float v)
{
    auto r = __builtin_amdgcn_permlane32_swap((unsigned)f2i(v), (unsigned)f2i(v), false, false);
    return i2f((int)r[0]) + i2f((int)r[1]);
}
__device__ __forceinline__ double allsum_x16(double v)
{
    uint64_t u = __builtin_bit_cast(uint64_t, v);
    auto lo = __builtin_amdgcn_permlane16_swap((unsigned)u, (unsigned)u, false, false);
    auto hi = __builtin_amdgcn_permlane16_swap((unsigned)(u >> 32), (unsigned)(u >> 32), false, false);
    double a = __builtin_bit_cast(double, ((uint64_t)hi[0] << 32) | lo[0]);
    double b = __builtin_bit_cast(double, ((uint64_t)hi[1] << 32) | lo[1]);
    return a + b;
}
__device__ __forceinline__ double allsum_x32(double v)
{
    uint64_t u = __builtin_bit_cast(uint64_t, v);
    auto lo = __builtin_amdgcn_permlane32_swap((unsigned)u, (unsigned)u, false, false);
    auto hi = __builtin_amdgcn_permlane32_swap((unsigned)(u >> 32), (unsigned)(u >> 32), false, false);
    double a = __builtin_bit_cast(double, ((uint64_t)hi[0] << 32) | lo[0]);
    double b = __builtin_bit_cast(double, ((uint64_t)hi[1] << 32) | lo[1]);
    return a + b;
}

// sum over the whole wave, result on every lane
template <typename R> __device__ __forceinline__ R wave_allsum(R v)
{
    v += xlane_xor1(v);
    v += xlane_xor2(v);
    v += xlane_hmirror(v);          // quad-uniform by now
    v += xlane_xor8(v);
    v = allsum_x16(v);
    return allsum_x32(v);
}
// sum over lanes 0..7 (on each aligned group of 8), result on every lane of the group
template <typename R> __device__ __forceinline__ R oct_allsum(R v)
{
    v += xlane_xor1(v);
    v += xlane_xor2(v);
    v += xlane_hmirror(v);          // quad-uniform by now
    return v;
}

// Transpose-reduce: every lane holds p[0..5]; returns on each lane l the wave-wide sum of
// p[l & 7] (zero for (l & 7) >= 6).  The register count halves at every exchange, so the whole
// 6-value reduction costs ~30 VALU instead of 6 x 7 for six separate wave reductions.
template <typename R> __device__ __forceinline__ R wave_reduce6_to_lanes(const R (&p)[6], int lane)
{
    const bool b0 = lane & 1, b1 = lane & 2, b2 = lane & 4;
    R q0 = (b0 ? p[1] : p[0]) + xlane_xor1(b0 ? p[0] : p[1]);
    R q1 = (b0 ? p[3] : p[2]) + xlane_xor1(b0 ? p[2] : p[3]);
    R q2 = (b0 ? p[5] : p[4]) + xlane_xor1(b0 ? p[4] : p[5]);
    R r0 = (b1 ? q1 : q0) + xlane_xor2(b1 ? q0 : q1);
    R r1 = (b1 ? R(0) : q2) + xlane_xor2(b1 ? q2 : R(0));
    R s = (b2 ? r1 : r0) + xlane_xor4(b2 ? r0 : r1);
    s += xlane_xor8(s);
    s = allsum_x16(s);
    return allsum_x32(s);
}

// ------------------------------------------------------------------------------------------
// sum over the 8 lanes that share (lane & 7), result on all of them
template <typename R> __device__ __forceinline__ R group_sum8(R v)
{
    if constexpr (sizeof(R) == 4) {
        // v + row_ror:8(v) as ONE instruction (hipcc otherwise re-fuses the producer of v into a copy + v_fmac pair)
        float t = v;
        asm("s_nop 1\n\tv_add_f32_dpp %0, %0, %0 row_ror:8 row_mask:0xf bank_mask:0xf" : "+v"(t));
        v = t;
    } else {
        v += xlane_xor8(v);
    }
    v = allsum_x16(v);
    return allsum_x32(v);
}

// ------------------------------------------------------------------------------------------
// per-dtype math wrappers
template <typename R> __device__ __forceinline__ R rmax0(R v) { return v > R(0) ? v : R(0); }
__device__ __forceinline__ float rfma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double rfma(double a, double b, double c) { return __builtin_fma(a, b, c); }
__device__ __forceinline__ float rpow(float a, float b) { return powf(a, b); }
__device__ __forceinline__ double rpow(double a, double b) { return pow(a, b); }
__device__ __forceinline__ float rlog(float a) { return logf(a); }
__device__ __forceinline__ double rlog(double a) { return log(a); }
// a / b.  fp32: a * v_rcp_f32(b) (the reciprocal is good to 1 ulp; 2 VALU instead of the ~10 of an IEEE division -- a
// Newton step on the reciprocal, 2 more, bought nothing the fp32 parity bars can see); fp64 (parity runs): exact division.
__device__ __forceinline__ float rdiv(float a, float b) { return a * __builtin_amdgcn_rcpf(b); }
__device__ __forceinline__ double rdiv(double a, double b) { return a / b; }
__device__ __forceinline__ float rabs(float a) { return __builtin_fabsf(a); }
__device__ __forceinline__ double rabs(double a) { return __builtin_fabs(a); }

// ------------------------------------------------------------------------------------------
// Rotating operand, one instruction at a time (the adjoint's W^T products and the lab library's row-replicated layers; the forward
// layer of the product library is ONE asm statement, hode_mlp.h).
// acc += row_ror:N(x) * w as ONE instruction.  hipcc (ROCm 7.2) selects the VOP3 v_fma_f32 for fmaf() and
// its DPP-combine pass cannot fold a v_mov_b32_dpp into a VOP3 op on gfx9, so the VOP2 form is written out.
// Hazard note (cdna_hip_programming.md 5.7: hipcc pads nothing around asm): a DPP operand needs 2 wait
// states after the VALU that wrote it -- rows_replicate() ends with an explicit s_nop 1, and the
// accumulator / weight operands are ordinary (interlocked) VALU operands.
#define HODE_FMAC_ROR(N)                                                                                    \
    template <> __device__ __forceinline__ float fmac_ror<N>(float acc, float x, float w)                   \
    {                                                                                                       \
        asm("v_fmac_f32_dpp %0, %1, %2 row_ror:" #N " row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(x), "v"(w)); \
        return acc;                                                                                         \
    }
template <int N> __device__ __forceinline__ float fmac_ror(float acc, float x, float w);
template <> __device__ __forceinline__ float fmac_ror<0>(float acc, float x, float w) { return __builtin_fmaf(x, w, acc); }
HODE_FMAC_ROR(1) HODE_FMAC_ROR(2) HODE_FMAC_ROR(3) HODE_FMAC_ROR(4) HODE_FMAC_ROR(5) HODE_FMAC_ROR(6) HODE_FMAC_ROR(7)
HODE_FMAC_ROR(8) HODE_FMAC_ROR(9) HODE_FMAC_ROR(10) HODE_FMAC_ROR(11) HODE_FMAC_ROR(12) HODE_FMAC_ROR(13)
HODE_FMAC_ROR(14) HODE_FMAC_ROR(15)
#undef HODE_FMAC_ROR
__device__ __forceinline__ void rows_replicate(float h, float (&R)[4])
{
    auto s16 = __builtin_amdgcn_permlane16_swap((unsigned)f2i(h), (unsigned)f2i(h), false, false);   // [r0 r0 r2 r2] , [r1 r1 r3 r3]
    auto a = __builtin_amdgcn_permlane32_swap(s16[0], s16[0], false, false);                           // [r0 x4] , [r2 x4]
    auto b = __builtin_amdgcn_permlane32_swap(s16[1], s16[1], false, false);                           // [r1 x4] , [r3 x4]
    R[0] = i2f((int)a[0]); R[2] = i2f((int)a[1]); R[1] = i2f((int)b[0]); R[3] = i2f((int)b[1]);
    // 2 wait states between the swaps (VALU writes) and the first DPP read of R[] in the asm FMAs
    asm volatile("s_nop 1" : "+v"(R[0]), "+v"(R[1]), "+v"(R[2]), "+v"(R[3]));
}

__device__ __forceinline__ void atomic_add(float *p, float v) { unsafeAtomicAdd(p, v); }
__device__ __forceinline__ void atomic_add(double *p, double v) { unsafeAtomicAdd(p, v); }

}  // namespace hode

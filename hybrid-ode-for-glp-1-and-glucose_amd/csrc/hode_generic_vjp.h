// hode_generic_vjp.h -- the REVERSE right-hand side of the generic network path and the two kernels built on it: K5
// (rhs_bwd_generic_kernel, one wave per sample) and the one-trajectory K4 (solve_bwd_generic_kernel, a team of waves per trajectory).
// Both are templates on GIN: true adds the gradients of the external inputs (d/d meal, tVNS, GD; include/hode.h
// hode_{solve,rhs}_bwd_inputs_*), false is the production adjoint.  Two translation units instantiate them -- hode_generic_bwd.hip
// (GIN = false) and hode_generic_gin.hip (GIN = true) -- and must stay two: hipcc schedules a kernel template differently once a
// second variant of it shares the file, and the production instantiations are to keep their code exactly.
#pragma once
#include "hode_generic_rhs.h"
#include "hode_adjoint.h"

namespace hode {

// J^T kb for an arbitrary network from a stage record.  g: gradient vector of this parameter set (or nullptr).
// NW > 1: a TEAM of NW waves works on the same stage of the same trajectory (solve_bwd_generic_kernel).  Every wave runs the whole
// function on identical data -- identical results, identical control flow -- except for the two loops over the rows of a hidden
// matrix, which are split: wave `part` takes rows [j0, j1) of W^T delta (partial sums exchanged through xch[NW][2][64] in LDS and
// added in wave order) and of the atomics dW += delta (x) h_in.  A trajectory of such a network is one long chain of L2 round
// trips; with the batches these shapes are trained on (32 trajectories) one wave per trajectory left 97 % of the chip idle.
// Register accumulators of a team wave for its eight rows of up to kGenAccMats hidden matrices (fp32 adjoint of the solve, H <=
// 8 NW, L - 1 <= kGenAccMats): dW[j0 + u][lane], dW[j0 + u][lane + 64].  With them the hidden-matrix gradients leave the chip once
// per workgroup instead of once per stage (280 KB of atomics per stage of the 5 x 128 network: what bound the adjoint above a few
// hundred trajectories).  NoAcc: the atomics of round 2 (K5, fp64, deeper networks).
struct NoAcc {};
template <int RPW> struct TeamAccT {
    static constexpr int kRows = RPW;          // rows of every hidden matrix this wave owns: 8 (H <= 8 NW) or 16 (H <= 16 NW)
    // four separate arrays, not one [4][8][2]: hipcc folds a switch over identical case bodies into a dynamically indexed access,
    // and a dynamically indexed register array lives in scratch
    float m0[RPW][2], m1[RPW][2], m2[RPW][2], m3[RPW][2];
    // The gradients of everything that is NOT a hidden matrix -- first layer, output layer, every bias: 2 566 values for 5 x 128 --
    // were the other half of the adjoint's time as atomics (every team adds to the same 10 KB at every stage: 92 ms -> 46 ms for
    // 1 024 x 61 without them, 8.7 -> 6.7 ms for 32 x 61).  All waves of a team hold the same cotangents, so the pieces are dealt
    // out over the waves, twelve registers each (units j = lane and lane + 64 in [.][0] and [.][1]):
    //   wave 0: the six rows of the output matrix             wave 1: columns 0..4 of the first matrix, and the output bias
    //   wave 2: columns 5..8 of the first matrix, its bias     wave 3 + l: the bias of hidden matrix l
    float e[6][2];
    static constexpr int kEdgeOut = 0, kEdgeIn0 = 1, kEdgeIn1 = 2, kEdgeBias = 3;
    __device__ __forceinline__ void zero()
    {
#pragma unroll
        for (int u = 0; u < RPW; ++u) m0[u][0] = m0[u][1] = m1[u][0] = m1[u][1] = m2[u][0] = m2[u][1] = m3[u][0] = m3[u][1] = 0.f;
#pragma unroll
        for (int u = 0; u < 6; ++u) e[u][0] = e[u][1] = 0.f;
    }
    // ST: the workgroup owns g (its gradient ROW, solve_bwd_generic_kernel): plain stores, no atomics
    template <bool ST> static __device__ __forceinline__ void emit(float *p, float v)
    {
        if constexpr (ST) *p = v; else atomic_add(p, v);
    }
    // one atomic per entry and WORKGROUP for this wave's edge piece
    template <bool ST> __device__ __forceinline__ void flush_edge(const StreamNet<float> &n, float *__restrict__ g, int part, int lane)
    {
        const int H = n.H;
        const bool vA = lane < H, vB = lane + 64 < H;
        if (part == kEdgeOut) {
#pragma unroll
            for (int q = 0; q < 6; ++q) {
                if (vA) emit<ST>(g + n.out_off() + q * H + lane, e[q][0]);
                if (vB) emit<ST>(g + n.out_off() + q * H + lane + 64, e[q][1]);
            }
        } else if (part == kEdgeIn0) {
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                if (vA) emit<ST>(g + lane * 9 + i, e[i][0]);
                if (vB) emit<ST>(g + (lane + 64) * 9 + i, e[i][1]);
            }
            if (lane < 6) emit<ST>(g + n.out_off() + 6 * H + lane, e[5][0]);
        } else if (part == kEdgeIn1) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (vA) emit<ST>(g + lane * 9 + 5 + i, e[i][0]);
                if (vB) emit<ST>(g + (lane + 64) * 9 + 5 + i, e[i][1]);
            }
            if (vA) emit<ST>(g + 9 * H + lane, e[4][0]);
            if (vB) emit<ST>(g + 9 * H + lane + 64, e[4][1]);
        } else if (part - kEdgeBias < n.L - 1) {
            float *__restrict__ gb = g + n.hid_off(part - kEdgeBias) + (size_t)H * H;
            if (vA) emit<ST>(gb + lane, e[0][0]);
            if (vB) emit<ST>(gb + lane + 64, e[0][1]);
        }
    }
    // accumulators of the matrix at compile-time position SLOT (0 = the LAST hidden matrix, see rhs_vjp_stream), row u of this wave
    template <int SLOT> __device__ __forceinline__ void fma(int u, float dj, float inA, float inB)
    {
        static_assert(SLOT >= 0 && SLOT < 4, "kGenAccMats");
        float(&m)[RPW][2] = SLOT == 0 ? m0 : SLOT == 1 ? m1 : SLOT == 2 ? m2 : m3;
        m[u][0] = __builtin_fmaf(dj, inA, m[u][0]);
        m[u][1] = __builtin_fmaf(dj, inB, m[u][1]);
    }
    template <bool ST> __device__ __forceinline__ void flush_one(const float (&m)[RPW][2], float *__restrict__ gW, int H, int j0, int lane)
    {
#pragma unroll
        for (int u = 0; u < RPW; ++u) {
            const int j = j0 + u;
            if (j < H) {
                if (lane < H) emit<ST>(gW + (size_t)j * H + lane, m[u][0]);
                if (lane + 64 < H) emit<ST>(gW + (size_t)j * H + lane + 64, m[u][1]);
            }
        }
    }
    // one atomic per entry and WORKGROUP (after all its trajectories of a parameter set)
    template <bool ST = false> __device__ __forceinline__ void flush(const StreamNet<float> &n, float *__restrict__ g, int j0, int lane, int part)
    {
        if (g == nullptr) return;
        flush_edge<ST>(n, g, part, lane);
        const int nm = n.L - 1;                            // slot i holds hidden matrix nm - 1 - i
        if (nm > 0) flush_one<ST>(m0, g + n.hid_off(nm - 1), n.H, j0, lane);
        if (nm > 1) flush_one<ST>(m1, g + n.hid_off(nm - 2), n.H, j0, lane);
        if (nm > 2) flush_one<ST>(m2, g + n.hid_off(nm - 3), n.H, j0, lane);
        if (nm > 3) flush_one<ST>(m3, g + n.hid_off(nm - 4), n.H, j0, lane);
    }
};

template <typename T> struct IsTeamAcc { static constexpr bool v = false; static constexpr int rows = 8; };
template <int RPW> struct IsTeamAcc<TeamAccT<RPW>> { static constexpr bool v = true; static constexpr int rows = RPW; };

// GIN: *gin_out = the input cotangents of this evaluation (input_vjp, hode_adjoint.h); otherwise gin_out is not touched (nullptr).
template <typename R, bool GODE, bool GT, int NW = 1, typename ACC = NoAcc, typename EW = EdgeFromParams<R>, bool GIN = false>
__device__ __forceinline__ R rhs_vjp_stream(const StreamNet<R> &n, const EW &ew, R *__restrict__ g, const OdeP<R> &o, R t, R tvns, R gde, R gd_in,
                                            bool use_gd, int lane, const R *__restrict__ rec, R kb, R &go, R *gt_out, int part,
                                            R *__restrict__ xch, ACC &acc, int &xpar, R *gin_out)
{
    const int H = n.H, L = n.L;
    const R *__restrict__ sx = rec + 2 * L * kWave;            // the stage state: wave-uniform loads
    const R G = sx[0], I = sx[1], Glu = sx[2], GLP1 = sx[3], GE = sx[4], FFA = sx[5];
    const R lq[6] = {lane_bcast(kb, 0), lane_bcast(kb, 1), lane_bcast(kb, 2), lane_bcast(kb, 3), lane_bcast(kb, 4), lane_bcast(kb, 5)};
    const int c8 = lane & 7;
    const R mech = mech_vjp<R, GODE>(o, G, I, Glu, GLP1, FFA, lq[0], lq[1], lq[2], lq[3], lq[5], gde, gd_in, use_gd, lane, go);
    const bool vA = lane < H, vB = lane + 64 < H;
    const int jA = vA ? lane : 0, jB = vB ? lane + 64 : 0;
    // this wave's rows of every hidden matrix (multiples of 8: the chunked loads below), and who adds the non-matrix gradients
    const int rows_per = (((H + NW - 1) / NW) + 7) & ~7;
    const int j0 = (part * rows_per < H) ? part * rows_per : H, j1 = (j0 + rows_per < H) ? j0 + rows_per : H;
    constexpr bool kAcc = IsTeamAcc<ACC>::v;
    using TeamAcc = TeamAccT<IsTeamAcc<ACC>::rows>;       // (the edge-piece constants; the type itself only when kAcc)
    R *__restrict__ dloc = kAcc ? xch + (NW * 4 + part * 2) * kWave : nullptr;       // this wave's delta slice (kernel: xch[NW * 6 * 64])
    // biases, first and last layer: atomics of the team's first wave -- or, with register accumulators, dealt out over the waves
    R *__restrict__ gedge = (part == 0 && !kAcc) ? g : nullptr;
    // output layer
    R hA = rec[(2 * (L - 1)) * kWave + lane], hB = rec[(2 * (L - 1) + 1) * kWave + lane];
    R dA = R(0), dB = R(0);
#pragma unroll
    for (int q = 0; q < 6; ++q) {
        dA = rfma(ew.Wo()[q * H + jA], lq[q], dA);
        dB = rfma(ew.Wo()[q * H + jB], lq[q], dB);
        if (gedge) {
            if (vA) atomic_add(gedge + n.out_off() + q * H + jA, lq[q] * hA);
            if (vB) atomic_add(gedge + n.out_off() + q * H + jB, lq[q] * hB);
        }
    }
    if (gedge && lane < 6) atomic_add(gedge + n.out_off() + 6 * H + lane, kb);
    if constexpr (kAcc) {
        if (g) {
            if (part == TeamAcc::kEdgeOut) {
#pragma unroll
                for (int q = 0; q < 6; ++q) { acc.e[q][0] = rfma(lq[q], hA, acc.e[q][0]); acc.e[q][1] = rfma(lq[q], hB, acc.e[q][1]); }
            } else if (part == TeamAcc::kEdgeIn0) {
                acc.e[5][0] += kb;                             // output bias: lanes 0..5 carry the six components
            }
        }
    }
    dA = vA ? act_bwd(dA, hA, n.act) : R(0);
    dB = vB ? act_bwd(dB, hB, n.act) : R(0);
    // hidden matrices, last to first: matrix l maps h_l (rows 2l, 2l+1 of the record) to h_{l+1}
    // one hidden matrix; `slot` = the matrix's position counted from the LAST one, as a compile-time constant (TeamAcc only)
    auto hidden_bwd = [&](const int l, auto slot) {
        const R inA = rec[(2 * l) * kWave + lane], inB = rec[(2 * l + 1) * kWave + lane];
        if constexpr (kAcc) {
            // delta_{l+1} of this wave into ITS slice of LDS: the sixteen delta_j of the wave's rows then come back as two or four
            // 16-byte broadcast reads instead of sixteen v_readlane from a run-time lane (select + readlane + copy each)
            dloc[lane] = dA;
            dloc[kWave + lane] = dB;
        }
        const R *__restrict__ W = n.Wh(l);
        R *__restrict__ gW = g ? g + n.hid_off(l) : nullptr;
        if (gedge) {
            if (vA) atomic_add(gW + (size_t)H * H + jA, dA);
            if (vB) atomic_add(gW + (size_t)H * H + jB, dB);
        }
        if constexpr (kAcc) {
            if (g && part == TeamAcc::kEdgeBias + l) { acc.e[0][0] += dA; acc.e[0][1] += dB; }    // d is 0 on masked lanes
        }
        // Two passes over the rows.  vmcnt retires in issue order, so a load issued behind an atomic waits for that atomic's
        // round trip to memory: with loads and atomics interleaved row by row every chunk of loads waited ~1 000 cycles for
        // the previous chunk's atomics (29 ms per 32 x 61 adjoint of the 5 x 128 network).  Pass 1 only loads (W^T delta),
        // pass 2 only adds (dW += delta (x) h_in).
        R pA = R(0), pB = R(0);
        int j = j0;
        // (unsigned column offsets on a running wave-uniform row pointer: two scalar adds and two loads per row.  With `int` columns
        //  and row * H recomputed per row hipcc spent six scalar and two 64-bit vector instructions on every row's addresses --
        //  a quarter of the instructions of a stage, and the adjoint is bound by what its waves issue)
        // fp32: BUFFER loads -- descriptor of the matrix in four SGPRs, the lane's column as a 32-bit VGPR byte offset, the row as
        // the instruction's scalar offset: one scalar add and two loads per row.  As flat global loads hipcc spent six scalar and two
        // 64-bit vector instructions on every row's addresses (a quarter of a stage's instructions, and the adjoint is bound by what
        // its waves issue); precomputed per-lane row offsets cost 32 VGPRs and spill.
        const unsigned oA = (unsigned)jA * (unsigned)sizeof(R), oB = (unsigned)jB * (unsigned)sizeof(R);   // byte offsets of the lane's columns
        unsigned roff = (unsigned)j0 * (unsigned)H * (unsigned)sizeof(R);                                   // byte offset of row j in the matrix
        const unsigned rstride = (unsigned)H * (unsigned)sizeof(R);
        auto ld = [&](unsigned o) -> R {
            if constexpr (sizeof(R) == 4) {
                const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<R *>(W), 0, (int)((unsigned)H * (unsigned)H * 4u), 0x00020000);
                return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, (int)o, (int)roff, 0));
            } else {
                return *reinterpret_cast<const R *>(reinterpret_cast<const char *>(W) + roff + o);
            }
        };
        for (; j + 8 <= j1; j += 8) {                          // eight rows at a time: 16 independent loads in flight
            R wA[8], wB[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                wA[u] = ld(oA);                                 // column jA / jB of row j: 256 contiguous bytes per wave
                wB[u] = ld(oB);
                roff += rstride;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                R dj;
                if constexpr (kAcc) dj = dloc[j + u];          // (own write above: LDS is in order per wave)
                else dj = unit_bcast(dA, dB, j + u);           // a dead unit (ReLU, dj == 0) adds nothing
                pA = rfma(wA[u], dj, pA);
                pB = rfma(wB[u], dj, pB);
            }
        }
        for (; j < j1; ++j) {
            const R dj = unit_bcast(dA, dB, j);
            pA = rfma(ld(oA), dj, pA);
            pB = rfma(ld(oB), dj, pB);
            roff += rstride;
        }
        if constexpr (NW > 1) {
            // partial sums of the team, added in wave order on every wave (same bits everywhere).  Two exchange areas used in turn
            // (xpar: a toggle that runs on across layers AND stages): the writes of the next exchange go to the other area, so ONE
            // barrier per layer is enough -- a wave can be at most one barrier ahead of the slowest reader of the area it writes
            // next but one
            R *__restrict__ xl = xch + xpar * (NW * 2 * kWave);
            xpar ^= 1;
            xl[(part * 2 + 0) * kWave + lane] = pA;
            xl[(part * 2 + 1) * kWave + lane] = pB;
            __syncthreads();
            pA = R(0); pB = R(0);
#pragma unroll
            for (int w = 0; w < NW; ++w) { pA += xl[(w * 2 + 0) * kWave + lane]; pB += xl[(w * 2 + 1) * kWave + lane]; }
        }
        if constexpr (kAcc) {
            if (g) {
                // this wave's rows of dW += delta (x) h_in (masked lanes: h_in = 0), straight into the registers of `slot`
#pragma unroll
                for (int u = 0; u < IsTeamAcc<ACC>::rows; ++u)      // (rows beyond H: delta is zero there -- dloc holds all 128 entries)
                    acc.template fma<decltype(slot)::value>(u, dloc[j0 + u], inA, inB);
            }
        } else if (g) {
            for (j = j0; j < j1; ++j) {
                const R dj = unit_bcast(dA, dB, j);
                if (dj == R(0)) continue;                      // wave-uniform: no atomics for dead units
                if (vA) atomic_add(gW + (size_t)j * H + jA, dj * inA);
                if (vB) atomic_add(gW + (size_t)j * H + jB, dj * inB);
            }
        }
        dA = vA ? act_bwd(pA, inA, n.act) : R(0);
        dB = vB ? act_bwd(pB, inB, n.act) : R(0);
    };
    if constexpr (kAcc) {
        // The accumulators must be addressed by a COMPILE-TIME index.  With the matrix index a run-time value hipcc merges the four
        // "which matrix" branches into one body that addresses the accumulators through a selected offset -- and an array with a
        // dynamic offset lives in scratch: sixteen scratch_load / s_waitcnt vmcnt(0) / v_fmac / scratch_store round trips per
        // matrix and stage (472 B of scratch; 79 % of the wave's time in waits, tools/pmc_generic.sh).  A fixed-trip loop over
        // the POSITION of the matrix from the last one unrolls fully and makes that position a constant.
#pragma unroll
        for (int i = 0; i < kGenAccMats; ++i) {
            if (i > L - 2) break;
            if (i == 0) hidden_bwd(L - 2, std::integral_constant<int, 0>{});
            else if (i == 1) hidden_bwd(L - 3, std::integral_constant<int, 1>{});
            else if (i == 2) hidden_bwd(L - 4, std::integral_constant<int, 2>{});
            else hidden_bwd(L - 5, std::integral_constant<int, 3>{});
        }
    } else {
        for (int l = L - 2; l >= 0; --l) hidden_bwd(l, std::integral_constant<int, 0>{});
    }
    // first layer: input row [t, G, I, Glu, GLP1, GE, FFA, glp1 := GLP1, tvns]
    const R in[9] = {t, G, I, Glu, GLP1, GE, FFA, GLP1, tvns};
    if (gedge) {
        if (vA) atomic_add(gedge + 9 * H + jA, dA);
        if (vB) atomic_add(gedge + 9 * H + jB, dB);
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            if (vA) atomic_add(gedge + jA * 9 + i, dA * in[i]);
            if (vB) atomic_add(gedge + jB * 9 + i, dB * in[i]);
        }
    }
    if constexpr (kAcc) {
        if (g) {
            if (part == TeamAcc::kEdgeIn0) {
#pragma unroll
                for (int i = 0; i < 5; ++i) { acc.e[i][0] = rfma(dA, in[i], acc.e[i][0]); acc.e[i][1] = rfma(dB, in[i], acc.e[i][1]); }
            } else if (part == TeamAcc::kEdgeIn1) {
#pragma unroll
                for (int i = 0; i < 4; ++i) { acc.e[i][0] = rfma(dA, in[5 + i], acc.e[i][0]); acc.e[i][1] = rfma(dB, in[5 + i], acc.e[i][1]); }
                acc.e[4][0] += dA;
                acc.e[4][1] += dB;
            }
        }
    }
    R w[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) w[i] = ew.W1()[jA * 9 + i] * dA + ew.W1()[jB * 9 + i] * dB;       // d is 0 on masked lanes
    const R p[6] = {w[1], w[2], w[3], w[4] + w[7], w[5], w[6]};                                   // GLP1 feeds inputs 4 and 7
    const R nn = wave_reduce6_to_lanes(p, lane);
    if constexpr (GT) *gt_out = wave_allsum(w[0]);
    if constexpr (GIN) *gin_out = input_vjp(o, G, lq[0], wave_allsum(w[8]), gd_in, use_gd, lane);
    return (c8 < 6) ? (mech + nn) : R(0);
}

// ------------------------------------------------------------------------------------------ K5
template <typename R, bool GODE, bool GIN>
__global__ __launch_bounds__(256) void rhs_bwd_generic_kernel(const RhsArgs<R> a, int L)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int lane = threadIdx.x & 63;
    const int wave = first_lane((int)(threadIdx.x >> 6));
    R *rec = reinterpret_cast<R *>(smem_raw) + (size_t)wave * (2 * L * kWave + 8);      // this wave's record
    const StreamNet<R> n{a.nn_p, a.H, L, a.act};
    OdeP<R> o;
    ode_load(o, a.ode_p);
    R go = R(0);
    for (int s = blockIdx.x * 4 + wave; s < a.B; s += gridDim.x * 4) {
        const R Y = (lane < 6) ? a.x[(size_t)s * 6 + lane] : R(0);
        const R kb = (lane < 6) ? a.gout[(size_t)s * 6 + lane] : R(0);
        const R t = a.t ? a.t[s] : R(0), tvns = a.tvns ? a.tvns[s] : R(0), gdv = a.gd ? a.gd[s] : R(0);
        const R gde = a.gd ? gd_effect(o, gdv) : R(0);
        (void)rhs_stream<R>(n, EdgeFromParams<R>{n}, o, t, Y, a.meal ? a.meal[s] : R(0), tvns, gde, lane, rec);
        __builtin_amdgcn_wave_barrier();
        R gt, cin;                                               // (cin: GIN only)
        NoAcc na;
        int xpar = 0;                                            // (one wave per sample: no exchange)
        const R Z = rhs_vjp_stream<R, GODE, true, 1, NoAcc, EdgeFromParams<R>, GIN>(n, EdgeFromParams<R>{n}, a.gnn, o, t, tvns, gde, gdv, a.gd != nullptr, lane,
                                                                                   rec, kb, go, &gt, 0, (R *)nullptr, na, xpar, GIN ? &cin : nullptr);
        __builtin_amdgcn_wave_barrier();
        if (lane < 6) a.gx[(size_t)s * 6 + lane] = Z;
        if (a.gt && lane == 0) a.gt[s] = gt;
        if constexpr (GIN) {
            // lane 2q holds input q's cotangent (input_vjp)
            R *__restrict__ gq = (lane == 0) ? a.gmeal : (lane == 2) ? a.gtvns : (lane == 4) ? a.ggd : nullptr;
            if (gq) gq[s] = cin;
        }
    }
    if constexpr (GODE) {
        if (a.gode && lane < 17) atomic_add(a.gode + lane, go);
    }
}

template <typename R, bool GIN> static int launch_rhs_bwd_generic_t(hipStream_t s, const RhsArgs<R> &a, int L)
{
    int blocks = (a.B + 3) / 4;
    if (blocks > 1024) blocks = 1024;
    if (blocks < 1) return HODE_OK;
    const size_t lds = (size_t)4 * (2 * L * kWave + 8) * sizeof(R);
    if (a.gode) hipLaunchKernelGGL((rhs_bwd_generic_kernel<R, true, GIN>), dim3(blocks), dim3(256), lds, s, a, L);
    else hipLaunchKernelGGL((rhs_bwd_generic_kernel<R, false, GIN>), dim3(blocks), dim3(256), lds, s, a, L);
    return hipGetLastError() == hipSuccess ? HODE_OK : HODE_ELAUNCH;
}

// ------------------------------------------------------------------------------------------ K4
// Same walk over the tape as solve_bwd_kernel (hode_solve_bwd.hip); records are read from HBM with plain loads (L2 hits: the
// forward has just written them).  Teams of 8 waves (16 for the atomics variant above 64 hidden units); ACCREG: the team's
// register accumulators (TeamAccT), else gradients leave through atomics inside rhs_vjp_stream (fp64, more than four hidden
// matrices, no parameter gradient wanted).  GIN: also the gradients of the external inputs (GinCarry; the argument block is AdjInArgs).
template <typename R, bool GODE, bool GD, int kGenTeam, int ACCREG, bool GIN>      // ACCREG: accumulator rows per wave (8 / 16), 0 = atomics
__global__ __launch_bounds__(64 * kGenTeam) void solve_bwd_generic_kernel(const AdjArgsT<R, GIN> a, const int method, const int L, const int rows_grid)
{
    using Acc = std::conditional_t<ACCREG != 0, TeamAccT<ACCREG ? ACCREG : 8>, NoAcc>;
    Acc acc;
    int acc_set = -1;                                       // the parameter set the accumulators belong to
    __shared__ R rowsT[8 * kWave];
    __shared__ R xch[kGenTeam * 6 * kWave];                  // partial sums, two areas [2][NW][2][64] | every wave's delta slice [NW][2][64]
    __shared__ R edge_img[kEdgeImageMax];                   // the edge parameters of the current set (EdgeImage)
    int img_set = -1;
    int xpar = 0;                                           // which of the two exchange areas the next layer writes (rhs_vjp_stream)
    const int lane = threadIdx.x & 63;
    const int part = first_lane((int)(threadIdx.x >> 6));      // every wave of the team walks the tape; the matrix rows are split
    const int c8 = lane & 7, grp = lane >> 3;
    const int T = a.T;
    const TableauData &tab = kTableau[method];
    const int S = tab.S;
    const int kSlot = 2 * L * kWave + 8;
    tableau_rowsT_store<R>(rowsT, method, threadIdx.x, 64 * kGenTeam);
    __syncthreads();
    const int per_set = a.B / a.n_sets;
    constexpr bool use_gd = GD;
    const int rows_per_k = (((a.H + kGenTeam - 1) / kGenTeam) + 7) & ~7;
    const int j0_k = (part * rows_per_k < a.H) ? part * rows_per_k : a.H;
    // ROWS mode (a 2-D grid: blockIdx.y = parameter set, register accumulators, a partials area): the workgroup serves trajectories
    // of ONE set and leaves its gradient as ONE row of a.partials with plain stores; adj_reduce_kernel adds the rows of a set in
    // workgroup order -- no floating-point atomics, the same bits run to run (the tuned path's scheme, round 4 for these shapes).
    const bool rows_mode = ACCREG != 0 && rows_grid != 0;
    R go_sum = R(0);
    R *__restrict__ prow = nullptr;
    if (rows_mode) {
        const size_t rowlen = adj_partial_rowlen(a.P);
        prow = a.partials + (size_t)(blockIdx.y * gridDim.x + blockIdx.x) * rowlen;
        for (size_t i = threadIdx.x; i < rowlen; i += 64 * kGenTeam) prow[i] = R(0);
        __syncthreads();
    }
    const int b_first = rows_mode ? (int)blockIdx.y * per_set + (int)blockIdx.x : (int)blockIdx.x;
    const int b_end = rows_mode ? ((int)blockIdx.y + 1) * per_set : a.B;
    for (int b = b_first; b < b_end; b += gridDim.x) {
        const int set = b / per_set;
        const StreamNet<R> n{a.nn_p + (size_t)set * a.P, a.H, L, a.act};
        R *__restrict__ g = a.gnn ? a.gnn + (size_t)set * a.P : nullptr;
        if (set != img_set) {                               // (every wave of the workgroup walks the same b: uniform branch)
            __syncthreads();                                // nobody reads the previous set's image any more
            EdgeImage<R>::fill(edge_img, n, threadIdx.x, 64 * kGenTeam);
            __syncthreads();
            img_set = set;
        }
        const EdgeImage<R> ew{edge_img, a.H, L};
        if constexpr (ACCREG != 0) {
            if (set != acc_set) {                           // a workgroup's trajectories come set by set: flush when the set changes
                if (acc_set >= 0) acc.flush(StreamNet<R>{a.nn_p + (size_t)acc_set * a.P, a.H, L, a.act}, a.gnn ? a.gnn + (size_t)acc_set * a.P : nullptr, j0_k, lane, part);
                acc.zero();
                acc_set = set;
            }
        }
        OdeP<R> o;
        ode_load(o, a.ode_p + 17 * set);
        const R *__restrict__ tg = a.t + (a.t_batched ? (size_t)b * T : 0);
        const R *__restrict__ tape = a.tape + (size_t)b * a.max_steps * 8;
        const int *__restrict__ tseg = a.tape_seg + (size_t)b * a.max_steps;
        const R *__restrict__ stg = a.tape_stage + (size_t)b * a.max_steps * 6 * kSlot;
        const R *__restrict__ gyb = a.gy + (size_t)b * T * 6;
        const int nst = a.nsteps[b] < a.max_steps ? a.nsteps[b] : a.max_steps;
        const bool ok = a.status[b] == HODE_ST_OK;
        auto gy_row = [&](int r) -> R { return (c8 < 6) ? gyb[(size_t)r * 6 + c8] : R(0); };
        R lam = R(0), go = R(0);
        int knext = T - 1;
        // GIN: input gradients in the one-register layout and with the flush rule of solve_bwd_kernel (hode_solve_bwd.hip, where the comment
        // on `gin` explains both); every wave of the team carries the same sums, the team's first wave writes.  Dead code without GIN.
        // (Three locals and a lambda, as there, not a carrier struct with member functions: with the sums as members hipcc orders the
        //  input-gradient kernels' instructions differently -- same registers, 1.4 % slower at 5 x 128, B = 32 -- and with gin_row() in
        //  place of the conditionals below the register and scratch figures of all 24 of them change.)
        R gin = R(0);
        int kin = T, whi = T - 1;                          // interval of the sums in gin (T: none yet); rows above whi are written
        auto gin_flush = [&](int knew) {
            if constexpr (GIN) {
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    R *__restrict__ gq = (q == 0) ? a.gmeal : (q == 1) ? a.gtvns : a.ggd;
                    const int mq = (q == 0) ? a.meal_mode : (q == 1) ? a.tvns_mode : a.gd_mode;
                    if (gq == nullptr || mq != 2) continue;
                    const R lo = lane_bcast(gin, 2 * q), up = lane_bcast(gin, 2 * q + 1);
                    for (int r = knew + 2; r <= whi; ++r)
                        if (part == 0 && lane == 0) gq[(size_t)b * T + r] = (r == kin + 1) ? up : (r == kin) ? lo : R(0);
                }
                const bool row2 = ((lane >> 1) == 0) ? a.meal_mode == 2 : ((lane >> 1) == 1) ? a.tvns_mode == 2 : a.gd_mode == 2;
                const R nb = xlane_xor1(gin);
                gin = row2 ? (((lane & 1) && kin == knew + 1) ? nb : R(0)) : gin;
                kin = knew;
                whi = knew + 1;
            }
        };
        for (int st = nst - 1; st >= 0; --st) {
            const int kraw = tseg[st];
            const int k = kraw & (kSegClosed - 1);
            if constexpr (GIN) {
                if (k != kin) gin_flush(k);
            }
            int hi = knext;                                   // rows this step produced: see solve_bwd_kernel
            if (st == nst - 1) {
                hi = T - 1;
                if (!ok) {
                    hi = k;
                    if (kraw & kSegClosed) {
                        hi = k + 1;
                        while (hi + 1 < T && !(tg[hi + 1] > tg[hi])) ++hi;
                    }
                }
            }
            for (int r = k + 1; r <= hi; ++r) lam += gy_row(r);
            knext = k;
            const R tc = tape[(size_t)st * 8 + 0], h = tape[(size_t)st * 8 + 1];
            const R t0 = tg[k], t1 = tg[k + 1];
            const R v0 = inp_at(a.tvns, a.tvns_mode, b, T, k), v1 = inp_at(a.tvns, a.tvns_mode, b, T, k + 1);
            const R d0 = inp_at(a.gd, a.gd_mode, b, T, k), d1 = inp_at(a.gd, a.gd_mode, b, T, k + 1);
            const R inv_len = first_lane(R(1) / (t1 - t0));
            const R dv = first_lane(v1 - v0), dd = first_lane(d1 - d0);
            R ZZ = R(0);
            for (int s = S - 1; s >= 0; --s) {
                const R bw_s = rowsT[6 * kWave + s], c_s = rowsT[6 * kWave + 8 + s];
                const R kb = h * rfma(bw_s, lam, group_sum8(rowsT[s * kWave + lane] * ZZ));
                const R ts = rfma(c_s, h, tc);
                const R al = (ts - t0) * inv_len;
                const R gdv = rfma(al, dd, d0);
                R gde = R(0);
                if constexpr (use_gd) gde = gd_effect(o, gdv);
                R cin;                                          // (GIN only)
                const R Z = rhs_vjp_stream<R, GODE, false, kGenTeam, Acc, EdgeImage<R>, GIN>(n, ew, g, o, ts, rfma(al, dv, v0), gde, gdv, use_gd, lane,
                                                                               stg + ((size_t)st * 6 + s) * kSlot, kb, go, nullptr, part, xch, acc, xpar,
                                                                               GIN ? &cin : nullptr);
                if constexpr (GIN) {
                    const int mq = ((lane >> 1) == 0) ? a.meal_mode : ((lane >> 1) == 1) ? a.tvns_mode : a.gd_mode;
                    const R w = (mq == 2) ? ((lane & 1) ? al : R(1) - al) : (mq == 1 && !(lane & 1)) ? R(1) : R(0);
                    gin = rfma(w, cin, gin);
                }
                ZZ = (grp == s) ? Z : ZZ;
            }
            lam += group_sum8(rowsT[7 * kWave + lane] * ZZ);
        }
        int kf = 0;                                           // rows 0..kf are (copies of) x0
        while (kf + 1 < T && !(tg[kf + 1] > tg[kf])) ++kf;
        for (int r = 0; r <= kf; ++r) lam += gy_row(r);
        if constexpr (GIN) {
            gin_flush(-2);                                    // rows 0 .. whi
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                R *__restrict__ gq = (q == 0) ? a.gmeal : (q == 1) ? a.gtvns : a.ggd;
                const int mq = (q == 0) ? a.meal_mode : (q == 1) ? a.tvns_mode : a.gd_mode;
                const R v = lane_bcast(gin, 2 * q);
                if (gq != nullptr && mq == 1 && part == 0 && lane == 0) gq[b] = v;
            }
        }
        if (part == 0) {
            if (lane < 6) a.gx0[(size_t)b * 6 + lane] = lam;
            if constexpr (GODE) {
                if (rows_mode) go_sum += go;
                else if (a.gode && lane < 17) atomic_add(a.gode + 17 * set + lane, go);
            }
        }
    }
    if constexpr (ACCREG != 0) {
        if (rows_mode) {
            if (acc_set >= 0) acc.template flush<true>(StreamNet<R>{a.nn_p + (size_t)acc_set * a.P, a.H, L, a.act}, prow, j0_k, lane, part);
            if constexpr (GODE) {
                if (part == 0 && lane < 17) prow[a.P + lane] = go_sum;
            }
        } else if (acc_set >= 0) {
            acc.flush(StreamNet<R>{a.nn_p + (size_t)acc_set * a.P, a.H, L, a.act}, a.gnn ? a.gnn + (size_t)acc_set * a.P : nullptr, j0_k, lane, part);
        }
    }
}

template <typename R, int NW, int ACCREG, bool GIN> static int launch_bwd_generic_t(hipStream_t s, const AdjArgsT<R, GIN> &a, int L, int method)
{
    // with register accumulators a workgroup flushes once: fewer, longer-lived workgroups (a few per CU) beat one per trajectory
    int blocks = a.B < 4096 ? a.B : 4096;
    if (ACCREG && blocks > 1024) blocks = 1024;
    dim3 grid(blocks);
    const dim3 block(64 * NW);
    // gradient rows instead of atomics (fp32 register accumulators, enough rows for one workgroup per set at least)
    const int per_set = a.B / a.n_sets;
    int bps = 0;
    if constexpr (ACCREG != 0 && sizeof(R) == 4) {
        if (a.partials != nullptr && a.gnn != nullptr && a.n_sets <= a.partial_rows && a.n_sets <= 65535) {
            bps = a.partial_rows / a.n_sets;
            if (bps > per_set) bps = per_set;
            if (bps > 1024) bps = 1024;
            if (bps < 1) bps = 1;
            grid = dim3(bps, a.n_sets);
        }
    }
    const bool gd = a.gd_mode != 0;
    if (a.gode) {
        if (gd) hipLaunchKernelGGL((solve_bwd_generic_kernel<R, true, true, NW, ACCREG, GIN>), grid, block, 0, s, a, method, L, bps > 0 ? 1 : 0);
        else hipLaunchKernelGGL((solve_bwd_generic_kernel<R, true, false, NW, ACCREG, GIN>), grid, block, 0, s, a, method, L, bps > 0 ? 1 : 0);
    } else {
        if (gd) hipLaunchKernelGGL((solve_bwd_generic_kernel<R, false, true, NW, ACCREG, GIN>), grid, block, 0, s, a, method, L, bps > 0 ? 1 : 0);
        else hipLaunchKernelGGL((solve_bwd_generic_kernel<R, false, false, NW, ACCREG, GIN>), grid, block, 0, s, a, method, L, bps > 0 ? 1 : 0);
    }
    if constexpr (sizeof(R) == 4) {
        if (bps > 0)
            launch_adj_reduce(s, reinterpret_cast<const float *>(a.partials), (int)adj_partial_rowlen(a.P), bps, a.n_sets, a.P,
                              reinterpret_cast<float *>(a.gnn), reinterpret_cast<float *>(a.gode));
    }
    return hipGetLastError() == hipSuccess ? HODE_OK : HODE_ELAUNCH;
}

}  // namespace hode

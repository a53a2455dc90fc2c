// hode_generic_rhs.h -- the FORWARD right-hand side of the generic network path: f(t, x, u) for any MLP up to 8 x 128, as one wave
// walking the matrices (rhs_stream: K1 / K5 and the stage records they make), as a team of waves that splits the hidden layers by
// output rows (rhs_rows), and as a team that serves several trajectories at once (RhsMulti); RhsStream / RhsMulti are the functors
// solve_one (hode_solve_body.h) integrates.  Used by: hode_generic.hip (K1, K2 + K3), hode_generic_vjp.h (K5 records its stage with
// rhs_stream), hode_generic_bwd_multi.hip (kGenAccMats).  Nothing of the adjoint is in here.
#pragma once
#include "hode_solve_body.h"
#include "hode_generic_net.h"
#include <type_traits>

namespace hode {

// activation (wave-uniform code, include/hode.h HODE_ACT_*) and "cotangent times its derivative" from the POST-activation value:
// h > 0 iff the pre-activation is > 0 for all four; ELU'(x <= 0) = exp(x) = h + 1  (torch: nn.ReLU / Tanh / ELU / LeakyReLU(0.1),
// reference models/nn_residual.py:50-56)
__device__ __forceinline__ float act_f(float s, int act)
{
    if (act == HODE_ACT_RELU) return rmax0(s);
    if (act == HODE_ACT_TANH) return tanhf(s);
    if (act == HODE_ACT_ELU) return s > 0.f ? s : expm1f(s);
    return s > 0.f ? s : 0.1f * s;
}
__device__ __forceinline__ double act_f(double s, int act)
{
    if (act == HODE_ACT_RELU) return rmax0(s);
    if (act == HODE_ACT_TANH) return tanh(s);
    if (act == HODE_ACT_ELU) return s > 0.0 ? s : expm1(s);
    return s > 0.0 ? s : 0.1 * s;
}
__device__ __forceinline__ float bcast_dyn(float v, int k) { return i2f(__builtin_amdgcn_readlane(f2i(v), k)); }
__device__ __forceinline__ double bcast_dyn(double v, int k) { return lane_bcast(v, k); }
// activation k of a layer whose units live two per lane (k < 64: register a of lane k; else register b of lane k - 64)
template <typename R> __device__ __forceinline__ R unit_bcast(R a, R b, int k) { return k < 64 ? bcast_dyn(a, k) : bcast_dyn(b, k - 64); }

// f(t, x, u) for an arbitrary network.  rec != nullptr: record h_1..h_L (two rows of 64 each) and the stage state (8 reals).
// NW > 1: a team of NW waves evaluates the same f on identical data (see rhs_vjp_stream); the columns k of every hidden matrix
// are split over the waves, partial sums exchanged through xch[NW][2][64] and added in wave order on every wave.
template <typename R, int NW = 1, typename EW = EdgeFromParams<R>>
__device__ __forceinline__ R rhs_stream(const StreamNet<R> &n, const EW &ew, const OdeP<R> &o, R t, R Y, R meal, R tvns, R gde, int lane,
                                        R *__restrict__ rec, int part = 0, R *__restrict__ xch = nullptr)
{
    const int H = n.H, L = n.L;
    const R G = lane_bcast(Y, 0), I = lane_bcast(Y, 1), Glu = lane_bcast(Y, 2), GLP1 = lane_bcast(Y, 3),
            GE = lane_bcast(Y, 4), FFA = lane_bcast(Y, 5);
    const int c8 = lane & 7;
    const R mech = mech_eval(o, G, I, Glu, GLP1, FFA, meal, gde, c8);
    const bool vA = lane < H, vB = lane + 64 < H;
    const int jA = vA ? lane : 0, jB = vB ? lane + 64 : 0;              // clamped: masked lanes read a valid address
    const R in[9] = {t, G, I, Glu, GLP1, GE, FFA, GLP1, tvns};          // models/nn_residual.py:138-143
    R hA = ew.b1()[jA], hB = ew.b1()[jB];
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        hA = rfma(ew.W1()[jA * 9 + i], in[i], hA);
        hB = rfma(ew.W1()[jB * 9 + i], in[i], hB);
    }
    hA = vA ? act_f(hA, n.act) : R(0);
    hB = vB ? act_f(hB, n.act) : R(0);
    if (rec) { rec[lane] = hA; rec[kWave + lane] = hB; }
    const int cols_per = (((H + NW - 1) / NW) + 7) & ~7;             // this wave's columns: a multiple of 8 (the chunked loads)
    const int k0 = (part * cols_per < H) ? part * cols_per : H, k1 = (k0 + cols_per < H) ? k0 + cols_per : H;
    for (int l = 0; l + 1 < L; ++l) {
        const R *__restrict__ rowA = n.Wh(l) + (size_t)jA * H, *__restrict__ rowB = n.Wh(l) + (size_t)jB * H;
        R aA = (NW == 1) ? ew.bh(l)[jA] : R(0), aB = (NW == 1) ? ew.bh(l)[jB] : R(0);
        // chunks of 8 columns: 16 independent loads in flight, then the 16 FMAs (one load, one dependent FMA at a time left
        // a lone wave waiting out an L2 round trip per column: 21.9 ms per 32 x 61 forward of the 5 x 128 network, 7.7 ms now)
        int k = k0;
        for (; k + 8 <= k1; k += 8) {
            R wA[8], wB[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) { wA[u] = rowA[k + u]; wB[u] = rowB[k + u]; }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const R hk = unit_bcast(hA, hB, k + u);        // k + u < 64 for the whole chunk or >= 64 for the whole chunk
                aA = rfma(wA[u], hk, aA);
                aB = rfma(wB[u], hk, aB);
            }
        }
        for (; k < k1; ++k) {
            const R hk = unit_bcast(hA, hB, k);
            aA = rfma(rowA[k], hk, aA);
            aB = rfma(rowB[k], hk, aB);
        }
        if constexpr (NW > 1) {
            xch[(part * 2 + 0) * kWave + lane] = aA;
            xch[(part * 2 + 1) * kWave + lane] = aB;
            __syncthreads();
            aA = ew.bh(l)[jA]; aB = ew.bh(l)[jB];
#pragma unroll
            for (int w = 0; w < NW; ++w) { aA += xch[(w * 2 + 0) * kWave + lane]; aB += xch[(w * 2 + 1) * kWave + lane]; }
            __syncthreads();
        }
        hA = vA ? act_f(aA, n.act) : R(0);
        hB = vB ? act_f(aB, n.act) : R(0);
        if (rec) { rec[(2 * (l + 1)) * kWave + lane] = hA; rec[(2 * (l + 1) + 1) * kWave + lane] = hB; }
    }
    R p[6];
#pragma unroll
    for (int q = 0; q < 6; ++q) p[q] = ew.Wo()[q * H + jA] * hA + ew.Wo()[q * H + jB] * hB;     // h is 0 on masked lanes
    const R nn = wave_reduce6_to_lanes(p, lane);
    if (rec && lane < 8) rec[2 * L * kWave + lane] = Y;
    const R bout = (c8 < 6) ? ew.bo()[(c8 < 6) ? c8 : 0] : R(0);
    return (c8 < 6) ? (mech + nn + bout) : R(0);
}

// f(t, x, u) by a TEAM of NW waves, hidden layers split by OUTPUT ROWS (solve_fwd_generic_kernel, NW > 1, L >= 2).
// The column split above makes every wave add up NW partial vectors per layer (2 NW LDS reads and adds per wave, two barriers): at 16
// waves a wave issued ~1 100 instructions per evaluation for 128 useful FMAs, and four such waves share a SIMD's issue slots
// (tools/pmc_generic.sh: the forward of 32 x 61 was issue-bound).  Here the activation vector lives in LDS (hb[2][128], zero beyond
// H) and lane (r, c) = (lane >> 3, lane & 7) of wave w owns row 8 (w + NW blk) + r and the 16-column chunk c of it: 16 FMAs, a
// 3-step sum over the eight lanes of the row, bias + activation, one 4-byte LDS write per row, ONE barrier per layer -- an
// all-gather of eight finished outputs per wave instead of an all-reduce of 128 partial sums.  The first layer (9 inputs) and the
// output layer (6 rows: lane (component, chunk), summed over the chunks into the replicated state layout) are computed by every
// wave from identical data, so every wave ends with identical bits.
constexpr int kGenAccMats = 4;       // hidden matrices whose weights (forward) / gradients (adjoint) a team can keep in registers
// CC = columns per lane (16: H <= 128; 8: H <= 64, all eight lanes of a row busy).  NB > 0: the wave's NB row blocks of up to
// kGenAccMats hidden matrices are REGISTER-RESIDENT (wres, loaded once per trajectory): 8-wave teams, NB = 2, CC = 16 for 128 hidden
// units = 128 weight registers per lane and no weight load left in the evaluation; NB = 0 streams them from L2 as above.
template <typename R, int CC, int NB> struct RowWeights { R w[kGenAccMats][NB > 0 ? NB : 1][CC]; };

template <typename R, int NW, int CC, int NB>
__device__ __forceinline__ void rows_preload(RowWeights<R, CC, NB> &rw, const StreamNet<R> &n, int lane, int part)
{
    if constexpr (NB > 0) {
        const int H = n.H, k0 = CC * (lane & 7), r8 = lane >> 3;
#pragma unroll
        for (int l = 0; l < kGenAccMats; ++l) {
#pragma unroll
            for (int blk = 0; blk < NB; ++blk) {
                const int row = 8 * (part + NW * blk) + r8;
                const bool ok = l + 1 < n.L && row < H;
                const R *__restrict__ wrow = n.Wh(ok ? l : 0) + (size_t)(ok ? row : 0) * H;
#pragma unroll
                for (int u = 0; u < CC; ++u) rw.w[l][blk][u] = (ok && k0 + u < H) ? wrow[(k0 + u < H) ? k0 + u : 0] : R(0);
            }
        }
    }
}

template <typename R, int NW, typename EW, int CC, int NB>
__device__ __forceinline__ R rhs_rows(const StreamNet<R> &n, const EW &ew, const RowWeights<R, CC, NB> &rw, const OdeP<R> &o, R t, R Y, R meal,
                                      R tvns, R gde, int lane, R *__restrict__ rec, int part, R *__restrict__ hb)
{
    const int H = n.H, L = n.L;
    const R G = lane_bcast(Y, 0), I = lane_bcast(Y, 1), Glu = lane_bcast(Y, 2), GLP1 = lane_bcast(Y, 3),
            GE = lane_bcast(Y, 4), FFA = lane_bcast(Y, 5);
    const int c8 = lane & 7, r8 = lane >> 3;
    const R mech = mech_eval(o, G, I, Glu, GLP1, FFA, meal, gde, c8);
    const bool vA = lane < H, vB = lane + 64 < H;
    const int jA = vA ? lane : 0, jB = vB ? lane + 64 : 0;
    const R in[9] = {t, G, I, Glu, GLP1, GE, FFA, GLP1, tvns};          // models/nn_residual.py:138-143
    R hA = ew.b1()[jA], hB = ew.b1()[jB];
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        hA = rfma(ew.W1()[jA * 9 + i], in[i], hA);
        hB = rfma(ew.W1()[jB * 9 + i], in[i], hB);
    }
    hA = vA ? act_f(hA, n.act) : R(0);
    hB = vB ? act_f(hB, n.act) : R(0);
    // every wave writes the SAME h_1: a wave's own LDS writes are visible to its later reads, no barrier needed
    hb[hx<CC>(lane)] = hA;
    hb[hx<CC>(kWave + lane)] = hB;
    if (rec) { rec[lane] = hA; rec[kWave + lane] = hB; }
    const int k0 = CC * c8;                                  // this lane's column chunk [k0, k0 + CC)
    // one hidden layer; slot = its index as a compile-time constant when its weights are register-resident (NB > 0), else unused
    auto layer = [&](const int l, auto slot) {
        const R *__restrict__ hin = hb + (l & 1) * kHbStride;
        R *__restrict__ hout = hb + ((l + 1) & 1) * kHbStride;
        R hc[CC];
#pragma unroll
        for (int u = 0; u < CC; ++u) hc[u] = hin[hx<CC>(k0) + u];    // (zero beyond H; a chunk is contiguous under the skew)
        auto finish = [&](R acc, int row, bool vr) {
            acc = oct_allsum(acc);
            const R v = act_f(acc + ew.bh(l)[vr ? row : 0], n.act);
            if (c8 == 0 && vr) hout[hx<CC>(row)] = v;
        };
        if constexpr (NB > 0) {
#pragma unroll
            for (int blk = 0; blk < NB; ++blk) {
                const int row = 8 * (part + NW * blk) + r8;
                R acc = R(0);
#pragma unroll
                for (int u = 0; u < CC; ++u) acc = rfma(rw.w[decltype(slot)::value][blk][u], hc[u], acc);
                finish(acc, row, row < H);
            }
        } else {
            const R *__restrict__ W = n.Wh(l);
            // vector path: whole chunks only (H a multiple of CC: a chunk lies inside the row or, clamped to column 0, is discarded)
            const bool al16 = (H % CC) == 0 && (reinterpret_cast<uintptr_t>(W) & 15) == 0;      // wave-uniform
            for (int row0 = 8 * part; row0 < H; row0 += 8 * NW) {
                const int row = row0 + r8;
                const bool vr = row < H;
                const R *__restrict__ wr0 = W + (size_t)(vr ? row : 0) * H;
                R w[CC];
                if (al16) {
                    load_chunk<R, CC>(wr0 + (k0 < H ? k0 : 0), w, true);
                } else {
#pragma unroll
                    for (int u = 0; u < CC; ++u) w[u] = wr0[(k0 + u < H) ? k0 + u : 0];      // never past the row
                }
                R acc = R(0);
#pragma unroll
                for (int u = 0; u < CC; ++u) acc = rfma((k0 + u < H) ? w[u] : R(0), hc[u], acc);
                finish(acc, row, vr);
            }
        }
        __syncthreads();
        if (rec) { rec[(2 * (l + 1)) * kWave + lane] = hout[hx<CC>(lane)]; rec[(2 * (l + 1) + 1) * kWave + lane] = hout[hx<CC>(kWave + lane)]; }
    };
    if constexpr (NB > 0) {
        // (a fixed-trip loop, fully unrolled: the register-resident weights need a compile-time layer index)
#pragma unroll
        for (int i = 0; i < kGenAccMats; ++i) {
            if (i + 1 >= L) break;
            if (i == 0) layer(0, std::integral_constant<int, 0>{});
            else if (i == 1) layer(1, std::integral_constant<int, 1>{});
            else if (i == 2) layer(2, std::integral_constant<int, 2>{});
            else layer(3, std::integral_constant<int, 3>{});
        }
    } else {
        for (int l = 0; l + 1 < L; ++l) layer(l, std::integral_constant<int, 0>{});
    }
    // output layer: lane (component c8 < 6, chunk r8) takes 16 columns of row c8; group_sum8 adds the eight chunks and leaves the
    // sum on every lane with that component -- the replicated layout of the state
    const R *__restrict__ hf = hb + ((L - 1) & 1) * kHbStride;
    const int q = (c8 < 6) ? c8 : 0, ko = 16 * r8;
    R acc = R(0);
#pragma unroll
    for (int u = 0; u < 16; ++u) {
        const int k = ko + u;
        acc = rfma((k < H) ? ew.Wo()[q * H + ((k < H) ? k : 0)] : R(0), hf[hx<CC>(k)], acc);
    }
    acc = (c8 < 6) ? acc : R(0);
    const R nn = group_sum8(acc);
    if (rec && lane < 8) rec[2 * L * kWave + lane] = Y;
    const R bout = (c8 < 6) ? ew.bo()[q] : R(0);
    __syncthreads();                                         // the next evaluation overwrites hb
    return (c8 < 6) ? (mech + nn + bout) : R(0);
}

template <typename R, int NW = 1, typename EW = EdgeFromParams<R>, int CC = 16, int NB = 0> struct RhsStream {
    StreamNet<R> n;
    EW ew;                  // where the edge parameters come from (the workgroup's LDS image in the solve kernels)
    const OdeP<R> &o;
    int lane;
    int part;               // this wave's index in its team (NW > 1: hode_generic.hip solve_fwd_generic_kernel)
    R *xch;                 // the team's exchange area (column split: partial sums; row split: hb[2][128])
    RowWeights<R, CC, NB> rw;   // row split with NB > 0: this wave's rows of the hidden matrices (rows_preload)
    static constexpr bool kUnrollStages = false;
    __device__ __forceinline__ int slot_elems() const { return 2 * n.L * kWave + 8; }
    __device__ __forceinline__ R operator()(R ts, R Ys, R meal, R tvns, R gde, R *__restrict__ rec) const
    {
        // every wave of a team computes the same f; only the first one writes the stage record
        if constexpr (NW > 1) {
            if (n.L >= 2) return rhs_rows<R, NW, EW, CC, NB>(n, ew, rw, o, ts, Ys, meal, tvns, gde, lane, part == 0 ? rec : nullptr, part, xch);
        }
        return rhs_stream<R, NW, EW>(n, ew, o, ts, Ys, meal, tvns, gde, lane, part == 0 ? rec : nullptr, part, xch);
    }
};

// ---- SEVERAL trajectories per team (solve_fwd_generic_multi_kernel; fp32, register-resident rows) ------------------------------------
// rhs_rows gives a whole team to ONE trajectory: every wave repeats the integrator, the first and the output layer, and a layer costs a
// barrier per trajectory; above a few hundred trajectories the teams stream the hidden matrices from L2 instead of keeping them (262 KB
// per evaluation for 5 x 128: 17 TB/s at 1 024 x 61, the bound of that launch).  Here a workgroup of eight waves serves TB trajectories:
// wave w INTEGRATES trajectory w % TB (controller, first layer, output layer, tape: once per trajectory, not once per wave) and owns its
// row blocks of every hidden matrix in registers FOR ALL of them -- per layer one barrier, TB x (4 LDS reads of 16 bytes + 32 FMAs + the
// 8-lane sums).  The trajectories of a team need not be in step: a round is "every wave has published the first-layer output of its
// next evaluation", whatever stage, step or grid interval that evaluation belongs to.  A wave whose trajectory is finished (or that has
// none) keeps serving rounds until all are (done counter in LDS, read behind the round's first barrier by the waves that are serving:
// they all see the same value and leave together).
template <int TB, int CC, int NB> struct RhsMulti {
    static constexpr int kNW = 8;
    StreamNet<float> n;
    EdgeImage<float> ew;
    const OdeP<float> &o;
    int lane, part;
    float *hbm;                  // [TB][3][kHbStride] activation vectors (zero beyond H): h_1 in buffer 2, h_{l+2} in buffer l & 1 -- the
                                 // first layer of a trajectory's NEXT evaluation never writes what a slower wave still reads
    RowWeights<float, CC, NB> rw;
    static constexpr bool kUnrollStages = false;
    __device__ __forceinline__ int slot_elems() const { return 2 * n.L * kWave + 8; }
    // the hidden layers of one round for all TB trajectories; barriers: one behind every layer.  rec != nullptr: this wave's own
    // trajectory is being taped -- h_{l+1} is copied out of LDS right behind the layer's barrier (the buffer is next written two
    // layers on, behind a barrier this wave has not passed yet)
    __device__ __forceinline__ void layers(float *__restrict__ rec) const
    {
        const float *__restrict__ hb_own = hbm + (part % TB) * 3 * kHbStride;
        const int H = n.H, L = n.L;
        const int c8 = lane & 7, r8 = lane >> 3, k0 = CC * c8;
        auto layer = [&](const int l, auto slot) {
            float bias[NB > 0 ? NB : 1];
#pragma unroll
            for (int blk = 0; blk < NB; ++blk) {
                const int row = 8 * (part + kNW * blk) + r8;
                bias[blk] = ew.bh(l)[row < H ? row : 0];
            }
#pragma unroll 2
            for (int tt = 0; tt < TB; ++tt) {
                const float *__restrict__ hin = hbm + (tt * 3 + (l == 0 ? 2 : (l - 1) & 1)) * kHbStride;
                float *__restrict__ hout = hbm + (tt * 3 + (l & 1)) * kHbStride;
                float hc[CC];
#pragma unroll
                for (int u = 0; u < CC; ++u) hc[u] = hin[hx<CC>(k0) + u];
#pragma unroll
                for (int blk = 0; blk < NB; ++blk) {
                    const int row = 8 * (part + kNW * blk) + r8;
                    float acc = 0.f;
#pragma unroll
                    for (int u = 0; u < CC; ++u) acc = rfma(rw.w[decltype(slot)::value][blk][u], hc[u], acc);
                    acc = oct_allsum(acc);
                    const float v = act_f(acc + bias[blk], n.act);
                    if (c8 == 0 && row < H) hout[hx<CC>(row)] = v;
                }
            }
            __syncthreads();
            if (rec) {
                const float *__restrict__ ho = hb_own + (l & 1) * kHbStride;
                rec[(2 * (l + 1)) * kWave + lane] = ho[hx<CC>(lane)];
                rec[(2 * (l + 1) + 1) * kWave + lane] = ho[hx<CC>(kWave + lane)];
            }
        };
#pragma unroll
        for (int i = 0; i < kGenAccMats; ++i) {
            if (i + 1 >= L) break;
            if (i == 0) layer(0, std::integral_constant<int, 0>{});
            else if (i == 1) layer(1, std::integral_constant<int, 1>{});
            else if (i == 2) layer(2, std::integral_constant<int, 2>{});
            else layer(3, std::integral_constant<int, 3>{});
        }
    }
    __device__ __forceinline__ float operator()(float t, float Y, float meal, float tvns, float gde, float *__restrict__ rec) const
    {
        const int H = n.H, L = n.L;
        rec = part < TB ? rec : nullptr;                    // (TB < 8: waves w and w + TB integrate the same trajectory; one writes)
        float *__restrict__ hb = hbm + (part % TB) * 3 * kHbStride;
        const float G = lane_bcast(Y, 0), I = lane_bcast(Y, 1), Glu = lane_bcast(Y, 2), GLP1 = lane_bcast(Y, 3), GE = lane_bcast(Y, 4),
                    FFA = lane_bcast(Y, 5);
        const int c8 = lane & 7, r8 = lane >> 3;
        const float mech = mech_eval(o, G, I, Glu, GLP1, FFA, meal, gde, c8);
        const bool vA = lane < H, vB = lane + 64 < H;
        const int jA = vA ? lane : 0, jB = vB ? lane + 64 : 0;
        const float in[9] = {t, G, I, Glu, GLP1, GE, FFA, GLP1, tvns};          // models/nn_residual.py:138-143
        float hA = ew.b1()[jA], hB = ew.b1()[jB];
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            hA = rfma(ew.W1()[jA * 9 + i], in[i], hA);
            hB = rfma(ew.W1()[jB * 9 + i], in[i], hB);
        }
        hA = vA ? act_f(hA, n.act) : 0.f;
        hB = vB ? act_f(hB, n.act) : 0.f;
        hb[2 * kHbStride + hx<CC>(lane)] = hA;
        hb[2 * kHbStride + hx<CC>(kWave + lane)] = hB;
        if (rec) { rec[lane] = hA; rec[kWave + lane] = hB; }
        __syncthreads();                                    // the round's first barrier: every trajectory's h_1 is in LDS
        layers(rec);
        const float *__restrict__ hf = hb + (L >= 2 ? (L - 2) & 1 : 2) * kHbStride;
        const int q = (c8 < 6) ? c8 : 0, ko = 16 * r8;
        float acc = 0.f;
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int k = ko + u;
            acc = rfma((k < H) ? ew.Wo()[q * H + ((k < H) ? k : 0)] : 0.f, hf[hx<CC>(k)], acc);
        }
        acc = (c8 < 6) ? acc : 0.f;
        const float nn = group_sum8(acc);
        if (rec && lane < 8) rec[2 * L * kWave + lane] = Y;
        const float bout = (c8 < 6) ? ew.bo()[q] : 0.f;
        return (c8 < 6) ? (mech + nn + bout) : 0.f;
    }
};

}  // namespace hode

// hode_generic_jvp.hip -- K6 for the GENERIC network path: the tangent-linear pass over the tape of solve_fwd_generic_kernel, for every
// network the forward can tape outside the tuned envelope (H <= 128, L <= 8, ReLU / tanh / ELU / leaky ReLU).
//
// Semantics are those of solve_jvp_kernel (hode_solve_jvp.hip) and of hode_oracle_solve_jvp: the taped accepted steps walked forward
// with their step sizes held constant, rows replayed from the interval indices, non-finite tangents returned as computed, the tape
// read-only.  The mechanistic part J_x f . dY + J_theta f . v is jvp_coeffs / kJvpPar of hode_jvp.h, shared with the tuned kernel.
//
// Mapping: one workgroup = a TEAM of 8 waves = one trajectory and a tile of KT directions (blockIdx.y tiles K).
//   * every wave walks the tape and keeps the stage bookkeeping (dy, dKK packed by stage, the tableau rows in LDS) on identical data:
//     identical bits, identical control flow, every wave reaches every barrier.  Wave 0 writes dy.
//   * the tangent of the network at a stage recomputes nothing of the primal: act' comes from the taped post-activation values
//     (act_bwd, as in the generic adjoint), so there is no transcendental in it.
//       first layer   d_1 = act'(h_1) (W1[:, 1..6] dY + W1[:, 7] dY_GLP1): every wave, units two per lane (j, j + 64), weights in
//                     registers for the whole walk (from the EdgeImage copy in LDS)
//       hidden layer  split by OUTPUT ROWS as the forward's rhs_rows: lane (r, c) of wave w owns row 8 (w + 8 blk) + r and the 16-column
//                     chunk c.  The chunk of weights is loaded ONCE (16-byte loads from L2) and applied to all KT directions: 16 KT FMAs,
//                     the 3-step sum over the row's eight lanes, act' of the row's taped h, one LDS write per direction.  The KT direction
//                     vectors of a layer live in LDS (double-buffered, the forward's skew hx<16>); ONE barrier per layer serves the tile
//       output layer  lane (component c, chunk r) takes 16 columns of row c (registers for the whole walk), group_sum8 adds the chunks
//   * the stage record (2 L rows of 64 + the stage state) is read from HBM once per team and tile, one stage ahead: every thread keeps
//     its three elements of the next record in registers across the stage and parks them in the other LDS record buffer at its end.
//   * no atomics, no MFMA; every floating-point sum has a fixed order that depends on neither B, K nor the tile: a direction's bits
//     are those of a one-direction launch, and of any launch that contains it.
#include "hode_tableau.h"
#include "hode_rhs_eval.h"
#include "hode_kernels.h"
#include "hode_jvp.h"
#include "hode_generic_net.h"

namespace hode {

// directions per team.  fp32: 8 (a dy row is written by lanes 8 k + c: at most 8); fp64 (parity runs): 2
template <typename R> constexpr int kGenJvpTile = (sizeof(R) == 4) ? 8 : 2;
constexpr int kGenJvpWaves = 8;
constexpr int kGenJvpThreads = 64 * kGenJvpWaves;
constexpr int kGenRecMax = 2 * HODE_MAX_LAYERS * kWave + 8;                         // reals of the largest stage record
constexpr int kGenRecPer = (kGenRecMax + kGenJvpThreads - 1) / kGenJvpThreads;      // of them per thread

template <typename R, int KT, bool GD>
__global__ __launch_bounds__(kGenJvpThreads) void solve_jvp_generic_kernel(const JvpArgs<R> a, const int method, const int L, const int act)
{
#pragma clang fp contract(off)         // (every product-sum below is an explicit rfma: a direction's code must not depend on its slot)
    static_assert(KT >= 1 && KT <= 8, "a dy row is written by lanes 8 k + c");
    static_assert(HODE_MAX_HIDDEN <= 128 && HODE_MAX_LAYERS <= 8, "two units per lane, kEdgeImageMax");
    __shared__ R rows[8 * kWave];                                       // tableau coefficient rows (hode_tableau.h)
    __shared__ R edge_img[kEdgeImageMax];                               // the edge parameters of this trajectory's set (EdgeImage)
    __shared__ __attribute__((aligned(16))) R hb[2 * KT * kHbStride];   // [buffer][direction] tangent vector of a layer, zero beyond H
    __shared__ R recs[2 * kGenRecMax];                                  // [buffer] stage record in use | the next one
    const int tid = threadIdx.x, lane = tid & 63, c8 = lane & 7, r8 = lane >> 3;
    const int part = first_lane((int)(threadIdx.x >> 6));
    const int b = blockIdx.x;                                           // (grid.x = B: no workgroup without a trajectory)
    const int k0 = blockIdx.y * KT;
    const int kt = (a.K - k0) < KT ? a.K - k0 : KT;                     // directions of this tile (workgroup-uniform)
    const int T = a.T, H = a.H;
    const int set = b / (a.B / a.n_sets);
    const TableauData &tab = kTableau[method];
    const int S = tab.S;
    const int rowb = (method == HODE_METHOD_DP54) ? 6 : 7;              // solution weights: DP5(4) row 6 (FSAL row), RK4 row 7

    const StreamNet<R> net{a.nn_p + (size_t)set * a.P, H, L, act};
    tableau_rows_store<R>(rows, method, tid, kGenJvpThreads);
    EdgeImage<R>::fill(edge_img, net, tid, kGenJvpThreads);
    for (int i = tid; i < 2 * KT * kHbStride; i += kGenJvpThreads) hb[i] = R(0);
    const EdgeImage<R> ew{edge_img, H, L};
    OdeP<R> o;
    ode_load(o, a.ode_p + 17 * set);

    const R *__restrict__ tg = a.t + (a.t_batched ? (size_t)b * T : 0);
    const R *__restrict__ tape = a.tape + (size_t)b * a.max_steps * 8;
    const int *__restrict__ tseg = a.tape_seg + (size_t)b * a.max_steps;
    const int slot = 2 * L * kWave + 8;                                 // stage record: h_1 .. h_L, two rows of 64 each | the stage state
    const R *__restrict__ stg = a.tape_stage + (size_t)b * a.max_steps * 6 * slot;
    const int n = a.nsteps[b] < a.max_steps ? a.nsteps[b] : a.max_steps;    // never walk past the tape

    // the next stage record: this thread's elements, in registers from the top of a stage to its end
    R pre[kGenRecPer] = {};
    auto fetch = [&](int rec) {
        const R *__restrict__ r = stg + (size_t)rec * slot;
#pragma unroll
        for (int j = 0; j < kGenRecPer; ++j) {
            const int i = tid + j * kGenJvpThreads;
            pre[j] = (i < slot) ? r[(i < slot) ? i : 0] : R(0);
        }
    };
    auto park = [&](int buf) {
#pragma unroll
        for (int j = 0; j < kGenRecPer; ++j) {
            const int i = tid + j * kGenJvpThreads;
            if (i < slot) recs[buf * kGenRecMax + i] = pre[j];
        }
    };
    int cur = 0;                                                        // the record buffer in use
    if (n > 0) {
        fetch(0);
        park(0);
    }
    __syncthreads();                                                    // rows, edge image, hb zeros, the first record

    // edge weights of this lane, for the whole walk: columns 1..7 of the first matrix for units lane and lane + 64; the lane's 16-column
    // chunk of output row c8
    const bool vA = lane < H, vB = lane + 64 < H;
    const int jA = vA ? lane : 0, jB = vB ? lane + 64 : 0;
    // (fp32.  fp64 -- parity runs -- reads them from the image at every use: 60 registers of them spilled)
    constexpr bool kEdgeRegs = sizeof(R) == 4;
    const int qo = (c8 < 6) ? c8 : 0, ko = 16 * r8;
    auto w1_at = [&](int j, int i) -> R { return ew.W1()[j * 9 + 1 + i]; };
    auto wo_at = [&](int u) -> R { return (c8 < 6 && ko + u < H) ? ew.Wo()[qo * H + ((ko + u < H) ? ko + u : 0)] : R(0); };
    [[maybe_unused]] R w1A[kEdgeRegs ? 7 : 1], w1B[kEdgeRegs ? 7 : 1], wo[kEdgeRegs ? 16 : 1];
    if constexpr (kEdgeRegs) {
#pragma unroll
        for (int i = 0; i < 7; ++i) {
            w1A[i] = w1_at(jA, i);
            w1B[i] = w1_at(jB, i);
        }
#pragma unroll
        for (int u = 0; u < 16; ++u) wo[u] = wo_at(u);
    }

    // directions: the state tangent (replicated layout) and, per lane, the v_ode entries of the lane's component
    R dy[KT], vl[KT][5];
#pragma unroll
    for (int k = 0; k < KT; ++k) {
        const bool on = k < kt;
        const size_t kg = (size_t)(on ? k0 + k : 0);
        dy[k] = (on && a.v_x0 && c8 < 6) ? a.v_x0[((size_t)b * a.K + kg) * 6 + c8] : R(0);
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            const int p = kJvpPar[c8][i];
            vl[k][i] = (on && a.v_ode && p >= 0) ? a.v_ode[((size_t)set * a.K + kg) * 17 + (p >= 0 ? p : 0)] : R(0);
        }
    }

    // output rows (the team's first wave): lanes 8k + c (c < 6) write component c of direction k
    R *__restrict__ out = a.dy + ((size_t)b * a.K + k0) * T * 6;
    auto put_row = [&](int r, bool zero) {
        R v = R(0);
#pragma unroll
        for (int k = 0; k < KT; ++k) v = (r8 == k) ? dy[k] : v;
        if (part == 0 && c8 < 6 && r8 < kt) out[((size_t)r8 * T + r) * 6 + c8] = zero ? R(0) : v;
    };
    put_row(0, false);

    const int kc = 16 * c8;                                             // this lane's column chunk of a hidden matrix
    // The forward's row logic (hode_solve_body.h), as in solve_jvp_kernel: a repeated grid time copies the state; a grid row gets the
    // state at the end of the step that closes its interval; after an interval that no taped step closes every remaining row is 0.
    int st = 0, r = 1;
#pragma unroll 1
    for (int kiv = 0; kiv + 1 < T; ++kiv) {
        if (!(tg[kiv + 1] - tg[kiv] > R(0))) {
            put_row(r++, false);
            continue;
        }
        bool closed = false;
#pragma unroll 1
        while (st < n && (tseg[st] & (kSegClosed - 1)) == kiv) {
            const R *__restrict__ e = tape + (size_t)st * 8;
            const R tc = e[0], h = e[1], t0 = e[2], inv_len = e[3], d0 = e[6], dd = e[7];
            closed = (tseg[st] & kSegClosed) != 0;
            R dKK[KT];                                                  // stage tangents, packed: lanes 8s .. 8s+7 = stage s
#pragma unroll
            for (int k = 0; k < KT; ++k) dKK[k] = R(0);
#pragma unroll 1
            for (int s = 0; s < S; ++s) {
                const R *__restrict__ rc = recs + cur * kGenRecMax;
                const int nxt = (s + 1 < S) ? st * 6 + s + 1 : (st + 1 < n) ? (st + 1) * 6 : -1;
                if (nxt >= 0) fetch(nxt);
                const R ts = rfma((R)tab.c[s], h, tc);
                const R gdv = rfma((ts - t0) * inv_len, dd, d0);
                const R gde = GD ? gd_effect(o, gdv) : R(0);
                const R *__restrict__ sx = rc + 2 * L * kWave;          // the stage state (uniform LDS reads)
                R js[5], jp[5];
                jvp_coeffs<R, GD>(o, sx[0], sx[1], sx[2], sx[3], sx[5], gde, gdv, c8, js, jp);
                const R coef = rows[s * kWave + lane];
                // mechanistic part and first layer, per direction; d_1 into buffer 0 (every wave writes the same bits)
                const R h1A = rc[lane], h1B = rc[kWave + lane];
                R m[KT];
#pragma unroll
                for (int k = 0; k < KT; ++k) {
                    m[k] = R(0);
                    if (k < kt) {
                        const R dYs = rfma(h, group_sum8(coef * dKK[k]), dy[k]);
                        const R gG = state_bcast<0>(dYs), gI = state_bcast<1>(dYs), gGlu = state_bcast<2>(dYs),
                                gGLP = state_bcast<3>(dYs), gGE = state_bcast<4>(dYs), gF = state_bcast<5>(dYs);
                        R mk = js[0] * gG;
                        mk = rfma(js[1], gI, mk);
                        mk = rfma(js[2], gGlu, mk);
                        mk = rfma(js[3], gGLP, mk);
                        mk = rfma(js[4], gF, mk);
#pragma unroll
                        for (int i = 0; i < 5; ++i) mk = rfma(jp[i], vl[k][i], mk);
                        m[k] = mk;
                        const R g[7] = {gG, gI, gGlu, gGLP, gGE, gF, gGLP};     // input columns 1..7 (models/nn_residual.py:138-143)
                        R dA, dB;
                        if constexpr (kEdgeRegs) {
                            dA = w1A[0] * g[0];
                            dB = w1B[0] * g[0];
#pragma unroll
                            for (int i = 1; i < 7; ++i) {
                                dA = rfma(w1A[i], g[i], dA);
                                dB = rfma(w1B[i], g[i], dB);
                            }
                        } else {
                            dA = w1_at(jA, 0) * g[0];
                            dB = w1_at(jB, 0) * g[0];
#pragma unroll
                            for (int i = 1; i < 7; ++i) {
                                dA = rfma(w1_at(jA, i), g[i], dA);
                                dB = rfma(w1_at(jB, i), g[i], dB);
                            }
                        }
                        R *__restrict__ h0 = hb + k * kHbStride;
                        h0[hx<16>(lane)] = vA ? act_bwd(dA, h1A, act) : R(0);
                        h0[hx<16>(kWave + lane)] = vB ? act_bwd(dB, h1B, act) : R(0);
                    }
                }
                // hidden layers: matrix l maps d_{l+1} (buffer l & 1) to d_{l+2} (the other buffer)
#pragma unroll 1
                for (int l = 0; l + 1 < L; ++l) {
                    const R *__restrict__ hin = hb + (l & 1) * (KT * kHbStride);
                    R *__restrict__ hout = hb + ((l + 1) & 1) * (KT * kHbStride);
                    const R *__restrict__ W = net.Wh(l);
                    const R *__restrict__ hl = rc + 2 * (l + 1) * kWave;        // the taped h_{l+2}: unit j at hl[j] (rows 2l+2, 2l+3)
                    // vector path: whole chunks only (H a multiple of 16: a chunk lies inside the row or, clamped to column 0, is discarded)
                    const bool al16 = (H % 16) == 0 && (reinterpret_cast<uintptr_t>(W) & 15) == 0;      // workgroup-uniform
#pragma unroll 1
                    for (int row0 = 8 * part; row0 < H; row0 += 8 * kGenJvpWaves) {
                        const int row = row0 + r8;
                        const bool vr = row < H;
                        const R *__restrict__ wr0 = W + (size_t)(vr ? row : 0) * H;
                        R w[16];
                        if (al16) {
                            load_chunk<R, 16>(wr0 + (kc < H ? kc : 0), w, true);
                        } else {
#pragma unroll
                            for (int u = 0; u < 16; ++u) w[u] = wr0[(kc + u < H) ? kc + u : 0];      // never past the row
                        }
#pragma unroll
                        for (int u = 0; u < 16; ++u) w[u] = (kc + u < H) ? w[u] : R(0);
                        const R hrow = hl[vr ? row : 0];
#pragma unroll
                        for (int k = 0; k < KT; ++k) {
                            if (k < kt) {
                                const R *__restrict__ hk = hin + k * kHbStride + hx<16>(kc);     // (a chunk is contiguous under the skew)
                                R acc = R(0);
#pragma unroll
                                for (int u = 0; u < 16; ++u) acc = rfma(w[u], hk[u], acc);
                                acc = oct_allsum(acc);
                                const R v = act_bwd(acc, hrow, act);
                                if (c8 == 0 && vr) hout[k * kHbStride + hx<16>(row)] = v;
                            }
                        }
                    }
                    __syncthreads();
                }
                // output layer + the stage's tangent
                const R *__restrict__ hf = hb + ((L - 1) & 1) * (KT * kHbStride) + hx<16>(ko);
#pragma unroll
                for (int k = 0; k < KT; ++k) {
                    if (k < kt) {
                        R acc = R(0);
#pragma unroll
                        for (int u = 0; u < 16; ++u) {
                            if constexpr (kEdgeRegs) acc = rfma(wo[u], hf[k * kHbStride + u], acc);
                            else acc = rfma(wo_at(u), hf[k * kHbStride + u], acc);
                        }
                        const R nn = group_sum8(acc);                   // (wo is 0 on the lanes of slots 6, 7: exact zeros there)
                        dKK[k] = stage_put(dKK[k], nn + m[k], s);
                    }
                }
                if (nxt >= 0) park(cur ^ 1);
                cur ^= 1;
                __syncthreads();                                        // the next stage overwrites hb; its record is in place
            }
            const R wb = rows[rowb * kWave + lane];
#pragma unroll
            for (int k = 0; k < KT; ++k)
                if (k < kt) dy[k] = rfma(h, group_sum8(wb * dKK[k]), dy[k]);
            ++st;
        }
        if (!closed) break;
        put_row(r++, false);
    }
    for (; r < T; ++r) put_row(r, true);
}

template <typename R, int KT> static int launch_gen_jvp_t(hipStream_t s, const JvpArgs<R> &a, int L, int act, int method)
{
    const dim3 grid(a.B, (a.K + KT - 1) / KT), block(kGenJvpThreads);
    if (a.gd_mode != 0) hipLaunchKernelGGL((solve_jvp_generic_kernel<R, KT, true>), grid, block, 0, s, a, method, L, act);
    else hipLaunchKernelGGL((solve_jvp_generic_kernel<R, KT, false>), grid, block, 0, s, a, method, L, act);
    return hipGetLastError() == hipSuccess ? HODE_OK : HODE_ELAUNCH;
}

// The tile of a launch.  A team costs a fixed part per stage (the tape walk, the barriers, the weight chunks) plus a part per direction
// (32 windows x 61 points of 128 x 5: 2.2 ms + 0.58 ms per direction), and 32 windows x 7 constants in tiles of 8 are 32 workgroups on
// 256 CUs.  So fp32 halves the tile while the half still holds all K directions, or while the grid is below one workgroup per CU of an
// MI355X: 32 x 7 runs as 224 teams of one direction.  A direction's bits do not depend on the tile it rides in, so the rule is free
// to change; it reads only B and K (the same launch on another device gives the same grid).
constexpr long kGenJvpFill = 256;
template <typename R> int launch_solve_jvp_generic(hipStream_t s, const JvpArgs<R> &a, int L, int act, int method)
{
    if constexpr (sizeof(R) == 4) {
        int kt = kGenJvpTile<R>;
        while (kt > 1 && (kt / 2 >= a.K || (long)a.B * ((a.K + kt - 1) / kt) < kGenJvpFill)) kt /= 2;
        switch (kt) {
        case 1: return launch_gen_jvp_t<R, 1>(s, a, L, act, method);
        case 2: return launch_gen_jvp_t<R, 2>(s, a, L, act, method);
        case 4: return launch_gen_jvp_t<R, 4>(s, a, L, act, method);
        }
    }
    return launch_gen_jvp_t<R, kGenJvpTile<R>>(s, a, L, act, method);
}
template int launch_solve_jvp_generic<float>(hipStream_t, const JvpArgs<float> &, int, int, int);
template int launch_solve_jvp_generic<double>(hipStream_t, const JvpArgs<double> &, int, int, int);

}  // namespace hode

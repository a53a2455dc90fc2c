// hode_solve_jvp.hip -- K6: tangent-linear (forward-mode) pass over the tape of the forward solve.
//
// The reference has no sensitivities; the CPU restatement is hode_oracle_solve_jvp (oracle/hode_oracle_impl.h).  For K tangent
// directions per trajectory it computes
//     dy[b, k] = (d y_b / d ode_p) v_ode[set(b), k] + (d y_b / d x0_b) v_x0[b, k]
// as the exact derivative of the discrete scheme the forward ran: the taped accepted steps, their step sizes held constant,
// the same tableau and grid breaks.  It walks the tape FORWARD, as the adjoint (hode_solve_bwd.hip) walks it backward, and
// differentiates the same thing: the two are transposes of each other, so <gy, J v> = <J^T gy, v> to rounding.
// hode_oracle_solve_jvp walks the same tape with Jacobians taken from the oracle's rhs_vjp_one (not from the coefficient table
// below); tests/test_jvp_enum_gpu.py holds every instantiation of this kernel to it, column by column (tests/_jvp_cases.py).
//
// Mapping: one trajectory per wavefront, one hidden unit per lane (hode_xlane.h), K_TILE directions per wave.
//   * the hidden matrices are loaded into VGPRs once per wave in the forward's register order (mlp_load), so a layer of the
//     tangent, W_l d, is the forward's packed-FMA / DPP layer (mlp_hidden_blk) with a zero bias;
//   * the ReLU derivative is the mask h_l > 0 of the taped activations (what the adjoint uses); nothing of the primal is
//     recomputed and there is no step control: h, t0, 1 / (t1 - t0) and the GD values come from the step's tape entry;
//   * every stage record (L rows of 64 + the stage state) is read ONCE per trajectory and tile, one stage ahead into
//     registers, and serves all directions of the tile: the direction loop sits inside the stage;
//   * the mechanistic part J_x f . dY + J_theta f . v: the per-lane coefficients of the lane's component are computed once
//     per stage (they depend on the stage state only) and every direction then costs 10 FMAs;
//   * no atomics, no scratch in fp32, the tape is read-only.
// Tuned shapes only; generic networks have hode_generic_jvp.hip (a team per trajectory), with which this file shares hode_jvp.h.
#include "hode_tableau.h"
#include "hode_rhs_eval.h"
#include "hode_kernels.h"
#include "hode_jvp.h"

namespace hode {

// directions per wave (a launch tiles K over blockIdx.y).  fp64 (parity runs) holds 384 weight registers already: one
// direction per wave (two per wave spilled, and the second direction's code was not bit-identical to the first's)
template <typename R> constexpr int kJvpTile = (sizeof(R) == 4) ? 8 : 1;
constexpr int kJvpWaves = 4;

// J_x f . dY of the MLP residual at a taped stage (biases drop out of a derivative; ReLU' = taped activation > 0), in the
// replicated layout.  gG .. gF: the broadcast components of dY.
template <typename R, int NL>
__device__ __forceinline__ R mlp_jvp(const MlpRegs<R, NL> &W, const R (&hs)[NL], R gG, R gI, R gGlu, R gGLP, R gGE, R gF, int lane)
{
    R d = W.w1[1] * gG;
    d = rfma(W.w1[2], gI, d);
    d = rfma(W.w1[3], gGlu, d);
    d = rfma(W.w1g, gGLP, d);                    // columns 4 and 7 (both GLP1)
    d = rfma(W.w1[5], gGE, d);
    d = rfma(W.w1[6], gF, d);
    d = (hs[0] > R(0)) ? d : R(0);
#pragma unroll
    for (int l = 0; l < NL - 1; ++l) {
        if constexpr (sizeof(R) == 4) d = mlp_hidden_blk<false>(W.wh[l], 0.f, d);
        else d = mlp_hidden(W.wh[l], 0.0, d);
        d = (hs[l + 1] > R(0)) ? d : R(0);
    }
    if constexpr (sizeof(R) == 4) {
        return out_rot(W.w5r, 0.f, d);           // slots 6, 7: exact zeros
    } else {
        R p[6];
#pragma unroll
        for (int q = 0; q < 6; ++q) p[q] = W.w5[q] * d;
        const R nn = wave_reduce6_to_lanes(p, lane);
        return ((lane & 7) < 6) ? nn : R(0);
    }
}

template <typename R, int NL, bool GD>
__global__ __launch_bounds__(64 * kJvpWaves, 1) void solve_jvp_kernel(const JvpArgs<R> a, const int method)
{
    constexpr int KT = kJvpTile<R>;
    __shared__ R rows[8 * kWave];                 // tableau coefficient rows (hode_tableau.h: tableau_rows_store)
    const int lane = threadIdx.x & 63;
    const int c8 = lane & 7, grp = lane >> 3;
    const int wave = first_lane((int)(threadIdx.x >> 6));
    tableau_rows_store<R>(rows, method, threadIdx.x, 64 * kJvpWaves);
    __syncthreads();
    const int b = blockIdx.x * kJvpWaves + wave;
    if (b >= a.B) return;
    const int k0 = blockIdx.y * KT;
    const int kt = (a.K - k0) < KT ? a.K - k0 : KT;   // directions of this tile (wave-uniform)
    const int T = a.T;
    const int set = b / (a.B / a.n_sets);
    const TableauData &tab = kTableau[method];
    const int S = tab.S;
    const int rowb = (method == HODE_METHOD_DP54) ? 6 : 7;   // solution weights: DP5(4) row 6 (FSAL row), RK4 row 7

    MlpRegs<R, NL> W;
    mlp_load<R, NL>(W, a.nn_p + (size_t)set * a.P, a.H, lane);
    OdeP<R> o;
    ode_load(o, a.ode_p + 17 * set);

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

    // output rows: lanes 8k + c (c < 6) write component c of direction k
    R *__restrict__ out = a.dy + ((size_t)b * a.K + k0) * T * 6;
    auto put_row = [&](int r, bool zero) {
        R v = R(0);
#pragma unroll
        for (int k = 0; k < KT; ++k) v = (grp == k) ? dy[k] : v;
        if (c8 < 6 && grp < kt) out[((size_t)grp * T + r) * 6 + c8] = zero ? R(0) : v;
    };
    put_row(0, false);

    const R *__restrict__ tg = a.t + (a.t_batched ? (size_t)b * T : 0);
    const R *__restrict__ tape = a.tape + (size_t)b * a.max_steps * 8;
    const int *__restrict__ tseg = a.tape_seg + (size_t)b * a.max_steps;
    constexpr int kSlot = NL * kWave + 8;         // stage record: h_1 .. h_NL | the stage state in 8 reals
    const R *__restrict__ stg = a.tape_stage + (size_t)b * a.max_steps * 6 * kSlot;
    const int n = a.nsteps[b] < a.max_steps ? a.nsteps[b] : a.max_steps;   // never walk past the tape

    // the next stage record, one stage ahead of its use
    R nh[NL], nY = R(0);
#pragma unroll
    for (int l = 0; l < NL; ++l) nh[l] = R(0);
    auto fetch = [&](int rec) {
        const R *__restrict__ r = stg + (size_t)rec * kSlot;
#pragma unroll
        for (int l = 0; l < NL; ++l) nh[l] = r[l * kWave + lane];
        nY = r[NL * kWave + c8];
    };
    if (n > 0) fetch(0);

    // The forward's row logic (hode_solve_body.h): a repeated grid time copies the state; a grid row gets the state at the end
    // of the step that closes its interval; after an interval that no taped step closes (the trajectory failed there) every
    // remaining row is 0.
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
            R dKK[KT];                            // stage tangents, packed: lanes 8s .. 8s+7 = stage s
#pragma unroll
            for (int k = 0; k < KT; ++k) dKK[k] = R(0);
#pragma unroll 1
            for (int s = 0; s < S; ++s) {
                R hs[NL];
#pragma unroll
                for (int l = 0; l < NL; ++l) hs[l] = nh[l];
                const R Ys = nY;
                const int nxt = (s + 1 < S) ? st * 6 + s + 1 : (st + 1 < n) ? (st + 1) * 6 : -1;
                if (nxt >= 0) fetch(nxt);
                const R ts = rfma((R)tab.c[s], h, tc);
                const R gdv = rfma((ts - t0) * inv_len, dd, d0);
                const R gde = GD ? gd_effect(o, gdv) : R(0);
                R js[5], jp[5];
                jvp_coeffs<R, GD>(o, lane_bcast(Ys, 0), lane_bcast(Ys, 1), lane_bcast(Ys, 2), lane_bcast(Ys, 3), lane_bcast(Ys, 5), gde,
                                  gdv, c8, js, jp);
                const R coef = rows[s * kWave + lane];
#pragma unroll
                for (int k = 0; k < KT; ++k) {
                    if (k < kt) {
                        const R dYs = rfma(h, group_sum8(coef * dKK[k]), dy[k]);
                        const R gG = state_bcast<0>(dYs), gI = state_bcast<1>(dYs), gGlu = state_bcast<2>(dYs),
                                gGLP = state_bcast<3>(dYs), gGE = state_bcast<4>(dYs), gF = state_bcast<5>(dYs);
                        R m = js[0] * gG;
                        m = rfma(js[1], gI, m);
                        m = rfma(js[2], gGlu, m);
                        m = rfma(js[3], gGLP, m);
                        m = rfma(js[4], gF, m);
#pragma unroll
                        for (int i = 0; i < 5; ++i) m = rfma(jp[i], vl[k][i], m);
                        const R dk = mlp_jvp<R, NL>(W, hs, gG, gI, gGlu, gGLP, gGE, gF, lane) + m;
                        dKK[k] = stage_put(dKK[k], dk, s);
                    }
                }
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

template <typename R, int NL> static int launch_jvp_nl(hipStream_t s, const JvpArgs<R> &a, int method)
{
    const dim3 grid((a.B + kJvpWaves - 1) / kJvpWaves, (a.K + kJvpTile<R> - 1) / kJvpTile<R>), block(64 * kJvpWaves);
    if (a.gd_mode != 0) hipLaunchKernelGGL((solve_jvp_kernel<R, NL, true>), grid, block, 0, s, a, method);
    else hipLaunchKernelGGL((solve_jvp_kernel<R, NL, false>), grid, block, 0, s, a, method);
    return hipGetLastError() == hipSuccess ? HODE_OK : HODE_ELAUNCH;
}

template <typename R> int launch_solve_jvp(hipStream_t s, const JvpArgs<R> &a, int L, int method)
{
    switch (L) {
    case 1: return launch_jvp_nl<R, 1>(s, a, method);
    case 2: return launch_jvp_nl<R, 2>(s, a, method);
    case 3: return launch_jvp_nl<R, 3>(s, a, method);
    case 4: return launch_jvp_nl<R, 4>(s, a, method);
    }
    return HODE_EUNSUPPORTED;
}
template int launch_solve_jvp<float>(hipStream_t, const JvpArgs<float> &, int, int);
template int launch_solve_jvp<double>(hipStream_t, const JvpArgs<double> &, int, int);

}  // namespace hode

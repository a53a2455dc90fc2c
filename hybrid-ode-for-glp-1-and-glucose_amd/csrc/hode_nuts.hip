// hode_nuts.hip -- the per-chain passes of multi-chain No-U-Turn sampling (inference/nuts.py; include/hode.h, "MCMC").
//
// Multinomial NUTS with the generalised U-turn criterion (Hoffman & Gelman 2014; Betancourt 2017), built iteratively: every
// call of pre / post places ONE leaf of every active chain's tree, so C chains whose trees have different sizes advance in
// lockstep.  A chain whose tree has ended is inactive: pre and post return at once for it, and compact gives the active
// chains consecutive slots (rank) in chain order, so the driver's solve runs on the active chains only.
//
// Per-chain state (rows [C][ld] as in hode_hmc.hip; tree = [HODE_NUTS_ROWS][C][ld]):
//   frontier (z, p, g): the last leaf placed; left / right edges (z, p, g); tree proposal and subtree proposal (z, g);
//   rho (momentum sum of the merged tree) and rho_sub (of the subtree being built);
//   ckpt [C][max_depth][2][ld]: for every open aligned block of 2^k leaves (k = 1..j) inside the subtree, p# = M^-1 p at the
//   block's first leaf and rho_sub just before it (Phan et al. 2019: one open block per size, so j checkpoints suffice);
//   dst fp64 [C][8] = {H0, log_w, log_w_sub, sum_acc, U of the proposal, U of the subtree proposal};
//   ist int32 [C][8] = {j, leaf index in the subtree, n_leaf, active, divergent, failed, direction, doublings started}.
// Random numbers: Philox streams kRngNutsDir (group j), kRngNutsLeaf (group n_leaf), kRngNutsMerge (group j) of the chain
// and iteration: a chain's draws depend on (seed, chain, iteration) only, never on C, the slot or the launch geometry.
// Every chain sum is taken in a fixed order; no floating-point atomics; the same call gives the same bits.
#include "hode_chains.h"
#include "hode_philox.h"

namespace hode {
namespace {

enum Row { kFZ, kFP, kFG, kLZ, kLP, kLG, kRZ, kRP, kRG, kPZ, kPG, kSZ, kSG, kRho, kRhoSub };
enum DSlot { kH0, kLogW, kLogWSub, kSumAcc, kUProp, kUSub };
enum ISlot { kJ, kLeaf, kNLeaf, kActive, kDivergent, kFailed, kDir, kDepth };

__device__ __forceinline__ double log_add_exp(double a, double b)
{
    const double m = a > b ? a : b, l = a > b ? b : a;
    return m + log1p(exp(l - m));
}

template <typename R> struct Rows {                     // the rows of chain c in the tree buffer
    R *base;
    int64_t stride, row;                                 // stride = C * ld
    __device__ R *operator()(int r) const { return base + r * stride + row; }
};

// ---------------------------------------------------------------- tree set-up after hode_hmc_refresh
template <typename R>
__global__ __launch_bounds__(kThreads) void nuts_begin_kernel(int C, int D, int ld, bool vec, const R *__restrict__ z,
                                                              const R *__restrict__ p, const R *__restrict__ g,
                                                              const double *__restrict__ U, const double *__restrict__ U0,
                                                              const double *__restrict__ ke0, R *__restrict__ tree,
                                                              double *__restrict__ dst, int32_t *__restrict__ ist)
{
    const int c = blockIdx.x;
    const int64_t row = (int64_t)c * ld;
    const Rows<R> t{tree, (int64_t)C * ld, row};
    for (int d0 = 4 * threadIdx.x; d0 < D; d0 += 4 * kThreads) {
        const int n = D - d0 < 4 ? D - d0 : 4;
        R zz[4], pp[4], gg[4];
        ld4(z + row + d0, vec, n, zz);
        ld4(p + row + d0, vec, n, pp);
        ld4(g + row + d0, vec, n, gg);
        st4(t(kLZ) + d0, vec, n, zz); st4(t(kLP) + d0, vec, n, pp); st4(t(kLG) + d0, vec, n, gg);
        st4(t(kRZ) + d0, vec, n, zz); st4(t(kRP) + d0, vec, n, pp); st4(t(kRG) + d0, vec, n, gg);
        st4(t(kPZ) + d0, vec, n, zz); st4(t(kPG) + d0, vec, n, gg);
        st4(t(kRho) + d0, vec, n, pp);
    }
    if (threadIdx.x == 0) {
        double *ds = dst + 8 * (int64_t)c;
        int32_t *is = ist + 8 * (int64_t)c;
        ds[kH0] = U0[c] + ke0[c];
        ds[kLogW] = 0.0;                                 // leaf weights relative to H0: the start has weight 1
        ds[kLogWSub] = -INFINITY;
        ds[kSumAcc] = 0.0;
        ds[kUProp] = U[c];
        ds[kUSub] = U[c];
        is[kJ] = 0; is[kLeaf] = 0; is[kNLeaf] = 0; is[kActive] = 1;
        is[kDivergent] = 0; is[kFailed] = 0; is[kDir] = 1; is[kDepth] = 0;
    }
}

// ---------------------------------------------------------------- start of a leaf: direction, half kick, drift, parameters
template <typename R>
__global__ __launch_bounds__(kThreads) void nuts_pre_kernel(int C, int D, int ld, bool vec, uint64_t seed, uint32_t iter,
                                                            const double *__restrict__ eps, const R *__restrict__ minv,
                                                            R *__restrict__ tree, int32_t *__restrict__ ist,
                                                            const int32_t *__restrict__ rank, uint32_t ode_mask, int n_ode,
                                                            const double *__restrict__ mu, const double *__restrict__ sd,
                                                            int sample_nn, int P, R *__restrict__ nn_p, R *__restrict__ ode_p)
{
    const int c = blockIdx.x;
    int32_t *is = ist + 8 * (int64_t)c;
    if (!is[kActive]) return;
    const int leaf = is[kLeaf], j = is[kJ];
    int v = is[kDir];
    if (leaf == 0)                                       // a doubling starts: its direction
        v = u01(hmc_rng(seed, (uint32_t)c, iter, kRngNutsDir, (uint32_t)j).x) < 0.5 ? 1 : -1;
    __syncthreads();                                     // every lane has read the state before lane 0 writes it
    if (leaf == 0 && threadIdx.x == 0) {
        is[kDir] = v;
        is[kDepth] = j + 1;
    }
    const Rows<R> t{tree, (int64_t)C * ld, (int64_t)c * ld};
    // a new subtree grows from the edge on its side, a running one from the frontier
    const int src = leaf ? kFZ : (v > 0 ? kRZ : kLZ);
    const R *sz = t(src), *sp = t(src + 1), *sg = t(src + 2);
    R *fz = t(kFZ), *fp = t(kFP);
    const double e = v * eps[c];
    const R eh = (R)(0.5 * e), ed = (R)e;
    const int64_t s = rank[c];                           // the chain's slot in the compacted solve
    for (int d0 = 4 * threadIdx.x; d0 < D; d0 += 4 * kThreads) {
        const int n = D - d0 < 4 ? D - d0 : 4;
        R zz[4], pp[4], gg[4], mi[4];
        ld4(sz + d0, vec, n, zz);
        ld4(sp + d0, vec, n, pp);
        ld4(sg + d0, vec, n, gg);
        ld4(minv + d0, vec, n, mi);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            pp[k] -= eh * gg[k];
            zz[k] += ed * mi[k] * pp[k];
        }
        st4(fp + d0, vec, n, pp);
        st4(fz + d0, vec, n, zz);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int d = d0 + k;
            if (k < n) {
                if (d < n_ode) {
                    if (ode_p) ode_p[s * 17 + ode_index(ode_mask, d)] = (R)(mu[d] + sd[d] * (double)zz[k]);
                } else if (sample_nn && nn_p) {
                    nn_p[s * P + (d - n_ode)] = zz[k];
                }
            }
        }
    }
}

// ---------------------------------------------------------------- end of a leaf: gradient, half kick, tree bookkeeping
template <typename R>
__global__ __launch_bounds__(kThreads) void nuts_post_kernel(NutsPostArgs<R> a)
{
    __shared__ double sh[8];
    __shared__ int shi[4];
    __shared__ int flag[3];                              // divergent, leaf taken, subtree taken
    const int c = blockIdx.x, D = a.D, ld = a.ld;
    const bool vec = a.vec;
    int32_t *is = a.ist + 8 * (int64_t)c;
    double *ds = a.dst + 8 * (int64_t)c;
    if (!is[kActive]) return;
    const int leaf = is[kLeaf], j = is[kJ], v = is[kDir], n_leaf = is[kNLeaf] + 1;
    const int64_t s = a.rank[c];
    const Rows<R> t{a.tree, (int64_t)a.C * ld, (int64_t)c * ld};
    R *fz = t(kFZ), *fp = t(kFP), *fg = t(kFG);
    const R eh = (R)(0.5 * v * a.eps[c]);
    const R *minv = a.minv;

    // 1. grad U = likelihood gradient (the chain's slot) + z; second half kick; U = lik + |z|^2 / 2, ke = p^T M^-1 p / 2
    double zz2 = 0.0, ke = 0.0;
    for (int d0 = 4 * threadIdx.x; d0 < D; d0 += 4 * kThreads) {
        const int n = D - d0 < 4 ? D - d0 : 4;
        R zz[4], pp[4], gg[4], mi[4];
        ld4(fz + d0, vec, n, zz);
        ld4(fp + d0, vec, n, pp);
        ld4(minv + d0, vec, n, mi);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int d = d0 + k;
            R lik = R(0);
            if (k < n) {
                if (d < a.n_ode) {
                    if (a.gode) lik = a.gode[s * 17 + ode_index(a.ode_mask, d)] * (R)a.sd[d];
                } else if (a.gnn) {
                    lik = a.gnn[s * a.P + (d - a.n_ode)];
                }
            }
            gg[k] = k < n ? lik + zz[k] : R(0);
            pp[k] -= eh * gg[k];
            if (k < n) {
                zz2 += (double)zz[k] * (double)zz[k];
                ke += (double)pp[k] * (double)pp[k] * (double)mi[k];
            }
        }
        st4(fg + d0, vec, n, gg);
        st4(fp + d0, vec, n, pp);
    }
    int bad = 0;
    if (a.status)
        for (int b = threadIdx.x; b < a.n_traj; b += kThreads) bad |= a.status[s * a.n_traj + b] != 0;
    bad = block_or(bad, shi);
    block_sum2(zz2, ke, sh);

    // 2. divergence, accept statistic, multinomial choice inside the subtree
    if (threadIdx.x == 0) {
        const double U = (a.loss_sum ? a.lik_scale * a.loss_sum[s] : 0.0) + 0.5 * zz2;
        const double H = U + 0.5 * ke, H0 = ds[kH0];
        is[kNLeaf] = n_leaf;
        if (bad) is[kFailed] = 1;
        const bool div = bad || !isfinite(H) || H - H0 > 1000.0;
        int take = 0;
        if (div) {                                       // rejects the subtree, ends the tree; adds 0 to the accept statistic
            is[kDivergent] = 1;
            is[kActive] = 0;
        } else {
            const double lw = H0 - H;
            ds[kSumAcc] += lw >= 0.0 ? 1.0 : exp(lw);
            const double lws = leaf == 0 ? lw : log_add_exp(ds[kLogWSub], lw);
            ds[kLogWSub] = lws;
            const double u = u01(hmc_rng(a.seed, (uint32_t)c, a.iter, kRngNutsLeaf, (uint32_t)n_leaf).x);
            take = u < exp(lw - lws);
            if (take) ds[kUSub] = U;
        }
        flag[0] = div;
        flag[1] = take;
    }
    __syncthreads();
    if (flag[0]) return;
    const bool take = flag[1] != 0;

    // 3. subtree proposal, rho_sub, checkpoints of the aligned blocks that start at this leaf (k = 1..j, 2^k | leaf)
    int starts = 0;
    while (starts < j && (leaf & ((2 << starts) - 1)) == 0) ++starts;
    R *rs = t(kRhoSub);
    const int64_t ck = (int64_t)c * a.max_depth * 2;   // checkpoint rows of chain c: ck + 2 (k - 1) + {0: p#, 1: rho before}
    for (int d0 = 4 * threadIdx.x; d0 < D; d0 += 4 * kThreads) {
        const int n = D - d0 < 4 ? D - d0 : 4;
        R pp[4], mi[4], rr[4], ps[4];
        ld4(fp + d0, vec, n, pp);
        ld4(minv + d0, vec, n, mi);
        if (leaf) {
            ld4(rs + d0, vec, n, rr);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) rr[k] = R(0);
        }
        if (take) {
            R zz[4], gg[4];
            ld4(fz + d0, vec, n, zz);
            ld4(fg + d0, vec, n, gg);
            st4(t(kSZ) + d0, vec, n, zz);
            st4(t(kSG) + d0, vec, n, gg);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) ps[k] = mi[k] * pp[k];
        for (int k = 0; k < starts; ++k) {
            st4(a.ckpt + (ck + 2 * k) * ld + d0, vec, n, ps);
            st4(a.ckpt + (ck + 2 * k + 1) * ld + d0, vec, n, rr);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) rr[k] += pp[k];
        st4(rs + d0, vec, n, rr);
    }

    // 4. U-turn checks of the aligned blocks that end at this leaf (k = 1..j, 2^k | leaf + 1)
    int turn = 0;
    for (int lv = 0; lv < j && ((leaf + 1) & ((2 << lv) - 1)) == 0 && !turn; ++lv) {
        const R *cp = a.ckpt + (ck + 2 * lv) * ld, *cr = a.ckpt + (ck + 2 * lv + 1) * ld;
        double first = 0.0, last = 0.0;
        for (int d0 = 4 * threadIdx.x; d0 < D; d0 += 4 * kThreads) {
            const int n = D - d0 < 4 ? D - d0 : 4;
            R pf[4], rb[4], rr[4], pp[4], mi[4];
            ld4(cp + d0, vec, n, pf);
            ld4(cr + d0, vec, n, rb);
            ld4(rs + d0, vec, n, rr);
            ld4(fp + d0, vec, n, pp);
            ld4(minv + d0, vec, n, mi);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < n) {
                    const double blk = (double)rr[k] - (double)rb[k];
                    first += (double)pf[k] * blk;
                    last += (double)mi[k] * (double)pp[k] * blk;
                }
        }
        block_sum2(first, last, sh);
        turn = !(first > 0.0 && last > 0.0);
    }
    if (turn) {                                          // rejects the subtree, ends the tree
        if (threadIdx.x == 0) is[kActive] = 0;
        return;
    }
    if (leaf + 1 < (1 << j)) {
        if (threadIdx.x == 0) is[kLeaf] = leaf + 1;
        return;
    }

    // 5. the subtree is complete: biased progressive sampling, merge, U-turn check of the whole tree
    if (threadIdx.x == 0) {
        const double lw = ds[kLogW], lws = ds[kLogWSub];
        const double u = u01(hmc_rng(a.seed, (uint32_t)c, a.iter, kRngNutsMerge, (uint32_t)j).x);
        const int take2 = u < exp(lws - lw);
        if (take2) ds[kUProp] = ds[kUSub];
        ds[kLogW] = log_add_exp(lw, lws);
        flag[2] = take2;
    }
    __syncthreads();
    const bool take2 = flag[2] != 0;
    const int e = v > 0 ? kRZ : kLZ, o = v > 0 ? kLZ : kRZ;
    R *rho = t(kRho);
    double dv = 0.0, dopp = 0.0;
    for (int d0 = 4 * threadIdx.x; d0 < D; d0 += 4 * kThreads) {
        const int n = D - d0 < 4 ? D - d0 : 4;
        R zz[4], pp[4], gg[4], rr[4], rsub[4], po[4], mi[4];
        ld4(fz + d0, vec, n, zz);
        ld4(fp + d0, vec, n, pp);
        ld4(fg + d0, vec, n, gg);
        ld4(rho + d0, vec, n, rr);
        ld4(rs + d0, vec, n, rsub);
        ld4(t(o + 1) + d0, vec, n, po);
        ld4(minv + d0, vec, n, mi);
        st4(t(e) + d0, vec, n, zz);
        st4(t(e + 1) + d0, vec, n, pp);
        st4(t(e + 2) + d0, vec, n, gg);
        if (take2) {
            R sz[4], sg[4];
            ld4(t(kSZ) + d0, vec, n, sz);
            ld4(t(kSG) + d0, vec, n, sg);
            st4(t(kPZ) + d0, vec, n, sz);
            st4(t(kPG) + d0, vec, n, sg);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            rr[k] += rsub[k];
            if (k < n) {
                dv += (double)mi[k] * (double)pp[k] * (double)rr[k];
                dopp += (double)mi[k] * (double)po[k] * (double)rr[k];
            }
        }
        st4(rho + d0, vec, n, rr);
    }
    block_sum2(dv, dopp, sh);
    if (threadIdx.x == 0) {
        is[kJ] = j + 1;
        is[kLeaf] = 0;
        if (!(dv > 0.0 && dopp > 0.0) || j + 1 >= a.max_depth) is[kActive] = 0;
    }
}

// ---------------------------------------------------------------- active flags -> slots in chain order, and their count
__global__ __launch_bounds__(kThreads) void nuts_compact_kernel(int C, const int32_t *__restrict__ ist, int32_t *__restrict__ rank,
                                                                int32_t *__restrict__ count)
{
    __shared__ int wsum[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int base = 0;
    for (int c0 = 0; c0 < C; c0 += kThreads) {
        const int c = c0 + threadIdx.x;
        const bool on = c < C && ist[8 * (int64_t)c + kActive] != 0;
        const unsigned long long m = __ballot(on);
        const int before = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wsum[w] = __popcll(m);
        __syncthreads();
        int off = base;
        for (int k = 0; k < w; ++k) off += wsum[k];
        if (c < C) rank[c] = on ? off + before : -1;
        base += (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
        __syncthreads();
    }
    if (threadIdx.x == 0) count[0] = base;
}

// ---------------------------------------------------------------- end of an iteration: the proposal, dual averaging, draws
template <typename R>
__global__ __launch_bounds__(kThreads) void nuts_finish_kernel(int C, int D, int ld, bool vec, int adapt, double delta,
                                                               R *__restrict__ z, R *__restrict__ g, double *__restrict__ U,
                                                               const R *__restrict__ tree, const double *__restrict__ dst,
                                                               const int32_t *__restrict__ ist, double *__restrict__ log_eps,
                                                               double *__restrict__ da, int n_ode, const double *__restrict__ mu,
                                                               const double *__restrict__ sd, R *__restrict__ draws,
                                                               double *__restrict__ stats, int n_slots, int slot)
{
    const int c = blockIdx.x;
    const int64_t row = (int64_t)c * ld, stride = (int64_t)C * ld;
    const double *ds = dst + 8 * (int64_t)c;
    const int32_t *is = ist + 8 * (int64_t)c;
    const R *pz = tree + kPZ * stride + row, *pg = tree + kPG * stride + row;
    for (int d0 = 4 * threadIdx.x; d0 < D; d0 += 4 * kThreads) {
        const int n = D - d0 < 4 ? D - d0 : 4;
        R zz[4], gg[4];
        ld4(pz + d0, vec, n, zz);
        ld4(pg + d0, vec, n, gg);
        st4(z + row + d0, vec, n, zz);
        st4(g + row + d0, vec, n, gg);
        if (draws && slot >= 0) {
            R *dr = draws + ((int64_t)c * n_slots + slot) * D;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int d = d0 + k;
                if (k < n) dr[d] = d < n_ode ? (R)(mu[d] + sd[d] * (double)zz[k]) : zz[k];
            }
        }
    }
    if (threadIdx.x == 0) {
        const int n_leaf = is[kNLeaf];
        const double acc = n_leaf > 0 ? ds[kSumAcc] / n_leaf : 0.0;
        U[c] = ds[kUProp];
        if (adapt) dual_average(da + 4 * (int64_t)c, delta, acc, &log_eps[c]);
        if (slot >= 0) {
            double *st = stats + ((int64_t)c * n_slots + slot) * 6;
            st[0] = acc;
            st[1] = -ds[kUProp];
            st[2] = is[kDivergent] ? 1.0 : 0.0;
            st[3] = is[kFailed] ? 1.0 : 0.0;
            st[4] = (double)is[kDepth];
            st[5] = (double)n_leaf;
        }
    }
}

}  // namespace

template <typename R> int launch_nuts_begin(hipStream_t s, int C, int D, int ld, const R *z, const R *p, const R *g, const double *U,
                                            const double *U0, const double *ke0, R *tree, double *dst, int32_t *ist)
{
    const bool vec = rows_vec<R>(ld, {z, p, g, tree});
    hipLaunchKernelGGL(nuts_begin_kernel<R>, dim3(C), dim3(kThreads), 0, s, C, D, ld, vec, z, p, g, U, U0, ke0, tree, dst, ist);
    return done();
}

template <typename R> int launch_nuts_pre(hipStream_t s, const NutsPreArgs<R> &a)
{
    const bool vec = rows_vec<R>(a.ld, {a.minv, a.tree});
    hipLaunchKernelGGL(nuts_pre_kernel<R>, dim3(a.C), dim3(kThreads), 0, s, a.C, a.D, a.ld, vec, a.seed, a.iter, a.eps, a.minv, a.tree,
                       a.ist, a.rank, a.ode_mask, a.n_ode, a.mu, a.sd, a.sample_nn, a.P, a.nn_p, a.ode_p);
    return done();
}

template <typename R> int launch_nuts_post(hipStream_t s, NutsPostArgs<R> a)
{
    a.vec = rows_vec<R>(a.ld, {a.minv, a.tree, a.ckpt});
    hipLaunchKernelGGL(nuts_post_kernel<R>, dim3(a.C), dim3(kThreads), 0, s, a);
    return done();
}

int launch_nuts_compact(hipStream_t s, int C, const int32_t *ist, int32_t *rank, int32_t *count)
{
    hipLaunchKernelGGL(nuts_compact_kernel, dim3(1), dim3(kThreads), 0, s, C, ist, rank, count);
    return done();
}

template <typename R> int launch_nuts_finish(hipStream_t s, const NutsFinishArgs<R> &a)
{
    const bool vec = rows_vec<R>(a.ld, {a.z, a.g, a.tree});
    hipLaunchKernelGGL(nuts_finish_kernel<R>, dim3(a.C), dim3(kThreads), 0, s, a.C, a.D, a.ld, vec, a.adapt, a.delta, a.z, a.g, a.U,
                       a.tree, a.dst, a.ist, a.log_eps, a.da, a.n_ode, a.mu, a.sd, a.draws, a.stats, a.n_slots, a.slot);
    return done();
}

#define HODE_NUTS_INST(R)                                                                                                         \
    template int launch_nuts_begin<R>(hipStream_t, int, int, int, const R *, const R *, const R *, const double *, const double *,  \
                                      const double *, R *, double *, int32_t *);                                                  \
    template int launch_nuts_pre<R>(hipStream_t, const NutsPreArgs<R> &);                                                         \
    template int launch_nuts_post<R>(hipStream_t, NutsPostArgs<R>);                                                               \
    template int launch_nuts_finish<R>(hipStream_t, const NutsFinishArgs<R> &);
HODE_NUTS_INST(float)
HODE_NUTS_INST(double)

}  // namespace hode

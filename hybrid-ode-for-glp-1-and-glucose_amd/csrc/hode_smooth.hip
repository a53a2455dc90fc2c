// hode_smooth.hip -- backward-simulation smoothing of a stored particle filter (inference/filter.py, FilterResult.smooth;
// include/hode.h, "Particle smoother"): M backward trajectories per patient, the whole pass in ONE launch.
//
// One workgroup of kThreads lanes per (patient, 256 trajectories); lane = one trajectory, which keeps its current state x~ (six
// doubles) and slot in registers from step to step.  At step s the workgroup stages the N candidates of that step into LDS,
// kTile at a time: the log-weight and, per state, the one number the transition density needs of the candidate (log p - s^2 / 2
// under the log link, p otherwise), so a logarithm is taken once per candidate and not once per pair.  Every lane then walks the
// tile; all lanes read the same address, which LDS serves as a broadcast, 16 bytes at a time.
//   pass 1   mx = max_i l_i                           (no exponential)
//   pass 2   tot = sum_i exp(l_i - mx), i = 0..N-1 in order: the header's sequential c_{N-1}
//   pass 3   the same running sum again, counting the i with c_i < u * tot: that count is min{k : c_k >= u * tot}
// l_i is recomputed in every pass (about 25 flops; nothing of size N per lane can stay on chip).  With N <= kTile the tile is
// staged once per step, otherwise once per pass.  A lane's sum is sequential, so c_k > c_{k-1} at the chosen k and the chosen
// candidate always has w_k > 0: the "moved back" clause of the header never has anything to do here.
// fp64 throughout, contraction off, no atomics: a trajectory's bits depend on (seed, id0 + b, m) and the patient's data only.
#include "hode_chains.h"
#include "hode_philox.h"
#include <limits>

#pragma clang fp contract(off)

namespace hode {
namespace {

constexpr int kTile = 1024;            // candidates in LDS at a time: 7 doubles each, 56 KB, two workgroups per CU

template <typename R> struct SmoothArgs {
    int B, N, M, S, link, n_mblk;
    uint32_t id0;
    uint64_t seed;
    const R *hist, *pred;
    const double *lwh, *q, *dt;
    int32_t *idx;
    R *paths;
};

struct SmoothTile {
    double2 c01[kTile], c23[kTile], c45[kTile];
    double lw[kTile];
};

// l_i of the candidate at tile position t for a lane whose state enters as a[] (log x~ - or x~ itself - per state)
__device__ __forceinline__ double pair_logit(const SmoothTile &T, int t, const double (&a)[6], const double (&r)[6], uint32_t pos, bool trans)
{
    const double ninf = -std::numeric_limits<double>::infinity();
    double l = T.lw[t];
    if (trans) {
        const double2 c01 = T.c01[t], c23 = T.c23[t], c45 = T.c45[t];
        const double c[6] = {c01.x, c01.y, c23.x, c23.y, c45.x, c45.y};
        double acc = 0.0;
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            if (pos >> j & 1u) {                               // (uniform over the workgroup)
                const double z = (a[j] - c[j]) * r[j];
                acc += -0.5 * (z * z);
            } else {
                acc += a[j] == c[j] ? 0.0 : ninf;
            }
        }
        l = l + acc;
    }
    return __builtin_isfinite(l) ? l : ninf;
}

template <typename R> __global__ __launch_bounds__(kThreads) void pf_smooth_kernel(const SmoothArgs<R> a)
{
    __shared__ SmoothTile T;
    const double ninf = -std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const int N = a.N, B = a.B, M = a.M, tid = threadIdx.x;
    const int b = (int)(blockIdx.x / (uint32_t)a.n_mblk);
    const int64_t m = (int64_t)(blockIdx.x % (uint32_t)a.n_mblk) * kThreads + tid;
    const bool mine = m < M;
    const uint32_t key = a.id0 + (uint32_t)b;
    const int n_tiles = (N + kTile - 1) / kTile;

    double xt[6] = {nan, nan, nan, nan, nan, nan};            // x~ = hist[s + 1][k_{s + 1}]
    bool lost = !mine;

    for (int s = a.S - 1; s >= 0; --s) {
        const bool trans = s < a.S - 1;
        const int64_t row = ((int64_t)s * B + b) * N;                       // candidates of step s
        const int64_t row1 = ((int64_t)(s + 1) * B + b) * N;                // their pred rows are stored with step s + 1
        double r[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, half_s2[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, al[6];
        uint32_t pos = 0u;
        if (trans) {
            const double rdt = sqrt(a.dt[(int64_t)(s + 1) * B + b]);
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                const double sg = a.q[j] * rdt;
                if (sg > 0.0) {
                    pos |= 1u << j;
                    r[j] = 1.0 / sg;
                    half_s2[j] = 0.5 * (sg * sg);
                }
            }
        }
        const bool lg = a.link == HODE_PF_LINK_LOG;
#pragma unroll
        for (int j = 0; j < 6; ++j) al[j] = (lg && (pos >> j & 1u)) ? log(xt[j]) : xt[j];

        double mx = ninf, tot = 0.0, target = 0.0, run = 0.0;
        int k = 0;
        for (int pass = 0; pass < 3; ++pass) {
            for (int t0 = 0, tile = 0; tile < n_tiles; ++tile, t0 += kTile) {
                const int nt = min(kTile, N - t0);
                if (n_tiles > 1 || pass == 0) {
                    if (n_tiles > 1) __syncthreads();               // the walk of the tile before is over
                    for (int t = tid; t < nt; t += kThreads) {
                        T.lw[t] = a.lwh[row + t0 + t];
                        if (trans) {
                            const R *p = a.pred + 6 * (row1 + t0 + t);
                            double c[6];
#pragma unroll
                            for (int j = 0; j < 6; ++j) {
                                const double pj = (double)p[j];
                                c[j] = (lg && (pos >> j & 1u)) ? log(pj) - half_s2[j] : pj;
                            }
                            T.c01[t] = make_double2(c[0], c[1]);
                            T.c23[t] = make_double2(c[2], c[3]);
                            T.c45[t] = make_double2(c[4], c[5]);
                        }
                    }
                    __syncthreads();
                }
                if (pass == 0) {
#pragma unroll 2
                    for (int t = 0; t < nt; ++t) mx = fmax(mx, pair_logit(T, t, al, r, pos, trans));
                } else if (pass == 1) {
#pragma unroll 2
                    for (int t = 0; t < nt; ++t) {
                        const double l = pair_logit(T, t, al, r, pos, trans);
                        tot += l > ninf ? exp(l - mx) : 0.0;
                    }
                } else {
#pragma unroll 2
                    for (int t = 0; t < nt; ++t) {
                        const double l = pair_logit(T, t, al, r, pos, trans);
                        run += l > ninf ? exp(l - mx) : 0.0;
                        k += run < target ? 1 : 0;
                    }
                }
            }
            if (pass == 1) {
                const uint32_t grp = (uint32_t)(mine ? m : 0);
                target = u01(hmc_rng(a.seed, key, (uint32_t)s, kRngFilterSmooth, grp).x) * tot;
            }
        }
        __syncthreads();                                            // every lane is done with the tile before step s - 1 restages it

        // no candidate alive: this step and all earlier ones of the trajectory are lost (x~ = NaN keeps every later l non-finite)
        lost = lost || !(mx > ninf);
        if (k > N - 1) k = N - 1;                                   // (cannot happen: u < 1 and c_{N-1} = tot)
        if (mine) {
            const int64_t o = ((int64_t)s * B + b) * M + m;
            a.idx[o] = lost ? -1 : k;
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                const R v = lost ? (R)nan : a.hist[6 * (row + k) + j];
                a.paths[6 * o + j] = v;
                xt[j] = (double)v;
            }
        }
    }
}

template <typename R>
int pf_smooth(void *stream, int B, int N, int M, int S, uint64_t seed, uint32_t id0, const R *hist, const double *lwh, const R *pred,
              const double *q, const double *dt, int link, int32_t *idx, R *paths)
{
    if (B < 1 || N < 1 || M < 1 || S < 1 || (link != HODE_PF_LINK_ADD && link != HODE_PF_LINK_LOG)) return HODE_EINVAL;
    if (!hist || !lwh || !pred || !q || !dt || !idx || !paths) return HODE_EINVAL;
    if (N > HODE_PF_MAX_PARTICLES) return HODE_EUNSUPPORTED;
    const int64_t n_mblk = ((int64_t)M + kThreads - 1) / kThreads;
    if (n_mblk * B > 0x7fffffffLL) return HODE_EUNSUPPORTED;         // one grid: B * ceil(M / 256) workgroups
    SmoothArgs<R> a{};
    a.B = B; a.N = N; a.M = M; a.S = S; a.link = link; a.n_mblk = (int)n_mblk; a.id0 = id0; a.seed = seed;
    a.hist = hist; a.pred = pred; a.lwh = lwh; a.q = q; a.dt = dt; a.idx = idx; a.paths = paths;
    hipLaunchKernelGGL((pf_smooth_kernel<R>), dim3((uint32_t)(n_mblk * B)), dim3(kThreads), 0, (hipStream_t)stream, a);
    return done();
}

}  // namespace
}  // namespace hode

extern "C" {

int hode_pf_smooth_f32(void *stream, int B, int N, int M, int S, uint64_t seed, uint32_t id0, const float *hist, const double *lwh,
                       const float *pred, const double *q, const double *dt, int link, int32_t *idx, float *paths)
{
    return hode::pf_smooth<float>(stream, B, N, M, S, seed, id0, hist, lwh, pred, q, dt, link, idx, paths);
}
int hode_pf_smooth_f64(void *stream, int B, int N, int M, int S, uint64_t seed, uint32_t id0, const double *hist, const double *lwh,
                       const double *pred, const double *q, const double *dt, int link, int32_t *idx, double *paths)
{
    return hode::pf_smooth<double>(stream, B, N, M, S, seed, id0, hist, lwh, pred, q, dt, link, idx, paths);
}

}  // extern "C"

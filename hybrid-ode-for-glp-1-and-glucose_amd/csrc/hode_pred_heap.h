// hode_pred_heap.h -- what the per-entry folds over posterior draws share (hode_predictive.hip, hode_loo.hip): the "observed"
// test, the binary heaps an entry keeps in global memory (slot-major, so a wave's accesses at one depth coalesce), their
// in-place sort, and the last pass of a per-state table reduction.
#pragma once
#include "hode_chains.h"

namespace hode {
namespace {

constexpr double kHalfLog2Pi = 0.91893853320467274178;

template <typename R> __device__ __forceinline__ bool seen(R o, unsigned m) { return m != 0u && __builtin_isfinite(o); }

// heap order: in a max-heap a parent is not below its children, in a min-heap not above.  `max` is a run-time value so that
// the lanes of a wave that walk lo and the lanes that walk hi share one loop
template <typename R> __device__ __forceinline__ bool below(bool max, R a, R b) { return max ? a < b : b < a; }

// v into the hole at slot p of entry i's heap, the hole rising while its parent is below v
template <typename R> __device__ __forceinline__ void sift_up(R *h, bool max, int64_t N, int64_t i, int64_t p, R v)
{
    while (p > 0) {
        const int64_t q = (p - 1) >> 1;
        const R u = h[q * N + i];
        if (!below(max, u, v)) break;
        h[p * N + i] = u;
        p = q;
    }
    h[p * N + i] = v;
}

// v into the hole at the root of entry i's heap of `size` slots, the hole sinking while v is below its greater child;
// returns the new root
template <typename R> __device__ __forceinline__ R sift_down(R *h, bool max, int64_t N, int64_t i, int64_t size, R v)
{
    int64_t p = 0;
    R root = v;
    for (;;) {
        int64_t c = 2 * p + 1;
        if (c >= size) break;
        R u = h[c * N + i];
        if (c + 1 < size) {
            const R w = h[(c + 1) * N + i];
            if (below(max, u, w)) { u = w; c += 1; }
        }
        if (!below(max, v, u)) break;
        h[p * N + i] = u;
        if (p == 0) root = u;
        p = c;
    }
    h[p * N + i] = v;
    return root;
}

// entry i's heap of m slots sorted in place, greatest first for a max-heap and least first for a min-heap (so it is still a
// heap): heapsort leaves the opposite order, which is then reversed
template <typename R> __device__ __forceinline__ void sort_heap(R *h, bool max, int64_t N, int64_t i, int64_t m)
{
    for (int64_t end = m - 1; end > 0; --end) {
        const R v = h[end * N + i];
        h[end * N + i] = h[i];
        sift_down(h, max, N, i, end, v);
    }
    for (int64_t l = 0, r = m - 1; l < r; ++l, --r) {
        const R u = h[l * N + i], w = h[r * N + i];
        h[l * N + i] = w;
        h[r * N + i] = u;
    }
}

// table[k][c] = the partial rows added in index order
__global__ __launch_bounds__(kThreads) void pred_score_finish_kernel(int n_rows, int len, const double *work, double *table)
{
    for (int i = threadIdx.x; i < len; i += kThreads) {
        double t = 0.0;
        for (int r = 0; r < n_rows; ++r) t += work[(int64_t)r * len + i];
        table[i] = t;
    }
}

}  // namespace
}  // namespace hode

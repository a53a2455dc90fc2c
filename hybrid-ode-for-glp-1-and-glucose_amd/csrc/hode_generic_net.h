// hode_generic_net.h -- what the kernels of the GENERIC network path share about a network (K1 .. K5: hode_generic_rhs.h and
// hode_generic_vjp.h with the sources that include them, hode_generic_bwd_multi.hip; K6: hode_generic_jvp.hip): the derivative of
// an activation from its taped value, the flat parameter layout, the LDS image of the edge parameters, and the skewed LDS
// activation vector with its chunked weight loads.
#pragma once
#include "hode_xlane.h"
#include "../../include/hode.h"

namespace hode {

// "cotangent (or tangent) times the activation's derivative" from the POST-activation value:
// h > 0 iff the pre-activation is > 0 for all four; ELU'(x <= 0) = exp(x) = h + 1  (torch: nn.ReLU / Tanh / ELU / LeakyReLU(0.1),
// reference models/nn_residual.py:50-56)
template <typename R> __device__ __forceinline__ R act_bwd(R d, R h, int act)
{
    if (act == HODE_ACT_RELU) return h > R(0) ? d : R(0);            // (a select, not a product: 0 * inf stays 0)
    if (act == HODE_ACT_TANH) return d * (R(1) - h * h);
    if (act == HODE_ACT_ELU) return h > R(0) ? d : d * (h + R(1));
    return h > R(0) ? d : R(0.1) * d;
}

// one parameter set in the flat PyTorch parameters() layout (include/hode.h)
template <typename R> struct StreamNet {
    const R *p;
    int H, L;
    int act = HODE_ACT_RELU;
    __device__ __forceinline__ const R *W1() const { return p; }                       // [H][9]
    __device__ __forceinline__ const R *b1() const { return p + 9 * H; }
    __device__ __forceinline__ size_t hid_off(int l) const { return (size_t)9 * H + H + (size_t)l * ((size_t)H * H + H); }
    __device__ __forceinline__ const R *Wh(int l) const { return p + hid_off(l); }       // hidden matrix l = 0..L-2: [H][H]
    __device__ __forceinline__ const R *bh(int l) const { return Wh(l) + (size_t)H * H; }
    __device__ __forceinline__ size_t out_off() const { return hid_off(L - 1); }
    __device__ __forceinline__ const R *Wo() const { return p + out_off(); }             // [6][H]
    __device__ __forceinline__ const R *bo() const { return Wo() + 6 * H; }
};

// Where the EDGE parameters -- first matrix, output matrix, every bias: (16 + L) H + 6 values, 11.5 KB for 5 x 128 -- are read from.
//   EdgeFromParams  the flat parameter vector in global memory (K1 / K5: one evaluation per sample, nothing to amortise)
//   EdgeImage       a copy in the workgroup's LDS, made once per trajectory (solve kernels).  These ~35 loads per evaluation were
//                   issued again at every one of the 360+ evaluations of a trajectory -- hipcc cannot hoist them over the kernel's
//                   stores -- and each group of them is an L2 round trip in front of a dependent computation.
// Image layout: W1[H][9] | b1[H] | b_hidden[L-1][H] | Wout[6][H] | bout[6].
template <typename R> struct EdgeFromParams {
    const StreamNet<R> &n;
    __device__ __forceinline__ const R *W1() const { return n.W1(); }
    __device__ __forceinline__ const R *b1() const { return n.b1(); }
    __device__ __forceinline__ const R *bh(int l) const { return n.bh(l); }
    __device__ __forceinline__ const R *Wo() const { return n.Wo(); }
    __device__ __forceinline__ const R *bo() const { return n.bo(); }
};
constexpr int kEdgeImageMax = (16 + 8) * 128 + 8;        // H <= 128, L <= 8
template <typename R> struct EdgeImage {
    const R *img;
    int H, L;
    __device__ __forceinline__ const R *W1() const { return img; }
    __device__ __forceinline__ const R *b1() const { return img + 9 * H; }
    __device__ __forceinline__ const R *bh(int l) const { return img + (10 + l) * H; }
    __device__ __forceinline__ const R *Wo() const { return img + (9 + L) * H; }
    __device__ __forceinline__ const R *bo() const { return img + (15 + L) * H; }
    // cooperative copy by the whole workgroup (nthreads threads); the caller synchronises before the first use
    static __device__ __forceinline__ void fill(R *__restrict__ img, const StreamNet<R> &n, int tid, int nthreads)
    {
        const int H = n.H, L = n.L;
        for (int i = tid; i < 10 * H; i += nthreads) img[i] = n.p[i];                         // W1 | b1: contiguous
        for (int i = tid; i < (L - 1) * H; i += nthreads) img[10 * H + i] = n.bh(i / H)[i % H];
        for (int i = tid; i < 6 * H + 6; i += nthreads) img[(9 + L) * H + i] = n.Wo()[i];     // Wout | bout: contiguous
    }
};

constexpr int kHbStride = 160;       // 128 values + the skew below
// Position of activation k in an LDS vector read in chunks of CC by eight lanes at a time: every chunk start moves 4 banks on
// (CC = 16: chunk c starts at dword 20 c; CC = 8: the upper four chunks shift by 4), so the eight 16-byte reads of a ds_read_b128
// fall into eight different bank quads.  Unskewed, chunk starts 16 c hit two bank quads: 68 % of the LDS cycles of the forward
// were bank conflicts (tools/pmc_generic.sh).
template <int CC> __device__ __forceinline__ int hx(int k) { return k + 4 * (k >> (CC == 16 ? 4 : 5)); }

// CC consecutive weights of one matrix row.  fp32 rows that start on a 16-byte boundary (H a multiple of 4 and the parameter set
// itself aligned: always for a single set) are read as dwordx4; left to itself hipcc vectorises the scalar loop with a peeled first
// element -- dwordx4 loads at offsets 4, 20, 36 that straddle every 16-byte boundary (8.1 against 5.6 ms for the 1 024 x 61 forward).
template <typename R, int CC> __device__ __forceinline__ void load_chunk(const R *__restrict__ wrow, R (&w)[CC], bool aligned16)
{
    if constexpr (sizeof(R) == 4) {
        if (aligned16) {
            typedef float __attribute__((ext_vector_type(4))) f4;
            const f4 *__restrict__ q = reinterpret_cast<const f4 *>(wrow);
#pragma unroll
            for (int v = 0; v < CC / 4; ++v) {
                const f4 x = q[v];
                w[4 * v] = x.x; w[4 * v + 1] = x.y; w[4 * v + 2] = x.z; w[4 * v + 3] = x.w;
            }
            return;
        }
    }
#pragma unroll
    for (int u = 0; u < CC; ++u) w[u] = wrow[u];
}

}  // namespace hode

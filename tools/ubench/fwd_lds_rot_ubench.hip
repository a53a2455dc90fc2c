// The late rotations of a row-block hidden layer through LDS instead of DPP: does it pay?
// Production form (csrc/hode_mlp.h mlp_hidden_blk): 2 v_pk_mul + 15 x (v_mov_b32_dpp row_ror:n + 2 v_pk_fma_f32) + finish, the
// accumulators in v[4:7], the moved operand in v8, the input in v10 -- all by name, two asm statements per layer.
// Hybrid form, K in {4, 8, 12}: the wave writes its input to a private LDS buffer of 4 rows x 48 dwords (row r = its 16 activations
// twice, at entries j and j + 16: ONE ds_write2_b32, offsets 0 and 16) and fetches the operands of rotations 16-K..15 at the layer's
// start, two per ds_read2_b32 into an aligned pair (lane (r, i) reads rotation n at entry i + 16 - n); rotations 0..15-K stay DPP and
// hide the round trip; one s_waitcnt lgkmcnt(0) that ends the first statement, as in the product; the packed FMAs of rotation n take the pair's low half, those of n + 1 its high half.
// Same products, same order per accumulator: every form prints the same [out].  Row stride 48: rows 0/1 and 2/3 fall on disjoint
// halves of the 32 banks inside each 32-lane group, so neither the write nor a read has a bank conflict.
//   k_tput<K>    throughput loop: layers back to back on a fixed input, nothing in between
//   k_chain<K>   the forward kernel's own shape: a dependent chain of three layers, then 75 plain v_fma_f32 (five independent
//                chains, the mechanistic part / stage sums stand-in) that feed the next chain's input; cycles are per LAYER,
//                the 75 FMAs included (a third of them per layer)
//   <8, 1>      the LEAN K = 8 that ships in the four-layer kernels: rotations 8 and 9 by two ds_read_b32 into v9 and v11
//   <12, 3> / <12, 2>   K = 12 from three / two register pairs, each pair fetched again behind the FMAs that consumed it (the
//                register footprint of K = 6 / 4): the second round trip is NOT hidden
// 256-thread blocks, 256 x wps of them: every CU carries wps waves on each of its four SIMDs, so the LDS pipe sees all of them.
// Build: hipcc -O3 --offload-arch=gfx950 fwd_lds_rot_ubench.hip -o fwd_lds_rot_ubench ; prints shader cycles per layer per SIMD at
// 1 / 2 waves per SIMD, three repeats of every row (their spread is the noise to beat).
#include <hip/hip_runtime.h>
#include <cstdio>

typedef float f2_t __attribute__((ext_vector_type(2)));

#define MOV(n) "v_mov_b32_dpp v8, v10 row_ror:" #n " row_mask:0xf bank_mask:0xf\n\t"
#define FMA(n)                                                                                                                 \
    "v_pk_fma_f32 v[4:5], %[wa" #n "], v[8:9], v[4:5] op_sel_hi:[1,0,1]\n\t"                                                    \
    "v_pk_fma_f32 v[6:7], %[wb" #n "], v[8:9], v[6:7] op_sel_hi:[1,0,1]\n\t"
#define STEP(n) MOV(n) FMA(n)
// rotation n from the LOW half of the fetched pair q, rotation n + 1 from its HIGH half
#define LDS2(n, m, q)                                                                                                          \
    "v_pk_fma_f32 v[4:5], %[wa" #n "], %[" #q "], v[4:5] op_sel_hi:[1,0,1]\n\t"                                                 \
    "v_pk_fma_f32 v[6:7], %[wb" #n "], %[" #q "], v[6:7] op_sel_hi:[1,0,1]\n\t"                                                 \
    "v_pk_fma_f32 v[4:5], %[wa" #m "], %[" #q "], v[4:5] op_sel:[0,1,0] op_sel_hi:[1,1,1]\n\t"                                  \
    "v_pk_fma_f32 v[6:7], %[wb" #m "], %[" #q "], v[6:7] op_sel:[0,1,0] op_sel_hi:[1,1,1]\n\t"
// one rotation from the HIGH half of the named pair p
#define HI(n, p)                                                                                                               \
    "v_pk_fma_f32 v[4:5], %[wa" #n "], " p ", v[4:5] op_sel:[0,1,0] op_sel_hi:[1,1,1]\n\t"                                      \
    "v_pk_fma_f32 v[6:7], %[wb" #n "], " p ", v[6:7] op_sel:[0,1,0] op_sel_hi:[1,1,1]\n\t"
#define WR "ds_write2_b32 %[ad], v10, v10 offset1:16\n\t"
#define RD(q, o0, o1) "ds_read2_b32 %[" #q "], %[ad] offset0:" #o0 " offset1:" #o1 "\n\t"
#define WAIT "s_waitcnt lgkmcnt(0)\n\t"
#define HEAD                                                                                                                   \
    "s_nop 1\n\t"                                                                                                              \
    "v_pk_mul_f32 v[4:5], %[wa0], v[10:11] op_sel_hi:[1,0]\n\t"                                                                \
    "v_pk_mul_f32 v[6:7], %[wb0], v[10:11] op_sel_hi:[1,0]\n\t"
#define FINISH                                                                                                                 \
    "s_nop 1\n\t"                                                                                                              \
    "v_permlane16_swap_b32 v5, v7\n\t"                                                                                         \
    "v_permlane16_swap_b32 v4, v6\n\t"                                                                                         \
    "v_pk_add_f32 v[4:5], v[4:5], v[6:7]\n\t"                                                                                  \
    "s_nop 1\n\t"                                                                                                              \
    "v_permlane32_swap_b32 v4, v5\n\t"                                                                                         \
    "v_add_f32 v4, v4, v5\n\t"                                                                                                 \
    "v_add_f32 v4, v4, %[bias]\n\t"                                                                                            \
    "v_max_f32 v4, 0, v4"
#define W(n) [wa##n] "v"(wp[2 * n]), [wb##n] "v"(wp[2 * n + 1])
#define W_LO W(0), W(1), W(2), W(3), W(4), W(5), W(6), W(7)
#define W_HI W(8), W(9), W(10), W(11), W(12), W(13), W(14), W(15)
#define OUT1 "=&{v[4:5]}"(a02), "=&{v[6:7]}"(a13), "=&{v8}"(lo)
#define IO2 "+{v[4:5]}"(a02), "+{v[6:7]}"(a13), "+{v8}"(lo)
#define IN1 "{v[10:11]}"(hh), [ad] "v"(ad), W_LO
#define IN2 "{v[10:11]}"(hh), [bias] "v"(bias), W_HI

// ad: byte address of the lane's entry i of its row r in the wave's buffer, (192 wave + 48 r + i) * 4
template <int K, int P = 0> __device__ __forceinline__ float layer(const f2_t (&wp)[32], float bias, float h, unsigned ad)
{
    f2_t a02, a13, hh, q0, q1, q2, q3, q4, q5;
    float lo;
    hh.x = h;
    if constexpr (K == 0) {
        asm volatile(HEAD STEP(1) STEP(2) STEP(3) STEP(4) STEP(5) STEP(6) STEP(7) MOV(8) : OUT1 : IN1);
        asm volatile(FMA(8) STEP(9) STEP(10) STEP(11) STEP(12) STEP(13) STEP(14) STEP(15) FINISH : IO2 : IN2);
    } else if constexpr (K == 4) {
        asm volatile(WR RD(q0, 4, 3) RD(q1, 2, 1) HEAD STEP(1) STEP(2) STEP(3) STEP(4) STEP(5) STEP(6) STEP(7) STEP(8) STEP(9) STEP(10) MOV(11) WAIT
                     : OUT1, [q0] "=&v"(q0), [q1] "=&v"(q1) : IN1, W(8), W(9), W(10));
        asm volatile(FMA(11) LDS2(12, 13, q0) LDS2(14, 15, q1) FINISH
                     : IO2 : "{v[10:11]}"(hh), [bias] "v"(bias), W(11), W(12), W(13), W(14), W(15), [q0] "v"(q0), [q1] "v"(q1));
    } else if constexpr (K == 8 && P == 1) {
        // the lean form: the first two LDS rotations land in v9 and v11, the unselected high halves of the moved-operand and input pairs
        f2_t lo2;
        asm volatile(WR "ds_read_b32 v9, %[ad] offset:32\n\tds_read_b32 v11, %[ad] offset:28\n\t" RD(q0, 6, 5) RD(q1, 4, 3) RD(q2, 2, 1)
                     HEAD STEP(1) STEP(2) STEP(3) STEP(4) STEP(5) STEP(6) STEP(7) WAIT
                     : "=&{v[4:5]}"(a02), "=&{v[6:7]}"(a13), "=&{v[8:9]}"(lo2), "+{v[10:11]}"(hh), [q0] "=&v"(q0), [q1] "=&v"(q1), [q2] "=&v"(q2)
                     : [ad] "v"(ad), W_LO);
        asm volatile(HI(8, "v[8:9]") HI(9, "v[10:11]") LDS2(10, 11, q0) LDS2(12, 13, q1) LDS2(14, 15, q2) FINISH
                     : "+{v[4:5]}"(a02), "+{v[6:7]}"(a13)
                     : "{v[8:9]}"(lo2), "{v[10:11]}"(hh), [bias] "v"(bias), W_HI, [q0] "v"(q0), [q1] "v"(q1), [q2] "v"(q2));
    } else if constexpr (K == 8) {
        asm volatile(WR RD(q0, 8, 7) RD(q1, 6, 5) RD(q2, 4, 3) RD(q3, 2, 1) HEAD STEP(1) STEP(2) STEP(3) STEP(4) STEP(5) STEP(6) STEP(7) WAIT
                     : OUT1, [q0] "=&v"(q0), [q1] "=&v"(q1), [q2] "=&v"(q2), [q3] "=&v"(q3) : IN1);
        asm volatile(LDS2(8, 9, q0) LDS2(10, 11, q1) LDS2(12, 13, q2) LDS2(14, 15, q3) FINISH
                     : IO2 : IN2, [q0] "v"(q0), [q1] "v"(q1), [q2] "v"(q2), [q3] "v"(q3));
    } else if constexpr (K == 12 && P == 3) {
        // three pairs, each fetched twice: a pair's second fetch is issued behind the FMAs that consumed its first
        asm volatile(WR RD(q0, 12, 11) RD(q1, 10, 9) RD(q2, 8, 7) HEAD STEP(1) STEP(2) STEP(3) WAIT
                     LDS2(4, 5, q0) RD(q0, 6, 5) LDS2(6, 7, q1) RD(q1, 4, 3) LDS2(8, 9, q2) RD(q2, 2, 1) WAIT
                     : OUT1, [q0] "=&v"(q0), [q1] "=&v"(q1), [q2] "=&v"(q2) : IN1, W(8), W(9));
        asm volatile(LDS2(10, 11, q0) LDS2(12, 13, q1) LDS2(14, 15, q2) FINISH
                     : IO2 : "{v[10:11]}"(hh), [bias] "v"(bias), W(10), W(11), W(12), W(13), W(14), W(15), [q0] "v"(q0), [q1] "v"(q1), [q2] "v"(q2));
    } else if constexpr (K == 12 && P == 2) {
        // two pairs, each fetched three times (the register footprint of K = 4)
        asm volatile(WR RD(q0, 12, 11) RD(q1, 10, 9) HEAD STEP(1) STEP(2) STEP(3) WAIT
                     LDS2(4, 5, q0) RD(q0, 8, 7) LDS2(6, 7, q1) RD(q1, 6, 5) "s_waitcnt lgkmcnt(1)\n\t" LDS2(8, 9, q0) RD(q0, 4, 3) WAIT
                     : OUT1, [q0] "=&v"(q0), [q1] "=&v"(q1) : IN1, W(8), W(9));
        asm volatile(LDS2(10, 11, q1) RD(q1, 2, 1) LDS2(12, 13, q0) WAIT LDS2(14, 15, q1) FINISH
                     : IO2, [q1] "+v"(q1) : "{v[10:11]}"(hh), [bias] "v"(bias), [ad] "v"(ad), W(10), W(11), W(12), W(13), W(14), W(15), [q0] "v"(q0));
    } else {
        static_assert(K == 12 && P == 0, "K is 0, 4, 8 or 12");
        asm volatile(WR RD(q0, 12, 11) RD(q1, 10, 9) RD(q2, 8, 7) RD(q3, 6, 5) RD(q4, 4, 3) RD(q5, 2, 1) HEAD STEP(1) STEP(2) STEP(3)
                     WAIT LDS2(4, 5, q0) LDS2(6, 7, q1)
                     : OUT1, [q0] "=&v"(q0), [q1] "=&v"(q1), [q2] "=&v"(q2), [q3] "=&v"(q3), [q4] "=&v"(q4), [q5] "=&v"(q5) : IN1);
        asm volatile(LDS2(8, 9, q2) LDS2(10, 11, q3) LDS2(12, 13, q4) LDS2(14, 15, q5) FINISH
                     : IO2 : IN2, [q2] "v"(q2), [q3] "v"(q3), [q4] "v"(q4), [q5] "v"(q5));
    }
    return a02.x;
}

#define SETUP                                                                                                                  \
    __shared__ float rot[4 * 192];                                                                                             \
    f2_t wp[32];                                                                                                               \
    for (int i = 0; i < 32; ++i) wp[i] = f2_t{1e-2f + i * 5e-4f - threadIdx.x * 1e-5f, 1e-2f - i * 5e-4f};                     \
    for (int i = 0; i < 32; ++i) asm volatile("" : "+v"(wp[i]));                                                               \
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;                                                                \
    const unsigned ad = (unsigned)(size_t)(__attribute__((address_space(3))) float *)rot                                       \
                        + 4u * (192 * wave + 48 * (lane >> 4) + (lane & 15));                                                  \
    float h = 1.0001f + threadIdx.x * 1e-3f;

template <int K, int P = 0> __global__ __launch_bounds__(256) void k_tput(float *out, unsigned long long *st, int iters)
{
    SETUP
    float s = 0.f;
    unsigned long long t0 = __builtin_amdgcn_s_memtime();
    for (int it = 0; it < iters; ++it) s = layer<K, P>(wp, 0.5f, h, ad);
    unsigned long long t1 = __builtin_amdgcn_s_memtime();
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
    if (threadIdx.x == 0) st[blockIdx.x] = t1 - t0;
}

template <int K, int P = 0> __global__ __launch_bounds__(256) void k_chain(float *out, unsigned long long *st, int iters)
{
    SETUP
    float c0 = 0.3f, c1 = 0.7f;
    asm volatile("" : "+v"(c0), "+v"(c1));
    unsigned long long t0 = __builtin_amdgcn_s_memtime();
    for (int it = 0; it < iters; it += 3) {
        h = layer<K, P>(wp, 0.5f, h, ad);
        h = layer<K, P>(wp, 0.25f, h, ad);
        h = layer<K, P>(wp, 0.125f, h, ad);
        float m[5] = {h, h, h, h, h};
#pragma unroll
        for (int u = 0; u < 15; ++u)
#pragma unroll
            for (int j = 0; j < 5; ++j) asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(m[j]) : "v"(c0), "v"(c1));
        h = ((m[0] + m[1]) + (m[2] + m[3])) + m[4];
    }
    unsigned long long t1 = __builtin_amdgcn_s_memtime();
    out[blockIdx.x * blockDim.x + threadIdx.x] = h;
    if (threadIdx.x == 0) st[blockIdx.x] = t1 - t0;
}

template <typename Kern> void run(const char *name, int rep, Kern kern, float *out, unsigned long long *st)
{
    const int iters = 3000;
    printf("%-14s #%d", name, rep);
    for (int wps : {1, 2}) {
        const int blocks = 256 * wps;                   // one 4-wave block per CU per requested wave-per-SIMD
        kern<<<blocks, 256>>>(out, st, 30); (void)hipDeviceSynchronize();
        kern<<<blocks, 256>>>(out, st, iters); (void)hipDeviceSynchronize();
        static unsigned long long h[512];
        (void)hipMemcpy(h, st, sizeof(unsigned long long) * blocks, hipMemcpyDeviceToHost);
        double avg = 0; for (int i = 0; i < blocks; ++i) avg += (double)h[i]; avg /= blocks;
        printf("  %dw/SIMD: %7.1f cyc/layer/wave = %6.1f cyc/layer/SIMD", wps, avg / iters, avg / iters / wps);
    }
    float v[2]; (void)hipMemcpy(v, out + 77, 8, hipMemcpyDeviceToHost);
    printf("   [out %.9g %.9g]\n", v[0], v[1]);
}
#define RUN(...) run(#__VA_ARGS__, rep, __VA_ARGS__, out, st)
int main()
{
    float *out; unsigned long long *st;
    (void)hipMalloc(&out, 4 * 256 * 512); (void)hipMalloc(&st, 8 * 512);
    for (int rep = 1; rep <= 3; ++rep) {
        RUN(k_tput<0>); RUN(k_tput<4>); RUN(k_tput<8>); RUN(k_tput<8,1>); RUN(k_tput<12>); RUN(k_tput<12,3>); RUN(k_tput<12,2>);
        RUN(k_chain<0>); RUN(k_chain<4>); RUN(k_chain<8>); RUN(k_chain<8,1>); RUN(k_chain<12>); RUN(k_chain<12,3>); RUN(k_chain<12,2>);
    }
    if (hipDeviceSynchronize() != hipSuccess) { printf("FAILED: %s\n", hipGetErrorString(hipGetLastError())); return 1; }
    return 0;
}

// hode_philox.h -- Philox4x32-10 (Salmon et al., SC'11) for the samplers (hode_hmc.hip, hode_nuts.hip), host- and device-callable.
//
// Stream layout (include/hode.h, "MCMC"): key = (seed bits 0..31, chain), counter = (coordinate group, stream tag,
// iteration, seed bits 32..63).  One call gives four 32-bit words: four coordinates' normals (two Box-Muller pairs), or one
// uniform.  A chain's draws therefore depend on (seed, chain, iteration, coordinate) only: not on the number of chains, the
// launch geometry or which thread computes them.  The same words as rocRAND's philox4x32_10_engine(seed | chain << 32,
// subsequence = iteration | seed_hi << 32, offset = 4 * (group | tag << 32)).next4() (tests/test_hmc_host.py checks this).
#pragma once
#include <stdint.h>
#include <math.h>

#if defined(__HIPCC__)
#define HODE_HD __host__ __device__ inline
#else
#define HODE_HD inline
#endif

namespace hode {

// stream tags (counter word 1); the last three are the No-U-Turn sampler's (hode_nuts.hip): the direction of doubling j
// (group j), the multinomial choice of leaf n (group n, counted over the tree from 1), the merge of subtree j (group j)
constexpr uint32_t kRngMomentum = 0, kRngAccept = 1, kRngJitter = 2, kRngInit = 3;
constexpr uint32_t kRngNutsDir = 4, kRngNutsLeaf = 5, kRngNutsMerge = 6;
// the bootstrap of the Sobol indices (hode_sobol.hip): resample r as the iteration, base sample q / 4 as the group, chain 0
constexpr uint32_t kRngSobol = 7;
// the particle filter (hode_filter.hip): the patient's key id0 + b as the chain, the filter step as the iteration.  Noise:
// group 2 i + (j >> 2) gives particle i the normals of its states 4 (j >> 2) .. 4 (j >> 2) + 3; resampling: group 0, one
// uniform per patient and step
constexpr uint32_t kRngFilterNoise = 8, kRngFilterResample = 9;
// backward simulation over a stored filter (hode_smooth.hip): the step whose slot is drawn as the iteration, the trajectory m
// as the group, one uniform per draw
constexpr uint32_t kRngFilterSmooth = 10;
// the parameter move of the particle filter (hode_pf_params.hip): the patient's key as the chain, the filter step as the
// iteration; group 5 i + (k >> 2) gives particle i the normals of its payload columns 4 (k >> 2) .. 4 (k >> 2) + 3
constexpr uint32_t kRngFilterParam = 11;

struct Philox4 { uint32_t x, y, z, w; };

HODE_HD Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1)
{
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c0 = n0; c1 = (uint32_t)p1; c2 = n2; c3 = (uint32_t)p0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return Philox4{c0, c1, c2, c3};
}

HODE_HD Philox4 hmc_rng(uint64_t seed, uint32_t chain, uint32_t iter, uint32_t tag, uint32_t group)
{
    return philox4x32_10(group, tag, iter, (uint32_t)(seed >> 32), (uint32_t)seed, chain);
}

// (0, 1): never 0 or 1, so log() and the Box-Muller radius stay finite
HODE_HD double u01(uint32_t x) { return ((double)x + 0.5) * 2.3283064365386963e-10; }

// four standard normals from one Philox block (Box-Muller on (x, y) and (z, w)), in fp64
HODE_HD void normals4(const Philox4 &r, double out[4])
{
    const double r0 = sqrt(-2.0 * log(u01(r.x))), r1 = sqrt(-2.0 * log(u01(r.z)));
    const double a0 = 6.283185307179586 * u01(r.y), a1 = 6.283185307179586 * u01(r.w);
    out[0] = r0 * cos(a0); out[1] = r0 * sin(a0);
    out[2] = r1 * cos(a1); out[3] = r1 * sin(a1);
}

}  // namespace hode

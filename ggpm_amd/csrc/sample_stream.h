// The seeded counter stream ("Sampled decoding and the prior"; include/ggpm_hip.h) for the kernels that draw from it
// (csrc/sample.hip, csrc/latent_prior.hip): every random word is a function of (seed_lo, seed_hi, site, sample id, step, slot)
// alone.
#pragma once
#include "common.h"

__device__ __forceinline__ unsigned int fmix32(unsigned int h) {
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return h;
}

// the 24-bit uniform m of (seed, site, id, step, slot)
__device__ __forceinline__ unsigned int sample_m(unsigned int seed_lo, unsigned int seed_hi, unsigned int site,
                                                 unsigned int id, unsigned int step, unsigned int slot) {
    const unsigned int base = fmix32(fmix32(id * 0x9E3779B1u + seed_lo) ^ (seed_hi + site * 0x7F4A7C15u));
    return fmix32(base + (step * 64u + slot) * 0x9E3779B1u) >> 8;
}

constexpr float TWO_M24 = 5.9604644775390625e-08f;       // 2^-24

// Box-Muller from two words per element: sqrt(-2 log u1) cos(2 pi u2), u1 = (m0 + 1) 2^-24 in (0, 1], u2 = m1 2^-24
__device__ __forceinline__ float sample_gauss(unsigned int seed_lo, unsigned int seed_hi, unsigned int site,
                                              unsigned int id, unsigned int counter) {
    const unsigned int m0 = sample_m(seed_lo, seed_hi, site, id, counter, 0u);
    const unsigned int m1 = sample_m(seed_lo, seed_hi, site, id, counter, 1u);
    const float u1 = (float)(m0 + 1u) * TWO_M24, u2 = (float)m1 * TWO_M24;
    return sqrtf(-2.f * logf(u1)) * cospif(2.f * u2);
}

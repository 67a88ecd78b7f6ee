// The random draws of the kernels that sample (synthetic.hip, scan.hip): one definition of the stream and of its conventions.
// Philox4x32-10 (multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85, ten rounds);
// U(w) = (w >> 8) * 2^-24;  Box-Muller(wa, wb): m = sqrtf(-2 * logf(((wa >> 8) + 1) * 2^-24)), phi = 2 pi * (((wb >> 8) + 1) * 2^-24),
// pair = (m * cosf(phi), m * sinf(phi)).  Moved here from synthetic.hip unchanged.
#pragma once

#include "st_common.h"

struct SyWords { uint32_t w0, w1, w2, w3; };

__host__ __device__ __forceinline__ SyWords sy_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int round = 0; round < 10; round++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return SyWords{c0, c1, c2, c3};
}

#define SY_2POW_M24 5.9604644775390625e-8f
#define SY_TWO_PI 6.28318530717958647692f

__device__ __forceinline__ float sy_uniform(uint32_t w) { return (float)(w >> 8) * SY_2POW_M24; }
__device__ __forceinline__ void sy_normal_pair(uint32_t wa, uint32_t wb, float& n0, float& n1) {
    const float u1 = (float)((wa >> 8) + 1u) * SY_2POW_M24;  // (0, 1]: the logarithm never sees 0
    const float u2 = (float)((wb >> 8) + 1u) * SY_2POW_M24;
    const float m = sqrtf(-2.0f * logf(u1));
    const float phi = SY_TWO_PI * u2;
    n0 = m * cosf(phi);
    n1 = m * sinf(phi);
}

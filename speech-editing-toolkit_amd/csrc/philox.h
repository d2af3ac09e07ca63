// Philox4x32-10 (counter based) and what is drawn from it: Box-Muller normals (set_randn, set_posterior_step, the step-boundary kernels of
// csrc/boundary.hip) and the dropout keep decisions of csrc/train.hip.  One counter value gives four 32-bit words = four elements.
#pragma once
#include "common.h"

namespace {

__device__ __forceinline__ void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0;
        const uint32_t n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
        const uint32_t n3 = (uint32_t)p0;
        c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}
__device__ __forceinline__ void randn4(uint64_t seed, uint64_t ctr, float out[4]) {
    uint32_t c[4] = {(uint32_t)ctr, (uint32_t)(ctr >> 32), 0u, 0u};
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    // (0,1] uniforms, Box-Muller
    const float u0 = ((float)(c[0] >> 8) + 1.0f) * (1.0f / 16777216.0f);
    const float u1 = ((float)(c[1] >> 8) + 1.0f) * (1.0f / 16777216.0f);
    const float u2 = ((float)(c[2] >> 8) + 1.0f) * (1.0f / 16777216.0f);
    const float u3 = ((float)(c[3] >> 8) + 1.0f) * (1.0f / 16777216.0f);
    const float r0 = sqrtf(-2.0f * logf(u0)), r1 = sqrtf(-2.0f * logf(u2));
    float s0, c0, s1, c1;
    sincosf(6.28318530717958647692f * u1, &s0, &c0);
    sincosf(6.28318530717958647692f * u3, &s1, &c1);
    out[0] = r0 * c0; out[1] = r0 * s0; out[2] = r1 * c1; out[3] = r1 * s1;
}
// Dropout with rate p: keep[k] is the decision for element 4 q + k.  Quad q draws once, at counter offset + q (third counter word 0x5eed:
// a stream of its own next to randn4's); word k gives the uniform u = (its top 24 bits) / 2^24 in [0, 1), and the element is kept when u >= p.
__device__ __forceinline__ void dropout_keep4(uint64_t seed, uint64_t offset, int64_t q, float p, bool keep[4]) {
    const uint64_t ctr = offset + (uint64_t)q;
    uint32_t c[4] = {(uint32_t)ctr, (uint32_t)(ctr >> 32), 0x5eedu, 0u};
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
#pragma unroll
    for (int k = 0; k < 4; ++k) keep[k] = (float)(c[k] >> 8) * (1.0f / 16777216.0f) >= p;
}

}  // namespace

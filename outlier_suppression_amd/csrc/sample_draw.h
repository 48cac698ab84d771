// What sample_advance.hip and sample_nucleus.hip share of the draw: its arguments beside the step's (advance_step.h, which
// holds the step and the two tails every form ends with), the Philox draw, z and its weight.
#pragma once
#include <math.h>
#include <hip/hip_runtime.h>
#include "osq_device.h"
#include "token_argmax.h"
#include "advance_step.h"

namespace osq {

constexpr int kSaMaxTopK = 64;

struct SampleArgs {
    StepArgs s;
    const float* uniforms;     // nullptr: Philox; else [bsz] values in [0, 1) in the place of the draws
    BeamCand* cands;           // [bsz, chunks, top_k]  workspace, top_k >= 1
    float2* partials;          // [bsz, chunks] (m_c, s_c)  the same workspace, top_k == 0
    unsigned long long seed;
    float temperature, top_p;
    int top_k;
};

// Word 0 of Philox4x32-10 (Salmon et al., SC'11) for the counter (c0, c1, 0, 0) and the key (k0, k1).
__device__ __forceinline__ unsigned int philox_word0(unsigned int c0, unsigned int c1, unsigned int k0, unsigned int k1) {
    unsigned int c2 = 0u, c3 = 0u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
        const unsigned int n0 = static_cast<unsigned int>(p1 >> 32) ^ c1 ^ k0, n2 = static_cast<unsigned int>(p0 >> 32) ^ c3 ^ k1;
        c1 = static_cast<unsigned int>(p1);
        c3 = static_cast<unsigned int>(p0);
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c0;
}

// The draw of row b at history length cur: 24 bits, in [0, 1).
__device__ __forceinline__ float sample_uniform(unsigned long long seed, unsigned int b, unsigned int cur) {
    const unsigned int w = philox_word0(b, cur, static_cast<unsigned int>(seed), static_cast<unsigned int>(seed >> 32));
    return static_cast<float>(w >> 8) * 0x1p-24f;
}

// z of one element: x / temperature with -0.0 as +0.0; -inf for what is out of the draw (banned, NaN, -inf, past the row)
__device__ __forceinline__ float sample_z(float x, float temperature, bool out) {
    const float z = x / temperature;
    return (out || z != z) ? -INFINITY : z + 0.0f;
}

// what a survivor z weighs against the maximum m: 1 where equal (m = +inf included), else exp(z - m)
__device__ __forceinline__ float sample_weight(float z, float m) { return z == m ? 1.f : expf(z - m); }

}  // namespace osq

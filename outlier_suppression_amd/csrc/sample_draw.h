// What sample_advance.hip and sample_nucleus.hip share of the draw: its arguments beside the step's (advance_step.h, which
// holds the step and the two tails every form ends with), the rows of a group, the Philox draw, z, its weight and the
// log-probability of the drawn token.
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
    int group;                 // G >= 1: row r is sequence r % G of input r / G (bsz % G == 0)
    float* logprobs;           // nullptr, or bsz rows logprobs_stride floats apart: [r, cur] written, no other word
    int64_t logprobs_stride;
};

// Word 0 of Philox4x32-10 (Salmon et al., SC'11) for the counter (c0, c1, c2, 0) and the key (k0, k1).
__device__ __forceinline__ unsigned int philox_word0(unsigned int c0, unsigned int c1, unsigned int c2, unsigned int k0,
                                                     unsigned int k1) {
    unsigned int c3 = 0u;
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

// The draw of sequence j of input b at history length cur: 24 bits, in [0, 1).
__device__ __forceinline__ float sample_uniform(unsigned long long seed, unsigned int b, unsigned int cur, unsigned int j) {
    const unsigned int w = philox_word0(b, cur, j, static_cast<unsigned int>(seed), static_cast<unsigned int>(seed >> 32));
    return static_cast<float>(w >> 8) * 0x1p-24f;
}

// The draw of row r, a workgroup's: uniforms[r] where given, else that of sequence r % group of input r / group.  The group
// is launch-uniform and r the workgroup's, so the divide stays scalar (as step_of keeps cur).
__device__ __forceinline__ float sample_row_uniform(const SampleArgs& a, unsigned int r, int cur) {
    if (a.uniforms) return a.uniforms[r];
    const unsigned int g = static_cast<unsigned int>(a.group);
    const unsigned int b = __builtin_amdgcn_readfirstlane(r / g);
    return sample_uniform(a.seed, b, static_cast<unsigned int>(cur), r - b * g);
}

// z of one element: x / temperature with -0.0 as +0.0; -inf for what is out of the draw (banned, NaN, -inf, past the row)
__device__ __forceinline__ float sample_z(float x, float temperature, bool out) {
    const float z = x / temperature;
    return (out || z != z) ? -INFINITY : z + 0.0f;
}

// what a survivor z weighs against the maximum m: 1 where equal (m = +inf included), else exp(z - m)
__device__ __forceinline__ float sample_weight(float z, float m) { return z == m ? 1.f : expf(z - m); }

// The log of the probability with which a survivor z was drawn: its weight against m over the total of the kept weights.
__device__ __forceinline__ float sample_logprob(float z, float m, float total) { return (z == m ? 0.f : z - m) - logf(total); }

// The end of row r in one thread: finish_row, and the row's log-probability word where the call asks for one -- 0 on a
// forced step and for a row that was finished already (its token is the pad), else lp.
__device__ __forceinline__ void sample_finish_row(const SampleArgs& a, const Step& step, int64_t r, int64_t token, float lp) {
    const bool padded = finish_row(a.s, step, r, token);
    if (a.logprobs) a.logprobs[r * a.logprobs_stride + step.cur] = (step.forced >= 0 || padded) ? 0.f : lp;
}

// What the grouped entry points require beside their namesakes' requirements.
static inline int sample_group_check(const char* what, const StepCall& c, int64_t group, const float* logprobs,
                                     int64_t logprobs_stride) {
    if (group < 1 || c.bsz % group != 0) {
        set_error("%s: group must be at least 1 and divide bsz", what);
        return OSQ_ERR_INVALID_ARGUMENT;
    }
    if (logprobs && logprobs_stride < c.max_length) {
        set_error("%s: logprobs row stride below max_length", what);
        return OSQ_ERR_INVALID_ARGUMENT;
    }
    return OSQ_OK;
}

}  // namespace osq

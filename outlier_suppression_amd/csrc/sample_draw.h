// What sample_advance.hip and sample_nucleus.hip share: the arguments of a sampling step, the step a launch reads from the
// position word, the Philox draw, z and its weight, and the two tails every form ends with -- the row's pad / eos lines with
// its stores, and the stopping word.
#pragma once
#include <math.h>
#include <hip/hip_runtime.h>
#include "osq_device.h"
#include "token_argmax.h"

namespace osq {

constexpr int kSaMaxLength = kBsMaxCur, kSaMaxEos = 16, kSaMaxTopK = 64;
constexpr int kSaGoThreads = OSQ_WAVE;               // rows one trip of the go_on reduction covers

struct SampleArgs {
    const float* logits;       // bsz x vocab, rows logits_stride floats apart
    int64_t* seq;              // bsz x max_length, rows seq_stride apart: [0, cur) read with ngram > 0, [cur] written
    const int64_t* ban_ids;    // n_ban ids banned in every row
    const int64_t* eos_ids;    // n_eos ids that finish a row
    uint8_t* unfinished;       // [bsz]; touched only with n_eos > 0
    int64_t* next_tokens;      // [bsz]
    int32_t* go_on;            // 1
    const float* uniforms;     // nullptr: Philox; else [bsz] values in [0, 1) in the place of the draws
    BeamCand* cands;           // [bsz, chunks, top_k]  workspace, top_k >= 1
    float2* partials;          // [bsz, chunks] (m_c, s_c)  the same workspace, top_k == 0
    unsigned int* row_flags;   // [bsz]          workspace: the row is unfinished after this step
    int64_t logits_stride, seq_stride;
    int64_t pad;
    unsigned long long seed;
    float temperature, top_p;
    int top_k;
    int bsz, vocab, chunks, max_length, cur, ngram, n_ban, n_eos;
    int forced;                // static form: >= 0 is this step's token
    // osq_sample_advance_at: cur = *cur_dev + cur_add, read by the launches
    const int32_t* cur_dev;    // nullptr: the static form, cur / n_ban / forced above
    int cur_add, ban_below, forced_bos, forced_eos;
};

struct SampleStep {            // what a launch knows of its step: workgroup-uniform
    int cur;                   // -1: refused
    int n_ban, forced;
};

__device__ __forceinline__ SampleStep sample_step(const SampleArgs& a) {
    if (!a.cur_dev) return SampleStep{a.cur, a.n_ban, a.forced};
    const long long at = static_cast<long long>(__builtin_amdgcn_readfirstlane(*a.cur_dev)) + a.cur_add;
    if (at < 1 || at >= a.max_length) return SampleStep{-1, 0, -1};
    const int cur = static_cast<int>(at);
    int forced = cur == 1 ? a.forced_bos : -1;
    if (cur == a.max_length - 1 && a.forced_eos >= 0) forced = a.forced_eos;
    return SampleStep{cur, cur < a.ban_below ? a.n_ban : 0, forced};
}

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

// The end of row b in one thread: the pad of a finished row, the eos test, seq[b, cur], next_tokens[b] and the row's flag.
__device__ __forceinline__ void sample_finish_row(const SampleArgs& a, const SampleStep& step, int64_t b, int64_t token) {
    unsigned int unfinished = 1u;
    if (a.n_eos > 0) {
        unfinished = a.unfinished[b] != 0;
        if (!unfinished) token = a.pad;
        for (int e = 0; e < a.n_eos; ++e) unfinished &= token != a.eos_ids[e];
        a.unfinished[b] = static_cast<uint8_t>(unfinished);
    }
    if (a.seq) a.seq[b * a.seq_stride + step.cur] = token;
    a.next_tokens[b] = token;
    a.row_flags[b] = unfinished;
}

// The stopping word, by one wave of kSaGoThreads: go_on = (cur + 1 < max_length) && (n_eos == 0 || any row unfinished); -1
// for a refused position.
__device__ __forceinline__ void sample_go_on(const SampleArgs& a) {
    const SampleStep step = sample_step(a);
    if (step.cur < 0) {                                             // refused: the row flags are not this step's
        if (threadIdx.x == 0) *a.go_on = -1;
        return;
    }
    unsigned int any = a.n_eos == 0;
    if (a.n_eos > 0)
        for (int b = threadIdx.x; b < a.bsz; b += kSaGoThreads) any |= a.row_flags[b];
    const bool some = __any(any != 0u);
    if (threadIdx.x == 0) *a.go_on = step.cur + 1 < a.max_length && some;
}

}  // namespace osq

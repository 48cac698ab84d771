// What beam_select.hip, greedy_advance.hip and the sampling files share: a row of logits cut into chunks of kBsChunk tokens, one
// 256-thread workgroup per (row, chunk) holding 16 values per thread; the 64-bit candidate key; the workgroup arg-max over such
// keys; the chunk's bitmap of banned tokens (the min-length ids and the no-repeat-ngram rule); and the load of a chunk's values
// over the search for its bans (chunk_each).
//
// Order of a key: larger value first, NaN above every number; the low word carries ~position, so that among equal values the
// smaller position wins and the arg-max is a max of (hi, lo) pairs.  Key 0 is no value's (-inf has 0x007fffff): it marks a
// taken or absent candidate.  ordered_bits separates -0.0 from +0.0: a caller whose values can be -0.0 canonicalises first.
#pragma once
#include <hip/hip_runtime.h>
#include "osq_device.h"

namespace osq {

constexpr int kBsThreads = 256;
constexpr int kBsWaves = kBsThreads / OSQ_WAVE;
constexpr int kBsPer = 16;                          // elements of a chunk one thread holds
constexpr int kBsChunk = kBsThreads * kBsPer;       // 4096 tokens
constexpr int kBsMaxCur = 4096, kBsMaxBan = 16;

struct BeamCand {              // one candidate in the workspace
    unsigned int key;          // beam_key(value); 0: none
    int token;
};

__device__ __forceinline__ unsigned int beam_key(float v) { return v != v ? 0xffffffffu : ordered_bits(v); }
__device__ __forceinline__ float beam_value(unsigned int key) {
    return key == 0xffffffffu ? __builtin_nanf("") : from_ordered_bits(key);
}

// The largest (hi, lo) pair of the workgroup, lexicographically, in every thread.  s_red: [2][2 * kBsWaves] words, the two
// halves used by alternate calls (`parity`), so one barrier per call is enough.
__device__ __forceinline__ void block_argmax(unsigned int& hi, unsigned int& lo, unsigned int (*s_red)[2 * kBsWaves], int parity) {
    const int lane = threadIdx.x & (OSQ_WAVE - 1), w = threadIdx.x / OSQ_WAVE;
    const unsigned int wh = wave_max_u32(hi);
    const unsigned int wl = wave_max_u32(hi == wh ? lo : 0u);
    if (lane == 0) { s_red[parity][w] = wh; s_red[parity][kBsWaves + w] = wl; }
    __syncthreads();
    hi = s_red[parity][0];
    lo = s_red[parity][kBsWaves];
#pragma unroll
    for (int k = 1; k < kBsWaves; ++k) {
        const unsigned int h = s_red[parity][k], l = s_red[parity][kBsWaves + k];
        if (h > hi || (h == hi && l > lo)) { hi = h; lo = l; }
    }
}

// The banned tokens of the span [c0, c0 + len) of one row into s_ban (kWords words, one bit per token, len <= 32 kWords), by a
// workgroup of kThreads: the n_ban ids of ban_ids, and, with n = ngram > 0 and cur >= n, the last token of every window of
// s[0 : cur] that starts with the suffix s[cur - n + 1 : cur].  s is read only then.  The caller's next barrier publishes the
// bitmap.
template <int kThreads, int kWords>
__device__ __forceinline__ void span_bans(unsigned int* s_ban, const int64_t* ban_ids, int n_ban, const int64_t* s, int cur,
                                          int n, int c0, int len) {
    for (int i = threadIdx.x; i < kWords; i += kThreads) s_ban[i] = 0u;
    __syncthreads();
    if (threadIdx.x < n_ban) {
        const int64_t t = ban_ids[threadIdx.x] - c0;
        if (t >= 0 && t < len) atomicOr(&s_ban[t >> 5], 1u << (t & 31));
    }
    if (n > 0 && cur >= n) {                                      // window i bans its last token when it starts with the suffix
        const int64_t* suffix = s + (cur - n + 1);
        for (int i = threadIdx.x; i <= cur - n; i += kThreads) {
            bool same = true;
            for (int k = 0; k < n - 1 && same; ++k) same = s[i + k] == suffix[k];
            const int64_t t = s[i + n - 1] - c0;
            if (same && t >= 0 && t < len) atomicOr(&s_ban[t >> 5], 1u << (t & 31));
        }
    }
}

// The chunk [c0, c0 + len) of a kBsThreads workgroup: kBsChunk / 32 words.
__device__ __forceinline__ void chunk_bans(unsigned int* s_ban, const int64_t* ban_ids, int n_ban, const int64_t* s, int cur,
                                           int n, int c0, int len) {
    span_bans<kBsThreads, kBsChunk / 32>(s_ban, ban_ids, n_ban, s, cur, n, c0, len);
}

// The chunk [c0, c0 + len) of a row, x at its first token, through a kBsThreads workgroup: kBsPer values per thread, one 32-bit
// word per lane (a row of an odd vocab is only 4-byte aligned), issued before the bans are found -- the loads fly meanwhile
// -- then chunk_bans, a barrier, and keep(j, i, value, banned, in range) for the thread's elements i = threadIdx.x + j *
// kBsThreads in order; past the chunk the value is 0.f.
template <typename Keep>
__device__ __forceinline__ void chunk_each(const float* x, unsigned int* s_ban, const int64_t* ban_ids, int n_ban,
                                           const int64_t* s, int cur, int n, int c0, int len, Keep keep) {
    float v[kBsPer];
#pragma unroll
    for (int j = 0; j < kBsPer; ++j) {
        const int i = threadIdx.x + j * kBsThreads;
        v[j] = i < len ? x[i] : 0.f;
    }
    chunk_bans(s_ban, ban_ids, n_ban, s, cur, n, c0, len);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kBsPer; ++j) {
        const int i = threadIdx.x + j * kBsThreads;
        keep(j, i, v[j], ((s_ban[i >> 5] >> (i & 31)) & 1u) != 0u, i < len);
    }
}

}  // namespace osq

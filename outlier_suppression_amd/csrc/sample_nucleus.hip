// ONE sampling step after the model for top_k == 0, top_p <= 1 -- a nucleus over the whole vocabulary -- without a sort: the
// banned tokens, temperature, the top-p cut, a seeded draw from what is kept, the pad / eos arithmetic, the new token into the
// sequence and the stopping word, in two launches that read the logits once.
//
//   launch 1   sample_nucleus_row_kernel     one workgroup of kSnThreads = 1024 per row.  Thread t owns the kSnPer = 50 tokens
//                                            50 t .. 50 t + 49 (thread-blocked: token order is thread order, then register
//                                            order) and holds, for each, the ordered key of z (beam_key; 0: out of the draw) and
//                                            its weight w in registers.  Two bisections over the 32-bit keys, each round one
//                                            compare / select / add per element and one workgroup sum, find the cut and the
//                                            draw; a prefix count numbers the tokens of a tie group.  Then the forced token in
//                                            its place, pad / eos, seq[b, cur], next_tokens[b] and the row's unfinished flag
//                                            into the workspace.  A forced step reads no logit
//   launch 2   sample_nucleus_go_on_kernel   one wave: the stopping word of every advance call (advance_step.h, as the
//                                            step's arguments, the row's tail and the entry points' shared requirements)
//
// No workgroup waits for another; no atomics on device memory (the ban bitmap is built with LDS atomics, as chunk_bans does).
//
// The rule is include/osq_hip.h's ("a nucleus over the whole vocabulary").  With m the largest z left and w_i = 1 where
// z_i == m, else expf(z_i - m), let S(k) be the fp32 sum of w_i over the tokens whose key is above k, every other token adding
// 0.0f in its place, in ONE order:
//     thread t adds its tokens 0 .. 24 in order onto 0.0f, its tokens 25 .. 49 likewise, and the two halves; wave_sum_f32
//     (osq_device.h: four symmetric DPP steps, then (r0 + r16) + (r32 + r48)) over the 64 threads of a wave; the 16 wave sums
//     in wave order, left to right, by every thread.
// The order depends on vocab alone (tokens past the row add 0.0f): not on bsz, the row's stride or its alignment.  Every add
// rounds monotonically and every input is non-increasing in k, so S is non-increasing in k, and a bisection over k finds
//     the cut    k* = the smallest key with S(k*) < bound, bound = top_p * S(0): a key that is present (S steps only there); of
//                its n tokens, in token order, the j-th stays iff S(k*) + float(j) * w(k*) < bound -- true at 0 and monotone
//                in j, so the first r >= 1 stay, r found by bisection over j; W = S(k*) + float(r) * w(k*)
//     the draw   kv = the smallest key >= k* with S(kv) <= target, target = u * W: present too; the token is the first j of
//                its group (of the r kept ones when kv == k*) with S(kv) + float(j + 1) * w(kv) > target -- monotone in j, a
//                bisection again -- and the group's last eligible token when rounding leaves none (for kv == k* that is the
//                last kept rank).  The j-th token of a group is named by its owner from a prefix count of the group.
// Both bisections over keys end at key(m), where S = 0 is known, start at 0 and at k* - 1, and take at most 32 rounds each.
//
// Loads: one 32-bit word per lane, a wave reading the 3200 consecutive words its threads own, 64 at a time (a row of an odd
// vocab is only 4-byte aligned); the words reach their owners through the wave's 1600-word LDS stage in two phases of 32
// threads (stride 50 words over 32 lanes: no two lanes on one of the 64 banks).  Registers: 50 keys + 50 weights per thread
// within the 128 a wave may hold at 16 waves per CU; the build shows 128 VGPRs, 4 waves per SIMD and no scratch
// (-Rpass-analysis=kernel-resource-usage).  LDS: 102400 B of stage, 6400 B of bitmap, 128 B of reductions.
//
// osq_sample_nucleus_at is the same launches with the position read by them: cur = *cur_dev + cur_add, as osq_sample_advance_at.
//
// osq_sample_nucleus_group(_at): `group` sequences per input and the drawn token's log-probability, as
// osq_sample_advance_group (sample_draw.h): lp = (value(kv) - m) - logf(W) with W = S(k*) + float(r) * w(k*), all of them
// in registers when the draw ends; one more live value through the second bisection, still 128 VGPRs and no scratch.
#include <math.h>
#include <hip/hip_runtime.h>
#include "osq_device.h"
#include "osq_host.h"
#include "token_argmax.h"
#include "sample_draw.h"

namespace osq {

constexpr int kSnThreads = 1024, kSnWaves = kSnThreads / OSQ_WAVE;
constexpr int kSnPer = 50;                                      // tokens one thread owns
constexpr int kSnChains = 2;                                    // independent sums of 25 consecutive tokens inside a thread
static_assert(kSnPer % kSnChains == 0 && kSnChains == 2, "sn_above adds two halves as q0 + q1");
constexpr int kSnMaxVocab = kSnThreads * kSnPer;                // 51200
constexpr int kSnWaveTokens = OSQ_WAVE * kSnPer;                // 3200 consecutive tokens of one wave
constexpr int kSnPhases = 2, kSnPhaseLanes = OSQ_WAVE / kSnPhases, kSnPhaseWords = kSnPhaseLanes * kSnPer;   // 32 lanes, 1600 words
constexpr int kSnPhaseLoads = kSnPhaseWords / OSQ_WAVE;         // 25 wave-wide loads fill a phase
static_assert(kSnPhaseWords % OSQ_WAVE == 0, "a phase is whole wave-wide loads");
static_assert(kSnMaxVocab % 32 == 0 && kSnMaxVocab >= 50265, "the ban bitmap holds whole words; BART's vocabulary fits");

// True, in a way the compiler does not see through: a test of it ends a basic block.  The loops over a thread's 50 elements
// are unrolled (the elements are registers); ten divisions or exponentials to a block keep the blocks of a size the instruction
// selector and the register allocator handle.
constexpr int kSnBlock = 10;
static_assert(kSnPer % kSnBlock == 0, "whole blocks");
__device__ __forceinline__ bool sn_always() {
    int one = 1;
    asm volatile("" : "+s"(one));
    return one != 0;
}

// Workgroup reductions over kSnWaves waves; s_red: [2][kSnWaves] words, the halves used by alternate calls (`turn`), so one
// barrier per call is enough.  Every thread receives the result.
__device__ __forceinline__ float sn_block_sum(float v, unsigned int (*s_red)[kSnWaves], int& turn) {
    const int lane = threadIdx.x & (OSQ_WAVE - 1), w = threadIdx.x / OSQ_WAVE;
    v = wave_sum_f32(v);
    unsigned int* s = s_red[turn ^= 1];
    if (lane == 0) s[w] = __float_as_uint(v);
    __syncthreads();
    float sum = __uint_as_float(s[0]);
#pragma unroll
    for (int k = 1; k < kSnWaves; ++k) sum += __uint_as_float(s[k]);        // wave order, left to right
    return sum;
}

__device__ __forceinline__ unsigned int sn_block_max(unsigned int v, unsigned int (*s_red)[kSnWaves], int& turn) {
    const int lane = threadIdx.x & (OSQ_WAVE - 1), w = threadIdx.x / OSQ_WAVE;
    v = wave_max_u32(v);
    unsigned int* s = s_red[turn ^= 1];
    if (lane == 0) s[w] = v;
    __syncthreads();
    unsigned int best = s[0];
#pragma unroll
    for (int k = 1; k < kSnWaves; ++k) best = max(best, s[k]);
    return best;
}

// The sum of `count` over the threads before this one, and over all of them in `total`.
__device__ __forceinline__ unsigned int sn_block_before(unsigned int count, unsigned int& total, unsigned int (*s_red)[kSnWaves],
                                                        int& turn) {
    const int lane = threadIdx.x & (OSQ_WAVE - 1), w = threadIdx.x / OSQ_WAVE;
    const unsigned int upto = wave_inclusive_scan_u32(count);
    unsigned int* s = s_red[turn ^= 1];
    if (lane == OSQ_WAVE - 1) s[w] = upto;
    __syncthreads();
    unsigned int before = 0u;
    total = 0u;
#pragma unroll
    for (int k = 0; k < kSnWaves; ++k) {
        if (k < w) before += s[k];
        total += s[k];
    }
    return before + upto - count;
}

// sample_weight of a key, 0 for key 0, with the exponential taken before the selects: no branch around it per element.
__device__ __forceinline__ float sn_weight(unsigned int key, float m) {
    const float z = beam_value(key);
    const float e = expf(z - m);
    return key == 0u ? 0.f : (z == m ? 1.f : e);
}

// How many of the thread's tokens hold the key k.
__device__ __forceinline__ unsigned int sn_count(const unsigned int (&key)[kSnPer], unsigned int k) {
    unsigned int n = 0u;
#pragma unroll
    for (int j = 0; j < kSnPer; ++j) n += key[j] == k;
    return n;
}

// k, as a value the compiler takes for a new one: a second pass over the elements compares again instead of keeping the
// masks of the first alive in scalar registers.
__device__ __forceinline__ unsigned int sn_opaque(unsigned int k) {
    asm volatile("" : "+s"(k));
    return k;
}

// S(k): the weights of the tokens whose key is above k, in the file header's order.
__device__ __forceinline__ float sn_above(const unsigned int (&key)[kSnPer], const float (&wt)[kSnPer], unsigned int k,
                                          unsigned int (*s_red)[kSnWaves], int& turn) {
    float q[kSnChains];
#pragma unroll
    for (int c = 0; c < kSnChains; ++c) {
        q[c] = 0.f;
#pragma unroll
        for (int j = c * (kSnPer / kSnChains); j < (c + 1) * (kSnPer / kSnChains); ++j) q[c] += key[j] > k ? wt[j] : 0.f;
    }
    return sn_block_sum(q[0] + q[1], s_red, turn);
}

// The token of row b, in every thread, and its log-probability in `lp` (-inf for a row without a survivor).
__device__ __forceinline__ int64_t sn_pick(const SampleArgs& a, const Step& step, int64_t b, float u, float* s_stage,
                                           unsigned int* s_ban, unsigned int (*s_red)[kSnWaves], float& lp) {
    lp = -INFINITY;
    const int lane = threadIdx.x & (OSQ_WAVE - 1), w = threadIdx.x / OSQ_WAVE;
    const float* x = a.s.logits + b * a.s.logits_stride;
    unsigned int key[kSnPer];
    float wt[kSnPer];
    {
        float r[kSnPhaseLoads];
        const auto load = [&](int h) {                              // the words of lanes 32 h .. 32 h + 31 of this wave
#pragma unroll
            for (int k = 0; k < kSnPhaseLoads; ++k) {
                const int i = w * kSnWaveTokens + h * kSnPhaseWords + k * OSQ_WAVE + lane;
                r[k] = i < a.s.vocab ? x[i] : 0.f;
            }
        };
        load(0);                                                    // issued before the bans are found: the loads fly meanwhile
        span_bans<kSnThreads, kSnMaxVocab / 32>(s_ban, a.s.ban_ids, step.n_ban, a.s.seq + b * a.s.seq_stride, step.cur,
                                                a.s.ngram, 0, a.s.vocab);
        float* stage = s_stage + w * kSnPhaseWords;
#pragma unroll
        for (int h = 0; h < kSnPhases; ++h) {
            __syncthreads();                                        // the stage is free (h == 0: the bitmap is complete)
#pragma unroll
            for (int k = 0; k < kSnPhaseLoads; ++k) stage[k * OSQ_WAVE + lane] = r[k];
            if (h + 1 < kSnPhases) load(h + 1);                     // the next phase's loads fly over this one's hand-over
            __syncthreads();
            if (lane / kSnPhaseLanes == h) {
#pragma unroll
                for (int j = 0; j < kSnPer; ++j) wt[j] = stage[(lane % kSnPhaseLanes) * kSnPer + j];
            }
        }
    }
    unsigned int top = 0u;
#pragma unroll
    for (int g = 0; g < kSnPer / kSnBlock; ++g) {
        if (!sn_always()) continue;
#pragma unroll
        for (int j = g * kSnBlock; j < (g + 1) * kSnBlock; ++j) {
            const int i = threadIdx.x * kSnPer + j;
            const bool banned = (s_ban[i >> 5] >> (i & 31)) & 1u;   // i < kSnMaxVocab: inside the bitmap
            const float z = sample_z(wt[j], a.temperature, banned || i >= a.s.vocab);
            key[j] = z == -INFINITY ? 0u : beam_key(z);
            top = max(top, key[j]);
        }
    }
    int turn = 0;
    top = sn_block_max(top, s_red, turn);
    if (top == 0u) return 0;                                        // workgroup-uniform: no survivor in the row
    const float m = beam_value(top);
#pragma unroll
    for (int g = 0; g < kSnPer / kSnBlock; ++g) {
        if (!sn_always()) continue;
#pragma unroll
        for (int j = g * kSnBlock; j < (g + 1) * kSnBlock; ++j) wt[j] = sn_weight(key[j], m);
    }

    // ---- the cut
    const float bound = a.top_p * sn_above(key, wt, 0u, s_red, turn);
    unsigned int lo = 0u, cut = top;                                // S(lo) >= bound, S(cut) < bound
    float s_cut = 0.f;
    while (cut - lo > 1u) {
        const unsigned int mid = lo + (cut - lo) / 2u;
        const float s = sn_above(key, wt, mid, s_red, turn);
        if (s < bound) { cut = mid; s_cut = s; } else lo = mid;
    }
    // of the n tokens at the cut the first r stay: j -> S(cut) + float(j) * w(cut) < bound is true at 0 and monotone
    const float w_cut = sn_weight(cut, m);
    unsigned int n_cut;
    sn_block_before(sn_count(key, cut), n_cut, s_red, turn);
    unsigned int yes = 0u, no = n_cut;
    while (no - yes > 1u) {
        const unsigned int j = yes + (no - yes) / 2u;
        if (s_cut + static_cast<float>(j) * w_cut < bound) yes = j; else no = j;
    }
    const unsigned int n_kept = yes + 1u;
    const float kept = s_cut + static_cast<float>(n_kept) * w_cut;  // W
    const float target = u * kept;

    // ---- the draw
    unsigned int hit = top;                                         // S(hit) <= target; lo: above it, or just below the cut
    float s_hit = 0.f;
    lo = cut - 1u;
    while (hit - lo > 1u) {
        const unsigned int mid = lo + (hit - lo) / 2u;
        const float s = sn_above(key, wt, mid, s_red, turn);
        if (s <= target) { hit = mid; s_hit = s; } else lo = mid;
    }
    // of the group's eligible tokens the first with S(hit) + float(j + 1) * w(hit) > target (monotone in j), else the last
    const float w_hit = sn_weight(hit, m);
    const unsigned int mine = sn_count(key, hit);
    unsigned int n_hit;
    const unsigned int before = sn_block_before(mine, n_hit, s_red, turn);
    const unsigned int limit = hit == cut ? n_kept : n_hit;
    int below = -1;
    unsigned int pick = limit;
    while (static_cast<int>(pick) - below > 1) {
        const int j = below + (static_cast<int>(pick) - below) / 2;
        if (s_hit + static_cast<float>(j + 1) * w_hit > target) pick = j; else below = j;
    }
    if (pick == limit) pick = limit - 1u;
    // its owner names it: the (pick - before)-th of the thread's tokens with that key
    const unsigned int want = pick - before, same = sn_opaque(hit);
    unsigned int seen = 0u, token = 0u;
#pragma unroll
    for (int j = 0; j < kSnPer; ++j) {
        const bool is = key[j] == same;
        if (is && seen == want) token = threadIdx.x * kSnPer + j + 1u;
        seen += is;
    }
    if (a.logprobs) lp = sample_logprob(beam_value(hit), m, kept);
    return sn_block_max(token, s_red, turn) - 1u;                   // one thread holds it (limit >= 1: the key is present)
}

__global__ __launch_bounds__(kSnThreads) void sample_nucleus_row_kernel(SampleArgs a) {
    __shared__ float s_stage[kSnWaves * kSnPhaseWords];
    __shared__ unsigned int s_ban[kSnMaxVocab / 32];
    __shared__ unsigned int s_red[2][kSnWaves];
    const Step step = step_of(a.s);
    if (step.cur < 0) return;                                       // refused: nothing written (the go_on launch says so)
    const int64_t b = blockIdx.x;                                   // the row: sequence b % group of input b / group
    int64_t token = step.forced;
    float lp = 0.f;
    if (step.forced < 0) {                                          // a forced step reads no logit
        const float u = sample_row_uniform(a, blockIdx.x, step.cur);
        token = sn_pick(a, step, b, u, s_stage, s_ban, s_red, lp);
    }
    if (threadIdx.x == 0) sample_finish_row(a, step, b, token, lp);
}

__global__ __launch_bounds__(kStepGoThreads) void sample_nucleus_go_on_kernel(SampleArgs a) { step_go_on(a.s); }

static size_t nucleus_workspace_bytes(int64_t bsz) { return static_cast<size_t>(bsz) * sizeof(unsigned int); }

}  // namespace osq

using namespace osq;

extern "C" size_t osq_sample_nucleus_workspace_bytes(int64_t bsz, int64_t vocab) {
    return (bsz < 1 || vocab < 1 || vocab > kSnMaxVocab) ? 0 : nucleus_workspace_bytes(bsz);
}

// Both entry points: check, fill, launch.
static int sample_nucleus_run(const StepCall& c, uint64_t seed, float temperature, float top_p, const float* uniforms,
                              osq_stream stream, int64_t group = 1, float* logprobs = nullptr, int64_t logprobs_stride = 0) {
    if (const int rc = step_check("sample_nucleus", c)) return rc;
    if (const int rc = sample_group_check("sample_nucleus", c, group, logprobs, logprobs_stride)) return rc;
    OSQ_REQUIRE(c.bsz <= INT32_MAX, "sample_nucleus: bsz does not fit 31 bits");
    OSQ_REQUIRE(top_p > 0.f && top_p <= 1.f, "sample_nucleus: top_p outside (0, 1]");
    OSQ_REQUIRE(temperature > 0.f && temperature <= 3.4028234663852886e38f, "sample_nucleus: temperature not positive and finite");
    OSQ_REQUIRE(c.workspace_bytes >= nucleus_workspace_bytes(c.bsz), "sample_nucleus: workspace too small");
    if (c.vocab > kSnMaxVocab) {
        set_error("sample_nucleus: vocab %lld above %d, what one workgroup holds in registers", static_cast<long long>(c.vocab),
                  kSnMaxVocab);
        return OSQ_ERR_UNSUPPORTED;
    }
    const SampleArgs a{.s = step_args(c, 0, static_cast<unsigned int*>(c.workspace)), .uniforms = uniforms, .cands = nullptr,
                       .partials = nullptr, .seed = seed, .temperature = temperature, .top_p = top_p, .top_k = 0,
                       .group = static_cast<int>(group), .logprobs = logprobs, .logprobs_stride = logprobs_stride};
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(sample_nucleus_row_kernel, dim3(static_cast<unsigned>(c.bsz)), dim3(kSnThreads), 0, st, a);
    hipLaunchKernelGGL(sample_nucleus_go_on_kernel, dim3(1), dim3(kStepGoThreads), 0, st, a);
    return check_launch(c.cur_dev ? "sample_nucleus_at" : "sample_nucleus");
}

extern "C" int osq_sample_nucleus(const float* logits, int64_t logits_stride, int64_t* seq, int64_t seq_stride, int64_t cur,
                                  int64_t ngram, const int64_t* ban_ids, int64_t n_ban, int64_t forced, const int64_t* eos_ids,
                                  int64_t n_eos, int64_t pad, uint8_t* unfinished, int64_t bsz, int64_t vocab,
                                  int64_t max_length, int64_t* next_tokens, int32_t* go_on, void* workspace,
                                  size_t workspace_bytes, uint64_t seed, float temperature, float top_p, const float* uniforms,
                                  osq_stream stream) {
    return sample_nucleus_run({.logits = logits, .logits_stride = logits_stride, .seq = seq, .seq_stride = seq_stride, .cur = cur,
                               .ngram = ngram, .ban_ids = ban_ids, .n_ban = n_ban, .forced = forced, .eos_ids = eos_ids,
                               .n_eos = n_eos, .pad = pad, .unfinished = unfinished, .bsz = bsz, .vocab = vocab,
                               .max_length = max_length, .next_tokens = next_tokens, .go_on = go_on, .workspace = workspace,
                               .workspace_bytes = workspace_bytes}, seed, temperature, top_p, uniforms, stream);
}

extern "C" int osq_sample_nucleus_at(const float* logits, int64_t logits_stride, int64_t* seq, int64_t seq_stride,
                                     const int32_t* cur_dev, int64_t cur_add, int64_t ngram, const int64_t* ban_ids,
                                     int64_t n_ban, int64_t ban_below, int64_t forced_bos, int64_t forced_eos,
                                     const int64_t* eos_ids, int64_t n_eos, int64_t pad, uint8_t* unfinished, int64_t bsz,
                                     int64_t vocab, int64_t max_length, int64_t* next_tokens, int32_t* go_on, void* workspace,
                                     size_t workspace_bytes, uint64_t seed, float temperature, float top_p,
                                     const float* uniforms, osq_stream stream) {
    OSQ_REQUIRE(cur_dev, "sample_nucleus_at: null position word");
    OSQ_REQUIRE(cur_add >= INT32_MIN && cur_add <= INT32_MAX, "sample_nucleus_at: cur_add does not fit 32 bits");
    return sample_nucleus_run({.logits = logits, .logits_stride = logits_stride, .seq = seq, .seq_stride = seq_stride,
                               .cur_dev = cur_dev, .cur_add = cur_add, .ngram = ngram, .ban_ids = ban_ids, .n_ban = n_ban,
                               .ban_below = ban_below, .forced_bos = forced_bos, .forced_eos = forced_eos, .eos_ids = eos_ids,
                               .n_eos = n_eos, .pad = pad, .unfinished = unfinished, .bsz = bsz, .vocab = vocab,
                               .max_length = max_length, .next_tokens = next_tokens, .go_on = go_on, .workspace = workspace,
                               .workspace_bytes = workspace_bytes}, seed, temperature, top_p, uniforms, stream);
}

extern "C" int osq_sample_nucleus_group(const float* logits, int64_t logits_stride, int64_t* seq, int64_t seq_stride,
                                        int64_t cur, int64_t ngram, const int64_t* ban_ids, int64_t n_ban, int64_t forced,
                                        const int64_t* eos_ids, int64_t n_eos, int64_t pad, uint8_t* unfinished, int64_t bsz,
                                        int64_t vocab, int64_t max_length, int64_t* next_tokens, int32_t* go_on,
                                        void* workspace, size_t workspace_bytes, uint64_t seed, float temperature,
                                        float top_p, const float* uniforms, int64_t group, float* logprobs,
                                        int64_t logprobs_stride, osq_stream stream) {
    return sample_nucleus_run({.logits = logits, .logits_stride = logits_stride, .seq = seq, .seq_stride = seq_stride, .cur = cur,
                               .ngram = ngram, .ban_ids = ban_ids, .n_ban = n_ban, .forced = forced, .eos_ids = eos_ids,
                               .n_eos = n_eos, .pad = pad, .unfinished = unfinished, .bsz = bsz, .vocab = vocab,
                               .max_length = max_length, .next_tokens = next_tokens, .go_on = go_on, .workspace = workspace,
                               .workspace_bytes = workspace_bytes}, seed, temperature, top_p, uniforms, stream, group, logprobs,
                              logprobs_stride);
}

extern "C" int osq_sample_nucleus_group_at(const float* logits, int64_t logits_stride, int64_t* seq, int64_t seq_stride,
                                           const int32_t* cur_dev, int64_t cur_add, int64_t ngram, const int64_t* ban_ids,
                                           int64_t n_ban, int64_t ban_below, int64_t forced_bos, int64_t forced_eos,
                                           const int64_t* eos_ids, int64_t n_eos, int64_t pad, uint8_t* unfinished,
                                           int64_t bsz, int64_t vocab, int64_t max_length, int64_t* next_tokens,
                                           int32_t* go_on, void* workspace, size_t workspace_bytes, uint64_t seed,
                                           float temperature, float top_p, const float* uniforms, int64_t group,
                                           float* logprobs, int64_t logprobs_stride, osq_stream stream) {
    OSQ_REQUIRE(cur_dev, "sample_nucleus_at: null position word");
    OSQ_REQUIRE(cur_add >= INT32_MIN && cur_add <= INT32_MAX, "sample_nucleus_at: cur_add does not fit 32 bits");
    return sample_nucleus_run({.logits = logits, .logits_stride = logits_stride, .seq = seq, .seq_stride = seq_stride,
                               .cur_dev = cur_dev, .cur_add = cur_add, .ngram = ngram, .ban_ids = ban_ids, .n_ban = n_ban,
                               .ban_below = ban_below, .forced_bos = forced_bos, .forced_eos = forced_eos, .eos_ids = eos_ids,
                               .n_eos = n_eos, .pad = pad, .unfinished = unfinished, .bsz = bsz, .vocab = vocab,
                               .max_length = max_length, .next_tokens = next_tokens, .go_on = go_on, .workspace = workspace,
                               .workspace_bytes = workspace_bytes}, seed, temperature, top_p, uniforms, stream, group, logprobs,
                              logprobs_stride);
}

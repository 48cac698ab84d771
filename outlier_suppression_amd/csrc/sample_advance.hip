// ONE sampling step after the model: the banned tokens, temperature, top-k / top-p, a seeded draw from what is left, the pad /
// eos arithmetic, the new token into the sequence and the stopping word, in three small launches.
//
// For a step at history length `cur`, a row cut into chunks of kBsChunk tokens (token_argmax.h), z = x / temperature (one IEEE
// division), a banned token, a NaN and -inf out of the draw (weight 0):
//
//   launch 1   sample_chunk_kernel   one workgroup per (row, chunk): the chunk's ban bitmap in LDS, the chunk's z in registers
//                                    (16 per thread).  top_k >= 1: top_k rounds of a workgroup arg-max, the chunk's first top_k
//                                    candidates (value key, token) go to the workspace.  top_k == 0: the chunk's maximum m_c and
//                                    s_c = sum exp(z - m_c) go there.  A forced step returns at once: it reads no logit
//   launch 2   sample_row_kernel     one workgroup per row.  top_k >= 1: top_k rounds of the same arg-max over the row's
//                                    candidates give the survivors in rank order (larger z first, equal z by smaller token);
//                                    weights w_i = exp(z_i - z_0), the top-p cut, the draw.  top_k == 0: the row's total from the
//                                    chunk sums in chunk order, the chunk the draw falls into, and that chunk read once more for
//                                    the token.  Then the forced token in its place, pad / eos, seq[b, cur], next_tokens[b] and
//                                    the row's unfinished flag into the workspace
//   launch 3   sample_go_on_kernel   one wave: go_on = (cur + 1 < max_length) && (n_eos == 0 || any row unfinished)
//
// No workgroup waits for another: the launches follow each other on the stream.  No atomics on device memory.
//
// The draw: u = (word 0 of Philox4x32-10 with key (seed lo, seed hi) and counter (row, cur, 0, 0)) >> 8, times 2^-24 -- no
// state to advance, so a captured graph of the call serves every step -- or uniforms[row] when given.  With C_i the running fp32
// sum of the kept weights in the survivors' order and W their total, the token is the first kept survivor with C_i > u * W, the
// last kept one when rounding leaves none.  A row without a survivor gives token 0.
//
// Summation order, fixed by (vocab, top_k) alone -- not by the row's alignment, stride or bsz.  top_k >= 1: ranks in order, one
// thread.  top_k == 0: s_c as beam_partials_kernel forms it (thread t adds elements t, t + 256, ... in order, wave_sum_f32, then
// (w0 + w1) + (w2 + w3)); the row total and the walk add s_c * exp(m_c - m) in chunk order; inside the chosen chunk thread t owns
// tokens 16 t .. 16 t + 15 and adds them in order onto the sum of the threads before it (16 groups of 16 threads, each summed in
// order).  Elements are loaded one 32-bit word per lane: a row of an odd vocab is only 4-byte aligned.
//
// osq_sample_advance_at is the same launches with the position read by them: cur = *cur_dev + cur_add, as osq_greedy_advance_at.
//
// osq_sample_advance_group(_at): the rows come in groups of `group` sequences per input, row r drawing at the counter
// (r / group, cur, r % group, 0), and -- with `logprobs` -- the thread that ends row r stores lp = (z_tok - m) - logf(W) into
// logprobs[r, cur] from what the pick already holds (top_k >= 1: the picked key, rank 0's and the kept total; top_k == 0: the
// row's m and total, and the token's logit read once more): 0 on a forced step and for a finished row, -inf without a
// survivor.  No further pass over the logits, no workspace; with logprobs == nullptr nothing is computed for it.  The
// ungrouped entry points are these with group 1 and no buffer.
//
// The step's arguments, the step read from the position word, the row's tail, the stopping word and the entry points' shared
// requirements are advance_step.h's (greedy_advance.hip ends with them too); what is about the draw is sample_draw.h's.
#include <math.h>
#include <hip/hip_runtime.h>
#include "osq_device.h"
#include "osq_host.h"
#include "token_argmax.h"
#include "sample_draw.h"

namespace osq {

constexpr int kSaGroup = 16;                         // threads whose sums one thread adds in order (the chosen chunk's scan)

__global__ __launch_bounds__(kBsThreads) void sample_chunk_kernel(SampleArgs a) {
    __shared__ unsigned int s_ban[kBsChunk / 32];
    __shared__ unsigned int s_red[2][2 * kBsWaves];
    __shared__ float s_sum[2][kBsWaves];
    const Step step = step_of(a.s);
    if (step.cur < 0 || step.forced >= 0) return;                   // refused, or forced: every logit is ignored
    const int lane = threadIdx.x & (OSQ_WAVE - 1), w = threadIdx.x / OSQ_WAVE;
    const int64_t row = blockIdx.x / a.s.chunks;
    const int c = blockIdx.x % a.s.chunks;
    const int c0 = c * kBsChunk;
    const int len = min(kBsChunk, a.s.vocab - c0);
    float v[kBsPer];
    chunk_each(a.s.logits + row * a.s.logits_stride + c0, s_ban, a.s.ban_ids, step.n_ban, a.s.seq + row * a.s.seq_stride,
               step.cur, a.s.ngram, c0, len,
               [&](int j, int, float x, bool banned, bool in) { v[j] = sample_z(x, a.temperature, banned || !in); });

    if (a.top_k == 0) {                                             // ---- the chunk's maximum and exp sum
        float mx = -INFINITY;
#pragma unroll
        for (int j = 0; j < kBsPer; ++j) mx = fmaxf(mx, v[j]);
        mx = wave_max(mx);
        if (lane == 0) s_sum[0][w] = mx;
        __syncthreads();
        mx = fmaxf(fmaxf(s_sum[0][0], s_sum[0][1]), fmaxf(s_sum[0][2], s_sum[0][3]));
        float sum = 0.f;
#pragma unroll
        for (int j = 0; j < kBsPer; ++j)
            if (v[j] != -INFINITY) sum += sample_weight(v[j], mx);
        sum = wave_sum_f32(sum);
        if (lane == 0) s_sum[1][w] = sum;
        __syncthreads();
        if (threadIdx.x == 0)
            a.partials[blockIdx.x] = make_float2(mx, (s_sum[1][0] + s_sum[1][1]) + (s_sum[1][2] + s_sum[1][3]));
        return;
    }

    // ---- the chunk's first top_k candidates; key 0: none
    unsigned int key[kBsPer];
#pragma unroll
    for (int j = 0; j < kBsPer; ++j) key[j] = v[j] == -INFINITY ? 0u : beam_key(v[j]);
    BeamCand* out = a.cands + static_cast<int64_t>(blockIdx.x) * a.top_k;
    unsigned int best = 0u, best_i = threadIdx.x;
#pragma unroll
    for (int j = 0; j < kBsPer; ++j)
        if (key[j] > best) { best = key[j]; best_i = threadIdx.x + j * kBsThreads; }      // strict: the smaller index stays
    for (int r = 0; r < a.top_k; ++r) {
        unsigned int hi = best, lo = ~best_i;
        block_argmax(hi, lo, s_red, r & 1);
        const unsigned int i = ~lo;
        if (threadIdx.x == 0) out[r] = BeamCand{hi, hi ? c0 + static_cast<int>(i) : -1};
        if (hi && (i & (kBsThreads - 1)) == threadIdx.x) {          // the owner takes it out and looks again
            best = 0u;
            best_i = threadIdx.x;
#pragma unroll
            for (int j = 0; j < kBsPer; ++j) {
                if (static_cast<unsigned int>(j) == i / kBsThreads) key[j] = 0u;
                if (key[j] > best) { best = key[j]; best_i = threadIdx.x + j * kBsThreads; }
            }
        }
    }
}

// The token of row b with top_k >= 1, in thread 0: the survivors by top_k rounds over the row's candidates, their weights, the
// top-p cut and the draw u; beside it, there too, its log-probability in `lp` (-inf for a row without a survivor).  Every
// thread of the workgroup calls it.
__device__ __forceinline__ int64_t sample_pick_top_k(const SampleArgs& a, int64_t b, float u, unsigned int (*s_red)[2 * kBsWaves],
                                                     unsigned int* s_key, int* s_tok, float* s_w, float& lp) {
    lp = -INFINITY;
    const int n = a.s.chunks * a.top_k;                             // among equal values slots run as tokens do
    BeamCand* cand = a.cands + b * n;
    unsigned int best = 0u, best_p = threadIdx.x;
    for (int p = threadIdx.x; p < n; p += kBsThreads) {
        const unsigned int k = cand[p].key;
        if (k > best) { best = k; best_p = p; }
    }
    int kept = 0;
    for (; kept < a.top_k; ++kept) {
        unsigned int hi = best, lo = ~best_p;
        block_argmax(hi, lo, s_red, kept & 1);
        if (!hi) break;                                             // workgroup-uniform: no candidate is left
        const unsigned int p = ~lo;
        if ((p & (kBsThreads - 1)) == threadIdx.x) {                // the owner notes it, takes it out and looks again
            s_key[kept] = hi;
            s_tok[kept] = cand[p].token;
            cand[p].key = 0u;
            best = 0u;
            best_p = threadIdx.x;
            for (int q = threadIdx.x; q < n; q += kBsThreads) {
                const unsigned int k = cand[q].key;
                if (k > best) { best = k; best_p = q; }
            }
        }
    }
    __syncthreads();
    if (kept == 0) return 0;
    if (threadIdx.x < kept) s_w[threadIdx.x] = sample_weight(beam_value(s_key[threadIdx.x]), beam_value(s_key[0]));
    __syncthreads();
    if (threadIdx.x != 0) return 0;
    float total = 0.f;
    for (int i = 0; i < kept; ++i) total += s_w[i];
    if (a.top_p < 1.f) {                                            // rank i stays iff the weights above it sum below top_p * total
        const float bound = a.top_p * total;
        float above = s_w[0];
        int i = 1;
        for (; i < kept && above < bound; ++i) above += s_w[i];
        kept = i;
        total = above;
    }
    const float target = u * total;
    float upto = 0.f;
    int pick = kept - 1;
    for (int i = 0; i < kept; ++i) {
        upto += s_w[i];
        if (upto > target) { pick = i; break; }
    }
    if (a.logprobs) lp = sample_logprob(beam_value(s_key[pick]), beam_value(s_key[0]), total);
    return s_tok[pick];
}

// The token of row b with top_k == 0, in every thread: the chunk the draw u falls into by the chunk sums, then that chunk's
// tokens in order; beside it its log-probability in `lp` (-inf for a row without a survivor), from the token's own logit
// read once more by the one thread that stores it.  s_w: kBsChunk + kBsThreads floats; s_tot: kBsThreads; s_grp: kSaGroup.
__device__ __forceinline__ int64_t sample_pick_full(const SampleArgs& a, const Step& step, int64_t b, float u,
                                                    unsigned int* s_ban, unsigned int (*s_red)[2 * kBsWaves], float* s_w,
                                                    float* s_tot, float* s_grp, float& lp) {
    const float2* part = a.partials + b * a.s.chunks;
    lp = -INFINITY;
    float m = -INFINITY;
    for (int k = 0; k < a.s.chunks; ++k) m = fmaxf(m, part[k].x);
    if (m == -INFINITY) return 0;                                   // no survivor in the row
    float total = 0.f;
    for (int k = 0; k < a.s.chunks; ++k) {
        const float2 p = part[k];
        total += p.y * sample_weight(p.x, m);
    }
    float target = u * total;
    float before = 0.f;
    int chosen = -1, last = 0;
    for (int k = 0; k < a.s.chunks; ++k) {
        const float2 p = part[k];
        const float wc = p.y * sample_weight(p.x, m);
        if (wc > 0.f) last = k;
        if (before + wc > target) { chosen = k; break; }
        before += wc;
    }
    if (chosen < 0) {                                               // rounding left none: the last survivor of the last chunk that has one
        chosen = last;
        target = INFINITY;
    }

    // ---- the chosen chunk once more: its weights in token order
    const int c0 = chosen * kBsChunk;
    const int len = min(kBsChunk, a.s.vocab - c0);
    const float mc = part[chosen].x;
    const float scale = sample_weight(mc, m);
    chunk_each(a.s.logits + b * a.s.logits_stride + c0, s_ban, a.s.ban_ids, step.n_ban, a.s.seq + b * a.s.seq_stride, step.cur,
               a.s.ngram, c0, len, [&](int, int i, float x, bool banned, bool in) {
                   const float z = sample_z(x, a.temperature, banned || !in);
                   s_w[i + (i >> 4)] = z == -INFINITY ? 0.f : sample_weight(z, mc) * scale;   // one pad word per 16: thread t reads 17 t + j
               });
    __syncthreads();
    float v[kBsPer];
    float own = 0.f;
#pragma unroll
    for (int j = 0; j < kBsPer; ++j) {
        v[j] = s_w[threadIdx.x * (kBsPer + 1) + j];
        own += v[j];
    }
    s_tot[threadIdx.x] = own;
    __syncthreads();
    if (threadIdx.x < kBsThreads / kSaGroup) {                      // the sums before each thread of a group, and the group's
        float run = 0.f;
        for (int q = 0; q < kSaGroup; ++q) {
            const float t = s_tot[threadIdx.x * kSaGroup + q];
            s_tot[threadIdx.x * kSaGroup + q] = run;
            run += t;
        }
        s_grp[threadIdx.x] = run;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float run = 0.f;
        for (int q = 0; q < kBsThreads / kSaGroup; ++q) {
            const float t = s_grp[q];
            s_grp[q] = run;
            run += t;
        }
    }
    __syncthreads();
    const float base = before + (s_grp[threadIdx.x / kSaGroup] + s_tot[threadIdx.x]);
    unsigned int hit = 0u, hit_i = 0u, live = 0u, live_i = 0u;      // the first token past the target; the last with a weight
    float upto = 0.f;
#pragma unroll
    for (int j = 0; j < kBsPer; ++j) {
        upto += v[j];
        if (v[j] > 0.f) {
            const unsigned int i = threadIdx.x * kBsPer + j;
            live = 1u;
            live_i = i;
            if (!hit && base + upto > target) { hit = 1u; hit_i = i; }
        }
    }
    unsigned int lo = ~hit_i;
    block_argmax(hit, lo, s_red, 0);                                // the largest ~i: the smallest token
    block_argmax(live, live_i, s_red, 1);
    const int token = c0 + static_cast<int>(hit ? ~lo : live_i);    // live: the chunk's maximum weighs `scale` > 0
    if (a.logprobs && threadIdx.x == 0)                             // a survivor: not banned, inside the row
        lp = sample_logprob(sample_z(a.s.logits[b * a.s.logits_stride + token], a.temperature, false), m, total);
    return token;
}

__global__ __launch_bounds__(kBsThreads) void sample_row_kernel(SampleArgs a) {
    __shared__ unsigned int s_ban[kBsChunk / 32];
    __shared__ unsigned int s_red[2][2 * kBsWaves];
    __shared__ float s_w[kBsChunk + kBsThreads];
    __shared__ float s_tot[kBsThreads], s_grp[kBsThreads / kSaGroup];
    __shared__ unsigned int s_key[kSaMaxTopK];
    __shared__ int s_tok[kSaMaxTopK];
    const Step step = step_of(a.s);
    if (step.cur < 0) return;                                       // refused: nothing written (sample_go_on_kernel says so)
    const int64_t b = blockIdx.x;                                   // the row: sequence b % group of input b / group
    int64_t token = step.forced;
    float lp = 0.f;
    if (step.forced < 0) {
        const float u = sample_row_uniform(a, blockIdx.x, step.cur);
        token = a.top_k > 0 ? sample_pick_top_k(a, b, u, s_red, s_key, s_tok, s_w, lp)
                            : sample_pick_full(a, step, b, u, s_ban, s_red, s_w, s_tot, s_grp, lp);
    }
    if (threadIdx.x == 0) sample_finish_row(a, step, b, token, lp);
}

__global__ __launch_bounds__(kStepGoThreads) void sample_go_on_kernel(SampleArgs a) { step_go_on(a.s); }

__global__ __launch_bounds__(kBsThreads) void sample_uniforms_kernel(unsigned long long seed, int bsz, unsigned int group,
                                                                     unsigned int cur, float* out) {
    const unsigned int r = blockIdx.x * kBsThreads + threadIdx.x;
    if (r < static_cast<unsigned int>(bsz)) out[r] = sample_uniform(seed, r / group, cur, r % group);
}

static size_t sample_workspace_bytes(int64_t bsz, int64_t vocab, int64_t top_k) {
    if (bsz < 1 || vocab < 1 || top_k < 0 || top_k > kSaMaxTopK) return 0;
    static_assert(sizeof(BeamCand) == sizeof(float2), "one workspace slot holds a candidate or a chunk's (m_c, s_c)");
    const int64_t slots = bsz * step_chunks(vocab) * (top_k > 0 ? top_k : 1);
    return static_cast<size_t>(slots) * sizeof(BeamCand) + static_cast<size_t>(bsz) * sizeof(unsigned int);
}

}  // namespace osq

using namespace osq;

extern "C" size_t osq_sample_advance_workspace_bytes(int64_t bsz, int64_t vocab, int64_t top_k) {
    return sample_workspace_bytes(bsz, vocab, top_k);
}

// Both entry points: check, fill, launch.
static int sample_advance_run(const StepCall& c, uint64_t seed, float temperature, int64_t top_k, float top_p,
                              const float* uniforms, osq_stream stream, int64_t group = 1, float* logprobs = nullptr,
                              int64_t logprobs_stride = 0) {
    if (const int rc = step_check("sample_advance", c)) return rc;
    if (const int rc = sample_group_check("sample_advance", c, group, logprobs, logprobs_stride)) return rc;
    OSQ_REQUIRE(top_k >= 0 && top_k <= kSaMaxTopK, "sample_advance: top_k outside [0, 64]");
    OSQ_REQUIRE(top_p > 0.f && top_p <= 1.f, "sample_advance: top_p outside (0, 1]");
    OSQ_REQUIRE(temperature > 0.f && temperature <= 3.4028234663852886e38f, "sample_advance: temperature not positive and finite");
    const int64_t chunks = step_chunks(c.vocab);
    OSQ_REQUIRE(c.bsz <= INT32_MAX / (chunks * (top_k > 0 ? top_k : 1)), "sample_advance: too many elements");
    OSQ_REQUIRE(c.workspace_bytes >= sample_workspace_bytes(c.bsz, c.vocab, top_k), "sample_advance: workspace too small");
    if (top_k == 0 && top_p < 1.f) {
        set_error("%s", "sample_advance: top_p below 1 without top_k (a nucleus over the whole vocabulary) has no kernel");
        return OSQ_ERR_UNSUPPORTED;
    }
    BeamCand* cands = static_cast<BeamCand*>(c.workspace);
    const int64_t slots = c.bsz * chunks * (top_k > 0 ? top_k : 1);
    const SampleArgs a{.s = step_args(c, chunks, reinterpret_cast<unsigned int*>(cands + slots)), .uniforms = uniforms,
                       .cands = cands, .partials = static_cast<float2*>(c.workspace), .seed = seed, .temperature = temperature,
                       .top_p = top_p, .top_k = static_cast<int>(top_k), .group = static_cast<int>(group), .logprobs = logprobs,
                       .logprobs_stride = logprobs_stride};
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(sample_chunk_kernel, dim3(static_cast<unsigned>(c.bsz * chunks)), dim3(kBsThreads), 0, st, a);
    hipLaunchKernelGGL(sample_row_kernel, dim3(static_cast<unsigned>(c.bsz)), dim3(kBsThreads), 0, st, a);
    hipLaunchKernelGGL(sample_go_on_kernel, dim3(1), dim3(kStepGoThreads), 0, st, a);
    return check_launch(c.cur_dev ? "sample_advance_at" : "sample_advance");
}

extern "C" int osq_sample_advance(const float* logits, int64_t logits_stride, int64_t* seq, int64_t seq_stride, int64_t cur,
                                  int64_t ngram, const int64_t* ban_ids, int64_t n_ban, int64_t forced, const int64_t* eos_ids,
                                  int64_t n_eos, int64_t pad, uint8_t* unfinished, int64_t bsz, int64_t vocab,
                                  int64_t max_length, int64_t* next_tokens, int32_t* go_on, void* workspace,
                                  size_t workspace_bytes, uint64_t seed, float temperature, int64_t top_k, float top_p,
                                  const float* uniforms, osq_stream stream) {
    return sample_advance_run({.logits = logits, .logits_stride = logits_stride, .seq = seq, .seq_stride = seq_stride, .cur = cur,
                               .ngram = ngram, .ban_ids = ban_ids, .n_ban = n_ban, .forced = forced, .eos_ids = eos_ids,
                               .n_eos = n_eos, .pad = pad, .unfinished = unfinished, .bsz = bsz, .vocab = vocab,
                               .max_length = max_length, .next_tokens = next_tokens, .go_on = go_on, .workspace = workspace,
                               .workspace_bytes = workspace_bytes}, seed, temperature, top_k, top_p, uniforms, stream);
}

extern "C" int osq_sample_advance_at(const float* logits, int64_t logits_stride, int64_t* seq, int64_t seq_stride,
                                     const int32_t* cur_dev, int64_t cur_add, int64_t ngram, const int64_t* ban_ids,
                                     int64_t n_ban, int64_t ban_below, int64_t forced_bos, int64_t forced_eos,
                                     const int64_t* eos_ids, int64_t n_eos, int64_t pad, uint8_t* unfinished, int64_t bsz,
                                     int64_t vocab, int64_t max_length, int64_t* next_tokens, int32_t* go_on, void* workspace,
                                     size_t workspace_bytes, uint64_t seed, float temperature, int64_t top_k, float top_p,
                                     const float* uniforms, osq_stream stream) {
    OSQ_REQUIRE(cur_dev, "sample_advance_at: null position word");
    OSQ_REQUIRE(cur_add >= INT32_MIN && cur_add <= INT32_MAX, "sample_advance_at: cur_add does not fit 32 bits");
    return sample_advance_run({.logits = logits, .logits_stride = logits_stride, .seq = seq, .seq_stride = seq_stride,
                               .cur_dev = cur_dev, .cur_add = cur_add, .ngram = ngram, .ban_ids = ban_ids, .n_ban = n_ban,
                               .ban_below = ban_below, .forced_bos = forced_bos, .forced_eos = forced_eos, .eos_ids = eos_ids,
                               .n_eos = n_eos, .pad = pad, .unfinished = unfinished, .bsz = bsz, .vocab = vocab,
                               .max_length = max_length, .next_tokens = next_tokens, .go_on = go_on, .workspace = workspace,
                               .workspace_bytes = workspace_bytes}, seed, temperature, top_k, top_p, uniforms, stream);
}

extern "C" int osq_sample_advance_group(const float* logits, int64_t logits_stride, int64_t* seq, int64_t seq_stride,
                                        int64_t cur, int64_t ngram, const int64_t* ban_ids, int64_t n_ban, int64_t forced,
                                        const int64_t* eos_ids, int64_t n_eos, int64_t pad, uint8_t* unfinished, int64_t bsz,
                                        int64_t vocab, int64_t max_length, int64_t* next_tokens, int32_t* go_on,
                                        void* workspace, size_t workspace_bytes, uint64_t seed, float temperature,
                                        int64_t top_k, float top_p, const float* uniforms, int64_t group, float* logprobs,
                                        int64_t logprobs_stride, osq_stream stream) {
    return sample_advance_run({.logits = logits, .logits_stride = logits_stride, .seq = seq, .seq_stride = seq_stride, .cur = cur,
                               .ngram = ngram, .ban_ids = ban_ids, .n_ban = n_ban, .forced = forced, .eos_ids = eos_ids,
                               .n_eos = n_eos, .pad = pad, .unfinished = unfinished, .bsz = bsz, .vocab = vocab,
                               .max_length = max_length, .next_tokens = next_tokens, .go_on = go_on, .workspace = workspace,
                               .workspace_bytes = workspace_bytes}, seed, temperature, top_k, top_p, uniforms, stream, group,
                              logprobs, logprobs_stride);
}

extern "C" int osq_sample_advance_group_at(const float* logits, int64_t logits_stride, int64_t* seq, int64_t seq_stride,
                                           const int32_t* cur_dev, int64_t cur_add, int64_t ngram, const int64_t* ban_ids,
                                           int64_t n_ban, int64_t ban_below, int64_t forced_bos, int64_t forced_eos,
                                           const int64_t* eos_ids, int64_t n_eos, int64_t pad, uint8_t* unfinished,
                                           int64_t bsz, int64_t vocab, int64_t max_length, int64_t* next_tokens,
                                           int32_t* go_on, void* workspace, size_t workspace_bytes, uint64_t seed,
                                           float temperature, int64_t top_k, float top_p, const float* uniforms,
                                           int64_t group, float* logprobs, int64_t logprobs_stride, osq_stream stream) {
    OSQ_REQUIRE(cur_dev, "sample_advance_at: null position word");
    OSQ_REQUIRE(cur_add >= INT32_MIN && cur_add <= INT32_MAX, "sample_advance_at: cur_add does not fit 32 bits");
    return sample_advance_run({.logits = logits, .logits_stride = logits_stride, .seq = seq, .seq_stride = seq_stride,
                               .cur_dev = cur_dev, .cur_add = cur_add, .ngram = ngram, .ban_ids = ban_ids, .n_ban = n_ban,
                               .ban_below = ban_below, .forced_bos = forced_bos, .forced_eos = forced_eos, .eos_ids = eos_ids,
                               .n_eos = n_eos, .pad = pad, .unfinished = unfinished, .bsz = bsz, .vocab = vocab,
                               .max_length = max_length, .next_tokens = next_tokens, .go_on = go_on, .workspace = workspace,
                               .workspace_bytes = workspace_bytes}, seed, temperature, top_k, top_p, uniforms, stream, group,
                              logprobs, logprobs_stride);
}

extern "C" int osq_sample_uniforms_group(uint64_t seed, int64_t bsz, int64_t group, int64_t cur, float* out, osq_stream stream) {
    OSQ_REQUIRE(bsz >= 1 && bsz <= INT32_MAX - kBsThreads, "sample_uniforms: bsz outside [1, 2^31)");
    OSQ_REQUIRE(group >= 1 && bsz % group == 0, "sample_uniforms: group must be at least 1 and divide bsz");
    OSQ_REQUIRE(cur >= 0 && cur <= 0xffffffffll, "sample_uniforms: cur does not fit 32 bits");
    OSQ_REQUIRE(out, "sample_uniforms: null tensor");
    hipLaunchKernelGGL(sample_uniforms_kernel, dim3(static_cast<unsigned>((bsz + kBsThreads - 1) / kBsThreads)), dim3(kBsThreads),
                       0, static_cast<hipStream_t>(stream), static_cast<unsigned long long>(seed), static_cast<int>(bsz),
                       static_cast<unsigned int>(group), static_cast<unsigned int>(cur), out);
    return check_launch("sample_uniforms");
}

extern "C" int osq_sample_uniforms(uint64_t seed, int64_t bsz, int64_t cur, float* out, osq_stream stream) {
    return osq_sample_uniforms_group(seed, bsz, 1, cur, out, stream);
}

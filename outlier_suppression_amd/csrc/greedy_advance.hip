// ONE greedy decoding step after the model: the banned tokens, the arg-max of every row, the pad / eos arithmetic, the new
// token into the sequence and the stopping word, in three small launches that read the logits once.
//
// model/generation.py::_greedy runs, per token, one clone / masked_fill of [bsz, vocab] per logits processor (unfold and
// scatter_ for the n-gram rule), argmax, the pad / isin lines, a torch.cat that reallocates the sequence and a host read of
// unfinished.max().  Here, for a step at history length `cur`, a row cut into chunks of kBsChunk tokens:
//
//   launch 1   greedy_chunk_kernel   one workgroup per (row, chunk): the chunk's ban bitmap in LDS (token_argmax.h), the
//                                    chunk's values in registers (16 per thread), one workgroup arg-max: the chunk's
//                                    candidate (value key, token) goes to the workspace.  A forced step returns at once: it
//                                    reads no logit
//   launch 2   greedy_row_kernel     one workgroup per row: the arg-max over the row's candidates (equal keys by smaller
//                                    chunk), the forced token in its place, then pad / eos, seq[b, cur], next_tokens[b] and
//                                    the row's unfinished flag into the workspace
//   launch 3   greedy_go_on_kernel   one wave: go_on = (cur + 1 < max_length) && (n_eos == 0 || any row unfinished)
//
// No workgroup waits for another: the launches follow each other on the stream.  No float arithmetic but v + 0.0f, no atomics
// on device memory: the same inputs give the same words on every run.
//
// Order: torch.argmax's (and numpy's) -- larger value first, equal values by smaller index, -0.0 equal to +0.0, NaN above every
// number, NaNs among themselves by smaller index.  A value is the key (ordered_bits(v + 0.0f) with every NaN as 0xffffffff,
// ~token); v + 0.0f turns -0.0 into +0.0 and changes no other value: ordered_bits separates the two zeros, torch does not.
// A banned token counts as -inf, a banned NaN included, so a row that is all -inf or all banned gives token 0.
//
// osq_greedy_advance_at is the same launches with the position read by them: cur = *cur_dev + cur_add, one scalar read per
// workgroup.  ban_ids then apply while cur < ban_below, forced_bos fires at cur == 1 and forced_eos at cur == max_length - 1
// (where both fire, eos: the later processor).  A cur outside [1, max_length) is refused before any address is formed from
// it: the first two launches write nothing, the third writes go_on = -1.
#include <math.h>
#include <hip/hip_runtime.h>
#include "osq_device.h"
#include "osq_host.h"
#include "token_argmax.h"

namespace osq {

constexpr int kGaMaxLength = kBsMaxCur, kGaMaxEos = 16;
constexpr int kGaGoThreads = OSQ_WAVE;               // rows one trip of the go_on reduction covers

struct GreedyArgs {
    const float* logits;       // bsz x vocab, rows logits_stride floats apart
    int64_t* seq;              // bsz x max_length, rows seq_stride apart: [0, cur) read with ngram > 0, [cur] written
    const int64_t* ban_ids;    // n_ban ids banned in every row
    const int64_t* eos_ids;    // n_eos ids that finish a row
    uint8_t* unfinished;       // [bsz]; touched only with n_eos > 0
    int64_t* next_tokens;      // [bsz]
    int32_t* go_on;            // 1
    BeamCand* cands;           // [bsz, chunks]  workspace
    unsigned int* row_flags;   // [bsz]          workspace: the row is unfinished after this step
    int64_t logits_stride, seq_stride;
    int64_t pad;
    int bsz, vocab, chunks, max_length, cur, ngram, n_ban, n_eos;
    int forced;                // static form: >= 0 is this step's token
    // osq_greedy_advance_at: cur = *cur_dev + cur_add, read by the launches
    const int32_t* cur_dev;    // nullptr: the static form, cur / n_ban / forced above
    int cur_add, ban_below, forced_bos, forced_eos;
};

struct GreedyStep {            // what a launch knows of its step: workgroup-uniform
    int cur;                   // -1: refused
    int n_ban, forced;
};

__device__ __forceinline__ GreedyStep greedy_step(const GreedyArgs& a) {
    if (!a.cur_dev) return GreedyStep{a.cur, a.n_ban, a.forced};
    const long long at = static_cast<long long>(__builtin_amdgcn_readfirstlane(*a.cur_dev)) + a.cur_add;
    if (at < 1 || at >= a.max_length) return GreedyStep{-1, 0, -1};
    const int cur = static_cast<int>(at);
    int forced = cur == 1 ? a.forced_bos : -1;
    if (cur == a.max_length - 1 && a.forced_eos >= 0) forced = a.forced_eos;
    return GreedyStep{cur, cur < a.ban_below ? a.n_ban : 0, forced};
}

__global__ __launch_bounds__(kBsThreads) void greedy_chunk_kernel(GreedyArgs a) {
    __shared__ unsigned int s_ban[kBsChunk / 32];
    __shared__ unsigned int s_red[2][2 * kBsWaves];
    const GreedyStep step = greedy_step(a);
    if (step.cur < 0 || step.forced >= 0) return;                   // refused, or forced: every logit is ignored
    const int64_t row = blockIdx.x / a.chunks;
    const int c = blockIdx.x % a.chunks;
    const int c0 = c * kBsChunk;
    const int len = min(kBsChunk, a.vocab - c0);
    const float* x = a.logits + row * a.logits_stride + c0;
    float v[kBsPer];
#pragma unroll
    for (int j = 0; j < kBsPer; ++j) {                              // issued before the bans are found: the loads fly meanwhile
        const int i = threadIdx.x + j * kBsThreads;
        v[j] = i < len ? x[i] : 0.f;
    }
    chunk_bans(s_ban, a.ban_ids, step.n_ban, a.seq + row * a.seq_stride, step.cur, a.ngram, c0, len);
    __syncthreads();

    unsigned int best = 0u, best_i = threadIdx.x;
#pragma unroll
    for (int j = 0; j < kBsPer; ++j) {
        const int i = threadIdx.x + j * kBsThreads;
        const bool banned = (s_ban[i >> 5] >> (i & 31)) & 1u;
        const unsigned int key = i < len ? beam_key(banned ? -INFINITY : v[j] + 0.0f) : 0u;
        if (key > best) { best = key; best_i = i; }                 // strict: the smaller index stays
    }
    unsigned int hi = best, lo = ~best_i;
    block_argmax(hi, lo, s_red, 0);
    if (threadIdx.x == 0) a.cands[blockIdx.x] = BeamCand{hi, c0 + static_cast<int>(~lo)};
}

__global__ __launch_bounds__(kBsThreads) void greedy_row_kernel(GreedyArgs a) {
    __shared__ unsigned int s_red[2][2 * kBsWaves];
    const GreedyStep step = greedy_step(a);
    if (step.cur < 0) return;                                       // refused: nothing written (greedy_go_on_kernel says so)
    const int64_t b = blockIdx.x;
    int64_t token = step.forced;
    if (step.forced < 0) {
        const BeamCand* cand = a.cands + b * a.chunks;
        unsigned int best = 0u, best_c = threadIdx.x;
        for (int c = threadIdx.x; c < a.chunks; c += kBsThreads) {
            const unsigned int k = cand[c].key;
            if (k > best) { best = k; best_c = c; }
        }
        unsigned int hi = best, lo = ~best_c;
        block_argmax(hi, lo, s_red, 0);                             // hi == 0 cannot be: chunk 0 holds a value
        token = cand[hi ? ~lo : 0u].token;
    }
    if (threadIdx.x != 0) return;
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

__global__ __launch_bounds__(kGaGoThreads) void greedy_go_on_kernel(GreedyArgs a) {
    const GreedyStep step = greedy_step(a);
    if (step.cur < 0) {                                             // refused: the row flags are not this step's
        if (threadIdx.x == 0) *a.go_on = -1;
        return;
    }
    unsigned int any = a.n_eos == 0;
    if (a.n_eos > 0)
        for (int b = threadIdx.x; b < a.bsz; b += kGaGoThreads) any |= a.row_flags[b];
    const bool some = __any(any != 0u);
    if (threadIdx.x == 0) *a.go_on = step.cur + 1 < a.max_length && some;
}

static int64_t greedy_chunks(int64_t vocab) { return (vocab + kBsChunk - 1) / kBsChunk; }

static size_t greedy_workspace_bytes(int64_t bsz, int64_t vocab) {
    if (bsz < 1 || vocab < 1) return 0;
    return static_cast<size_t>(bsz * greedy_chunks(vocab)) * sizeof(BeamCand) + static_cast<size_t>(bsz) * sizeof(unsigned int);
}

}  // namespace osq

using namespace osq;

extern "C" size_t osq_greedy_advance_workspace_bytes(int64_t bsz, int64_t vocab) { return greedy_workspace_bytes(bsz, vocab); }

// Both entry points.  cur_dev == nullptr: the static form at `cur` with n_ban ids and `forced`; else the position is the device
// word, the ids apply below ban_below and the forced tokens fire at their positions.
static int greedy_advance_launch(const float* logits, int64_t logits_stride, int64_t* seq, int64_t seq_stride, int64_t cur,
                                 const int32_t* cur_dev, int64_t cur_add, int64_t ngram, const int64_t* ban_ids, int64_t n_ban,
                                 int64_t ban_below, int64_t forced, int64_t forced_bos, int64_t forced_eos,
                                 const int64_t* eos_ids, int64_t n_eos, int64_t pad, uint8_t* unfinished, int64_t bsz,
                                 int64_t vocab, int64_t max_length, int64_t* next_tokens, int32_t* go_on, void* workspace,
                                 size_t workspace_bytes, osq_stream stream) {
    OSQ_REQUIRE(bsz >= 1 && vocab >= 1 && max_length >= 1, "greedy_advance: a non-positive extent");
    OSQ_REQUIRE(vocab <= INT32_MAX, "greedy_advance: vocab does not fit 31 bits");
    OSQ_REQUIRE(max_length <= kGaMaxLength, "greedy_advance: max_length above 4096");
    OSQ_REQUIRE(cur_dev || (cur >= 1 && cur < max_length), "greedy_advance: cur outside [1, max_length)");
    OSQ_REQUIRE(n_ban >= 0 && n_ban <= kBsMaxBan, "greedy_advance: n_ban outside [0, 16]");
    OSQ_REQUIRE(n_eos >= 0 && n_eos <= kGaMaxEos, "greedy_advance: n_eos outside [0, 16]");
    OSQ_REQUIRE(ngram >= 0, "greedy_advance: negative ngram");
    OSQ_REQUIRE(n_eos == 0 || unfinished, "greedy_advance: n_eos without unfinished");
    OSQ_REQUIRE(n_eos == 0 || eos_ids, "greedy_advance: n_eos without eos_ids");
    OSQ_REQUIRE(n_ban == 0 || ban_ids, "greedy_advance: n_ban without ban_ids");
    // a stored token is an index of the row: what is stored unchecked is checked here (a negative forced id: none)
    OSQ_REQUIRE(forced < vocab && forced_bos < vocab && forced_eos < vocab, "greedy_advance: a forced token outside [0, vocab)");
    OSQ_REQUIRE(n_eos == 0 || (pad >= 0 && pad < vocab), "greedy_advance: pad outside [0, vocab)");
    OSQ_REQUIRE(logits_stride >= vocab, "greedy_advance: logits row stride below vocab");
    OSQ_REQUIRE(!seq || seq_stride >= max_length, "greedy_advance: seq row stride below max_length");
    OSQ_REQUIRE(ngram == 0 || seq, "greedy_advance: ngram without seq");
    const int64_t chunks = greedy_chunks(vocab);
    OSQ_REQUIRE(bsz <= INT32_MAX / chunks, "greedy_advance: too many elements");
    OSQ_REQUIRE(workspace_bytes >= greedy_workspace_bytes(bsz, vocab), "greedy_advance: workspace too small");
    OSQ_REQUIRE(logits && next_tokens && go_on && workspace, "greedy_advance: null tensor");
    OSQ_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7u) == 0, "greedy_advance: workspace not 8-byte aligned");
    const auto id = [](int64_t t) { return static_cast<int>(t < 0 ? -1 : t); };
    BeamCand* cands = static_cast<BeamCand*>(workspace);
    GreedyArgs a{logits, seq, ban_ids, eos_ids, unfinished, next_tokens, go_on, cands,
                 reinterpret_cast<unsigned int*>(cands + bsz * chunks), logits_stride, seq_stride, pad,
                 static_cast<int>(bsz), static_cast<int>(vocab), static_cast<int>(chunks), static_cast<int>(max_length),
                 static_cast<int>(cur), static_cast<int>(ngram > kBsMaxCur ? kBsMaxCur + 1 : ngram), static_cast<int>(n_ban),
                 static_cast<int>(n_eos), id(forced), cur_dev, static_cast<int>(cur_add),
                 static_cast<int>(ban_below < 0 ? 0 : (ban_below > kBsMaxCur ? kBsMaxCur + 1 : ban_below)), id(forced_bos),
                 id(forced_eos)};
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(greedy_chunk_kernel, dim3(static_cast<unsigned>(bsz * chunks)), dim3(kBsThreads), 0, st, a);
    hipLaunchKernelGGL(greedy_row_kernel, dim3(static_cast<unsigned>(bsz)), dim3(kBsThreads), 0, st, a);
    hipLaunchKernelGGL(greedy_go_on_kernel, dim3(1), dim3(kGaGoThreads), 0, st, a);
    return check_launch(cur_dev ? "greedy_advance_at" : "greedy_advance");
}

extern "C" int osq_greedy_advance(const float* logits, int64_t logits_stride, int64_t* seq, int64_t seq_stride, int64_t cur,
                                  int64_t ngram, const int64_t* ban_ids, int64_t n_ban, int64_t forced, const int64_t* eos_ids,
                                  int64_t n_eos, int64_t pad, uint8_t* unfinished, int64_t bsz, int64_t vocab,
                                  int64_t max_length, int64_t* next_tokens, int32_t* go_on, void* workspace,
                                  size_t workspace_bytes, osq_stream stream) {
    return greedy_advance_launch(logits, logits_stride, seq, seq_stride, cur, nullptr, 0, ngram, ban_ids, n_ban, 0, forced, -1,
                                 -1, eos_ids, n_eos, pad, unfinished, bsz, vocab, max_length, next_tokens, go_on, workspace,
                                 workspace_bytes, stream);
}

extern "C" int osq_greedy_advance_at(const float* logits, int64_t logits_stride, int64_t* seq, int64_t seq_stride,
                                     const int32_t* cur_dev, int64_t cur_add, int64_t ngram, const int64_t* ban_ids,
                                     int64_t n_ban, int64_t ban_below, int64_t forced_bos, int64_t forced_eos,
                                     const int64_t* eos_ids, int64_t n_eos, int64_t pad, uint8_t* unfinished, int64_t bsz,
                                     int64_t vocab, int64_t max_length, int64_t* next_tokens, int32_t* go_on, void* workspace,
                                     size_t workspace_bytes, osq_stream stream) {
    OSQ_REQUIRE(cur_dev, "greedy_advance_at: null position word");
    OSQ_REQUIRE(cur_add >= INT32_MIN && cur_add <= INT32_MAX, "greedy_advance_at: cur_add does not fit 32 bits");
    return greedy_advance_launch(logits, logits_stride, seq, seq_stride, 0, cur_dev, cur_add, ngram, ban_ids, n_ban, ban_below,
                                 -1, forced_bos, forced_eos, eos_ids, n_eos, pad, unfinished, bsz, vocab, max_length,
                                 next_tokens, go_on, workspace, workspace_bytes, stream);
}

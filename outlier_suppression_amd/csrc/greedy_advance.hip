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
//
// Only the arg-max is this file's.  The step's arguments, the step read from the position word, the row's pad / eos tail, the
// stopping word and the entry points' shared requirements are advance_step.h's, which the sampling files end with too.
#include <math.h>
#include <hip/hip_runtime.h>
#include "osq_device.h"
#include "osq_host.h"
#include "token_argmax.h"
#include "advance_step.h"

namespace osq {

struct GreedyArgs {
    StepArgs s;
    BeamCand* cands;           // [bsz, chunks]  workspace
};

__global__ __launch_bounds__(kBsThreads) void greedy_chunk_kernel(GreedyArgs a) {
    __shared__ unsigned int s_ban[kBsChunk / 32];
    __shared__ unsigned int s_red[2][2 * kBsWaves];
    const Step step = step_of(a.s);
    if (step.cur < 0 || step.forced >= 0) return;                   // refused, or forced: every logit is ignored
    const int64_t row = blockIdx.x / a.s.chunks;
    const int c = blockIdx.x % a.s.chunks;
    const int c0 = c * kBsChunk;
    const int len = min(kBsChunk, a.s.vocab - c0);
    unsigned int best = 0u, best_i = threadIdx.x;
    chunk_each(a.s.logits + row * a.s.logits_stride + c0, s_ban, a.s.ban_ids, step.n_ban, a.s.seq + row * a.s.seq_stride,
               step.cur, a.s.ngram, c0, len, [&](int, int i, float v, bool banned, bool in) {
                   const unsigned int key = in ? beam_key(banned ? -INFINITY : v + 0.0f) : 0u;
                   if (key > best) { best = key; best_i = i; }      // strict: the smaller index stays
               });
    unsigned int hi = best, lo = ~best_i;
    block_argmax(hi, lo, s_red, 0);
    if (threadIdx.x == 0) a.cands[blockIdx.x] = BeamCand{hi, c0 + static_cast<int>(~lo)};
}

__global__ __launch_bounds__(kBsThreads) void greedy_row_kernel(GreedyArgs a) {
    __shared__ unsigned int s_red[2][2 * kBsWaves];
    const Step step = step_of(a.s);
    if (step.cur < 0) return;                                       // refused: nothing written (greedy_go_on_kernel says so)
    const int64_t b = blockIdx.x;
    int64_t token = step.forced;
    if (step.forced < 0) {
        const BeamCand* cand = a.cands + b * a.s.chunks;
        unsigned int best = 0u, best_c = threadIdx.x;
        for (int c = threadIdx.x; c < a.s.chunks; c += kBsThreads) {
            const unsigned int k = cand[c].key;
            if (k > best) { best = k; best_c = c; }
        }
        unsigned int hi = best, lo = ~best_c;
        block_argmax(hi, lo, s_red, 0);                             // hi == 0 cannot be: chunk 0 holds a value
        token = cand[hi ? ~lo : 0u].token;
    }
    if (threadIdx.x == 0) finish_row(a.s, step, b, token);
}

__global__ __launch_bounds__(kStepGoThreads) void greedy_go_on_kernel(GreedyArgs a) { step_go_on(a.s); }

static size_t greedy_workspace_bytes(int64_t bsz, int64_t vocab) {
    if (bsz < 1 || vocab < 1) return 0;
    return static_cast<size_t>(bsz * step_chunks(vocab)) * sizeof(BeamCand) + static_cast<size_t>(bsz) * sizeof(unsigned int);
}

}  // namespace osq

using namespace osq;

extern "C" size_t osq_greedy_advance_workspace_bytes(int64_t bsz, int64_t vocab) { return greedy_workspace_bytes(bsz, vocab); }

// Both entry points: check, fill, launch.
static int greedy_advance_run(const StepCall& c, osq_stream stream) {
    if (const int rc = step_check("greedy_advance", c)) return rc;
    const int64_t chunks = step_chunks(c.vocab);
    OSQ_REQUIRE(c.bsz <= INT32_MAX / chunks, "greedy_advance: too many elements");
    OSQ_REQUIRE(c.workspace_bytes >= greedy_workspace_bytes(c.bsz, c.vocab), "greedy_advance: workspace too small");
    BeamCand* cands = static_cast<BeamCand*>(c.workspace);
    const GreedyArgs a{step_args(c, chunks, reinterpret_cast<unsigned int*>(cands + c.bsz * chunks)), cands};
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(greedy_chunk_kernel, dim3(static_cast<unsigned>(c.bsz * chunks)), dim3(kBsThreads), 0, st, a);
    hipLaunchKernelGGL(greedy_row_kernel, dim3(static_cast<unsigned>(c.bsz)), dim3(kBsThreads), 0, st, a);
    hipLaunchKernelGGL(greedy_go_on_kernel, dim3(1), dim3(kStepGoThreads), 0, st, a);
    return check_launch(c.cur_dev ? "greedy_advance_at" : "greedy_advance");
}

extern "C" int osq_greedy_advance(const float* logits, int64_t logits_stride, int64_t* seq, int64_t seq_stride, int64_t cur,
                                  int64_t ngram, const int64_t* ban_ids, int64_t n_ban, int64_t forced, const int64_t* eos_ids,
                                  int64_t n_eos, int64_t pad, uint8_t* unfinished, int64_t bsz, int64_t vocab,
                                  int64_t max_length, int64_t* next_tokens, int32_t* go_on, void* workspace,
                                  size_t workspace_bytes, osq_stream stream) {
    return greedy_advance_run({.logits = logits, .logits_stride = logits_stride, .seq = seq, .seq_stride = seq_stride, .cur = cur,
                               .ngram = ngram, .ban_ids = ban_ids, .n_ban = n_ban, .forced = forced, .eos_ids = eos_ids,
                               .n_eos = n_eos, .pad = pad, .unfinished = unfinished, .bsz = bsz, .vocab = vocab,
                               .max_length = max_length, .next_tokens = next_tokens, .go_on = go_on, .workspace = workspace,
                               .workspace_bytes = workspace_bytes}, stream);
}

extern "C" int osq_greedy_advance_at(const float* logits, int64_t logits_stride, int64_t* seq, int64_t seq_stride,
                                     const int32_t* cur_dev, int64_t cur_add, int64_t ngram, const int64_t* ban_ids,
                                     int64_t n_ban, int64_t ban_below, int64_t forced_bos, int64_t forced_eos,
                                     const int64_t* eos_ids, int64_t n_eos, int64_t pad, uint8_t* unfinished, int64_t bsz,
                                     int64_t vocab, int64_t max_length, int64_t* next_tokens, int32_t* go_on, void* workspace,
                                     size_t workspace_bytes, osq_stream stream) {
    OSQ_REQUIRE(cur_dev, "greedy_advance_at: null position word");
    OSQ_REQUIRE(cur_add >= INT32_MIN && cur_add <= INT32_MAX, "greedy_advance_at: cur_add does not fit 32 bits");
    return greedy_advance_run({.logits = logits, .logits_stride = logits_stride, .seq = seq, .seq_stride = seq_stride,
                               .cur_dev = cur_dev, .cur_add = cur_add, .ngram = ngram, .ban_ids = ban_ids, .n_ban = n_ban,
                               .ban_below = ban_below, .forced_bos = forced_bos, .forced_eos = forced_eos, .eos_ids = eos_ids,
                               .n_eos = n_eos, .pad = pad, .unfinished = unfinished, .bsz = bsz, .vocab = vocab,
                               .max_length = max_length, .next_tokens = next_tokens, .go_on = go_on, .workspace = workspace,
                               .workspace_bytes = workspace_bytes}, stream);
}

// The bookkeeping of ONE beam-search step after the selection: which continuations finished, the num_beams that go on, the
// merge into the finished set, the cache rows of the kept beams, the early-stop heuristic and the stopping word.
//
// model/generation.py::_advance_beams_torch issues this as about forty launches on [bsz, 2 * nb]-sized tensors (gathers, isin,
// three topk, four cat, a dozen elementwise ops).  Here, for a step at length `cur` with a prompt of one token:
//
//   launch 1   beam_advance_kernel   one wave-sized workgroup per batch row; everything of the row lives in LDS
//       beam = top_index // vocab, token = top_index % vocab                            keep candidates, lane k
//       hits = cur + 1 >= max_length  |  token in eos_ids
//       trl  = top_value + float(hits) * -1e9                                           (top_running_lp)
//       nxt  = the first nb of trl                                                      -> running, running_scores, beam_idx
//       cand = top_value / len_div; += float(full) * -1e9; += float(!improvable) * -1e9; += float(!just) * -1e9
//       merged = the first nb of (scores | cand)                                        -> finished, scores, finished_len, done
//       improvable &= any(running_scores_out[0] / best_div > where(done_out, min(scores_out), -1e9))
//       a word of three flags per row in the workspace: improvable, all done, all hits
//   launch 2   beam_go_on_kernel     one workgroup: go_on = any(improvable) & !(all(done) & early_stopping) & !all(hits)
//
// No workgroup waits for another: the second launch follows the first on the stream.
//
// Arithmetic: the torch lines, literally.  Every fp32 operation is rounded on its own (-ffp-contract=off), flags are
// multiplied (float(false) * -1e9 is -0.0), the three += on cand happen in the order of the source.  The division by the
// host scalar (a double, as Python holds it) is, with `reciprocal`, v * float(1.0 / div) -- the reciprocal taken in double and
// rounded to fp32 once, what torch's GPU kernel multiplies by -- and without it the correctly rounded v / float(div), torch's
// CPU kernel.  Either scalar is formed on the host by the entry point.
//
// Order of the two top-k: larger value first, equal values (-0.0 equals +0.0) by smaller index, NaN above every number, NaNs
// among themselves by index -- osq_beam_select's rule.  An element's rank is the number of elements that precede it, counted
// in LDS: nb + keep <= 128 elements.
//
// osq_beam_advance_at is the same two launches with the position read by them: cur = *cur_dev + cur_add, one scalar read per
// workgroup, and the two factors read from tables indexed by cur -- entry c the word the static form derives on the host for
// that cur, filled by the host: the launch re-derives no power.  A cur outside [1, max_length) is refused before any address
// is formed from it: the first launch writes nothing, the second writes go_on = -1.
//
// Token rows are copied over all max_length positions, lanes striding over positions; position cur of a continuation is its
// new token.  The gathers read the old state: no output may be its input.
#include <hip/hip_runtime.h>
#include "osq_device.h"
#include "osq_host.h"

namespace osq {

constexpr int kBaThreads = OSQ_WAVE;                 // one wave per batch row
constexpr int kBaMaxKeep = 64, kBaMaxBeams = 64, kBaMaxLength = 4096, kBaMaxEos = 16;
constexpr unsigned int kBaImprovable = 1u, kBaAllDone = 2u, kBaAllHits = 4u;

struct BeamAdvanceArgs {
    const float* top_value;          // [bsz, keep]
    const int64_t* top_index;        // [bsz, keep]
    const int64_t* running;          // [bsz, nb, max_length]
    const float* running_scores;     // [bsz, nb]  (not read: the selection has added it already)
    const int64_t* finished;         // [bsz, nb, max_length]
    const float* scores;             // [bsz, nb]
    const int64_t* finished_len;     // [bsz, nb]
    const uint8_t* done;             // [bsz, nb]
    const uint8_t* improvable;       // [bsz]
    const int64_t* eos_ids;          // n_eos
    int64_t* running_out;
    float* running_scores_out;
    int64_t* finished_out;
    float* scores_out;
    int64_t* finished_len_out;
    uint8_t* done_out;
    uint8_t* improvable_out;
    int64_t* beam_idx;               // [bsz * nb]
    int64_t* next_tokens;            // [bsz * nb]
    int32_t* go_on;                  // 1
    unsigned int* row_flags;         // [bsz]  workspace
    int64_t vocab;
    int bsz, nb, keep, max_length, cur, n_eos, early_stopping, reciprocal;
    float len_scale, best_scale;     // reciprocal: float(1.0 / div), the multiplier; else float(div), the divisor
    // osq_beam_advance_at: cur = *cur_dev + cur_add, read by the launch; the scales are len_table[cur] / best_table[cur]
    const int32_t* cur_dev;          // nullptr: the static form, cur and the scales above
    int cur_add;
    const float* len_table;          // [max_length]
    const float* best_table;         // [max_length]
};

// The position of an _at launch, or -1 when it is refused (outside [1, max_length)): workgroup-uniform, in an SGPR.
__device__ __forceinline__ int beam_advance_position(const BeamAdvanceArgs& a) {
    const long long at = static_cast<long long>(__builtin_amdgcn_readfirstlane(*a.cur_dev)) + a.cur_add;
    return at >= 1 && at < a.max_length ? static_cast<int>(at) : -1;
}

// a before b in the order of the top-k: (value a at index ia, value b at index ib), ia != ib
__device__ __forceinline__ bool beam_before(float a, int ia, float b, int ib) {
    const bool an = a != a, bn = b != b;
    if (an || bn) return an && (!bn || ia < ib);
    return a > b || (a == b && ia < ib);
}

__device__ __forceinline__ float beam_divide(float v, float scale, int reciprocal) {
    return reciprocal ? v * scale : v / scale;
}

__global__ __launch_bounds__(kBaThreads) void beam_advance_kernel(BeamAdvanceArgs a) {
    __shared__ float s_trl[kBaMaxKeep];                         // top_running_lp
    __shared__ float s_cat[kBaMaxBeams + kBaMaxKeep];           // scores | cand
    __shared__ float s_scores_out[kBaMaxBeams];
    __shared__ int64_t s_token[kBaMaxKeep];
    __shared__ int64_t s_eos[kBaMaxEos];
    __shared__ int s_beam[kBaMaxKeep];
    __shared__ int s_nxt[kBaMaxBeams], s_merged[kBaMaxBeams];
    __shared__ unsigned char s_just[kBaMaxKeep];
    const int lane = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int nb = a.nb, keep = a.keep, L = a.max_length;
    int cur = a.cur;
    float len_scale = a.len_scale, best_scale = a.best_scale;
    if (a.cur_dev) {
        cur = beam_advance_position(a);
        if (cur < 0) return;                                    // refused: nothing written (beam_go_on_kernel says so)
        len_scale = a.len_table[cur];
        best_scale = a.best_table[cur];
    }

    if (lane < a.n_eos) s_eos[lane] = a.eos_ids[lane];
    const bool was_done = lane < nb ? a.done[b * nb + lane] != 0 : true;
    const bool full = __all(was_done) && a.early_stopping == 1;
    const bool was_improvable = a.improvable[b] != 0;
    if (lane < nb) s_cat[lane] = a.scores[b * nb + lane];
    __syncthreads();

    // ---- d. the candidates: beam, token, hit; e. top_running_lp; f. cand
    bool hit = true;                                            // lanes past keep do not vote
    if (lane < keep) {
        const float v = a.top_value[b * keep + lane];
        const int64_t idx = a.top_index[b * keep + lane];
        int64_t beam = idx / a.vocab, token = idx - beam * a.vocab;
        if (token < 0) { token += a.vocab; beam -= 1; }         // floor division, as torch's //
        beam = beam < 0 ? 0 : (beam >= nb ? nb - 1 : beam);     // an index outside [0, nb * vocab): no read outside the state
        hit = cur + 1 >= L;
        for (int e = 0; e < a.n_eos; ++e) hit = hit || token == s_eos[e];
        const bool just = hit && lane < nb;
        s_beam[lane] = static_cast<int>(beam);
        s_token[lane] = token;
        s_just[lane] = just;
        s_trl[lane] = v + (hit ? 1.0f : 0.0f) * -1.0e9f;
        float cand = beam_divide(v, len_scale, a.reciprocal);
        cand += (full ? 1.0f : 0.0f) * -1.0e9f;
        cand += (was_improvable ? 0.0f : 1.0f) * -1.0e9f;
        cand += (just ? 0.0f : 1.0f) * -1.0e9f;
        s_cat[nb + lane] = cand;
    }
    const bool all_hits = __all(hit);
    __syncthreads();

    // ---- the ranks: nxt among keep, merged among nb + keep
    if (lane < keep) {
        const float v = s_trl[lane];
        int rank = 0;
        for (int j = 0; j < keep; ++j) rank += j != lane && beam_before(s_trl[j], j, v, lane);
        if (rank < nb) s_nxt[rank] = lane;
    }
    const int n = nb + keep;
    for (int e = lane; e < n; e += kBaThreads) {
        const float v = s_cat[e];
        int rank = 0;
        for (int j = 0; j < n; ++j) rank += j != e && beam_before(s_cat[j], j, v, e);
        if (rank < nb) s_merged[rank] = e;
    }
    __syncthreads();

    // ---- the [bsz, nb] outputs, lane j
    bool now_done = true;
    if (lane < nb) {
        const int k = s_nxt[lane], m = s_merged[lane];
        const int64_t o = b * nb + lane;
        a.running_scores_out[o] = s_trl[k];
        a.beam_idx[o] = s_beam[k] + b * nb;
        a.next_tokens[o] = s_token[k];
        const float so = s_cat[m];
        s_scores_out[lane] = so;
        a.scores_out[o] = so;
        a.finished_len_out[o] = m < nb ? a.finished_len[b * nb + m] : static_cast<int64_t>(cur);
        now_done = m < nb ? a.done[b * nb + m] != 0 : s_just[m - nb] != 0;
        a.done_out[o] = now_done;
    }
    const bool all_done = __all(now_done);
    __syncthreads();

    // ---- the early-stop heuristic
    const float best_running = beam_divide(s_trl[s_nxt[0]], best_scale, a.reciprocal);
    float worst = s_scores_out[0];                              // torch.min: a NaN wins
    for (int j = 1; j < nb; ++j) {
        const float v = s_scores_out[j];
        if (v != v || (worst == worst && v < worst)) worst = v;
    }
    const float worst_done = now_done ? worst : -1.0e9f;
    const bool beats = lane < nb && best_running > worst_done;
    const bool improvable = was_improvable && __any(beats);
    if (lane == 0) {
        a.improvable_out[b] = improvable;
        a.row_flags[b] = (improvable ? kBaImprovable : 0u) | (all_done ? kBaAllDone : 0u) | (all_hits ? kBaAllHits : 0u);
    }

    // ---- the token rows: running <- top_seq[nxt], finished <- (finished | top_seq)[merged]
    for (int j = 0; j < nb; ++j) {
        const int k = s_nxt[j], m = s_merged[j];
        const int64_t* src = a.running + (b * nb + s_beam[k]) * L;
        int64_t* dst = a.running_out + (b * nb + j) * L;
        const int64_t token = s_token[k];
        for (int p = lane; p < L; p += kBaThreads) dst[p] = p == cur ? token : src[p];
        dst = a.finished_out + (b * nb + j) * L;
        if (m < nb) {
            src = a.finished + (b * nb + m) * L;
            for (int p = lane; p < L; p += kBaThreads) dst[p] = src[p];
        } else {
            src = a.running + (b * nb + s_beam[m - nb]) * L;
            const int64_t t = s_token[m - nb];
            for (int p = lane; p < L; p += kBaThreads) dst[p] = p == cur ? t : src[p];
        }
    }
}

__global__ __launch_bounds__(kBaThreads) void beam_go_on_kernel(BeamAdvanceArgs a) {
    if (a.cur_dev && beam_advance_position(a) < 0) {            // refused: the row flags are not this step's
        if (threadIdx.x == 0) *a.go_on = -1;
        return;
    }
    unsigned int any = 0u, all = kBaAllDone | kBaAllHits;
    for (int b = threadIdx.x; b < a.bsz; b += kBaThreads) {
        const unsigned int f = a.row_flags[b];
        any |= f;
        all &= f;
    }
    const bool improvable = __any(any & kBaImprovable);
    const bool all_done = __all(all & kBaAllDone), all_hits = __all(all & kBaAllHits);
    if (threadIdx.x == 0) *a.go_on = improvable && !(all_done && a.early_stopping == 1) && !all_hits;
}

}  // namespace osq

using namespace osq;

// Both entry points.  cur_dev == nullptr: the static form at `cur` with the two divisors; else the position is the device word
// and the factors come from the tables.
static int beam_advance_launch(const float* top_value, const int64_t* top_index, const int64_t* running,
                               const float* running_scores, const int64_t* finished, const float* scores,
                               const int64_t* finished_len, const uint8_t* done, const uint8_t* improvable,
                               const int64_t* eos_ids, int64_t n_eos, int64_t bsz, int64_t nb, int64_t keep, int64_t vocab,
                               int64_t max_length, int64_t cur, const int32_t* cur_dev, int64_t cur_add, int early_stopping,
                               double len_div, double best_div, const float* len_table, const float* best_table,
                               int reciprocal, int64_t* running_out, float* running_scores_out, int64_t* finished_out,
                               float* scores_out, int64_t* finished_len_out, uint8_t* done_out, uint8_t* improvable_out,
                               int64_t* beam_idx, int64_t* next_tokens, int32_t* go_on, void* workspace,
                               size_t workspace_bytes, osq_stream stream) {
    OSQ_REQUIRE(bsz >= 1 && nb >= 1 && keep >= 1 && vocab >= 1 && max_length >= 1, "beam_advance: a non-positive extent");
    OSQ_REQUIRE(keep <= kBaMaxKeep && nb <= kBaMaxBeams, "beam_advance: keep and nb go up to 64");
    OSQ_REQUIRE(nb <= keep, "beam_advance: nb exceeds keep");
    OSQ_REQUIRE(n_eos >= 0 && n_eos <= kBaMaxEos, "beam_advance: n_eos outside [0, 16]");
    OSQ_REQUIRE(max_length <= kBaMaxLength, "beam_advance: max_length above 4096");
    OSQ_REQUIRE(cur_dev || (cur >= 1 && cur < max_length), "beam_advance: cur outside [1, max_length)");
    OSQ_REQUIRE(early_stopping >= 0 && early_stopping <= 2, "beam_advance: early_stopping is 0, 1 or 2");
    OSQ_REQUIRE(bsz <= INT32_MAX / (kBaMaxBeams * 2), "beam_advance: too many batch rows");
    OSQ_REQUIRE(top_value && top_index && running && running_scores && finished && scores && finished_len && done &&
                improvable, "beam_advance: null input");
    OSQ_REQUIRE(running_out && running_scores_out && finished_out && scores_out && finished_len_out && done_out &&
                improvable_out && beam_idx && next_tokens && go_on && workspace, "beam_advance: null output");
    OSQ_REQUIRE(n_eos == 0 || eos_ids, "beam_advance: n_eos without eos_ids");
    OSQ_REQUIRE(running_out != running && running_scores_out != running_scores && finished_out != finished &&
                scores_out != scores && finished_len_out != finished_len && done_out != done && improvable_out != improvable,
                "beam_advance: an output is its input (the gathers read the old state)");
    OSQ_REQUIRE(workspace_bytes >= static_cast<size_t>(bsz) * sizeof(unsigned int), "beam_advance: workspace too small");
    OSQ_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 3u) == 0, "beam_advance: workspace not 4-byte aligned");
    BeamAdvanceArgs a{top_value, top_index, running, running_scores, finished, scores, finished_len, done, improvable,
                      eos_ids, running_out, running_scores_out, finished_out, scores_out, finished_len_out, done_out,
                      improvable_out, beam_idx, next_tokens, go_on, static_cast<unsigned int*>(workspace), vocab,
                      static_cast<int>(bsz), static_cast<int>(nb), static_cast<int>(keep), static_cast<int>(max_length),
                      static_cast<int>(cur), static_cast<int>(n_eos), early_stopping, reciprocal != 0,
                      cur_dev ? 0.f : static_cast<float>(reciprocal ? 1.0 / len_div : len_div),
                      cur_dev ? 0.f : static_cast<float>(reciprocal ? 1.0 / best_div : best_div),
                      cur_dev, static_cast<int>(cur_add), len_table, best_table};
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(beam_advance_kernel, dim3(static_cast<unsigned>(bsz)), dim3(kBaThreads), 0, st, a);
    hipLaunchKernelGGL(beam_go_on_kernel, dim3(1), dim3(kBaThreads), 0, st, a);
    return check_launch(cur_dev ? "beam_advance_at" : "beam_advance");
}

extern "C" int osq_beam_advance(const float* top_value, const int64_t* top_index, const int64_t* running,
                                const float* running_scores, const int64_t* finished, const float* scores,
                                const int64_t* finished_len, const uint8_t* done, const uint8_t* improvable,
                                const int64_t* eos_ids, int64_t n_eos, int64_t bsz, int64_t nb, int64_t keep, int64_t vocab,
                                int64_t max_length, int64_t cur, int early_stopping, double len_div, double best_div,
                                int reciprocal, int64_t* running_out, float* running_scores_out, int64_t* finished_out,
                                float* scores_out, int64_t* finished_len_out, uint8_t* done_out, uint8_t* improvable_out,
                                int64_t* beam_idx, int64_t* next_tokens, int32_t* go_on, void* workspace,
                                size_t workspace_bytes, osq_stream stream) {
    return beam_advance_launch(top_value, top_index, running, running_scores, finished, scores, finished_len, done, improvable,
                               eos_ids, n_eos, bsz, nb, keep, vocab, max_length, cur, nullptr, 0, early_stopping, len_div,
                               best_div, nullptr, nullptr, reciprocal, running_out, running_scores_out, finished_out,
                               scores_out, finished_len_out, done_out, improvable_out, beam_idx, next_tokens, go_on,
                               workspace, workspace_bytes, stream);
}

extern "C" int osq_beam_advance_at(const float* top_value, const int64_t* top_index, const int64_t* running,
                                   const float* running_scores, const int64_t* finished, const float* scores,
                                   const int64_t* finished_len, const uint8_t* done, const uint8_t* improvable,
                                   const int64_t* eos_ids, int64_t n_eos, int64_t bsz, int64_t nb, int64_t keep,
                                   int64_t vocab, int64_t max_length, const int32_t* cur_dev, int64_t cur_add,
                                   int early_stopping, const float* len_table, const float* best_table, int reciprocal,
                                   int64_t* running_out, float* running_scores_out, int64_t* finished_out, float* scores_out,
                                   int64_t* finished_len_out, uint8_t* done_out, uint8_t* improvable_out, int64_t* beam_idx,
                                   int64_t* next_tokens, int32_t* go_on, void* workspace, size_t workspace_bytes,
                                   osq_stream stream) {
    OSQ_REQUIRE(cur_dev && len_table && best_table, "beam_advance_at: null position word or table");
    OSQ_REQUIRE(cur_add >= INT32_MIN && cur_add <= INT32_MAX, "beam_advance_at: cur_add does not fit 32 bits");
    return beam_advance_launch(top_value, top_index, running, running_scores, finished, scores, finished_len, done, improvable,
                               eos_ids, n_eos, bsz, nb, keep, vocab, max_length, 0, cur_dev, cur_add, early_stopping, 1.0, 1.0,
                               len_table, best_table, reciprocal, running_out, running_scores_out, finished_out, scores_out,
                               finished_len_out, done_out, improvable_out, beam_idx, next_tokens, go_on, workspace,
                               workspace_bytes, stream);
}

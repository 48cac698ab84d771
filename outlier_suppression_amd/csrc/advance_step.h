// What greedy_advance.hip, sample_advance.hip and sample_nucleus.hip share -- everything of a decoding step that is not the
// choice of the token.  Device: the arguments of a step, the step a launch reads from the position word, and the two tails
// every form ends with -- the row's pad / eos lines with its stores, and the stopping word.  Host: the arguments of the six
// entry points by name, their shared requirements, and the mapping of the one onto the other.
#pragma once
#include <hip/hip_runtime.h>
#include "osq_device.h"
#include "osq_host.h"
#include "token_argmax.h"

namespace osq {

constexpr int kStepMaxLength = kBsMaxCur, kStepMaxEos = 16;
constexpr int kStepGoThreads = OSQ_WAVE;             // rows one trip of the go_on reduction covers

struct StepArgs {
    const float* logits;       // bsz x vocab, rows logits_stride floats apart
    int64_t* seq;              // bsz x max_length, rows seq_stride apart: [0, cur) read with ngram > 0, [cur] written
    const int64_t* ban_ids;    // n_ban ids banned in every row
    const int64_t* eos_ids;    // n_eos ids that finish a row
    uint8_t* unfinished;       // [bsz]; touched only with n_eos > 0
    int64_t* next_tokens;      // [bsz]
    int32_t* go_on;            // 1
    unsigned int* row_flags;   // [bsz]          workspace: the row is unfinished after this step
    int64_t logits_stride, seq_stride;
    int64_t pad;
    int bsz, vocab, chunks, max_length, cur, ngram, n_ban, n_eos;
    int forced;                // static form: >= 0 is this step's token
    // the _at forms: cur = *cur_dev + cur_add, read by the launches
    const int32_t* cur_dev;    // nullptr: the static form, cur / n_ban / forced above
    int cur_add, ban_below, forced_bos, forced_eos;
};

struct Step {                  // what a launch knows of its step: workgroup-uniform
    int cur;                   // -1: refused
    int n_ban, forced;
};

__device__ __forceinline__ Step step_of(const StepArgs& a) {
    if (!a.cur_dev) return Step{a.cur, a.n_ban, a.forced};
    const long long at = static_cast<long long>(__builtin_amdgcn_readfirstlane(*a.cur_dev)) + a.cur_add;
    if (at < 1 || at >= a.max_length) return Step{-1, 0, -1};
    const int cur = static_cast<int>(at);
    int forced = cur == 1 ? a.forced_bos : -1;
    if (cur == a.max_length - 1 && a.forced_eos >= 0) forced = a.forced_eos;
    return Step{cur, cur < a.ban_below ? a.n_ban : 0, forced};
}

// The end of row b in one thread: the pad of a finished row, the eos test, seq[b, cur], next_tokens[b] and the row's flag.
// True where the row was finished before this step: its token is the pad.
__device__ __forceinline__ bool finish_row(const StepArgs& a, const Step& step, int64_t b, int64_t token) {
    unsigned int unfinished = 1u;
    bool padded = false;
    if (a.n_eos > 0) {
        unfinished = a.unfinished[b] != 0;
        padded = !unfinished;
        if (!unfinished) token = a.pad;
        for (int e = 0; e < a.n_eos; ++e) unfinished &= token != a.eos_ids[e];
        a.unfinished[b] = static_cast<uint8_t>(unfinished);
    }
    if (a.seq) a.seq[b * a.seq_stride + step.cur] = token;
    a.next_tokens[b] = token;
    a.row_flags[b] = unfinished;
    return padded;
}

// The stopping word, by one wave of kStepGoThreads: go_on = (cur + 1 < max_length) && (n_eos == 0 || any row unfinished); -1
// for a refused position.
__device__ __forceinline__ void step_go_on(const StepArgs& a) {
    const Step step = step_of(a);
    if (step.cur < 0) {                                             // refused: the row flags are not this step's
        if (threadIdx.x == 0) *a.go_on = -1;
        return;
    }
    unsigned int any = a.n_eos == 0;
    if (a.n_eos > 0)
        for (int b = threadIdx.x; b < a.bsz; b += kStepGoThreads) any |= a.row_flags[b];
    const bool some = __any(any != 0u);
    if (threadIdx.x == 0) *a.go_on = step.cur + 1 < a.max_length && some;
}

static inline int64_t step_chunks(int64_t vocab) { return (vocab + kBsChunk - 1) / kBsChunk; }

// The parameters the six entry points have in common, by name.  The static forms leave cur_dev null and take cur, n_ban ids
// and `forced`; the _at forms give the position word, the ids apply below ban_below and the forced tokens fire at their
// positions.
struct StepCall {
    const float* logits;
    int64_t logits_stride;
    int64_t* seq;
    int64_t seq_stride;
    int64_t cur = 0;
    const int32_t* cur_dev = nullptr;
    int64_t cur_add = 0;
    int64_t ngram;
    const int64_t* ban_ids;
    int64_t n_ban;
    int64_t ban_below = 0, forced = -1, forced_bos = -1, forced_eos = -1;
    const int64_t* eos_ids;
    int64_t n_eos, pad;
    uint8_t* unfinished;
    int64_t bsz, vocab, max_length;
    int64_t* next_tokens;
    int32_t* go_on;
    void* workspace;
    size_t workspace_bytes;
};

// What every family requires of a call; `what` is the family's name in the error text.  The workspace's size is the family's.
static inline int step_check(const char* what, const StepCall& c) {
#define OSQ_STEP_REQUIRE(cond, msg)                  \
    do {                                             \
        if (!(cond)) {                               \
            set_error("%s: %s", what, msg);          \
            return OSQ_ERR_INVALID_ARGUMENT;         \
        }                                            \
    } while (0)
    OSQ_STEP_REQUIRE(c.bsz >= 1 && c.vocab >= 1 && c.max_length >= 1, "a non-positive extent");
    OSQ_STEP_REQUIRE(c.vocab <= INT32_MAX, "vocab does not fit 31 bits");
    OSQ_STEP_REQUIRE(c.max_length <= kStepMaxLength, "max_length above 4096");
    OSQ_STEP_REQUIRE(c.cur_dev || (c.cur >= 1 && c.cur < c.max_length), "cur outside [1, max_length)");
    OSQ_STEP_REQUIRE(c.n_ban >= 0 && c.n_ban <= kBsMaxBan, "n_ban outside [0, 16]");
    OSQ_STEP_REQUIRE(c.n_eos >= 0 && c.n_eos <= kStepMaxEos, "n_eos outside [0, 16]");
    OSQ_STEP_REQUIRE(c.ngram >= 0, "negative ngram");
    OSQ_STEP_REQUIRE(c.n_eos == 0 || c.unfinished, "n_eos without unfinished");
    OSQ_STEP_REQUIRE(c.n_eos == 0 || c.eos_ids, "n_eos without eos_ids");
    OSQ_STEP_REQUIRE(c.n_ban == 0 || c.ban_ids, "n_ban without ban_ids");
    // a stored token is an index of the row: what is stored unchecked is checked here (a negative forced id: none)
    OSQ_STEP_REQUIRE(c.forced < c.vocab && c.forced_bos < c.vocab && c.forced_eos < c.vocab, "a forced token outside [0, vocab)");
    OSQ_STEP_REQUIRE(c.n_eos == 0 || (c.pad >= 0 && c.pad < c.vocab), "pad outside [0, vocab)");
    OSQ_STEP_REQUIRE(c.logits_stride >= c.vocab, "logits row stride below vocab");
    OSQ_STEP_REQUIRE(!c.seq || c.seq_stride >= c.max_length, "seq row stride below max_length");
    OSQ_STEP_REQUIRE(c.ngram == 0 || c.seq, "ngram without seq");
    OSQ_STEP_REQUIRE(c.logits && c.next_tokens && c.go_on && c.workspace, "null tensor");
    OSQ_STEP_REQUIRE((reinterpret_cast<uintptr_t>(c.workspace) & 7u) == 0, "workspace not 8-byte aligned");
#undef OSQ_STEP_REQUIRE
    return OSQ_OK;
}

// The device's arguments of a checked call over `chunks` chunks a row: a negative forced id is -1, and ngram and ban_below,
// which only compare with a position, stop just above the longest one.
static inline StepArgs step_args(const StepCall& c, int64_t chunks, unsigned int* row_flags) {
    const auto id = [](int64_t t) { return static_cast<int>(t < 0 ? -1 : t); };
    const auto position = [](int64_t p) { return static_cast<int>(p < 0 ? 0 : (p > kBsMaxCur ? kBsMaxCur + 1 : p)); };
    return StepArgs{.logits = c.logits, .seq = c.seq, .ban_ids = c.ban_ids, .eos_ids = c.eos_ids, .unfinished = c.unfinished,
                    .next_tokens = c.next_tokens, .go_on = c.go_on, .row_flags = row_flags, .logits_stride = c.logits_stride,
                    .seq_stride = c.seq_stride, .pad = c.pad, .bsz = static_cast<int>(c.bsz), .vocab = static_cast<int>(c.vocab),
                    .chunks = static_cast<int>(chunks), .max_length = static_cast<int>(c.max_length),
                    .cur = static_cast<int>(c.cur), .ngram = position(c.ngram), .n_ban = static_cast<int>(c.n_ban),
                    .n_eos = static_cast<int>(c.n_eos), .forced = id(c.forced), .cur_dev = c.cur_dev,
                    .cur_add = static_cast<int>(c.cur_add), .ban_below = position(c.ban_below), .forced_bos = id(c.forced_bos),
                    .forced_eos = id(c.forced_eos)};
}

}  // namespace osq

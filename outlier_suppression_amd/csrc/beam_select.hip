// The continuations of ONE beam-search step: log-softmax, the banned tokens, the running beam scores and the top `keep` of
// every batch row, in three small launches that write nothing of the logits' size.
//
// model/generation.py::_beam_search runs, per step, log_softmax over [rows, vocab] logits, one clone / masked_fill per
// logits processor, the add of the running scores and torch.topk over [bsz, nb * vocab]: eight to ten passes over the
// logits for bsz * keep numbers.  Here, with rows = bsz * nb and a row cut into chunks of kBsChunk tokens:
//
//     value(b, j, t) = ((x - m) - L) + running[b, j]      m = max_t x,  L = log(sum_t exp(x - m)), row r = b * nb + j;
//                      -inf + running[b, j]               when t is banned in row r
//
//   launch 1   beam_partials_kernel   one workgroup per (row, chunk): the chunk's maximum m_c and sum_t exp(x - m_c)
//   launch 2   beam_chunk_kernel      one workgroup per (row, chunk): m and L from the row's partials in chunk order (every
//                                     workgroup of a row forms the same two words), the chunk's ban bitmap in LDS, the
//                                     chunk's values in registers (16 per thread), then `keep` rounds of a workgroup arg-max:
//                                     the chunk's first `keep` candidates (value key, token) go to the workspace
//   launch 3   beam_merge_kernel      one workgroup per batch row: `keep` rounds of the same arg-max over the row's
//                                     nb * chunks * keep candidates
//
// Order: larger value first, equal values by smaller flat index beam * vocab + token, NaN above every number.  A candidate
// is the 64-bit key (ordered_bits(value) with every NaN as 0xffffffff, ~position): the arg-max is a max of keys.  Within a
// chunk the position is the token; in the merge it is the candidate's slot (beam, chunk, rank), which among equal values
// runs as the flat index does.  Key 0 is no value's (-inf has 0x007fffff): it marks a taken or absent candidate.
// A value is never -0.0 ((x - m) - L is +0.0 where it vanishes, and a + (-a) is +0.0), so equal values have equal keys.
//
// osq_beam_select_at is the same three launches with the position read by the second: cur = *cur_dev + cur_add, one scalar
// read per workgroup of beam_chunk_kernel (the only kernel that uses the position), so that a captured graph of the call
// serves every step.  ban_ids then apply while cur < ban_below, the min-length rule the host decides for the static form.
// A cur outside [0, cur_max] is refused before any address is formed from it: every candidate of the row becomes (NaN, token
// 0), so the merge writes the canonical NaN and index 0 everywhere, and seq is not read.
//
// Summation order, fixed by (vocab) alone -- not by the row's alignment or place, bsz or nb; no float atomics: thread t of a
// chunk's workgroup adds exp of elements t, t + 256, ... in order, wave_sum_f32, then (w0 + w1) + (w2 + w3); the row sum is
// sum_c s_c * exp(m_c - m) in chunk order.  Elements are loaded one 32-bit word per lane (a row of an odd vocab is only
// 4-byte aligned and the order above must not depend on where a row starts), 16 loads in flight per lane.
#include <math.h>
#include <hip/hip_runtime.h>
#include "osq_device.h"
#include "osq_host.h"
#include "token_argmax.h"

namespace osq {

constexpr int kBsMaxKeep = 64, kBsMaxBeams = 64;

struct BeamArgs {
    const float* logits;       // rows x vocab, rows logits_stride floats apart
    const float* running;      // [bsz, nb]
    const int64_t* seq;        // rows x >= cur, rows seq_stride apart; read only with ngram > 0
    const int64_t* ban_ids;    // n_ban ids banned in every row
    float2* partials;          // [rows, chunks] (m_c, s_c)
    BeamCand* cands;           // [rows, chunks, keep]
    float* top_value;          // [bsz, keep]
    int64_t* top_index;        // [bsz, keep]
    int64_t logits_stride, seq_stride;
    int nb, vocab, keep, chunks, cur, ngram, n_ban;
    // osq_beam_select_at: cur = *cur_dev + cur_add, read by the launch; outside [0, cur_max] -> NaN candidates, seq not read
    const int32_t* cur_dev;    // nullptr: the static form, cur above
    int cur_add, cur_max, ban_below;
};

__global__ __launch_bounds__(kBsThreads) void beam_partials_kernel(BeamArgs a) {
    __shared__ float s_red[2][kBsWaves];
    const int lane = threadIdx.x & (OSQ_WAVE - 1), w = threadIdx.x / OSQ_WAVE;
    const int64_t row = blockIdx.x / a.chunks;
    const int c = blockIdx.x % a.chunks;
    const int c0 = c * kBsChunk;
    const int len = min(kBsChunk, a.vocab - c0);
    const float* x = a.logits + row * a.logits_stride + c0;
    float v[kBsPer];
#pragma unroll
    for (int j = 0; j < kBsPer; ++j) {
        const int i = threadIdx.x + j * kBsThreads;
        v[j] = i < len ? x[i] : -INFINITY;
    }
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < kBsPer; ++j) mx = fmaxf(mx, v[j]);          // fmaxf drops a NaN: its exp makes the sum NaN
    mx = wave_max(mx);
    if (lane == 0) s_red[0][w] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(s_red[0][0], s_red[0][1]), fmaxf(s_red[0][2], s_red[0][3]));
    const float base = mx == -INFINITY ? 0.f : mx;                  // a chunk of -inf only: its sum is 0, not exp(-inf + inf)
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < kBsPer; ++j) {
        const int i = threadIdx.x + j * kBsThreads;
        if (i < len) sum += expf(v[j] - base);
    }
    sum = wave_sum_f32(sum);
    if (lane == 0) s_red[1][w] = sum;
    __syncthreads();
    if (threadIdx.x == 0)
        a.partials[blockIdx.x] = make_float2(mx, (s_red[1][0] + s_red[1][1]) + (s_red[1][2] + s_red[1][3]));
}

__global__ __launch_bounds__(kBsThreads) void beam_chunk_kernel(BeamArgs a) {
    __shared__ unsigned int s_ban[kBsChunk / 32];
    __shared__ unsigned int s_red[2][2 * kBsWaves];
    const int64_t row = blockIdx.x / a.chunks;
    const int c = blockIdx.x % a.chunks;
    const int c0 = c * kBsChunk;
    const int len = min(kBsChunk, a.vocab - c0);
    const float* x = a.logits + row * a.logits_stride + c0;
    float v[kBsPer];
#pragma unroll
    for (int j = 0; j < kBsPer; ++j) {                              // issued first: the loads fly while the bans are found
        const int i = threadIdx.x + j * kBsThreads;
        v[j] = i < len ? x[i] : 0.f;
    }

    int cur = a.cur, n_ban = a.n_ban;
    if (a.cur_dev) {                                                // workgroup-uniform: the position is a device word, read once into an SGPR
        const long long at = static_cast<long long>(__builtin_amdgcn_readfirstlane(*a.cur_dev)) + a.cur_add;
        if (at < 0 || at > a.cur_max) {                             // refused: NaN candidates with token 0, nothing else read
            if (threadIdx.x < a.keep) a.cands[static_cast<int64_t>(blockIdx.x) * a.keep + threadIdx.x] = BeamCand{0xffffffffu, 0};
            return;
        }
        cur = static_cast<int>(at);
        if (cur >= a.ban_below) n_ban = 0;
    }

    // ---- the chunk's banned tokens
    chunk_bans(s_ban, a.ban_ids, n_ban, a.seq + row * a.seq_stride, cur, a.ngram, c0, len);

    // ---- m and L of the row: the same words in every workgroup of the row
    const float2* part = a.partials + row * a.chunks;
    float m = -INFINITY;
    for (int k = 0; k < a.chunks; ++k) m = fmaxf(m, part[k].x);
    float total = 0.f;
    for (int k = 0; k < a.chunks; ++k) {
        const float2 p = part[k];
        total += p.y * expf(p.x - m);
    }
    const float L = logf(total);
    const float run = a.running[row];
    __syncthreads();

    // ---- the keys of this thread's elements; the best of them
    unsigned int key[kBsPer];
#pragma unroll
    for (int j = 0; j < kBsPer; ++j) {
        const int i = threadIdx.x + j * kBsThreads;
        const bool banned = (s_ban[i >> 5] >> (i & 31)) & 1u;
        const float lp = banned ? -INFINITY : (v[j] - m) - L;
        key[j] = i < len ? beam_key(lp + run) : 0u;
    }
    BeamCand* out = a.cands + static_cast<int64_t>(blockIdx.x) * a.keep;
    unsigned int best = 0u, best_i = threadIdx.x;
#pragma unroll
    for (int j = 0; j < kBsPer; ++j)
        if (key[j] > best) { best = key[j]; best_i = threadIdx.x + j * kBsThreads; }      // strict: the smaller index stays
    for (int r = 0; r < a.keep; ++r) {
        unsigned int hi = best, lo = ~best_i;
        block_argmax(hi, lo, s_red, r & 1);
        const unsigned int i = ~lo;
        if (threadIdx.x == 0) out[r] = BeamCand{hi, hi ? c0 + static_cast<int>(i) : -1};
        if ((i & (kBsThreads - 1)) == threadIdx.x) {                // the owner takes it out and looks again
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

__global__ __launch_bounds__(kBsThreads) void beam_merge_kernel(BeamArgs a) {
    __shared__ unsigned int s_red[2][2 * kBsWaves];
    const int64_t b = blockIdx.x;
    const int per_beam = a.chunks * a.keep;
    const int n = a.nb * per_beam;                                  // candidates of this batch row, in flat-index order of ties
    BeamCand* cand = a.cands + b * n;
    unsigned int best = 0u, best_p = threadIdx.x;
    for (int p = threadIdx.x; p < n; p += kBsThreads) {
        const unsigned int k = cand[p].key;
        if (k > best) { best = k; best_p = p; }
    }
    for (int r = 0; r < a.keep; ++r) {
        unsigned int hi = best, lo = ~best_p;
        block_argmax(hi, lo, s_red, r & 1);
        const unsigned int p = ~lo;
        if ((p & (kBsThreads - 1)) == threadIdx.x) {                // the owner writes it, takes it out and looks again
            const int token = hi ? cand[p].token : 0;               // hi == 0 cannot be: keep <= vocab candidates exist
            a.top_value[b * a.keep + r] = beam_value(hi);
            a.top_index[b * a.keep + r] = static_cast<int64_t>(p / per_beam) * a.vocab + token;
            if (hi) cand[p].key = 0u;
            best = 0u;
            best_p = threadIdx.x;
            for (int q = threadIdx.x; q < n; q += kBsThreads) {
                const unsigned int k = cand[q].key;
                if (k > best) { best = k; best_p = q; }
            }
        }
    }
}

static int64_t beam_chunks(int64_t vocab) { return (vocab + kBsChunk - 1) / kBsChunk; }

static size_t beam_workspace_bytes(int64_t bsz, int64_t nb, int64_t vocab, int64_t keep) {
    if (bsz < 0 || nb < 1 || vocab < 1 || keep < 1) return 0;
    const int64_t slots = bsz * nb * beam_chunks(vocab);
    return static_cast<size_t>(slots) * sizeof(float2) + static_cast<size_t>(slots * keep) * sizeof(BeamCand);
}

}  // namespace osq

using namespace osq;

extern "C" size_t osq_beam_select_workspace_bytes(int64_t bsz, int64_t nb, int64_t vocab, int64_t keep) {
    return beam_workspace_bytes(bsz, nb, vocab, keep);
}

// Both entry points.  cur_dev == nullptr: the static form at `cur`; else the position is the device word and `cur` is cur_max,
// the largest position the launch may meet: the host checks go by it.
static int beam_select_launch(const float* logits, int64_t logits_stride, const float* running_scores, const int64_t* seq,
                              int64_t seq_stride, int64_t cur, const int32_t* cur_dev, int64_t cur_add, int64_t ban_below,
                              int64_t ngram, const int64_t* ban_ids, int64_t n_ban, int64_t bsz, int64_t nb, int64_t vocab,
                              int64_t keep, float* top_value, int64_t* top_index, void* workspace, size_t workspace_bytes,
                              osq_stream stream) {
    OSQ_REQUIRE(bsz >= 0 && nb >= 1 && vocab >= 1 && keep >= 1, "beam_select: bad shape");
    OSQ_REQUIRE(keep <= kBsMaxKeep && nb <= kBsMaxBeams, "beam_select: keep and nb go up to 64");
    OSQ_REQUIRE(keep <= vocab, "beam_select: keep exceeds vocab");
    OSQ_REQUIRE(cur >= 0 && cur <= kBsMaxCur, "beam_select: cur outside [0, 4096]");
    OSQ_REQUIRE(n_ban >= 0 && n_ban <= kBsMaxBan, "beam_select: n_ban outside [0, 16]");
    OSQ_REQUIRE(ngram >= 0, "beam_select: negative ngram");
    OSQ_REQUIRE(logits_stride >= vocab, "beam_select: logits row stride below vocab");
    const int64_t chunks = beam_chunks(vocab);
    OSQ_REQUIRE(vocab <= INT32_MAX - kBsChunk && bsz * nb * chunks * keep <= INT32_MAX, "beam_select: too many elements");
    OSQ_REQUIRE(workspace_bytes >= beam_workspace_bytes(bsz, nb, vocab, keep), "beam_select: workspace too small");
    const bool windows = ngram > 0 && cur >= ngram;                 // else seq is not read
    OSQ_REQUIRE(!windows || seq_stride >= cur, "beam_select: seq row stride below cur");
    if (bsz == 0) return OSQ_OK;
    OSQ_REQUIRE(logits && running_scores && top_value && top_index && workspace, "beam_select: null tensor");
    OSQ_REQUIRE(!windows || seq, "beam_select: ngram without seq");
    OSQ_REQUIRE(n_ban == 0 || ban_ids, "beam_select: n_ban without ban_ids");
    OSQ_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7u) == 0, "beam_select: workspace not 8-byte aligned");
    const int64_t rows = bsz * nb;
    float2* partials = static_cast<float2*>(workspace);
    BeamArgs a{logits, running_scores, seq, ban_ids, partials, reinterpret_cast<BeamCand*>(partials + rows * chunks),
               top_value, top_index, logits_stride, seq_stride, static_cast<int>(nb), static_cast<int>(vocab),
               static_cast<int>(keep), static_cast<int>(chunks), static_cast<int>(cur),
               static_cast<int>(ngram > kBsMaxCur ? kBsMaxCur + 1 : ngram), static_cast<int>(n_ban),
               cur_dev, static_cast<int>(cur_add), static_cast<int>(cur),
               static_cast<int>(ban_below < 0 ? 0 : (ban_below > kBsMaxCur ? kBsMaxCur + 1 : ban_below))};
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(static_cast<unsigned>(rows * chunks));
    hipLaunchKernelGGL(beam_partials_kernel, grid, dim3(kBsThreads), 0, st, a);
    hipLaunchKernelGGL(beam_chunk_kernel, grid, dim3(kBsThreads), 0, st, a);
    hipLaunchKernelGGL(beam_merge_kernel, dim3(static_cast<unsigned>(bsz)), dim3(kBsThreads), 0, st, a);
    return check_launch(cur_dev ? "beam_select_at" : "beam_select");
}

extern "C" int osq_beam_select(const float* logits, int64_t logits_stride, const float* running_scores, const int64_t* seq,
                               int64_t seq_stride, int64_t cur, int64_t ngram, const int64_t* ban_ids, int64_t n_ban,
                               int64_t bsz, int64_t nb, int64_t vocab, int64_t keep, float* top_value, int64_t* top_index,
                               void* workspace, size_t workspace_bytes, osq_stream stream) {
    return beam_select_launch(logits, logits_stride, running_scores, seq, seq_stride, cur, nullptr, 0, 0, ngram, ban_ids, n_ban,
                              bsz, nb, vocab, keep, top_value, top_index, workspace, workspace_bytes, stream);
}

extern "C" int osq_beam_select_at(const float* logits, int64_t logits_stride, const float* running_scores, const int64_t* seq,
                                  int64_t seq_stride, const int32_t* cur_dev, int64_t cur_add, int64_t cur_max, int64_t ngram,
                                  const int64_t* ban_ids, int64_t n_ban, int64_t ban_below, int64_t bsz, int64_t nb,
                                  int64_t vocab, int64_t keep, float* top_value, int64_t* top_index, void* workspace,
                                  size_t workspace_bytes, osq_stream stream) {
    OSQ_REQUIRE(cur_dev, "beam_select_at: null position word");
    OSQ_REQUIRE(cur_add >= INT32_MIN && cur_add <= INT32_MAX, "beam_select_at: cur_add does not fit 32 bits");
    return beam_select_launch(logits, logits_stride, running_scores, seq, seq_stride, cur_max, cur_dev, cur_add, ban_below, ngram,
                              ban_ids, n_ban, bsz, nb, vocab, keep, top_value, top_index, workspace, workspace_bytes, stream);
}

// Teacher-forced scoring: the log-probability of a GIVEN token per row of logits, the language-model loss over the rows, and
// the gradient of either for the logits (include/osq_hip.h, "teacher-forced scoring", states the rule and every order).
//
//   launch 1   token_logprob_chunk_kernel     one workgroup per (row, chunk of kBsChunk tokens), the layout of
//                                             sample_chunk_kernel: the chunk in registers (16 per thread), the workgroup's
//                                             maximum m_c, each thread's sum of expf(z - m_c), the fixed-order workgroup sum
//                                             W_c; (m_c, W_c) to the workspace
//   launch 2   token_logprob_row_kernel       one THREAD per row: m and W from the row's partials in chunk order, the label's
//                                             logit read once more, logprob[r] and lse[r]
//   launch 3   token_logprob_tail_kernel      one workgroup: the sum of the rows' words in an order fixed by `rows`, the counts
//                                             of scored and bad rows, loss = -sum / scored
//   backward   token_logprob_backward_kernel  one workgroup per (row, chunk): coef_r * (p - [v == t]), p = expf(z - lse[r]),
//                                             divided by the workgroup's own sum of them where the row is one chunk
//
// No workgroup waits for another: the launches follow each other on the stream.  No atomics on device memory.
//
// Thread i holds the chunk's tokens 4 (i + 256 k) + e, k and e in 0..3: four 128-bit accesses, consecutive lanes on
// consecutive quads.  A row of an odd stride is only 4-byte aligned, and which thread adds which token must not follow the
// row's alignment (the order of W is fixed by vocab alone), so the quads are not peeled to a 16-byte boundary: they are
// accessed as 128-bit words of 4-byte alignment, which global memory instructions take (dword alignment is all a dwordx4
// access needs); a quad that crosses the row's end is accessed token by token, so nothing outside the row is touched.
#include <math.h>
#include <hip/hip_runtime.h>
#include "osq_device.h"
#include "osq_host.h"
#include "token_argmax.h"

namespace osq {

constexpr int kTlQuads = kBsPer / 4;
typedef float tl_quad __attribute__((ext_vector_type(4), aligned(4)));

struct TokenLogprobArgs {
    const float* logits;
    int64_t stride;
    const int64_t* labels;
    int64_t rows;
    int vocab, chunks;
    int64_t ignore_index;
    float* logprob;
    float* lse;
    float* loss;               // nullptr: not wanted
    int64_t* counts;           // nullptr: not wanted
    float2* partials;          // [rows, chunks] (m_c, W_c)
};

struct TokenLogprobBackwardArgs {
    const float* logits;
    int64_t stride;
    const int64_t* labels;
    const float* lse;
    const float* row_grad;     // nullptr: coef = scalar_grad[0] / counts[0]
    const float* scalar_grad;
    const int64_t* counts;
    int vocab, chunks;
    int64_t ignore_index;
    float* dlogits;
    int64_t dstride;
};

// The thread's 16 tokens of the chunk [x, x + len): v[4 k + e] = x[4 (threadIdx.x + 256 k) + e], `past` beyond the chunk.
__device__ __forceinline__ void tl_load_chunk(const float* x, int len, float past, float (&v)[kBsPer]) {
#pragma unroll
    for (int k = 0; k < kTlQuads; ++k) {
        const int i = 4 * (threadIdx.x + k * kBsThreads);
        if (i + 3 < len) {
            const tl_quad q = *reinterpret_cast<const tl_quad*>(x + i);
            v[4 * k] = q.x; v[4 * k + 1] = q.y; v[4 * k + 2] = q.z; v[4 * k + 3] = q.w;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[4 * k + e] = i + e < len ? x[i + e] : past;
        }
    }
}

__device__ __forceinline__ void tl_store_chunk(float* y, int len, const float (&v)[kBsPer]) {
#pragma unroll
    for (int k = 0; k < kTlQuads; ++k) {
        const int i = 4 * (threadIdx.x + k * kBsThreads);
        if (i + 3 < len) {
            tl_quad q;
            q.x = v[4 * k]; q.y = v[4 * k + 1]; q.z = v[4 * k + 2]; q.w = v[4 * k + 3];
            *reinterpret_cast<tl_quad*>(y + i) = q;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (i + e < len) y[i + e] = v[4 * k + e];
        }
    }
}

__global__ __launch_bounds__(kBsThreads) void token_logprob_chunk_kernel(TokenLogprobArgs a) {
    __shared__ float s_red[2][kBsWaves];
    const int lane = threadIdx.x & (OSQ_WAVE - 1), w = threadIdx.x / OSQ_WAVE;
    const int64_t row = blockIdx.x / a.chunks;
    const int c0 = (blockIdx.x % a.chunks) * kBsChunk;
    float v[kBsPer];
    tl_load_chunk(a.logits + row * a.stride + c0, min(kBsChunk, a.vocab - c0), -INFINITY, v);
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < kBsPer; ++j) mx = fmaxf(mx, v[j]);
    mx = wave_max(mx);
    if (lane == 0) s_red[0][w] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(s_red[0][0], s_red[0][1]), fmaxf(s_red[0][2], s_red[0][3]));
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < kBsPer; ++j) sum += v[j] == -INFINITY ? 0.f : expf(v[j] - mx);
    sum = wave_sum_f32(sum);
    if (lane == 0) s_red[1][w] = sum;
    __syncthreads();
    if (threadIdx.x == 0) a.partials[blockIdx.x] = make_float2(mx, (s_red[1][0] + s_red[1][1]) + (s_red[1][2] + s_red[1][3]));
}

__global__ __launch_bounds__(kBsThreads) void token_logprob_row_kernel(TokenLogprobArgs a) {
    const int64_t r = static_cast<int64_t>(blockIdx.x) * kBsThreads + threadIdx.x;
    if (r >= a.rows) return;
    const float2* part = a.partials + r * a.chunks;
    float m = -INFINITY;
    for (int c = 0; c < a.chunks; ++c) m = fmaxf(m, part[c].x);
    float total = 0.f;
    for (int c = 0; c < a.chunks; ++c) {
        const float2 p = part[c];
        total += p.y * expf(p.x - m);
    }
    const float ln_w = logf(total);
    a.lse[r] = m + ln_w;
    const int64_t t = a.labels[r];
    float lp = 0.f;
    if (t != a.ignore_index) {
        lp = __builtin_nanf("");
        if (t >= 0 && t < a.vocab) {                                // only such a label forms an address
            const float z = a.logits[r * a.stride + t];
            lp = (z == m ? 0.f : z - m) - ln_w;
        }
    }
    a.logprob[r] = lp;
}

__global__ __launch_bounds__(kBsThreads) void token_logprob_tail_kernel(TokenLogprobArgs a) {
    __shared__ float s_sum[kBsWaves];
    __shared__ long long s_cnt[2][kBsWaves];
    const int lane = threadIdx.x & (OSQ_WAVE - 1), w = threadIdx.x / OSQ_WAVE;
    float sum = 0.f;
    long long scored = 0, bad = 0;                                  // the wave's, in every lane
    for (int64_t base = 0; base < a.rows; base += kBsThreads) {
        const int64_t r = base + threadIdx.x;
        bool is_scored = false, is_bad = false;
        if (r < a.rows) {
            sum += a.logprob[r];
            const int64_t t = a.labels[r];
            const bool in = t >= 0 && t < a.vocab;
            is_scored = t != a.ignore_index && in;
            is_bad = t != a.ignore_index && !in;
        }
        scored += __popcll(__ballot(is_scored));
        bad += __popcll(__ballot(is_bad));
    }
    sum = wave_sum_f32(sum);
    if (lane == 0) { s_sum[w] = sum; s_cnt[0][w] = scored; s_cnt[1][w] = bad; }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const long long n = (s_cnt[0][0] + s_cnt[0][1]) + (s_cnt[0][2] + s_cnt[0][3]);
    if (a.counts) {
        a.counts[0] = n;
        a.counts[1] = (s_cnt[1][0] + s_cnt[1][1]) + (s_cnt[1][2] + s_cnt[1][3]);
    }
    if (a.loss) *a.loss = -((s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3])) / static_cast<float>(n);
}

// kWhole: the row is one chunk (vocab <= kBsChunk), so the workgroup holds all of it and divides by its own sum S of the
// row's expf(z - lse), formed in the order of W_c: the rounding of lse to one fp32 word, which moves every exponent of the
// row alike, leaves the gradient, and the row's dlogits add up to zero as closely as their own roundings allow.
template <bool kWhole>
__global__ __launch_bounds__(kBsThreads) void token_logprob_backward_kernel(TokenLogprobBackwardArgs a) {
    __shared__ float s_red[kBsWaves];
    const int64_t row = blockIdx.x / a.chunks;
    const int c0 = (blockIdx.x % a.chunks) * kBsChunk;
    const int len = min(kBsChunk, a.vocab - c0);
    const int64_t t = a.labels[row];
    float* y = a.dlogits + row * a.dstride + c0;
    float v[kBsPer];
    if (t == a.ignore_index || t < 0 || t >= a.vocab) {             // workgroup-uniform: no logit is read
#pragma unroll
        for (int j = 0; j < kBsPer; ++j) v[j] = 0.f;
        tl_store_chunk(y, len, v);
        return;
    }
    const float coef = a.row_grad ? a.row_grad[row] : a.scalar_grad[0] / static_cast<float>(a.counts[0]);
    const float lse = a.lse[row];
    const int64_t at = t - c0;                                      // the label's place in this chunk, if it is here
    tl_load_chunk(a.logits + row * a.stride + c0, len, -INFINITY, v);
#pragma unroll
    for (int j = 0; j < kBsPer; ++j) v[j] = expf(v[j] - lse);       // past the row: expf(-inf - lse) = 0
    float total = 1.f;
    if (kWhole) {
        float sum = 0.f;
#pragma unroll
        for (int j = 0; j < kBsPer; ++j) sum += v[j];
        sum = wave_sum_f32(sum);
        if ((threadIdx.x & (OSQ_WAVE - 1)) == 0) s_red[threadIdx.x / OSQ_WAVE] = sum;
        __syncthreads();
        total = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
    }
#pragma unroll
    for (int k = 0; k < kTlQuads; ++k)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int i = 4 * (threadIdx.x + k * kBsThreads) + e;
            const float p = kWhole ? v[4 * k + e] / total : v[4 * k + e];
            v[4 * k + e] = coef * (p - (i == at ? 1.f : 0.f));
        }
    tl_store_chunk(y, len, v);
}

static int64_t token_logprob_chunks(int64_t vocab) { return (vocab + kBsChunk - 1) / kBsChunk; }

// rows >= 0, 1 <= vocab <= 2^31 - 4097 and at most 2^31 - 1 (row, chunk) pairs: what one launch indexes
static bool token_logprob_fits(int64_t rows, int64_t vocab) {
    return rows >= 0 && vocab >= 1 && vocab <= INT32_MAX - kBsChunk && rows <= INT32_MAX / token_logprob_chunks(vocab);
}

}  // namespace osq

using namespace osq;

extern "C" size_t osq_token_logprob_workspace_bytes(int64_t rows, int64_t vocab) {
    if (!token_logprob_fits(rows, vocab)) return 0;
    return static_cast<size_t>(rows * token_logprob_chunks(vocab)) * sizeof(float2);
}

extern "C" int osq_token_logprob(const float* logits, int64_t stride, const int64_t* labels, int64_t rows, int64_t vocab,
                                 int64_t ignore_index, float* logprob, float* lse, float* loss, int64_t* counts, void* workspace,
                                 osq_stream stream) {
    OSQ_REQUIRE(rows >= 0, "token_logprob: rows below 0");
    OSQ_REQUIRE(vocab >= 1 && vocab <= INT32_MAX - kBsChunk, "token_logprob: vocab outside [1, 2^31 - 4097]");
    OSQ_REQUIRE(stride >= vocab, "token_logprob: row stride below vocab");
    OSQ_REQUIRE(token_logprob_fits(rows, vocab), "token_logprob: too many elements");
    OSQ_REQUIRE(rows == 0 || (logits && labels && logprob && lse && workspace), "token_logprob: null tensor");
    const int64_t chunks = token_logprob_chunks(vocab);
    const TokenLogprobArgs a{.logits = logits, .stride = stride, .labels = labels, .rows = rows, .vocab = static_cast<int>(vocab),
                             .chunks = static_cast<int>(chunks), .ignore_index = ignore_index, .logprob = logprob, .lse = lse,
                             .loss = loss, .counts = counts, .partials = static_cast<float2*>(workspace)};
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (rows > 0) {
        hipLaunchKernelGGL(token_logprob_chunk_kernel, dim3(static_cast<unsigned>(rows * chunks)), dim3(kBsThreads), 0, st, a);
        hipLaunchKernelGGL(token_logprob_row_kernel, dim3(static_cast<unsigned>((rows + kBsThreads - 1) / kBsThreads)),
                           dim3(kBsThreads), 0, st, a);
    }
    if (loss || counts) hipLaunchKernelGGL(token_logprob_tail_kernel, dim3(1), dim3(kBsThreads), 0, st, a);
    return check_launch("token_logprob");
}

extern "C" int osq_token_logprob_backward(const float* logits, int64_t stride, const int64_t* labels, const float* lse,
                                          const float* row_grad, const float* scalar_grad, const int64_t* counts, int64_t rows,
                                          int64_t vocab, int64_t ignore_index, float* dlogits, int64_t dstride,
                                          osq_stream stream) {
    OSQ_REQUIRE(rows >= 0, "token_logprob_backward: rows below 0");
    OSQ_REQUIRE(vocab >= 1 && vocab <= INT32_MAX - kBsChunk, "token_logprob_backward: vocab outside [1, 2^31 - 4097]");
    OSQ_REQUIRE(stride >= vocab && dstride >= vocab, "token_logprob_backward: row stride below vocab");
    OSQ_REQUIRE(token_logprob_fits(rows, vocab), "token_logprob_backward: too many elements");
    OSQ_REQUIRE(row_grad || (scalar_grad && counts), "token_logprob_backward: neither row_grad nor scalar_grad with counts");
    OSQ_REQUIRE(rows == 0 || (logits && labels && lse && dlogits), "token_logprob_backward: null tensor");
    if (rows == 0) return OSQ_OK;
    const int64_t chunks = token_logprob_chunks(vocab);
    const TokenLogprobBackwardArgs a{.logits = logits, .stride = stride, .labels = labels, .lse = lse, .row_grad = row_grad,
                                     .scalar_grad = scalar_grad, .counts = counts, .vocab = static_cast<int>(vocab),
                                     .chunks = static_cast<int>(chunks), .ignore_index = ignore_index, .dlogits = dlogits,
                                     .dstride = dstride};
    hipLaunchKernelGGL(chunks == 1 ? token_logprob_backward_kernel<true> : token_logprob_backward_kernel<false>,
                       dim3(static_cast<unsigned>(rows * chunks)), dim3(kBsThreads), 0, static_cast<hipStream_t>(stream), a);
    return check_launch("token_logprob_backward");
}

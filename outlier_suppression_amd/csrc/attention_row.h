// The register-resident row of the attention-probabilities site (attention.hip: the forward; site_backward.hip: its
// backward, which recomputes the forward's probabilities word for word): the argument record, the row's loads and the
// softmax of a row held as R float4 per lane of one wave.
#pragma once
#include <math.h>
#include "attention_seq.h"

namespace osq {

constexpr int kAttnThreads = 256;
constexpr int kAttnWaves = kAttnThreads / OSQ_WAVE;
constexpr int kAttnMaxCols = 4 * 8 * OSQ_WAVE;     // 2048: eight float4 per lane

struct AttnArgs {
    const float* scores;      // [rows, cols] contiguous; rows = batch * heads * tokens
    float* y;
    const float* mask;        // nullable; row (b, h, t) starts at b * mask_sb + h * mask_sh + t * mask_st
    int64_t mask_sb, mask_sh, mask_st;
    int64_t heads, tokens, rows;
    int cols;
    float alpha, divisor;
    DecQuant quant;           // the probabilities quantizer; scale == nullptr: softmax only
};

__device__ __forceinline__ int64_t mask_row(const AttnArgs& a, int64_t row) {
    const int64_t t = row % a.tokens, bh = row / a.tokens;
    return (bh / a.heads) * a.mask_sb + (bh % a.heads) * a.mask_sh + t * a.mask_st;
}

// float4s lane + k * 64 of row `row` of x ([rows, cols4] float4s), the row's last float4 repeated beyond its end
template <int R>
__device__ __forceinline__ void load_row(const float* x, int64_t row, int lane, int cols4, float4* v) {
    const float4* xr = reinterpret_cast<const float4*>(x) + row * cols4;
#pragma unroll
    for (int k = 0; k < R; ++k) {
        const int c = lane + k * OSQ_WAVE, cc = c < cols4 ? c : cols4 - 1;
        v[k] = load_stream(xr + cc);
    }
}

template <int R, bool MASK>
__device__ __forceinline__ void load_attn_row(const AttnArgs& a, int64_t row, int lane, int cols4, float4* v, float4* m) {
    const float4* xr = reinterpret_cast<const float4*>(a.scores) + row * cols4;
    const float4* mr = MASK ? reinterpret_cast<const float4*>(a.mask + mask_row(a, row)) : nullptr;
#pragma unroll
    for (int k = 0; k < R; ++k) {
        const int c = lane + k * OSQ_WAVE, cc = c < cols4 ? c : cols4 - 1;
        v[k] = load_stream(xr + cc);
        if (MASK) m[k] = mr[cc];           // a broadcast operand: plain loads, it stays in cache across rows
    }
}

// The softmax of the row in v (scores) and m (mask): pre-softmax rule, mask add, row max, exp, fp32 sum.  Leaves e = exp(t -
// max) in v and returns r = 1 / sum; the probabilities are e * r, one multiplication each.
template <int R, int PRE, bool MASK>
__device__ __forceinline__ float softmax_row(const AttnArgs& a, int lane, int cols4, float4* v, const float4* m) {
    float mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < R; ++k) {
        float t[4] = {v[k].x, v[k].y, v[k].z, v[k].w};
        const float mm[4] = {MASK ? m[k].x : 0.f, MASK ? m[k].y : 0.f, MASK ? m[k].z : 0.f, MASK ? m[k].w : 0.f};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            t[e] = pre_softmax(PRE, t[e], a.alpha, a.divisor);
            if (MASK) t[e] = t[e] + mm[e];
        }
        v[k] = make_float4(t[0], t[1], t[2], t[3]);
        // fmaxf drops a NaN: harmless, a NaN entry makes its exp and so the row's sum NaN
        if (lane + k * OSQ_WAVE < cols4) mx = fmaxf(mx, fmaxf(fmaxf(t[0], t[1]), fmaxf(t[2], t[3])));
    }
    mx = wave_max(mx);
    float sum = 0.f;
#pragma unroll
    for (int k = 0; k < R; ++k) {
        v[k] = make_float4(expf(v[k].x - mx), expf(v[k].y - mx), expf(v[k].z - mx), expf(v[k].w - mx));
        if (lane + k * OSQ_WAVE < cols4) sum += (v[k].x + v[k].y) + (v[k].z + v[k].w);
    }
    return 1.0f / wave_sum_f32(sum);
}

// the fast path's geometry: whole float4s, the row in at most eight of them per lane, 16-byte aligned rows of scores and mask
static bool attn_row_geometry(const float* scores, const float* mask, int64_t cols, int64_t mask_sb, int64_t mask_sh,
                              int64_t mask_st) {
    return cols % 4 == 0 && cols <= kAttnMaxCols && aligned16(scores) &&
           (!mask || (aligned16(mask) && mask_sb % 4 == 0 && mask_sh % 4 == 0 && mask_st % 4 == 0));
}

}  // namespace osq

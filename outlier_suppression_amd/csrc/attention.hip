// Attention-probabilities site: pre-softmax scaling + additive mask -> softmax -> fake-quant in ONE pass.
//
// The reference runs, per self-attention block (model/quant_bert.py:169-185, model/quant_bart.py:232-256):
//     v = scores / sqrt(d) + mask         one or two elementwise ops       1-2 reads + 1 write (+ the mask)
//     p = softmax(v, dim=-1)              one softmax                      1 read  + 1 write
//     y = fake_quantize(p)                attention_probs quantizer        1 read  + 1 write
// on the largest activation of the block ([B, h, T, S]: 226 MB at [32,12,384,384]) = about 28 B per element.
// Here: read scores, write y (the mask is a broadcast operand, read from cache): 8 B per element.
//
// Pre-softmax step: the rule of attention_seq.h, its form a template parameter here (a streaming kernel).
// Softmax as torch's CPU kernel computes it (vec_softmax_lastdim): subtract the row max, exp, sum, then MULTIPLY by the
// reciprocal of the sum (probed against torch.softmax on one thread: p == e * (1/sum) wherever the exps agree).  expf is
// ocml's accurate routine, not __expf; it is not Sleef's, so results are within a few ulp of torch's, not bit-equal.
// Special rows follow from the formula as they do in torch: a NaN anywhere, a +inf, or a row of -inf only gives a NaN
// sum and so a NaN row.  The fake-quant step is quantize_value / dequantize_value with tensor_params, the helpers of
// fq_tensor_vec_kernel: for a given p the output is word-equal to osq_fake_quant_per_tensor(p).
//
// Fast path (cols % 4 == 0, cols <= 2048, 16-byte aligned scores / y / mask rows): one wave per row, the row in
// registers (R float4 per lane), the next row's loads issued before the current row is reduced.  Anything else: the
// generic kernel, one wave per row with scalar accesses and the row re-read for each of its three sweeps.
#include <math.h>
#include <string>
#include <hip/hip_ext.h>
#include "attention_seq.h"

namespace osq {

constexpr int kAttnThreads = 256;
constexpr int kAttnWaves = kAttnThreads / OSQ_WAVE;
constexpr int kAttnMaxCols = 4 * 8 * OSQ_WAVE;     // 2048: eight float4 per lane
OSQ_AB_KNOB(int, g_attn_blocks, 2048);             // grid cap (osq_set_tuning("attn_blocks", n)); rows are grid-strided above it

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

template <int R, int PRE, bool MASK, bool WT>
__global__ __launch_bounds__(kAttnThreads) void attention_softmax_fq_kernel(AttnArgs a) {
    const int lane = threadIdx.x & (OSQ_WAVE - 1);
    const int64_t wave0 = (static_cast<int64_t>(blockIdx.x) * kAttnThreads + threadIdx.x) / OSQ_WAVE;
    const int64_t nwaves = static_cast<int64_t>(gridDim.x) * kAttnWaves;
    const int cols4 = a.cols >> 2;
    const QParams q = dec_params(a.quant);
    float4* y4 = reinterpret_cast<float4*>(a.y);
    const WtStore ywt(y4, WT ? a.rows * cols4 : 0);
    float4 v[R], m[R];
    if (wave0 < a.rows) load_attn_row<R, MASK>(a, wave0, lane, cols4, v, m);
    for (int64_t row = wave0; row < a.rows; row += nwaves) {
        float4 vn[R], mn[R];
        if (row + nwaves < a.rows) load_attn_row<R, MASK>(a, row + nwaves, lane, cols4, vn, mn);
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
        const float r = 1.0f / wave_sum_f32(sum);
        const int64_t base = row * cols4;
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const int c = lane + k * OSQ_WAVE;
            if (c < cols4) {
                const float4 o = make_float4(dec_fq(v[k].x * r, a.quant, q), dec_fq(v[k].y * r, a.quant, q),
                                             dec_fq(v[k].z * r, a.quant, q), dec_fq(v[k].w * r, a.quant, q));
                if (WT) ywt.put(base + c, o); else store_stream(y4 + base + c, o);
            }
        }
#pragma unroll
        for (int k = 0; k < R; ++k) {
            v[k] = vn[k];
            if (MASK) m[k] = mn[k];
        }
    }
}

// any row width and alignment: the same arithmetic, the row re-read from memory for the max, the sum and the output
template <int PRE, bool MASK>
__global__ __launch_bounds__(kAttnThreads) void attention_softmax_fq_generic_kernel(AttnArgs a) {
    const int lane = threadIdx.x & (OSQ_WAVE - 1);
    const int64_t wave0 = (static_cast<int64_t>(blockIdx.x) * kAttnThreads + threadIdx.x) / OSQ_WAVE;
    const int64_t nwaves = static_cast<int64_t>(gridDim.x) * kAttnWaves;
    const QParams q = dec_params(a.quant);
    for (int64_t row = wave0; row < a.rows; row += nwaves) {
        const float* xr = a.scores + row * a.cols;
        const float* mr = MASK ? a.mask + mask_row(a, row) : nullptr;
        float* yr = a.y + row * a.cols;
        float mx = -INFINITY;
        for (int j = lane; j < a.cols; j += OSQ_WAVE) {
            float t = pre_softmax(PRE, xr[j], a.alpha, a.divisor);
            if (MASK) t = t + mr[j];
            mx = fmaxf(mx, t);
        }
        mx = wave_max(mx);
        float sum = 0.f;
        for (int j = lane; j < a.cols; j += OSQ_WAVE) {
            float t = pre_softmax(PRE, xr[j], a.alpha, a.divisor);
            if (MASK) t = t + mr[j];
            sum += expf(t - mx);
        }
        const float r = 1.0f / wave_sum_f32(sum);
        for (int j = lane; j < a.cols; j += OSQ_WAVE) {
            float t = pre_softmax(PRE, xr[j], a.alpha, a.divisor);
            if (MASK) t = t + mr[j];
            yr[j] = dec_fq(expf(t - mx) * r, a.quant, q);
        }
    }
}

bool set_attention_tuning(const char* key, int value) {
#ifdef OSQ_TUNABLE
    if (std::string(key) == "attn_blocks" && value >= 1) { g_attn_blocks = value; return true; }
#endif
    return false;
}

}  // namespace osq

using namespace osq;

extern "C" int osq_attention_softmax_fake_quant(const float* scores, const float* mask, int64_t batch, int64_t heads,
                                                int64_t tokens, int64_t cols, int64_t mask_stride_b,
                                                int64_t mask_stride_h, int64_t mask_stride_t, float alpha,
                                                float divisor, float* y, float* scale, void* zero_point, int zp_type,
                                                int mode, float grad_factor, int quant_min, int quant_max,
                                                osq_stream stream) {
    OSQ_REQUIRE(batch >= 0 && heads >= 0 && tokens >= 0 && cols > 0 && cols <= INT32_MAX,
                "attention_softmax_fake_quant: bad shape");
    const int64_t rows = batch * heads * tokens;
    if (rows == 0) return OSQ_OK;
    OSQ_REQUIRE(scores && y, "attention_softmax_fake_quant: null tensor");
    OSQ_REQUIRE(!mask || (mask_stride_b >= 0 && mask_stride_h >= 0 && mask_stride_t >= 0),
                "attention_softmax_fake_quant: negative mask stride");
    OSQ_REQUIRE(alpha == 1.0f || divisor == 1.0f, "attention_softmax_fake_quant: give alpha or divisor, not both");
    OSQ_REQUIRE(!scale || zero_point, "attention_softmax_fake_quant: scale without zero_point");
    OSQ_REQUIRE(!scale || dec_mode_ok(mode), "attention_softmax_fake_quant: bad mode");
    AttnArgs a{scores, y, mask, mask_stride_b, mask_stride_h, mask_stride_t, heads, tokens, rows, static_cast<int>(cols),
               alpha, divisor, dec_quant(scale, zero_point, zp_type, mode, grad_factor, quant_min, quant_max)};
    const int pre = pre_of(alpha, divisor);
    int64_t blocks = (rows + kAttnWaves - 1) / kAttnWaves;
    if (blocks > g_attn_blocks) blocks = g_attn_blocks;
    const dim3 grid(static_cast<unsigned>(blocks));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const TimingHook th = take_timing_hook(OSQ_TIME_ATTENTION_SOFTMAX);
    const bool fast = cols % 4 == 0 && cols <= kAttnMaxCols && aligned16(scores) && aligned16(y) &&
                      (!mask || (aligned16(mask) && mask_stride_b % 4 == 0 && mask_stride_h % 4 == 0 && mask_stride_t % 4 == 0));
    if (!fast) {
#define OSQ_ATTN_G(PRE, MASK) \
    hipExtLaunchKernelGGL((attention_softmax_fq_generic_kernel<PRE, MASK>), grid, dim3(kAttnThreads), 0, st, th.start, th.stop, 0, a)
#define OSQ_ATTN_GM(PRE) if (mask) OSQ_ATTN_G(PRE, true); else OSQ_ATTN_G(PRE, false)
        if (pre == kPreDivide) { OSQ_ATTN_GM(kPreDivide); }
        else if (pre == kPreScale) { OSQ_ATTN_GM(kPreScale); }
        else { OSQ_ATTN_GM(kPrePlain); }
#undef OSQ_ATTN_GM
#undef OSQ_ATTN_G
        return check_launch("attention_softmax_fake_quant");
    }
    const int per_lane = static_cast<int>((cols / 4 + OSQ_WAVE - 1) / OSQ_WAVE);
    const bool wt = rows * (cols / 4) <= kWtMaxFloat4;   // write-through stores address the output with 32-bit offsets
#define OSQ_ATTN(R, PRE, MASK)                                                                                                  \
    do {                                                                                                                        \
        if (wt) hipExtLaunchKernelGGL((attention_softmax_fq_kernel<R, PRE, MASK, true>), grid, dim3(kAttnThreads), 0, st,      \
                                      th.start, th.stop, 0, a);                                                                 \
        else hipExtLaunchKernelGGL((attention_softmax_fq_kernel<R, PRE, MASK, false>), grid, dim3(kAttnThreads), 0, st,       \
                                   th.start, th.stop, 0, a);                                                                    \
    } while (0)
#define OSQ_ATTN_M(R, PRE) do { if (mask) OSQ_ATTN(R, PRE, true); else OSQ_ATTN(R, PRE, false); } while (0)
#define OSQ_ATTN_R(PRE)                                  \
    do {                                                 \
        if (per_lane <= 1) OSQ_ATTN_M(1, PRE);           \
        else if (per_lane <= 2) OSQ_ATTN_M(2, PRE);      \
        else if (per_lane <= 4) OSQ_ATTN_M(4, PRE);      \
        else OSQ_ATTN_M(8, PRE);                         \
    } while (0)
    if (pre == kPreDivide) OSQ_ATTN_R(kPreDivide);
    else if (pre == kPreScale) OSQ_ATTN_R(kPreScale);
    else OSQ_ATTN_R(kPrePlain);
#undef OSQ_ATTN_R
#undef OSQ_ATTN_M
#undef OSQ_ATTN
    return check_launch("attention_softmax_fake_quant");
}

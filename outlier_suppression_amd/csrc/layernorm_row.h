// The register-resident row of the residual + LayerNorm + fake-quant site (layernorm.hip: the forward; layernorm_backward.hip:
// its backward, which recomputes the forward's normalised words): the argument record, the per-column operands, the row's
// loads, r = x * gamma + hidden, the two-pass moments and the per-element steps up to the quantizer's input, for a row held
// as R float4 per lane of one wave.  Every arithmetic step is individually rounded (-ffp-contract=off), in the order
//     a = input*gamma; r = a + hidden; t = (r - mean) * rstd; t = t*w; t = t + b.
#pragma once
#include "osq_device.h"
#include "osq_host.h"

namespace osq {

constexpr int kLnThreads = 256;
constexpr int kLnWaves = kLnThreads / OSQ_WAVE;

struct LnArgs {
    const float4* x;
    const float4* hidden;     // nullable: no residual
    const float4* gamma;      // nullable: plain residual add (only read when hidden != NULL)
    const float4* weight;     // nullable: no elementwise scale
    const float4* bias;       // nullable
    float4* y;
    int64_t rows;
    int cols4;
    float inv_cols, eps;
    float* scale;             // nullable: no fake-quant (written only under OSQ_PARAM_SANITIZE)
    void* zero_point;
    int zp_type, mode;
    float grad_factor, qmin, qmax;
};

// per-column operands stay in registers across the rows of a wave while the row is short (<= 1024 columns: every LayerNorm
// of BERT / RoBERTa / BART); longer rows re-read them (L1/L2 hits) per row
template <int R> struct LnKeep {
    static constexpr bool keep = R <= 4;
    static constexpr int regs = keep ? R : 1;
};

__device__ __forceinline__ float4 ln_gamma_at(const LnArgs& a, int cc) {
    return (a.hidden && a.gamma) ? a.gamma[cc] : make_float4(1.f, 1.f, 1.f, 1.f);
}
__device__ __forceinline__ float4 ln_weight_at(const LnArgs& a, int cc) {
    return a.weight ? a.weight[cc] : make_float4(1.f, 1.f, 1.f, 1.f);
}
__device__ __forceinline__ float4 ln_bias_at(const LnArgs& a, int cc) {
    return a.bias ? a.bias[cc] : make_float4(0.f, 0.f, 0.f, 0.f);
}

// the kept form of gamma / weight / bias: float4s lane + k * 64, the last one repeated beyond the row's end
template <int R>
__device__ __forceinline__ void ln_load_cols(const LnArgs& a, int lane, float4* g, float4* w, float4* b) {
    if (LnKeep<R>::keep) {
#pragma unroll
        for (int k = 0; k < LnKeep<R>::regs; ++k) {
            const int c = lane + k * OSQ_WAVE, cc = c < a.cols4 ? c : a.cols4 - 1;
            g[k] = ln_gamma_at(a, cc);
            w[k] = ln_weight_at(a, cc);
            b[k] = ln_bias_at(a, cc);
        }
    }
}

// float4s lane + k * 64 of row `row` of x (and of hidden when `hid`), the row's last float4 repeated beyond its end
template <int R>
__device__ __forceinline__ void ln_load_row(const LnArgs& a, bool hid, int64_t row, int lane, float4* v, float4* h) {
    const float4* xr = a.x + row * a.cols4;
    const float4* hr = hid ? a.hidden + row * a.cols4 : nullptr;
#pragma unroll
    for (int k = 0; k < R; ++k) {
        const int c = lane + k * OSQ_WAVE, cc = c < a.cols4 ? c : a.cols4 - 1;
        v[k] = load_stream(xr + cc);
        if (hid) h[k] = load_stream(hr + cc);
    }
}

// r = x * gamma + hidden into v, then the row's moments: mean and rstd = 1 / sqrt(var + eps), two wave reductions (sum, then
// sum of squared deviations -- the two-pass form, no cancellation)
template <int R>
__device__ __forceinline__ void ln_row_moments(const LnArgs& a, bool hid, int lane, float4* v, const float4* h, const float4* g,
                                               float& mean, float& rstd) {
    constexpr bool KEEP = LnKeep<R>::keep;
    float sum = 0.f;
#pragma unroll
    for (int k = 0; k < R; ++k) {
        if (hid) {
            if (a.gamma) {
                const int c = lane + k * OSQ_WAVE;
                const float4 gk = KEEP ? g[KEEP ? k : 0] : a.gamma[c < a.cols4 ? c : a.cols4 - 1];
                v[k].x *= gk.x; v[k].y *= gk.y; v[k].z *= gk.z; v[k].w *= gk.w;
            }
            v[k].x += h[k].x; v[k].y += h[k].y; v[k].z += h[k].z; v[k].w += h[k].w;
        }
        if (lane + k * OSQ_WAVE < a.cols4) sum += (v[k].x + v[k].y) + (v[k].z + v[k].w);
    }
    mean = wave_sum_f32(sum) * a.inv_cols;
    float sq = 0.f;
#pragma unroll
    for (int k = 0; k < R; ++k) {
        if (lane + k * OSQ_WAVE < a.cols4) {
            const float dx = v[k].x - mean, dy = v[k].y - mean, dz = v[k].z - mean, dw = v[k].w - mean;
            sq += (dx * dx + dy * dy) + (dz * dz + dw * dw);
        }
    }
    const float var = wave_sum_f32(sq) * a.inv_cols;
    rstd = 1.0f / sqrtf(var + a.eps);
}

// weight / bias of float4 c of the row (c inside the row): the kept registers, or a re-read
template <int R>
__device__ __forceinline__ float4 ln_row_weight(const LnArgs& a, const float4* w, int k, int c) {
    constexpr bool KEEP = LnKeep<R>::keep;
    return KEEP ? w[KEEP ? k : 0] : ln_weight_at(a, c);
}
template <int R>
__device__ __forceinline__ float4 ln_row_bias(const LnArgs& a, const float4* b, int k, int c) {
    constexpr bool KEEP = LnKeep<R>::keep;
    return KEEP ? b[KEEP ? k : 0] : ln_bias_at(a, c);
}

// the normalised word and the quantizer's input made from it
__device__ __forceinline__ float ln_xhat(float r, float mean, float rstd) { return (r - mean) * rstd; }
__device__ __forceinline__ float ln_affine(const LnArgs& a, float u, float w, float b) {
    if (a.weight) u = u * w;
    if (a.bias) u = u + b;
    return u;
}

}  // namespace osq

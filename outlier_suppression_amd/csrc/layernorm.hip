// Residual + LayerNorm + fake-quant in ONE pass over the activation.
//
// The reference runs, per LayerNorm site of a quantized model (model/quant_bert.py:211-216, 298-303;
// model/util_layernorm.py:14-18, 32-37, 49-52):
//     r = input * gamma + hidden          GammaResidual               2 reads + 1 write
//     n = layer_norm(r) [* w + b]         LayerNorm                   1 read  + 1 write
//     n += beta / gamma                   split form only             1 read  + 1 write
//     y = fake_quantize(n)                8 eager ops                 1 read  + 1 write
// = 24..32 B per element.  Here: read input (+ hidden), write y: 8 (12) B per element.
//
// One wave per row; the row lives in registers (R float4 per lane, cols <= 4096); mean and variance are
// two wave reductions (sum, then sum of squared deviations -- the two-pass form, no cancellation);
// every arithmetic step is individually rounded (-ffp-contract=off) in the order of the eager ops:
//     a = input*gamma; r = a + hidden; t = (r - mean) * rstd; t = t*w; t = t + b; then quantize_value.
// The normalisation is not bit-comparable with torch's own kernel (Welford on the GPU, a different
// blocked summation on the CPU): callers that need the eager sequence keep using it (autograd passes do, unless
// FUSE_LAYERNORM_BACKWARD hands them this launch and layernorm_backward.hip's).
#include <string>
#include <hip/hip_ext.h>
#include "layernorm_row.h"

namespace osq {

OSQ_AB_KNOB(int, g_ln_blocks, 1024);      // grid cap (osq_set_tuning("ln_blocks", n)); rows are grid-strided above it.  tools/bwd_ab.py on MI355X,
                                    // [256,128,768]: one row per wave (8192 workgroups) 58.2 us, 2048: 51.6, 1024: 51.2, 768: 51.1, 512: 60.0; [32,384,768]: 23.6 -> 21.1

template <int R>
__global__ __launch_bounds__(kLnThreads) void residual_layernorm_fq_kernel(LnArgs a) {
    const int lane = threadIdx.x & (OSQ_WAVE - 1);
    const int64_t wave0 = (static_cast<int64_t>(blockIdx.x) * kLnThreads + threadIdx.x) / OSQ_WAVE;
    const int64_t nwaves = static_cast<int64_t>(gridDim.x) * kLnWaves;
    QParams p{1.f, 0.f};
    if (a.scale) p = tensor_params(a.scale, a.zero_point, a.zp_type, a.mode, a.grad_factor, a.qmin, a.qmax);
    // the row's loads, residual, moments and per-element steps are layernorm_row.h's: the backward recomputes them word for word
    constexpr int RK = LnKeep<R>::regs;
    float4 g[RK], w[RK], b[RK];
    ln_load_cols<R>(a, lane, g, w, b);
    for (int64_t row = wave0; row < a.rows; row += nwaves) {
        float4 v[R], h[R];
        ln_load_row<R>(a, a.hidden != nullptr, row, lane, v, h);
        float mean, rstd;
        ln_row_moments<R>(a, a.hidden != nullptr, lane, v, h, g, mean, rstd);
        float4* yr = a.y + row * a.cols4;
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const int c = lane + k * OSQ_WAVE;
            if (c < a.cols4) {
                float t[4] = {v[k].x, v[k].y, v[k].z, v[k].w};
                const float4 wk = ln_row_weight<R>(a, w, k, c);
                const float4 bk = ln_row_bias<R>(a, b, k, c);
                const float ww[4] = {wk.x, wk.y, wk.z, wk.w}, bb[4] = {bk.x, bk.y, bk.z, bk.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float u = ln_affine(a, ln_xhat(t[e], mean, rstd), ww[e], bb[e]);
                    if (a.scale) u = dequantize_value(quantize_value(u, p.scale, p.zp, a.qmin, a.qmax), p.scale, p.zp);
                    t[e] = u;
                }
                store_stream(yr + c, make_float4(t[0], t[1], t[2], t[3]));
            }
        }
    }
}

bool set_layernorm_tuning(const char* key, int value) {
#ifdef OSQ_TUNABLE
    if (std::string(key) == "ln_blocks" && value >= 1) { g_ln_blocks = value; return true; }
#endif
    return false;
}

}  // namespace osq

using namespace osq;

extern "C" int osq_residual_layernorm_fake_quant(const float* x, const float* hidden, const float* gamma,
                                                 const float* weight, const float* bias, double eps,
                                                 float* y, int64_t rows, int64_t cols,
                                                 float* scale, void* zero_point, int zp_type,
                                                 int mode, float grad_factor, int quant_min, int quant_max,
                                                 osq_stream stream) {
    OSQ_REQUIRE(rows >= 0 && cols > 0, "residual_layernorm_fake_quant: bad shape");
    if (rows == 0) return OSQ_OK;
    OSQ_REQUIRE(x && y, "residual_layernorm_fake_quant: null tensor");
    OSQ_REQUIRE(!scale || zero_point, "residual_layernorm_fake_quant: scale without zero_point");
    OSQ_REQUIRE(!scale || ((mode & ~(OSQ_PARAM_MODE_MASK | OSQ_PARAM_SANITIZE)) == 0 && (mode & OSQ_PARAM_MODE_MASK) <= OSQ_PARAM_LSQPLUS),
                "residual_layernorm_fake_quant: bad mode");
    if (cols % 4 != 0 || cols > 4 * 16 * OSQ_WAVE || !aligned16(x) || !aligned16(y) || (hidden && !aligned16(hidden)) ||
        (gamma && !aligned16(gamma)) || (weight && !aligned16(weight)) || (bias && !aligned16(bias))) {
        set_error("residual_layernorm_fake_quant: needs cols %% 4 == 0, cols <= 4096 and 16-byte aligned operands");
        return OSQ_ERR_UNSUPPORTED;
    }
    LnArgs a{reinterpret_cast<const float4*>(x), reinterpret_cast<const float4*>(hidden),
             reinterpret_cast<const float4*>(gamma), reinterpret_cast<const float4*>(weight),
             reinterpret_cast<const float4*>(bias), reinterpret_cast<float4*>(y), rows, static_cast<int>(cols / 4),
             static_cast<float>(1.0 / static_cast<double>(cols)), static_cast<float>(eps), scale, zero_point, zp_type, mode,
             grad_factor, static_cast<float>(quant_min), static_cast<float>(quant_max)};
    int64_t blocks = (rows + kLnWaves - 1) / kLnWaves;
    if (blocks > g_ln_blocks) blocks = g_ln_blocks;
    const dim3 grid(static_cast<unsigned>(blocks));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int per_lane = (a.cols4 + OSQ_WAVE - 1) / OSQ_WAVE;
    const TimingHook th = take_timing_hook(OSQ_TIME_LAYERNORM);
#define OSQ_LN(R) hipExtLaunchKernelGGL(residual_layernorm_fq_kernel<R>, grid, dim3(kLnThreads), 0, st, th.start, th.stop, 0, a)
    if (per_lane <= 1) OSQ_LN(1);
    else if (per_lane <= 2) OSQ_LN(2);
    else if (per_lane <= 3) OSQ_LN(3);
    else if (per_lane <= 4) OSQ_LN(4);
    else if (per_lane <= 8) OSQ_LN(8);
    else OSQ_LN(16);
#undef OSQ_LN
    return check_launch("residual_layernorm_fake_quant");
}

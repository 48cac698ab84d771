// What the decode-attention kernels share (decode_attention.hip, decode_attention_shared.hip): the workgroup shape, how a
// lane reads its four elements of a row of K or V from either storage format, the quantizers of the site and the two lane sums
// whose order the header comment of decode_attention.hip fixes.
#pragma once
#include <hip/hip_runtime.h>
#include "codes_device.h"
#include "osq_host.h"

namespace osq {

constexpr int kDecThreads = 256;
constexpr int kDecWaves = kDecThreads / OSQ_WAVE;

// How a lane reads its four elements of a row of K or V: the word it loads, how many such loads it issues before the first
// reduction, and the four fp32 values of a word.
struct DecCode {               // the record of a coded tensor; unused by the fp32 form
    const float* scale_eff;
    const float* zp_eff;
    int quant_min;
};
struct KvWords {               // fp32 cache: a float4, 4 x 16 B in flight per lane
    typedef float4 Word;
    static constexpr int kInFlight = 4;
    struct Params {};
    __device__ __forceinline__ static Params params(const DecCode&) { return Params{}; }
    __device__ __forceinline__ static Word load(const void* base, int64_t i) { return load_stream(static_cast<const float4*>(base) + i); }
    __device__ __forceinline__ static float4 values(const Word& w, const Params&) { return w; }
};
struct KvCodes {               // coded cache: four codes in 32 bits, 16 x 4 B in flight per lane
    typedef unsigned int Word;
    static constexpr int kInFlight = 16;
    struct Params { float s, z; int quant_min; };
    __device__ __forceinline__ static Params params(const DecCode& d) { return Params{d.scale_eff[0], d.zp_eff[0], d.quant_min}; }
    __device__ __forceinline__ static Word load(const void* base, int64_t i) {
        return __builtin_nontemporal_load(static_cast<const unsigned int*>(base) + i);
    }
    __device__ __forceinline__ static float4 values(const Word& w, const Params& p) {
        return make_float4(value_of(w & 255u, p.quant_min, p.s, p.z), value_of((w >> 8) & 255u, p.quant_min, p.s, p.z),
                           value_of((w >> 16) & 255u, p.quant_min, p.s, p.z), value_of(w >> 24, p.quant_min, p.s, p.z));
    }
};

struct DecQuant {              // one quantizer of the site; scale == nullptr: no quantizer, values pass through
    float* scale;              // written only under OSQ_PARAM_SANITIZE
    void* zero_point;
    int zp_type, mode;
    float grad_factor, qmin, qmax;
};

__device__ __forceinline__ QParams dec_params(const DecQuant& d) {
    if (!d.scale) return QParams{1.f, 0.f};
    return tensor_params(d.scale, d.zero_point, d.zp_type, d.mode, d.grad_factor, d.qmin, d.qmax);
}

__device__ __forceinline__ float dec_fq(float x, const DecQuant& d, const QParams& p) {
    return d.scale ? dequantize_value(quantize_value(x, p.scale, p.zp, d.qmin, d.qmax), p.scale, p.zp) : x;
}

// sum over the LPR consecutive lanes that share a row; every lane of the group ends with the same word.  All 64 lanes active.
template <int LPR>
__device__ __forceinline__ float row_lanes_sum(float v) {
    if (LPR >= 2) v = dpp_add_f32<kDppQuadXor1>(v);
    if (LPR >= 4) v = dpp_add_f32<kDppQuadXor2>(v);
    if (LPR >= 8) v = dpp_add_f32<kDppRowHalfMirror>(v);
    if (LPR >= 16) v = dpp_add_f32<kDppRowMirror>(v);
    if (LPR >= 32) v = v + __shfl_xor(v, 16, OSQ_WAVE);
    if (LPR >= 64) v = v + __shfl_xor(v, 32, OSQ_WAVE);
    return v;
}

// sum over the wave's 64 / LPR row groups, lane c of each; all 64 lanes active
template <int LPR>
__device__ __forceinline__ float row_groups_sum(float v) {
#pragma unroll
    for (int s = LPR; s < OSQ_WAVE; s <<= 1) v = v + __shfl_xor(v, s, OSQ_WAVE);
    return v;
}

static bool dec_mode_ok(int mode) {
    return (mode & ~(OSQ_PARAM_MODE_MASK | OSQ_PARAM_SANITIZE)) == 0 && (mode & OSQ_PARAM_MODE_MASK) <= OSQ_PARAM_LSQPLUS;
}

static DecQuant dec_quant(float* scale, void* zero_point, int zp_type, int mode, float grad_factor, int quant_min, int quant_max) {
    return DecQuant{scale, zero_point, zp_type, mode, grad_factor, static_cast<float>(quant_min), static_cast<float>(quant_max)};
}

}  // namespace osq

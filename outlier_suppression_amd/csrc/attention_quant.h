// The quantizer record of every one-launch attention kernel (decode_attention.hip: one query token over the KV cache;
// attention.hip, attention_block.hip, attention_int.hip: whole sequences, through attention_seq.h): a parameter group of the
// C ABI as the kernel holds it, the parameters that reach the quantiser (the repair under OSQ_PARAM_SANITIZE rides in
// tensor_params), the fake-quant of one value and the check of a group's mode.
#pragma once
#include "osq_device.h"
#include "osq_host.h"

namespace osq {

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

static bool dec_mode_ok(int mode) {
    return (mode & ~(OSQ_PARAM_MODE_MASK | OSQ_PARAM_SANITIZE)) == 0 && (mode & OSQ_PARAM_MODE_MASK) <= OSQ_PARAM_LSQPLUS;
}

static DecQuant dec_quant(float* scale, void* zero_point, int zp_type, int mode, float grad_factor, int quant_min, int quant_max) {
    return DecQuant{scale, zero_point, zp_type, mode, grad_factor, static_cast<float>(quant_min), static_cast<float>(quant_max)};
}

// the seven arguments of the quantizer named `site` (probs or ctx), site_scale .. site_quant_max, as the launcher's record
#define OSQ_DEC_QUANT(site) \
    dec_quant(site##_scale, site##_zero_point, site##_zp_type, site##_mode, site##_grad_factor, site##_quant_min, site##_quant_max)

}  // namespace osq

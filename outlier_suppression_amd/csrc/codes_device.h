// Integer codes of a quantised value, shared by the kernels that write or read them (codes.hip: weights of a checkpoint;
// kv_codes.hip and decode_attention.hip: the KV cache of incremental decoding).  u = x_quant - quant_min, one byte.
#pragma once
#include "osq_device.h"

namespace osq {

constexpr int kCodeThreads = 256;      // workgroup size of every kernel that counts rejected elements (add_rejected)

// The code of one element, or 0 and one more on `rejected` where x_quant is NaN or not an integer (a NaN or infinite x, a
// NaN parameter, a fractional zero point): such an element has no code.  A finite x_quant lies in [qmin, qmax] (the clamp),
// so q - qmin is exact and fits.
__device__ __forceinline__ unsigned int code_of(float x, const QParams& p, float qmin, float qmax, unsigned int& rejected) {
    const float q = quantize_value(x, p.scale, p.zp, qmin, qmax);
    const bool ok = (q == rintf(q));                    // false for NaN
    rejected += ok ? 0u : 1u;
    return ok ? static_cast<unsigned int>(static_cast<int>(q - qmin)) : 0u;
}

// x_quant back from its code, then util_quant.py:14
__device__ __forceinline__ float value_of(unsigned int u, int quant_min, float s, float z) {
    return dequantize_value(static_cast<float>(static_cast<int>(u) + quant_min), s, z);
}

// every thread of the workgroup calls (no early exit before it): lane counts -> wave -> workgroup -> ONE atomic add
__device__ __forceinline__ void add_rejected(int32_t* rejected, unsigned int mine) {
    __shared__ unsigned int s_rej[kCodeThreads / OSQ_WAVE];
    const unsigned int upto = wave_inclusive_scan_u32(mine);
    if ((threadIdx.x & (OSQ_WAVE - 1)) == OSQ_WAVE - 1) s_rej[threadIdx.x / OSQ_WAVE] = upto;
    __syncthreads();
    if (threadIdx.x == 0 && rejected) {
        unsigned int total = 0;
        for (int k = 0; k < kCodeThreads / OSQ_WAVE; ++k) total += s_rej[k];
        if (total) atomicAdd(rejected, static_cast<int32_t>(total));
    }
}

}  // namespace osq

// The LSQ / LSQ+ backward as its kernels share it (fake_quant.hip: the quantizer's own backward; site_backward.hip: the
// backward of the one-launch GELU and attention-probabilities sites): the per-element rule, the streaming body over a dense
// tensor with the quantizer's input made by a PRODUCER, and the deterministic float64 reduction that ends every one of them.
#pragma once
#include "osq_device.h"
#include "osq_host.h"

namespace osq {

constexpr int kBwdThreads = 256;      // the workgroup of every kernel that ends in lsq_bwd_finish

// torch's exact GELU (aten GeluCUDAKernelImpl, approximate='none'): x * 0.5 * (1 + erf(x * M_SQRT1_2)), fp32,
// same operation order; erff is the ocml routine torch's HIP build calls too, so the fused activation is
// bit-identical to F.gelu on the device (tests/test_gpu_parity.py::test_gelu_fake_quant_fused).
__device__ __forceinline__ float gelu_erf(float x) {
    constexpr float kAlpha = 0.70710678118654752440f;
    return (x * 0.5f) * (1.0f + erff(x * kAlpha));
}

// d gelu / dx = Phi(x) + x phi(x), fp32, in the operation order of aten's GeluBackwardCUDAKernelImpl: Phi from the erff the
// forward takes (the compiler shares the call), phi = exp(-x^2 / 2) / sqrt(2 pi).
__device__ __forceinline__ float gelu_erf_grad(float x) {
    constexpr float kAlpha = 0.70710678118654752440f;
    constexpr float kBeta = 0.39894228040143267794f;       // M_2_SQRTPI * M_SQRT1_2 * 0.5
    const float cdf = 0.5f * (1.0f + erff(x * kAlpha));
    const float pdf = expf(-0.5f * x * x) * kBeta;
    return cdf + x * pdf;
}

// Per element (autograd of util_quant.py:48-55, see oracle/fake_quant_oracle.py):
//   g_mul = gy * s ; g_in = inside ? g_mul : 0 ; dx = g_in / s
//   ds  += gy * (xq - z)  +  (-g_in) * ((x / s) / s)
//   dzp += g_in - g_mul
// Sums: fp32 per lane over a short run, then double across lanes / blocks; block
// partials are combined in block order by the last block (deterministic).
struct BwdAcc {
    float ds_mul, ds_div, dz;
};

__device__ __forceinline__ float bwd_elem(float x, float gy, float s, float z, float qmin, float qmax, BwdAcc& a) {
    float x_int;
    const float q = quantize_value(x, s, z, qmin, qmax, &x_int);
    const bool inside = (x_int >= qmin) && (x_int <= qmax);
    const float g_mul = gy * s;
    const float g_in = inside ? g_mul : 0.0f;
    a.ds_mul += gy * (q - z);
    a.ds_div += (-g_in) * ((x / s) / s);
    a.dz += g_in - g_mul;
    return g_in / s;
}

// What stands in front of the quantizer at a site: value(x) is the quantizer's input made from the saved tensor, chain(x, dg)
// the gradient of the saved tensor from the gradient dg of the quantizer's input.
struct PlainProducer {                // the quantizer alone: x is its input
    __device__ __forceinline__ float value(float x) const { return x; }
    __device__ __forceinline__ float chain(float, float dg) const { return dg; }
};
struct GeluProducer {                 // fake_quantize(gelu(x)): the words the forward quantised, then dg * gelu'(x)
    __device__ __forceinline__ float value(float x) const { return gelu_erf(x); }
    __device__ __forceinline__ float chain(float x, float dg) const { return dg * gelu_erf_grad(x); }
};

template <class Producer>
__device__ __forceinline__ float4 bwd_elem4(const Producer& f, const float4& x, const float4& gy, float s, float z, float qmin,
                                            float qmax, BwdAcc& acc) {
    float4 o;
    o.x = f.chain(x.x, bwd_elem(f.value(x.x), gy.x, s, z, qmin, qmax, acc));
    o.y = f.chain(x.y, bwd_elem(f.value(x.y), gy.y, s, z, qmin, qmax, acc));
    o.z = f.chain(x.z, bwd_elem(f.value(x.z), gy.z, s, z, qmin, qmax, acc));
    o.w = f.chain(x.w, bwd_elem(f.value(x.w), gy.w, s, z, qmin, qmax, acc));
    return o;
}

// The end of every LSQ / LSQ+ backward over a whole tensor, called by all kBwdThreads threads of every workgroup with the
// thread's float64 sums: wave tree, waves in order, the workgroup's pair published; the workgroup that arrives last adds the
// pairs in block order (lane-strided partial sums, wave tree, waves in order), applies grad_scale's factor and resets the
// tickets.  The same inputs on the same grid give the same words on every run.  gridDim.x <= kMaxBlocks.
__device__ __forceinline__ void lsq_bwd_finish(double t_ds, double t_dz, int mode, float g, float* __restrict__ dscale,
                                               float* __restrict__ dzp, double* __restrict__ partials,
                                               unsigned int* __restrict__ counter) {
    __shared__ double sh[2][kBwdThreads / OSQ_WAVE];
    t_ds = wave_sum(t_ds);
    t_dz = wave_sum(t_dz);
    const int lane = threadIdx.x & (OSQ_WAVE - 1), w = threadIdx.x / OSQ_WAVE;
    if (lane == 0) { sh[0][w] = t_ds; sh[1][w] = t_dz; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0.0, b = 0.0;
        for (int k = 0; k < kBwdThreads / OSQ_WAVE; ++k) { a += sh[0][k]; b += sh[1][k]; }
        publish_f64(&partials[2 * blockIdx.x], a);
        publish_f64(&partials[2 * blockIdx.x + 1], b);
    }
    if (grid_last_block(counter, gridDim.x)) {
        // all loads first (ordered agent-scope loads consumed one by one cost a memory round trip each),
        // then the same lane-strided summation order as before
        constexpr int kPer = kMaxBlocks / kBwdThreads;
        double pa[kPer], pb[kPer];
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
            const unsigned int k = threadIdx.x + j * kBwdThreads, kc = k < gridDim.x ? k : gridDim.x - 1;
            pa[j] = consume_f64(&partials[2 * kc]);
            pb[j] = consume_f64(&partials[2 * kc + 1]);
        }
        double a = 0.0, b = 0.0;
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
            const bool in = threadIdx.x + j * kBwdThreads < gridDim.x;
            a += in ? pa[j] : 0.0;
            b += in ? pb[j] : 0.0;
        }
        // fixed combination order: lane-strided partial sums, then wave tree, then waves in order
        a = wave_sum(a);
        b = wave_sum(b);
        __syncthreads();
        if (lane == 0) { sh[0][w] = a; sh[1][w] = b; }
        __syncthreads();
        if (threadIdx.x == 0) {
            double sa = 0.0, sb = 0.0;
            for (int k = 0; k < kBwdThreads / OSQ_WAVE; ++k) { sa += sh[0][k]; sb += sh[1][k]; }
            // grad_scale backward: d(t*g)/dt = g  (util_quant.py:70-71)
            const double gs = (mode == OSQ_PARAM_FIXED) ? 1.0 : static_cast<double>(g);
            if (dscale) dscale[0] = static_cast<float>(sa * gs);
            if (dzp) dzp[0] = static_cast<float>(sb * ((mode == OSQ_PARAM_LSQPLUS) ? static_cast<double>(g) : 1.0));
            grid_reset(counter, gridDim.x);
        }
    }
}

// The dense per-tensor backward: two 16-byte loads of x and of gy in flight per lane and trip, the tail (n % 4 elements) by
// workgroup 0, an fp32 BwdAcc per trip, doubles per thread, lsq_bwd_finish.  wt: grad_x leaves through write-through stores
// (n4 < 2^28).  With PlainProducer this is osq_lsq_backward_per_tensor; with another producer on the same grid the
// per-element terms of the sums are those of that call on value(x), so dscale / dzp are word-equal to it.
template <class Producer>
__global__ __launch_bounds__(kBwdThreads) void lsq_bwd_tensor_kernel(
    const float4* __restrict__ x, const float4* __restrict__ gy, float4* __restrict__ dx, int64_t n4,
    const float* __restrict__ xt, const float* __restrict__ gyt, float* __restrict__ dxt, int tail,
    const float* __restrict__ scale_p, const void* __restrict__ zp_p, int zp_type, int mode, float g,
    float qmin, float qmax, float* __restrict__ dscale, float* __restrict__ dzp,
    double* __restrict__ partials, unsigned int* __restrict__ counter, int wt) {
    const Producer f;
    const WtStore dwt(dx, wt ? n4 : 0);                   // wt: grad_x leaves through write-through stores (n4 < 2^28)
    const QParams p = effective_params(scale_p[0], load_zp(zp_p, zp_type), mode, g);
    const float s = p.scale, z = p.zp;
    const int64_t stride = static_cast<int64_t>(gridDim.x) * kBwdThreads;
    double t_ds = 0.0, t_dz = 0.0;
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBwdThreads + threadIdx.x; i < n4; i += 2 * stride) {
        const bool two = (i + stride) < n4;
        const float4 a0 = load_stream(&x[i]);
        const float4 b0 = load_stream(&gy[i]);
        float4 a1 = a0, b1 = b0;
        if (two) {
            a1 = load_stream(&x[i + stride]);
            b1 = load_stream(&gy[i + stride]);
        }
        BwdAcc acc = {0.f, 0.f, 0.f};
        float4 o;
        o.x = f.chain(a0.x, bwd_elem(f.value(a0.x), b0.x, s, z, qmin, qmax, acc));
        o.y = f.chain(a0.y, bwd_elem(f.value(a0.y), b0.y, s, z, qmin, qmax, acc));
        o.z = f.chain(a0.z, bwd_elem(f.value(a0.z), b0.z, s, z, qmin, qmax, acc));
        o.w = f.chain(a0.w, bwd_elem(f.value(a0.w), b0.w, s, z, qmin, qmax, acc));
        if (wt) dwt.put(i, o); else store_stream(&dx[i], o);
        if (two) {
            o.x = f.chain(a1.x, bwd_elem(f.value(a1.x), b1.x, s, z, qmin, qmax, acc));
            o.y = f.chain(a1.y, bwd_elem(f.value(a1.y), b1.y, s, z, qmin, qmax, acc));
            o.z = f.chain(a1.z, bwd_elem(f.value(a1.z), b1.z, s, z, qmin, qmax, acc));
            o.w = f.chain(a1.w, bwd_elem(f.value(a1.w), b1.w, s, z, qmin, qmax, acc));
            if (wt) dwt.put(i + stride, o); else store_stream(&dx[i + stride], o);
        }
        t_ds += static_cast<double>(acc.ds_mul) + static_cast<double>(acc.ds_div);
        t_dz += static_cast<double>(acc.dz);
    }
    if (blockIdx.x == 0 && static_cast<int>(threadIdx.x) < tail) {
        BwdAcc acc = {0.f, 0.f, 0.f};
        dxt[threadIdx.x] = f.chain(xt[threadIdx.x], bwd_elem(f.value(xt[threadIdx.x]), gyt[threadIdx.x], s, z, qmin, qmax, acc));
        t_ds += static_cast<double>(acc.ds_mul) + static_cast<double>(acc.ds_div);
        t_dz += static_cast<double>(acc.dz);
    }
    lsq_bwd_finish(t_ds, t_dz, mode, g, dscale, dzp, partials, counter);
}

// fake_quant.hip: the grid osq_lsq_backward_per_tensor launches for n4 float4s (its cap is that file's tuning knob)
int lsq_backward_grid(int64_t n4);

}  // namespace osq

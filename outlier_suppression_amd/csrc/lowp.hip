// bf16 / fp16 inputs for gfx950 (MI355X): what has no fp32 twin -- the fake-quant chain the reference runs in the input
// dtype and the per-tensor widening form.  The per-channel widening and the observer reductions are the fp32 kernels'
// bf16 / fp16 instantiations (fake_quant.hip, observer.hip; Granule<T> in osq_device.h).
//
// The reference is plain torch arithmetic on the CPU (README, "Defaults"; DESIGN.md, "16-bit inputs"):
//   * FixedFakeQuantize per-tensor (Python-number / 0-dim parameters) stays in x.dtype and rounds after EVERY op:
//       a = rd(x/s); r = rint(a); b = rd(rd(r - a) + a); c = clamp(rd(b + zp), qmin, qmax); y = rd(rd(c - zp) * s)
//     with rd = "compute in fp32, round to x.dtype" -- each rounding below is an explicit cast (hipcc: v_cvt_pk_bf16_f32 /
//     v_cvt_f16_f32, RNE, NaN stays NaN; the integer-rounding trick on the bits does not keep NaN);
//   * per-channel and the learnable rows meet fp32 [1] / [C] parameters, so their result is fp32 and equal to the same
//     call on x.float(): an exact widening load, then the fp32 kernels' arithmetic (quantize_value / dequantize_value).
// Grids and cache hints follow what the fp32 per-tensor kernel measured best (fake_quant.hip knob comments): 8192-block cap, two
// 16-byte loads in flight per lane, nt loads, write-through stores; fixed here, no osq_set_tuning key.
#include <hip/hip_ext.h>
#include "osq_device.h"
#include "osq_host.h"

namespace osq {

namespace {

constexpr int kThreads = 256;
constexpr int kUnroll = 2;                  // 16-byte loads in flight per lane of the chain (the per-tensor g_fq_unroll)
constexpr int kMaxGrid = 8192;              // the per-tensor g_fq_max_blocks

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// rd(v): round an fp32 value to T and back (exact widening)
template <typename T>
__device__ __forceinline__ float rd(float v) { return static_cast<float>(static_cast<T>(v)); }

// rd(a * b), the fp32 product held in a register before it is rounded.  Written as static_cast<T>(a * b), hipcc selects
// v_fma_mixlo_f16 a, b, +0 for T = _Float16, and (-0) * b + (+0) is +0: the sign of an exactly zero product is lost, which the
// reference keeps (an upstream gradient of -0.0 gives dx = -0.0; a product with a negative scale likewise).
template <typename T>
__device__ __forceinline__ float mul_rd(float a, float b) {
    float p = a * b;
    asm("" : "+v"(p));
    return rd<T>(p);
}

// ---------------------------------------------------------------- the in-dtype chain (FixedFakeQuantize per-tensor)

template <typename T>
struct Chain {
    float s, z, qmin, qmax;
    // x_int = rd(rd(rd(rint(a) - a) + a) + zp), a = rd(x / s)
    __device__ __forceinline__ float x_int(float x) const {
        const float a = rd<T>(x / s);
        const float r = rintf(a);
        const float b = rd<T>(rd<T>(r - a) + a);
        return rd<T>(b + z);
    }
    __device__ __forceinline__ T forward(float x) const {
        const float xi = x_int(x);
        float c = xi;                                    // torch.clamp: NaN passes
        c = (xi < qmin) ? qmin : c;
        c = (xi > qmax) ? qmax : c;
        c = rd<T>(c);
        return static_cast<T>(mul_rd<T>(rd<T>(c - z), s));
    }
    // clamp's backward keeps g where qmin <= x_int <= qmax, else +0.0 (torch.where with a zero tensor, not g * mask);
    // mul's backward g * s and div's backward g / s, each rounded to T
    __device__ __forceinline__ T backward(float x, float g) const {
        const float xi = x_int(x);
        const float gs = mul_rd<T>(g, s);
        const float m = (xi >= qmin && xi <= qmax) ? gs : 0.0f;
        return static_cast<T>(m / s);
    }
};

template <typename T>
__device__ __forceinline__ Chain<T> chain_params(const float* scale_p, const void* zp_p, int zp_type, float qmin, float qmax) {
    return Chain<T>{scale_p[0], load_zp(zp_p, zp_type), qmin, qmax};
}

// x, y: n elements; granules [0, n8) through 16-byte accesses (both pointers 16-byte aligned, else n8 == 0), the rest
// element by element over the whole grid
template <typename T, bool WT>
__global__ __launch_bounds__(kThreads) void lowp_chain_kernel(const T* __restrict__ x, T* __restrict__ y, int64_t n8, int64_t n,
                                                              const float* __restrict__ scale_p, const void* __restrict__ zp_p,
                                                              int zp_type, float qmin, float qmax) {
    typedef Granule<T> G;
    const Chain<T> ch = chain_params<T>(scale_p, zp_p, zp_type, qmin, qmax);
    const int64_t stride = static_cast<int64_t>(gridDim.x) * kThreads;
    const int64_t tid = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
    const typename G::V* x16 = reinterpret_cast<const typename G::V*>(x);
    u32x4* y16 = reinterpret_cast<u32x4*>(y);
    const WtStore yw(reinterpret_cast<float4*>(y), WT ? n8 : 0);
    int64_t i = tid;
    for (; i + (kUnroll - 1) * stride < n8; i += kUnroll * stride) {
        typename G::V v[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) v[u] = G::load_nt(&x16[i + u * stride]);
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            typename G::V o;
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = ch.forward(static_cast<float>(v[u][e]));
            if (WT) yw.put(i + u * stride, __builtin_bit_cast(float4, o));
            else __builtin_nontemporal_store(__builtin_bit_cast(u32x4, o), &y16[i + u * stride]);
        }
    }
    for (; i < n8; i += stride) {
        const typename G::V v = G::load(&x16[i]);
        typename G::V o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = ch.forward(static_cast<float>(v[e]));
        y16[i] = __builtin_bit_cast(u32x4, o);
    }
    for (int64_t j = n8 * 8 + tid; j < n; j += stride) y[j] = ch.forward(static_cast<float>(x[j]));
}

template <typename T>
__global__ __launch_bounds__(kThreads) void lowp_chain_backward_kernel(const T* __restrict__ x, const T* __restrict__ g,
                                                                       T* __restrict__ dx, int64_t n8, int64_t n,
                                                                       const float* __restrict__ scale_p,
                                                                       const void* __restrict__ zp_p, int zp_type, float qmin,
                                                                       float qmax) {
    typedef Granule<T> G;
    const Chain<T> ch = chain_params<T>(scale_p, zp_p, zp_type, qmin, qmax);
    const int64_t stride = static_cast<int64_t>(gridDim.x) * kThreads;
    const int64_t tid = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
    const typename G::V* x16 = reinterpret_cast<const typename G::V*>(x);
    const typename G::V* g16 = reinterpret_cast<const typename G::V*>(g);
    u32x4* d16 = reinterpret_cast<u32x4*>(dx);
    for (int64_t i = tid; i < n8; i += stride) {
        const typename G::V v = G::load_nt(&x16[i]), w = G::load_nt(&g16[i]);
        typename G::V o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = ch.backward(static_cast<float>(v[e]), static_cast<float>(w[e]));
        __builtin_nontemporal_store(__builtin_bit_cast(u32x4, o), &d16[i]);
    }
    for (int64_t j = n8 * 8 + tid; j < n; j += stride) dx[j] = ch.backward(static_cast<float>(x[j]), static_cast<float>(g[j]));
}

// ---------------------------------------------------------------- widening forward (fp32 result)

__device__ __forceinline__ float fq1(float x, float s, float z, float qmin, float qmax) {
    return dequantize_value(quantize_value(x, s, z, qmin, qmax), s, z);
}

// per-tensor, any parameter mode incl. OSQ_PARAM_SANITIZE (tensor_params).  A lane reads 4 elements (8 bytes) and writes
// their 16 fp32 bytes, so that every load and every store instruction of a wave covers one contiguous span (8-element
// granules would leave each 16-byte store of a wave strided by 32 bytes: measured 47.7 us at [256,128,768]).
// x 8-byte and y 16-byte aligned when n4 > 0.
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
template <typename T>
__device__ __forceinline__ float4 fq4_widen(const u32x2& w, float s, float z, float qmin, float qmax) {
    typedef T V4 __attribute__((ext_vector_type(4)));
    const V4 v = __builtin_bit_cast(V4, w);
    float4 o, q;
    fq4_plain(make_float4(static_cast<float>(v[0]), static_cast<float>(v[1]), static_cast<float>(v[2]), static_cast<float>(v[3])),
              o, q, s, z, qmin, qmax);
    return o;
}

constexpr int kWidenUnroll = 4;             // 8-byte loads in flight per lane: the bytes of two 16-byte ones

template <typename T, bool WT>
__global__ __launch_bounds__(kThreads) void lowp_widen_tensor_kernel(const T* __restrict__ x, float* __restrict__ y, int64_t n4,
                                                                     int64_t n, float* scale_p, void* zp_p, int zp_type, int mode,
                                                                     float g, float qmin, float qmax) {
    const QParams p = tensor_params(scale_p, zp_p, zp_type, mode, g, qmin, qmax);
    const int64_t stride = static_cast<int64_t>(gridDim.x) * kThreads;
    const int64_t tid = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
    const u32x2* x8 = reinterpret_cast<const u32x2*>(x);
    float4* y4 = reinterpret_cast<float4*>(y);
    const WtStore yw(y4, WT ? n4 : 0);
    int64_t i = tid;
    for (; i + (kWidenUnroll - 1) * stride < n4; i += kWidenUnroll * stride) {
        u32x2 v[kWidenUnroll];
#pragma unroll
        for (int u = 0; u < kWidenUnroll; ++u) v[u] = __builtin_nontemporal_load(&x8[i + u * stride]);
#pragma unroll
        for (int u = 0; u < kWidenUnroll; ++u) {
            const float4 o = fq4_widen<T>(v[u], p.scale, p.zp, qmin, qmax);
            if (WT) yw.put(i + u * stride, o); else store_stream(&y4[i + u * stride], o);
        }
    }
    for (; i < n4; i += stride) y4[i] = fq4_widen<T>(x8[i], p.scale, p.zp, qmin, qmax);
    for (int64_t j = n4 * 4 + tid; j < n; j += stride) y[j] = fq1(static_cast<float>(x[j]), p.scale, p.zp, qmin, qmax);
}

// ---- launchers, one per element type

template <typename T>
void launch_chain(const void* xv, void* yv, int64_t n, const float* scale, const void* zp, int zp_type, float qmin, float qmax,
                  hipStream_t st) {
    const T* x = static_cast<const T*>(xv);
    T* y = static_cast<T*>(yv);
    const int64_t n8 = (aligned16(x) && aligned16(y)) ? n / 8 : 0;
    const int grid = grid_for(n8 ? n8 : (n + 7) / 8, kThreads * kUnroll, kMaxGrid);
    if (n8 <= kWtMaxFloat4)
        hipLaunchKernelGGL((lowp_chain_kernel<T, true>), dim3(grid), dim3(kThreads), 0, st, x, y, n8, n, scale, zp, zp_type, qmin, qmax);
    else
        hipLaunchKernelGGL((lowp_chain_kernel<T, false>), dim3(grid), dim3(kThreads), 0, st, x, y, n8, n, scale, zp, zp_type, qmin, qmax);
}

template <typename T>
void launch_chain_backward(const void* xv, const void* gv, void* dv, int64_t n, const float* scale, const void* zp, int zp_type,
                           float qmin, float qmax, hipStream_t st) {
    const T* x = static_cast<const T*>(xv);
    const T* g = static_cast<const T*>(gv);
    T* dx = static_cast<T*>(dv);
    const int64_t n8 = (aligned16(x) && aligned16(g) && aligned16(dx)) ? n / 8 : 0;
    const int grid = grid_for(n8 ? n8 : (n + 7) / 8, kThreads * kUnroll, kMaxGrid);
    hipLaunchKernelGGL((lowp_chain_backward_kernel<T>), dim3(grid), dim3(kThreads), 0, st, x, g, dx, n8, n, scale, zp, zp_type,
                       qmin, qmax);
}

template <typename T>
void launch_widen_tensor(const void* xv, float* y, int64_t n, float* scale, void* zp, int zp_type, int mode, float g, float qmin,
                         float qmax, hipStream_t st) {
    const T* x = static_cast<const T*>(xv);
    const int64_t n4 = ((reinterpret_cast<uintptr_t>(x) & 7u) == 0 && aligned16(y)) ? n / 4 : 0;
    const int grid = grid_for(n4 ? n4 : (n + 3) / 4, kThreads * kWidenUnroll, kMaxGrid);
    if (n4 <= kWtMaxFloat4)
        hipLaunchKernelGGL((lowp_widen_tensor_kernel<T, true>), dim3(grid), dim3(kThreads), 0, st, x, y, n4, n, scale, zp, zp_type,
                           mode, g, qmin, qmax);
    else
        hipLaunchKernelGGL((lowp_widen_tensor_kernel<T, false>), dim3(grid), dim3(kThreads), 0, st, x, y, n4, n, scale, zp, zp_type,
                           mode, g, qmin, qmax);
}

}  // namespace
}  // namespace osq

using namespace osq;

extern "C" int osq_fake_quant_chain_lowp(int dtype, const void* x, void* y, int64_t n, const float* scale,
                                         const void* zero_point, int zp_type, int quant_min, int quant_max, osq_stream stream) {
    OSQ_REQUIRE(lowp_dtype(dtype), "fake_quant_chain_lowp: unknown dtype");
    OSQ_REQUIRE(n >= 0 && (n == 0 || (x && y)) && scale && zero_point, "fake_quant_chain_lowp: null pointer or n < 0");
    OSQ_REQUIRE(zp_type == OSQ_ZP_INT32 || zp_type == OSQ_ZP_FLOAT32, "fake_quant_chain_lowp: bad zp_type");
    if (n == 0) return OSQ_OK;
    const float qmin = static_cast<float>(quant_min), qmax = static_cast<float>(quant_max);
    OSQ_LOWP_DISPATCH(dtype, launch_chain<T>(x, y, n, scale, zero_point, zp_type, qmin, qmax, static_cast<hipStream_t>(stream)));
    return check_launch("fake_quant_chain_lowp");
}

extern "C" int osq_fake_quant_chain_backward_lowp(int dtype, const void* x, const void* grad_out, void* grad_x, int64_t n,
                                                  const float* scale, const void* zero_point, int zp_type, int quant_min,
                                                  int quant_max, osq_stream stream) {
    OSQ_REQUIRE(lowp_dtype(dtype), "fake_quant_chain_backward_lowp: unknown dtype");
    OSQ_REQUIRE(n >= 0 && (n == 0 || (x && grad_out && grad_x)) && scale && zero_point,
                "fake_quant_chain_backward_lowp: null pointer or n < 0");
    OSQ_REQUIRE(zp_type == OSQ_ZP_INT32 || zp_type == OSQ_ZP_FLOAT32, "fake_quant_chain_backward_lowp: bad zp_type");
    if (n == 0) return OSQ_OK;
    const float qmin = static_cast<float>(quant_min), qmax = static_cast<float>(quant_max);
    OSQ_LOWP_DISPATCH(dtype, launch_chain_backward<T>(x, grad_out, grad_x, n, scale, zero_point, zp_type, qmin, qmax,
                                                      static_cast<hipStream_t>(stream)));
    return check_launch("fake_quant_chain_backward_lowp");
}

extern "C" int osq_fake_quant_per_tensor_widen(int dtype, const void* x, float* y, int64_t n, float* scale, void* zero_point,
                                               int zp_type, int mode, float grad_factor, int quant_min, int quant_max,
                                               osq_stream stream) {
    OSQ_REQUIRE(lowp_dtype(dtype), "fake_quant_per_tensor_widen: unknown dtype");
    OSQ_REQUIRE(n >= 0 && (n == 0 || (x && y)) && scale && zero_point, "fake_quant_per_tensor_widen: null pointer or n < 0");
    OSQ_REQUIRE(zp_type == OSQ_ZP_INT32 || zp_type == OSQ_ZP_FLOAT32, "fake_quant_per_tensor_widen: bad zp_type");
    OSQ_REQUIRE((mode & ~(OSQ_PARAM_MODE_MASK | OSQ_PARAM_SANITIZE)) == 0 && (mode & OSQ_PARAM_MODE_MASK) <= OSQ_PARAM_LSQPLUS,
                "fake_quant_per_tensor_widen: bad mode");
    if (n == 0) return OSQ_OK;
    const float qmin = static_cast<float>(quant_min), qmax = static_cast<float>(quant_max);
    OSQ_LOWP_DISPATCH(dtype, launch_widen_tensor<T>(x, y, n, scale, zero_point, zp_type, mode, grad_factor, qmin, qmax,
                                                    static_cast<hipStream_t>(stream)));
    return check_launch("fake_quant_per_tensor_widen");
}

// bf16 / fp16 inputs for gfx950 (MI355X): the fake-quant chain the reference runs in the input dtype, the widening forms
// of the rows whose parameters promote the result to fp32, and the observer reductions, all reading 2-byte elements.
//
// The reference is plain torch arithmetic on the CPU (README, "Defaults"; DESIGN.md, "16-bit inputs"):
//   * FixedFakeQuantize per-tensor (Python-number / 0-dim parameters) stays in x.dtype and rounds after EVERY op:
//       a = rd(x/s); r = rint(a); b = rd(rd(r - a) + a); c = clamp(rd(b + zp), qmin, qmax); y = rd(rd(c - zp) * s)
//     with rd = "compute in fp32, round to x.dtype" -- each rounding below is an explicit cast (hipcc: v_cvt_pk_bf16_f32 /
//     v_cvt_f16_f32, RNE, NaN stays NaN; the integer-rounding trick on the bits does not keep NaN);
//   * per-channel and the learnable rows meet fp32 [1] / [C] parameters, so their result is fp32 and equal to the same
//     call on x.float(): an exact widening load, then the fp32 kernels' arithmetic (quantize_value / dequantize_value);
//   * the observers widen first (x_orig.to(min_val.dtype)): min / max of the widened values, then the unchanged finish.
// Grids and cache hints follow what the fp32 kernels measured best (fake_quant.hip knob comments): 8192-block cap, two
// 16-byte loads in flight per lane, nt loads, write-through stores; fixed here, no osq_set_tuning key.
#include <hip/hip_ext.h>
#include "osq_device.h"
#include "osq_host.h"

namespace osq {

namespace {

constexpr int kThreads = 256;
constexpr int kWavesPerBlock = kThreads / OSQ_WAVE;
constexpr int kUnroll = 2;                  // 16-byte loads in flight per lane (fp32 g_fq_unroll)
constexpr int kMaxGrid = 8192;              // fp32 g_fq_max_blocks
constexpr int kObsBlocks = 768;             // fp32 g_obs_blocks (grid cap of the flat min / max)

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// rd(v): round an fp32 value to T and back (exact widening)
template <typename T>
__device__ __forceinline__ float rd(float v) { return static_cast<float>(static_cast<T>(v)); }

// eight elements = one 16-byte granule
template <typename T>
struct Granule {
    typedef T V __attribute__((ext_vector_type(8)));
    __device__ static __forceinline__ V load_nt(const u32x4* p) { return __builtin_bit_cast(V, __builtin_nontemporal_load(p)); }
    __device__ static __forceinline__ V load(const u32x4* p) { return __builtin_bit_cast(V, *p); }
    __device__ static __forceinline__ float4 as_float4(const V& v) { return __builtin_bit_cast(float4, v); }
};

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
        return static_cast<T>(rd<T>(c - z) * s);
    }
    // clamp's backward keeps g where qmin <= x_int <= qmax, else +0.0 (torch.where with a zero tensor, not g * mask);
    // mul's backward g * s and div's backward g / s, each rounded to T
    __device__ __forceinline__ T backward(float x, float g) const {
        const float xi = x_int(x);
        const float gs = rd<T>(g * s);
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
    const u32x4* x16 = reinterpret_cast<const u32x4*>(x);
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
            if (WT) yw.put(i + u * stride, G::as_float4(o));
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
    const u32x4* x16 = reinterpret_cast<const u32x4*>(x);
    const u32x4* g16 = reinterpret_cast<const u32x4*>(g);
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

// eight widened elements through the fp32 chain of fq_tensor_vec_kernel / fq_channel_*_kernel
template <typename T>
__device__ __forceinline__ void fq8_widen(const typename Granule<T>::V& v, float4& o0, float4& o1, float s, float z, float qmin,
                                          float qmax) {
    float4 q;
    fq4_plain(make_float4(static_cast<float>(v[0]), static_cast<float>(v[1]), static_cast<float>(v[2]), static_cast<float>(v[3])),
              o0, q, s, z, qmin, qmax);
    fq4_plain(make_float4(static_cast<float>(v[4]), static_cast<float>(v[5]), static_cast<float>(v[6]), static_cast<float>(v[7])),
              o1, q, s, z, qmin, qmax);
}

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

// per-channel [rows = outer * channels, inner], inner % 8 == 0, 16-byte aligned: one wave per row (fq_channel_rows_kernel)
template <typename T>
__global__ __launch_bounds__(kThreads) void lowp_widen_channel_rows_kernel(const T* __restrict__ x, float* __restrict__ y,
                                                                           int64_t rows, int64_t channels, int inner8,
                                                                           const float* __restrict__ scale_p,
                                                                           const void* __restrict__ zp_p, int zp_type, int mode,
                                                                           float g, float qmin, float qmax) {
    typedef Granule<T> G;
    const int lane = threadIdx.x & (OSQ_WAVE - 1);
    const int64_t wave = (static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x) / OSQ_WAVE;
    const int64_t nwaves = static_cast<int64_t>(gridDim.x) * kWavesPerBlock;
    for (int64_t r = wave; r < rows; r += nwaves) {
        const int64_t c = r % channels;
        const QParams p = effective_params(scale_p[c], load_zp(zp_p, zp_type, c), mode, g);
        const u32x4* xr = reinterpret_cast<const u32x4*>(x) + r * inner8;
        float4* yr = reinterpret_cast<float4*>(y) + 2 * r * inner8;
        int j = lane;
        for (; j + OSQ_WAVE < inner8; j += 2 * OSQ_WAVE) {
            const typename G::V a = G::load(&xr[j]), b = G::load(&xr[j + OSQ_WAVE]);
            float4 o0, o1, o2, o3;
            fq8_widen<T>(a, o0, o1, p.scale, p.zp, qmin, qmax);
            fq8_widen<T>(b, o2, o3, p.scale, p.zp, qmin, qmax);
            yr[2 * j] = o0; yr[2 * j + 1] = o1;
            yr[2 * (j + OSQ_WAVE)] = o2; yr[2 * (j + OSQ_WAVE) + 1] = o3;
        }
        for (; j < inner8; j += OSQ_WAVE) {
            float4 o0, o1;
            fq8_widen<T>(G::load(&xr[j]), o0, o1, p.scale, p.zp, qmin, qmax);
            yr[2 * j] = o0; yr[2 * j + 1] = o1;
        }
    }
}

// generic [outer, channels, inner] (fq_channel_generic_kernel)
template <typename T>
__global__ __launch_bounds__(kThreads) void lowp_widen_channel_generic_kernel(const T* __restrict__ x, float* __restrict__ y,
                                                                              int64_t n, int64_t channels, int64_t inner,
                                                                              const float* __restrict__ scale_p,
                                                                              const void* __restrict__ zp_p, int zp_type,
                                                                              int mode, float g, float qmin, float qmax) {
    const int64_t stride = static_cast<int64_t>(gridDim.x) * kThreads;
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; i < n; i += stride) {
        const int64_t c = (i / inner) % channels;
        const QParams p = effective_params(scale_p[c], load_zp(zp_p, zp_type, c), mode, g);
        y[i] = fq1(static_cast<float>(x[i]), p.scale, p.zp, qmin, qmax);
    }
}

// ---------------------------------------------------------------- observers: min / max of the widened values

template <typename T>
__device__ __forceinline__ void add8(MinMax& acc, const typename Granule<T>::V& v) {
#pragma unroll
    for (int e = 0; e < 8; ++e) acc.add(static_cast<float>(v[e]));
}

// observe_flat_kernel on 2-byte elements: granules [0, n8) by 16-byte loads, the rest element by element; one 8-byte
// partial per workgroup, the last workgroup combines them and runs the finish step
template <typename T>
__global__ __launch_bounds__(kThreads) void lowp_observe_flat_kernel(const T* __restrict__ x, int64_t n8, int64_t n,
                                                                     float* __restrict__ partials,
                                                                     unsigned int* __restrict__ counter, Finish fin) {
    typedef Granule<T> G;
    MinMax acc;
    acc.init();
    const int64_t stride = static_cast<int64_t>(gridDim.x) * kThreads;
    const int64_t tid = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
    float st_min = 0.f, st_max = 0.f;
    if (threadIdx.x == 0 && fin.rule != OSQ_UPDATE_NONE && fin.min_val && fin.max_val) {
        st_min = fin.min_val[0];
        st_max = fin.max_val[0];
    }
    const u32x4* x16 = reinterpret_cast<const u32x4*>(x);
    int64_t i = tid;
    for (; i + 3 * stride < n8; i += 4 * stride) {
        const typename G::V a = G::load_nt(&x16[i]), b = G::load_nt(&x16[i + stride]), c = G::load_nt(&x16[i + 2 * stride]),
                            d = G::load_nt(&x16[i + 3 * stride]);
        add8<T>(acc, a); add8<T>(acc, b); add8<T>(acc, c); add8<T>(acc, d);
    }
    for (; i < n8; i += stride) add8<T>(acc, G::load(&x16[i]));
    for (int64_t j = n8 * 8 + tid; j < n; j += stride) acc.add(static_cast<float>(x[j]));
    acc = block_reduce(acc);
    unsigned long long* part64 = reinterpret_cast<unsigned long long*>(partials);
    if (threadIdx.x == 0) {
        const float pm = acc.bad ? __builtin_nanf("") : acc.mn;     // a NaN minimum flags "NaN seen"
        __hip_atomic_store(&part64[blockIdx.x],
                           (static_cast<unsigned long long>(__float_as_uint(acc.mx)) << 32) | __float_as_uint(pm),
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (grid_last_block(counter, gridDim.x)) {
        MinMax t;
        t.init();
        for (unsigned int k = threadIdx.x; k < gridDim.x; k += kThreads) {
            const unsigned long long raw = __hip_atomic_load(&part64[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const float pm = __uint_as_float(static_cast<unsigned int>(raw & 0xffffffffull));
            t.mn = fminf(t.mn, pm);
            t.mx = fmaxf(t.mx, __uint_as_float(static_cast<unsigned int>(raw >> 32)));
            t.bad |= (pm != pm);
        }
        t = block_reduce(t);
        if (threadIdx.x == 0) {
            t.poison();
            finish_entry(fin, 0, t.mn, t.mx, true, st_min, st_max);
            grid_reset(counter, gridDim.x);
        }
    }
}

// per-channel, outer == 1, inner % 8 == 0, 16-byte aligned: one wave per channel row (observe_rows_kernel)
template <typename T>
__global__ __launch_bounds__(kThreads) void lowp_observe_rows_kernel(const T* __restrict__ x, int64_t rows, int inner8, Finish fin) {
    typedef Granule<T> G;
    const int lane = threadIdx.x & (OSQ_WAVE - 1);
    const int64_t wave = (static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x) / OSQ_WAVE;
    const int64_t nwaves = static_cast<int64_t>(gridDim.x) * kWavesPerBlock;
    for (int64_t r = wave; r < rows; r += nwaves) {
        const u32x4* xr = reinterpret_cast<const u32x4*>(x) + r * inner8;
        MinMax acc;
        acc.init();
        int j = lane;
        for (; j + OSQ_WAVE < inner8; j += 2 * OSQ_WAVE) {
            const typename G::V a = G::load(&xr[j]), b = G::load(&xr[j + OSQ_WAVE]);
            add8<T>(acc, a); add8<T>(acc, b);
        }
        for (; j < inner8; j += OSQ_WAVE) add8<T>(acc, G::load(&xr[j]));
        acc.wave_reduce();
        if (lane == 0) {
            acc.poison();
            finish_entry(fin, r, acc.mn, acc.mx);
        }
    }
}

// generic [outer, channels, inner]: one workgroup per channel (observe_channels_kernel)
template <typename T>
__global__ __launch_bounds__(kThreads) void lowp_observe_channels_kernel(const T* __restrict__ x, int64_t outer, int64_t channels,
                                                                         int64_t inner, Finish fin) {
    const int64_t c = blockIdx.x;
    MinMax acc;
    acc.init();
    for (int64_t o = 0; o < outer; ++o) {
        const T* p = x + (o * channels + c) * inner;
        for (int64_t j = threadIdx.x; j < inner; j += kThreads) acc.add(static_cast<float>(p[j]));
    }
    acc = block_reduce(acc);
    if (threadIdx.x == 0) {
        acc.poison();
        finish_entry(fin, c, acc.mn, acc.mx);
    }
}

// per-token extrema, 16-byte path: stride_inner == 1, feat_inner % 8 == 0, the other strides % 8 == 0, x 16-byte aligned.
// As token_minmax_vec_kernel: workgroup = 16 consecutive tokens of one sample (blockIdx.y), chunk index rotated by the
// sample so late (mostly padded) chunks spread over the XCDs; a wave owns 4 tokens and loads all four before reducing;
// lanes split into groups of G = 2^lgG that walk the feature segments; tokens at or past lengths[b] are never read.
constexpr int kTokPerWave = 4;
constexpr int kTokPerBlock = kTokPerWave * kWavesPerBlock;

template <typename T>
__global__ __launch_bounds__(kThreads) void lowp_token_minmax_vec_kernel(const T* __restrict__ x, osq_token_view v,
                                                                         const int64_t* __restrict__ lengths,
                                                                         float* __restrict__ tok_min, float* __restrict__ tok_max,
                                                                         int lgG, int inner8) {
    typedef Granule<T> G;
    const int64_t b = blockIdx.y;
    int64_t len = v.tokens;
    if (lengths) {
        const int64_t l = lengths[b];
        len = l < len ? l : len;
    }
    const int lane = threadIdx.x & (OSQ_WAVE - 1), w = threadIdx.x / OSQ_WAVE;
    const int64_t chunk = (static_cast<int64_t>(blockIdx.x) + blockIdx.y) % gridDim.x;
    const int64_t t0 = chunk * kTokPerBlock + w * kTokPerWave;
    if (t0 >= len) return;
    const int ntok = (len - t0) < kTokPerWave ? static_cast<int>(len - t0) : kTokPerWave;
    const T* base = x + b * v.stride_batch + t0 * v.stride_token;
    MinMax acc[kTokPerWave];
#pragma unroll
    for (int k = 0; k < kTokPerWave; ++k) acc[k].init();
    const int Gs = 1 << lgG;
    const int grp = lane >> lgG, li = lane & (Gs - 1), ngrp = OSQ_WAVE >> lgG;
    for (int64_t o = grp; o < v.feat_outer; o += ngrp) {
        const T* seg = base + o * v.stride_outer;
        for (int j = li; j < inner8; j += Gs) {
            typename G::V val[kTokPerWave];
#pragma unroll
            for (int k = 0; k < kTokPerWave; ++k) {
                const int kk = k < ntok ? k : 0;             // short tail: re-read token 0, result unused
                val[k] = G::load_nt(reinterpret_cast<const u32x4*>(seg + kk * v.stride_token) + j);
            }
#pragma unroll
            for (int k = 0; k < kTokPerWave; ++k) add8<T>(acc[k], val[k]);
        }
    }
#pragma unroll
    for (int k = 0; k < kTokPerWave; ++k) {
        acc[k].wave_reduce();
        acc[k].poison();
    }
    if (lane < ntok) {
        float mn = acc[0].mn, mx = acc[0].mx;
#pragma unroll
        for (int k = 1; k < kTokPerWave; ++k)
            if (lane == k) { mn = acc[k].mn; mx = acc[k].mx; }
        const int64_t slot = b * v.tokens + t0 + lane;
        tok_min[slot] = mn;
        tok_max[slot] = mx;
    }
}

// any strides, element loads: one wave per token (token_minmax_generic_kernel)
template <typename T>
__global__ __launch_bounds__(kThreads) void lowp_token_minmax_generic_kernel(const T* __restrict__ x, osq_token_view v,
                                                                             const int64_t* __restrict__ lengths,
                                                                             float* __restrict__ tok_min,
                                                                             float* __restrict__ tok_max) {
    const int lane = threadIdx.x & (OSQ_WAVE - 1);
    const int64_t ntok = v.batch * v.tokens;
    const int64_t wave0 = (static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x) / OSQ_WAVE;
    const int64_t nwaves = static_cast<int64_t>(gridDim.x) * kWavesPerBlock;
    const int64_t F = v.feat_outer * v.feat_inner;
    for (int64_t tok = wave0; tok < ntok; tok += nwaves) {
        const int64_t b = tok / v.tokens, t = tok - b * v.tokens;
        if (lengths && t >= lengths[b]) continue;
        const T* base = x + b * v.stride_batch + t * v.stride_token;
        MinMax acc;
        acc.init();
        for (int64_t j = lane; j < F; j += OSQ_WAVE) {
            const int64_t o = j / v.feat_inner, i = j - o * v.feat_inner;
            acc.add(static_cast<float>(base[o * v.stride_outer + i * v.stride_inner]));
        }
        acc.wave_reduce();
        if (lane == 0) {
            acc.poison();
            tok_min[tok] = acc.mn;
            tok_max[tok] = acc.mx;
        }
    }
}

inline int lowp_grid(int64_t work_items, int per_block, int max_blocks) {
    int64_t b = (work_items + per_block - 1) / per_block;
    if (b < 1) b = 1;
    if (b > max_blocks) b = max_blocks;
    return static_cast<int>(b);
}

inline bool known_dtype(int dtype) { return dtype == OSQ_DTYPE_BF16 || dtype == OSQ_DTYPE_F16; }

inline int check_finish(int update_rule, const float* min_val, const float* max_val) {
    return update_rule >= OSQ_UPDATE_NONE && update_rule <= OSQ_UPDATE_AVERAGE &&
           (update_rule == OSQ_UPDATE_NONE || (min_val && max_val));
}

// ---- launchers, one per element type

template <typename T>
void launch_chain(const void* xv, void* yv, int64_t n, const float* scale, const void* zp, int zp_type, float qmin, float qmax,
                  hipStream_t st) {
    const T* x = static_cast<const T*>(xv);
    T* y = static_cast<T*>(yv);
    const int64_t n8 = (aligned16(x) && aligned16(y)) ? n / 8 : 0;
    const int grid = lowp_grid(n8 ? n8 : (n + 7) / 8, kThreads * kUnroll, kMaxGrid);
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
    const int grid = lowp_grid(n8 ? n8 : (n + 7) / 8, kThreads * kUnroll, kMaxGrid);
    hipLaunchKernelGGL((lowp_chain_backward_kernel<T>), dim3(grid), dim3(kThreads), 0, st, x, g, dx, n8, n, scale, zp, zp_type,
                       qmin, qmax);
}

template <typename T>
void launch_widen_tensor(const void* xv, float* y, int64_t n, float* scale, void* zp, int zp_type, int mode, float g, float qmin,
                         float qmax, hipStream_t st) {
    const T* x = static_cast<const T*>(xv);
    const int64_t n4 = ((reinterpret_cast<uintptr_t>(x) & 7u) == 0 && aligned16(y)) ? n / 4 : 0;
    const int grid = lowp_grid(n4 ? n4 : (n + 3) / 4, kThreads * kWidenUnroll, kMaxGrid);
    if (n4 <= kWtMaxFloat4)
        hipLaunchKernelGGL((lowp_widen_tensor_kernel<T, true>), dim3(grid), dim3(kThreads), 0, st, x, y, n4, n, scale, zp, zp_type,
                           mode, g, qmin, qmax);
    else
        hipLaunchKernelGGL((lowp_widen_tensor_kernel<T, false>), dim3(grid), dim3(kThreads), 0, st, x, y, n4, n, scale, zp, zp_type,
                           mode, g, qmin, qmax);
}

template <typename T>
void launch_widen_channel(const void* xv, float* y, int64_t outer, int64_t channels, int64_t inner, const float* scale,
                          const void* zp, int zp_type, int mode, float g, float qmin, float qmax, hipStream_t st) {
    const T* x = static_cast<const T*>(xv);
    if (aligned16(x) && aligned16(y) && inner % 8 == 0 && inner >= 64 && inner / 8 < (1 << 30)) {
        const int64_t rows = outer * channels;
        const int grid = lowp_grid(rows, kWavesPerBlock, kMaxBlocks * 2);
        hipLaunchKernelGGL((lowp_widen_channel_rows_kernel<T>), dim3(grid), dim3(kThreads), 0, st, x, y, rows, channels,
                           static_cast<int>(inner / 8), scale, zp, zp_type, mode, g, qmin, qmax);
    } else {
        const int64_t n = outer * channels * inner;
        const int grid = lowp_grid(n, kThreads, kMaxBlocks);
        hipLaunchKernelGGL((lowp_widen_channel_generic_kernel<T>), dim3(grid), dim3(kThreads), 0, st, x, y, n, channels, inner,
                           scale, zp, zp_type, mode, g, qmin, qmax);
    }
}

template <typename T>
void launch_observe_flat(const void* xv, int64_t n, const Finish& fin, const Workspace& ws, hipStream_t st) {
    const T* x = static_cast<const T*>(xv);
    const int64_t n8 = aligned16(x) ? n / 8 : 0;
    const int grid = lowp_grid(n8 ? n8 : (n + 7) / 8, kThreads * 4, kObsBlocks);
    hipLaunchKernelGGL((lowp_observe_flat_kernel<T>), dim3(grid), dim3(kThreads), 0, st, x, n8, n, ws.floats(kFamObserveFlat),
                       ws.counter(kFamObserveFlat), fin);
}

template <typename T>
void launch_observe_channels(const void* xv, int64_t outer, int64_t channels, int64_t inner, const Finish& fin, hipStream_t st) {
    const T* x = static_cast<const T*>(xv);
    if (outer == 1 && inner % 8 == 0 && aligned16(x) && inner / 8 < (1 << 30)) {
        const int grid = lowp_grid(channels, kWavesPerBlock, kMaxBlocks * 4);
        hipLaunchKernelGGL((lowp_observe_rows_kernel<T>), dim3(grid), dim3(kThreads), 0, st, x, channels, static_cast<int>(inner / 8),
                           fin);
    } else {
        hipLaunchKernelGGL((lowp_observe_channels_kernel<T>), dim3(static_cast<unsigned>(channels)), dim3(kThreads), 0, st, x, outer,
                           channels, inner, fin);
    }
}

template <typename T>
int launch_token_minmax(const void* xv, const osq_token_view& v, const int64_t* lengths, float* tmin, float* tmax, hipStream_t st) {
    const T* x = static_cast<const T*>(xv);
    const bool vec = v.stride_inner == 1 && v.feat_inner % 8 == 0 && aligned16(x) && v.stride_batch % 8 == 0 &&
                     v.stride_token % 8 == 0 && (v.feat_outer == 1 || v.stride_outer % 8 == 0) && v.feat_inner / 8 < (1 << 30) &&
                     v.batch <= 65535;
    if (vec) {
        const int inner8 = static_cast<int>(v.feat_inner / 8);
        int lgG = 6;
        if (v.feat_outer > 1) {
            lgG = 0;
            while ((1 << lgG) < inner8 && lgG < 6) ++lgG;
        }
        const dim3 tgrid(static_cast<unsigned>((v.tokens + kTokPerBlock - 1) / kTokPerBlock), static_cast<unsigned>(v.batch));
        hipLaunchKernelGGL((lowp_token_minmax_vec_kernel<T>), tgrid, dim3(kThreads), 0, st, x, v, lengths, tmin, tmax, lgG, inner8);
    } else {
        const int grid = lowp_grid(v.batch * v.tokens, kWavesPerBlock, kMaxBlocks * 8);
        hipLaunchKernelGGL((lowp_token_minmax_generic_kernel<T>), dim3(grid), dim3(kThreads), 0, st, x, v, lengths, tmin, tmax);
    }
    return OSQ_OK;
}

}  // namespace
}  // namespace osq

using namespace osq;

#define OSQ_LOWP_DISPATCH(dtype, CALL) \
    do {                                 \
        if ((dtype) == OSQ_DTYPE_BF16) { \
            typedef __bf16 T;            \
            CALL;                        \
        } else {                         \
            typedef _Float16 T;          \
            CALL;                        \
        }                                \
    } while (0)

extern "C" int osq_fake_quant_chain_lowp(int dtype, const void* x, void* y, int64_t n, const float* scale,
                                         const void* zero_point, int zp_type, int quant_min, int quant_max, osq_stream stream) {
    OSQ_REQUIRE(known_dtype(dtype), "fake_quant_chain_lowp: unknown dtype");
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
    OSQ_REQUIRE(known_dtype(dtype), "fake_quant_chain_backward_lowp: unknown dtype");
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
    OSQ_REQUIRE(known_dtype(dtype), "fake_quant_per_tensor_widen: unknown dtype");
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

extern "C" int osq_fake_quant_per_channel_widen(int dtype, const void* x, float* y, int64_t outer, int64_t channels, int64_t inner,
                                                const float* scale, const void* zero_point, int zp_type, int mode,
                                                float grad_factor, int quant_min, int quant_max, osq_stream stream) {
    OSQ_REQUIRE(known_dtype(dtype), "fake_quant_per_channel_widen: unknown dtype");
    OSQ_REQUIRE(outer >= 0 && channels >= 0 && inner >= 0 && scale && zero_point, "fake_quant_per_channel_widen: bad argument");
    OSQ_REQUIRE(zp_type == OSQ_ZP_INT32 || zp_type == OSQ_ZP_FLOAT32, "fake_quant_per_channel_widen: bad zp_type");
    OSQ_REQUIRE(mode >= OSQ_PARAM_FIXED && mode <= OSQ_PARAM_LSQPLUS, "fake_quant_per_channel_widen: bad mode");
    const int64_t n = outer * channels * inner;
    if (n == 0) return OSQ_OK;
    OSQ_REQUIRE(x && y, "fake_quant_per_channel_widen: null tensor");
    const float qmin = static_cast<float>(quant_min), qmax = static_cast<float>(quant_max);
    OSQ_LOWP_DISPATCH(dtype, launch_widen_channel<T>(x, y, outer, channels, inner, scale, zero_point, zp_type, mode, grad_factor,
                                                     qmin, qmax, static_cast<hipStream_t>(stream)));
    return check_launch("fake_quant_per_channel_widen");
}

extern "C" int osq_observe_flat_lowp(int dtype, const void* x, int64_t n, int update_rule, int64_t cnt, float* min_val,
                                     float* max_val, float* cur_minmax, int quant_min, int quant_max, int symmetric,
                                     float* scale_out, void* zero_point_out, int zp_type, void* workspace, osq_stream stream) {
    OSQ_REQUIRE(known_dtype(dtype), "observe_flat_lowp: unknown dtype");
    OSQ_REQUIRE(n > 0 && x && workspace, "observe_flat_lowp: empty tensor or null pointer");
    OSQ_REQUIRE(check_finish(update_rule, min_val, max_val), "observe_flat_lowp: bad update rule or missing min_val / max_val");
    const Finish fin{update_rule, cnt, min_val, max_val, cur_minmax, quant_min, quant_max, symmetric, scale_out, zero_point_out,
                     zp_type};
    const Workspace ws(workspace);
    OSQ_LOWP_DISPATCH(dtype, launch_observe_flat<T>(x, n, fin, ws, static_cast<hipStream_t>(stream)));
    return check_launch("observe_flat_lowp");
}

extern "C" int osq_observe_channels_lowp(int dtype, const void* x, int64_t outer, int64_t channels, int64_t inner,
                                         int update_rule, int64_t cnt, float* min_val, float* max_val, int quant_min,
                                         int quant_max, int symmetric, float* scale_out, void* zero_point_out, int zp_type,
                                         osq_stream stream) {
    OSQ_REQUIRE(known_dtype(dtype), "observe_channels_lowp: unknown dtype");
    OSQ_REQUIRE(outer > 0 && channels > 0 && inner > 0 && x, "observe_channels_lowp: empty tensor or null pointer");
    OSQ_REQUIRE(channels < (1ll << 31), "observe_channels_lowp: too many channels");
    OSQ_REQUIRE(check_finish(update_rule, min_val, max_val), "observe_channels_lowp: bad update rule or missing min_val / max_val");
    const Finish fin{update_rule, cnt, min_val, max_val, nullptr, quant_min, quant_max, symmetric, scale_out, zero_point_out,
                     zp_type};
    OSQ_LOWP_DISPATCH(dtype, launch_observe_channels<T>(x, outer, channels, inner, fin, static_cast<hipStream_t>(stream)));
    return check_launch("observe_channels_lowp");
}

extern "C" int osq_token_minmax_lowp(int dtype, const void* x, const osq_token_view* view, const int64_t* lengths,
                                     float* token_min, float* token_max, osq_stream stream) {
    OSQ_REQUIRE(known_dtype(dtype), "token_minmax_lowp: unknown dtype");
    OSQ_REQUIRE(x && view && token_min && token_max, "token_minmax_lowp: null pointer");
    const osq_token_view v = *view;
    OSQ_REQUIRE(v.batch > 0 && v.tokens > 0 && v.feat_outer > 0 && v.feat_inner > 0, "token_minmax_lowp: empty view");
    OSQ_LOWP_DISPATCH(dtype, launch_token_minmax<T>(x, v, lengths, token_min, token_max, static_cast<hipStream_t>(stream)));
    return check_launch("token_minmax_lowp");
}

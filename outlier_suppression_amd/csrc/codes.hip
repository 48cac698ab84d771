// Integer codes of a quantised tensor for gfx950 (MI355X): what a W8 / W4 checkpoint stores, and back.
//
// u = x_quant - quant_min of util_quant.py:12-13, an unsigned integer in [0, quant_max - quant_min], one byte per element
// (code_bits 8) or two elements per byte (code_bits 4: byte k of the flattened tensor = element 2k in the low nibble,
// 2k + 1 in the high one).  The arithmetic is quantize_value / dequantize_value / effective_params of osq_device.h -- the
// chain of fake_quant.hip, not a copy of it -- so that (float(u + quant_min) - zp) * s is the fake-quant y word for word.
// Quantising reads 4 B (2 B for bf16 / fp16) and writes 1 or 0.5 B per element; dequantising reads 1 or 0.5 B and writes
// 4 B: 5 or 4.5 B per element where the fake-quant refresh of the same weights moves 8.
#include <algorithm>
#include "codes_device.h"
#include "osq_host.h"

namespace osq {

constexpr int kThreads = kCodeThreads;
constexpr int kUnroll = 4;         // dequantiser: code words in flight per lane (one word = four elements = one float4 of y)

__device__ __forceinline__ void write_effective(float* scale_eff, float* zp_eff, int64_t c, const QParams& p) {
    if (scale_eff) scale_eff[c] = p.scale;
    if (zp_eff) zp_eff[c] = p.zp;
}

// ---------------------------------------------------------------- quantise: rows

// What one lane owns of a row: a run of kElems consecutive elements = kLoads 16-byte granules of T = kWords 32-bit words
// of codes, stored with ONE instruction -- 16 bytes (WIDE: the row's code bytes are a multiple of 16, so every lane's run
// starts on a 16-byte boundary) or else the fewest whole words a granule fills (4 bytes; 8 for a 16-bit T at 8 code bits).
// A lane owns whole bytes: no two lanes write one byte, nibbles included.
template <typename T, int BITS, bool WIDE>
struct CodeRun {
    typedef Granule<T> G;
    static constexpr int kNarrow = (32 / BITS > G::kPer) ? 32 / BITS : G::kPer;
    static constexpr int kElems = WIDE ? 128 / BITS : kNarrow;
    static constexpr int kLoads = kElems / G::kPer;
    static constexpr int kWords = kElems * BITS / 32;
    static constexpr int kTrip = (G::kRowLoads / kLoads > 1) ? G::kRowLoads / kLoads : 1;      // runs per lane per unrolled trip
    static_assert(kLoads >= 1 && kWords >= 1 && kLoads * G::kPer == kElems && kWords * 32 == kElems * BITS, "a run is whole granules and whole words");
};
constexpr int code_run_elems(int dtype, int code_bits, bool wide) {      // CodeRun<T, BITS, WIDE>::kElems for the launcher
    return wide ? 128 / code_bits : std::max(32 / code_bits, dtype == OSQ_DTYPE_F32 ? 4 : 8);
}

typedef unsigned int osq_v2u32 __attribute__((ext_vector_type(2)));

// [rows = outer * channels, inner], inner a whole number of runs: one wave walks whole rows (fq_channel_rows_kernel's
// scheme), the row's parameters are wave-uniform.  All of a trip's 16-byte loads leave before any arithmetic.
template <typename T, int BITS, bool WIDE>
__global__ __launch_bounds__(kThreads) void codes_quantize_rows_kernel(
    const typename Granule<T>::V* __restrict__ x, unsigned int* __restrict__ codes, int64_t rows, int64_t channels, int inner_runs,
    const float* __restrict__ scale_p, const void* __restrict__ zp_p, int zp_type, int mode, float g, float qmin, float qmax,
    float* __restrict__ scale_eff, float* __restrict__ zp_eff, int32_t* __restrict__ rejected) {
    typedef CodeRun<T, BITS, WIDE> C;
    typedef Granule<T> G;
    const int lane = threadIdx.x & (OSQ_WAVE - 1);
    const int64_t wave = (static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x) / OSQ_WAVE;
    const int64_t nwaves = static_cast<int64_t>(gridDim.x) * (kThreads / OSQ_WAVE);
    unsigned int rej = 0;
    for (int64_t r = wave; r < rows; r += nwaves) {
        const int64_t c = r % channels;
        const QParams p = effective_params(scale_p[c], load_zp(zp_p, zp_type, c), mode, g);
        if (r < channels && lane == 0) write_effective(scale_eff, zp_eff, c, p);          // once per channel: the rows of outer index 0
        const typename G::V* xr = x + r * inner_runs * C::kLoads;
        unsigned int* cr = codes + r * inner_runs * C::kWords;
        // run j of the row: its elements in order into the words, element e at bit e * BITS
        const auto put_run = [&](const typename G::V (&v)[C::kLoads], const int j) {
            unsigned int w[C::kWords];
#pragma unroll
            for (int k = 0; k < C::kWords; ++k) w[k] = 0u;
#pragma unroll
            for (int l = 0; l < C::kLoads; ++l) {
                float4 f[G::kWide];
                G::widen(v[l], f);
#pragma unroll
                for (int k = 0; k < G::kWide; ++k) {
                    const int e = l * G::kPer + 4 * k;
                    w[(e * BITS) / 32] |= (code_of(f[k].x, p, qmin, qmax, rej) << ((e * BITS) % 32)) |
                                          (code_of(f[k].y, p, qmin, qmax, rej) << (((e + 1) * BITS) % 32)) |
                                          (code_of(f[k].z, p, qmin, qmax, rej) << (((e + 2) * BITS) % 32)) |
                                          (code_of(f[k].w, p, qmin, qmax, rej) << (((e + 3) * BITS) % 32));
                }
            }
            unsigned int* dst = cr + static_cast<int64_t>(j) * C::kWords;
            if constexpr (C::kWords == 4) {
                osq_v4u32 o;
                o.x = w[0]; o.y = w[1]; o.z = w[2]; o.w = w[3];
                *reinterpret_cast<osq_v4u32*>(dst) = o;
            } else if constexpr (C::kWords == 2) {
                osq_v2u32 o;
                o.x = w[0]; o.y = w[1];
                *reinterpret_cast<osq_v2u32*>(dst) = o;
            } else {
                static_assert(C::kWords == 1, "a narrow run is one or two words");
                dst[0] = w[0];
            }
        };
        int j = lane;
        for (; j + (C::kTrip - 1) * OSQ_WAVE < inner_runs; j += C::kTrip * OSQ_WAVE) {
            typename G::V v[C::kTrip][C::kLoads];
#pragma unroll
            for (int u = 0; u < C::kTrip; ++u)
#pragma unroll
                for (int l = 0; l < C::kLoads; ++l) v[u][l] = G::load(&xr[static_cast<int64_t>(j + u * OSQ_WAVE) * C::kLoads + l]);
#pragma unroll
            for (int u = 0; u < C::kTrip; ++u) put_run(v[u], j + u * OSQ_WAVE);
        }
        for (; j < inner_runs; j += OSQ_WAVE) {
            typename G::V v[C::kLoads];
#pragma unroll
            for (int l = 0; l < C::kLoads; ++l) v[l] = G::load(&xr[static_cast<int64_t>(j) * C::kLoads + l]);
            put_run(v, j);
        }
    }
    add_rejected(rejected, rej);
}

// generic [outer, channels, inner], any alignment, any n: a thread owns one BYTE of codes -- one element, or the two that
// share it (element n of an odd n does not exist: its nibble is 0); channel = (i / inner) % channels per element
template <typename T, int BITS>
__global__ __launch_bounds__(kThreads) void codes_quantize_generic_kernel(
    const T* __restrict__ x, uint8_t* __restrict__ codes, int64_t n, int64_t channels, int64_t inner,
    const float* __restrict__ scale_p, const void* __restrict__ zp_p, int zp_type, int mode, float g, float qmin, float qmax,
    float* __restrict__ scale_eff, float* __restrict__ zp_eff, int32_t* __restrict__ rejected) {
    constexpr int kPerByte = 8 / BITS;
    const int64_t nbytes = (n + kPerByte - 1) / kPerByte;
    const int64_t stride = static_cast<int64_t>(gridDim.x) * kThreads;
    unsigned int rej = 0;
    for (int64_t b = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; b < nbytes; b += stride) {
        unsigned int byte = 0u;
#pragma unroll
        for (int k = 0; k < kPerByte; ++k) {
            const int64_t i = b * kPerByte + k;
            if (i < n) {
                const int64_t row = i / inner, c = row % channels;
                const QParams p = effective_params(scale_p[c], load_zp(zp_p, zp_type, c), mode, g);
                if (row < channels && i == row * inner) write_effective(scale_eff, zp_eff, c, p);     // outer index 0, first element
                byte |= code_of(static_cast<float>(x[i]), p, qmin, qmax, rej) << (BITS * k);
            }
        }
        codes[b] = static_cast<uint8_t>(byte);
    }
    add_rejected(rejected, rej);
}

// ---------------------------------------------------------------- dequantise

// four consecutive elements of a row = one float4 of y = one word of codes: 4 bytes, or 2 at four code bits
template <int BITS>
__device__ __forceinline__ unsigned int load_codes4(const uint8_t* row, int j) {
    if constexpr (BITS == 8) return reinterpret_cast<const unsigned int*>(row)[j];
    else return reinterpret_cast<const unsigned short*>(row)[j];
}
template <int BITS>
__device__ __forceinline__ float4 decode4(unsigned int w, int quant_min, float s, float z) {
    constexpr unsigned int kMask = (1u << BITS) - 1u;
    return make_float4(value_of(w & kMask, quant_min, s, z), value_of((w >> BITS) & kMask, quant_min, s, z),
                       value_of((w >> (2 * BITS)) & kMask, quant_min, s, z), value_of((w >> (3 * BITS)) & kMask, quant_min, s, z));
}

// One wave, one row of inner4 float4s: lane j takes word j, j + 64, ... -- code loads and y stores are both dense across
// the wave.  The row's first code words leave before its parameters are read (as in fq_weights_multi_kernel).
template <int BITS>
__device__ __forceinline__ void dequantize_row(const uint8_t* cr, float4* yr, int inner4, int lane, int quant_min,
                                               const float* scale_c, const float* zp_c) {
    for (int j = lane; j < inner4; j += kUnroll * OSQ_WAVE) {
        unsigned int w[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u)
            if (j + u * OSQ_WAVE < inner4) w[u] = load_codes4<BITS>(cr, j + u * OSQ_WAVE);
        const float s = *scale_c, z = *zp_c;
#pragma unroll
        for (int u = 0; u < kUnroll; ++u)
            if (j + u * OSQ_WAVE < inner4) yr[j + u * OSQ_WAVE] = decode4<BITS>(w[u], quant_min, s, z);     // plain stores: the next GEMM's operand
    }
}

template <int BITS>
__global__ __launch_bounds__(kThreads) void codes_dequantize_rows_kernel(
    const uint8_t* __restrict__ codes, float4* __restrict__ y, int64_t rows, int64_t channels, int inner4,
    const float* __restrict__ scale_eff, const float* __restrict__ zp_eff, int quant_min) {
    const int lane = threadIdx.x & (OSQ_WAVE - 1);
    const int64_t wave = (static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x) / OSQ_WAVE;
    const int64_t nwaves = static_cast<int64_t>(gridDim.x) * (kThreads / OSQ_WAVE);
    const int64_t row_bytes = static_cast<int64_t>(inner4) * (BITS / 2);
    for (int64_t r = wave; r < rows; r += nwaves) {
        const int64_t c = r % channels;
        dequantize_row<BITS>(codes + r * row_bytes, y + r * inner4, inner4, lane, quant_min, scale_eff + c, zp_eff + c);
    }
}

template <int BITS>
__global__ __launch_bounds__(kThreads) void codes_dequantize_generic_kernel(
    const uint8_t* __restrict__ codes, float* __restrict__ y, int64_t n, int64_t channels, int64_t inner,
    const float* __restrict__ scale_eff, const float* __restrict__ zp_eff, int quant_min) {
    const int64_t stride = static_cast<int64_t>(gridDim.x) * kThreads;
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; i < n; i += stride) {
        const int64_t c = (i / inner) % channels;
        const unsigned int u = BITS == 8 ? codes[i] : (codes[i >> 1] >> (4 * (i & 1))) & 15u;
        y[i] = value_of(u, quant_min, scale_eff[c], zp_eff[c]);
    }
}

// A table of coded tensors in ONE launch -- what loading a checkpoint of 77 weights needs.  fq_weights_multi_kernel's
// scheme: wave = one row of one tensor, found by bisection over the running row counts (in LDS up to kMultiLdsWeights
// entries, out of global memory beyond), the descriptor read through the scalar cache (wave-uniform index).
__global__ __launch_bounds__(kThreads) void codes_dequantize_multi_kernel(const osq_codes_desc* __restrict__ descs,
                                                                          const int64_t* __restrict__ row_end, int n,
                                                                          int64_t total_rows) {
    __shared__ int64_t s_end[kMultiLdsWeights];
    const bool in_lds = n <= kMultiLdsWeights;
    if (in_lds) {
        for (int k = threadIdx.x; k < n; k += kThreads) s_end[k] = row_end[k];
        __syncthreads();
    }
    const int64_t* ends = in_lds ? s_end : row_end;
    const int lane = threadIdx.x & (OSQ_WAVE - 1);
    const int64_t wave = (static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x) / OSQ_WAVE;
    const int64_t nwaves = static_cast<int64_t>(gridDim.x) * (kThreads / OSQ_WAVE);
    for (int64_t g = wave; g < total_rows; g += nwaves) {
        int lo = 0, hi = n - 1;                       // first tensor whose row_end exceeds g
        if (in_lds) {
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (s_end[mid] > g) hi = mid; else lo = mid + 1;
            }
        } else {
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (row_end[mid] > g) hi = mid; else lo = mid + 1;
            }
        }
        lo = __builtin_amdgcn_readfirstlane(lo);
        const osq_codes_desc d = descs[lo];
        const int64_t r = g - (lo ? ends[lo - 1] : 0);
        const int64_t c = d.channels == 1 ? 0 : r % d.channels;
        const int inner4 = static_cast<int>(d.inner / 4);
        float4* yr = reinterpret_cast<float4*>(d.y) + r * inner4;
        if (d.code_bits == 4) dequantize_row<4>(d.codes + r * inner4 * 2, yr, inner4, lane, d.quant_min, d.scale_eff + c, d.zp_eff + c);
        else dequantize_row<8>(d.codes + r * inner4 * 4, yr, inner4, lane, d.quant_min, d.scale_eff + c, d.zp_eff + c);
    }
}

// ---------------------------------------------------------------- launchers

// Which kernel: x and codes 16-byte aligned and inner a whole number of runs -> rows (16-byte code stores where a row's
// code bytes are a multiple of 16); anything else -- odd inner, a channel axis whose inner is 1, a misaligned pointer,
// an odd n -- the generic kernel, same results.  (Not OSQ_ERR_UNSUPPORTED plus a host-side copy: a copy of x costs more
// than the generic kernel's scalar accesses, and a byte-offset codes buffer has no aligned twin at all.)
template <typename T, int BITS>
static void launch_quantize_codes(const T* x, uint8_t* codes, int dtype, int64_t outer, int64_t channels, int64_t inner,
                                  const float* scale, const void* zero_point, int zp_type, int mode, float g, float qmin, float qmax,
                                  float* scale_eff, float* zp_eff, int32_t* rejected, hipStream_t st) {
    typedef Granule<T> G;
    const int64_t rows = outer * channels;
    const int narrow = code_run_elems(dtype, BITS, false), wide = code_run_elems(dtype, BITS, true);
    if (aligned16(x) && aligned16(codes) && inner % narrow == 0 && inner / narrow < (1ll << 30)) {
        const int grid = grid_for(rows, kThreads / OSQ_WAVE, kMaxBlocks * 2);
        const typename G::V* xg = reinterpret_cast<const typename G::V*>(x);
        unsigned int* cw = reinterpret_cast<unsigned int*>(codes);
        if (inner % wide == 0)
            hipLaunchKernelGGL((codes_quantize_rows_kernel<T, BITS, true>), dim3(grid), dim3(kThreads), 0, st, xg, cw, rows, channels,
                               static_cast<int>(inner / wide), scale, zero_point, zp_type, mode, g, qmin, qmax, scale_eff, zp_eff, rejected);
        else
            hipLaunchKernelGGL((codes_quantize_rows_kernel<T, BITS, false>), dim3(grid), dim3(kThreads), 0, st, xg, cw, rows, channels,
                               static_cast<int>(inner / narrow), scale, zero_point, zp_type, mode, g, qmin, qmax, scale_eff, zp_eff, rejected);
    } else {
        const int64_t n = rows * inner;
        const int grid = grid_for((n + 8 / BITS - 1) / (8 / BITS), kThreads);
        hipLaunchKernelGGL((codes_quantize_generic_kernel<T, BITS>), dim3(grid), dim3(kThreads), 0, st, x, codes, n, channels, inner,
                           scale, zero_point, zp_type, mode, g, qmin, qmax, scale_eff, zp_eff, rejected);
    }
}

static bool code_range_fits(int quant_min, int quant_max, int code_bits) {
    const int64_t span = static_cast<int64_t>(quant_max) - quant_min;
    return span >= 0 && span <= (code_bits == 4 ? 15 : 255);
}

}  // namespace osq

using namespace osq;

extern "C" int osq_quantize_codes(int dtype, const void* x, uint8_t* codes, int64_t outer, int64_t channels, int64_t inner,
                                  const float* scale, const void* zero_point, int zp_type, int mode, float grad_factor,
                                  int quant_min, int quant_max, int code_bits, float* scale_eff, float* zp_eff,
                                  int32_t* rejected, osq_stream stream) {
    OSQ_REQUIRE(known_dtype(dtype), "quantize_codes: unknown dtype");
    OSQ_REQUIRE(code_bits == 4 || code_bits == 8, "quantize_codes: code_bits must be 4 or 8");
    OSQ_REQUIRE(code_range_fits(quant_min, quant_max, code_bits), "quantize_codes: quant_max - quant_min does not fit code_bits (15 for 4, 255 for 8)");
    OSQ_REQUIRE(outer >= 0 && channels >= 1 && inner >= 0, "quantize_codes: need outer >= 0, channels >= 1, inner >= 0");
    OSQ_REQUIRE(scale && zero_point, "quantize_codes: null scale or zero_point");
    OSQ_REQUIRE(zp_type == OSQ_ZP_INT32 || zp_type == OSQ_ZP_FLOAT32, "quantize_codes: bad zp_type");
    OSQ_REQUIRE(mode >= OSQ_PARAM_FIXED && mode <= OSQ_PARAM_LSQPLUS, "quantize_codes: bad mode");
    if (outer * channels * inner == 0) return OSQ_OK;
    OSQ_REQUIRE(x && codes, "quantize_codes: null tensor");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const float qmin = static_cast<float>(quant_min), qmax = static_cast<float>(quant_max);
    if (code_bits == 4)
        OSQ_DTYPE_DISPATCH(dtype, (launch_quantize_codes<T, 4>(static_cast<const T*>(x), codes, dtype, outer, channels, inner, scale, zero_point,
                                                               zp_type, mode, grad_factor, qmin, qmax, scale_eff, zp_eff, rejected, st)));
    else
        OSQ_DTYPE_DISPATCH(dtype, (launch_quantize_codes<T, 8>(static_cast<const T*>(x), codes, dtype, outer, channels, inner, scale, zero_point,
                                                               zp_type, mode, grad_factor, qmin, qmax, scale_eff, zp_eff, rejected, st)));
    return check_launch("quantize_codes");
}

extern "C" int osq_dequantize_codes(const uint8_t* codes, float* y, int64_t outer, int64_t channels, int64_t inner,
                                    const float* scale_eff, const float* zp_eff, int quant_min, int code_bits, osq_stream stream) {
    OSQ_REQUIRE(code_bits == 4 || code_bits == 8, "dequantize_codes: code_bits must be 4 or 8");
    OSQ_REQUIRE(outer >= 0 && channels >= 1 && inner >= 0, "dequantize_codes: need outer >= 0, channels >= 1, inner >= 0");
    OSQ_REQUIRE(scale_eff && zp_eff, "dequantize_codes: null scale_eff or zp_eff");
    const int64_t rows = outer * channels, n = rows * inner;
    if (n == 0) return OSQ_OK;
    OSQ_REQUIRE(codes && y, "dequantize_codes: null tensor");
    hipStream_t st = static_cast<hipStream_t>(stream);
    // rows: y in float4s, a row's codes in whole 4-byte (2-byte at four code bits) words; anything else the generic kernel
    const uintptr_t word = code_bits == 8 ? 4u : 2u;
    if (aligned16(y) && inner % 4 == 0 && (reinterpret_cast<uintptr_t>(codes) & (word - 1u)) == 0 && inner / 4 < (1ll << 30)) {
        const int grid = grid_for(rows, kThreads / OSQ_WAVE, kMaxBlocks * 2);
        const int inner4 = static_cast<int>(inner / 4);
        if (code_bits == 4)
            hipLaunchKernelGGL(codes_dequantize_rows_kernel<4>, dim3(grid), dim3(kThreads), 0, st, codes, reinterpret_cast<float4*>(y), rows,
                               channels, inner4, scale_eff, zp_eff, quant_min);
        else
            hipLaunchKernelGGL(codes_dequantize_rows_kernel<8>, dim3(grid), dim3(kThreads), 0, st, codes, reinterpret_cast<float4*>(y), rows,
                               channels, inner4, scale_eff, zp_eff, quant_min);
    } else {
        const int grid = grid_for(n, kThreads);
        if (code_bits == 4)
            hipLaunchKernelGGL(codes_dequantize_generic_kernel<4>, dim3(grid), dim3(kThreads), 0, st, codes, y, n, channels, inner, scale_eff,
                               zp_eff, quant_min);
        else
            hipLaunchKernelGGL(codes_dequantize_generic_kernel<8>, dim3(grid), dim3(kThreads), 0, st, codes, y, n, channels, inner, scale_eff,
                               zp_eff, quant_min);
    }
    return check_launch("dequantize_codes");
}

extern "C" int osq_dequantize_codes_multi(const osq_codes_desc* descs, const int64_t* row_end, int n_tensors, int64_t total_rows,
                                          osq_stream stream) {
    OSQ_REQUIRE(n_tensors >= 0 && total_rows >= 0, "dequantize_codes_multi: negative size");
    if (n_tensors == 0 || total_rows == 0) return OSQ_OK;
    OSQ_REQUIRE(descs && row_end, "dequantize_codes_multi: null table");
    const int grid = static_cast<int>(std::min<int64_t>((total_rows + kThreads / OSQ_WAVE - 1) / (kThreads / OSQ_WAVE), kMaxBlocks * 4));
    hipLaunchKernelGGL(codes_dequantize_multi_kernel, dim3(grid), dim3(kThreads), 0, static_cast<hipStream_t>(stream), descs, row_end,
                       n_tensors, total_rows);
    return check_launch("dequantize_codes_multi");
}

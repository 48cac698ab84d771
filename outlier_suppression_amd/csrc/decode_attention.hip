// Attention of ONE decoding step over the KV cache: scores, mask, softmax, probabilities quantizer, context, merge-heads
// context quantizer in ONE launch.
//
// QuantizedBartAttention._attend (model/quant_bart.py) runs, for a step's single query token, a batched matmul with M = 1,
// a mask add, a softmax, the probabilities quantizer, a second M = 1 batched matmul and the merge-heads context quantizer:
// five or six launches per attention block.  With one query row attention is two matrix-vector products over the cache
// with a softmax between them -- a streaming job: every byte of K and V is read once, nothing is reused.
//
//     s[j] = dot(q, k[j]) + mask[j]            q already fake-quantised and scaled (osq_fake_quant_kv_append's query site)
//     p    = softmax(s)                        row max subtracted, ocml's accurate expf, p = e * (1 / sum): the arithmetic of
//                                              attention_softmax_fq_kernel (attention.hip)
//     p'   = fq(p)                             attention_probs quantizer (quantize_value / dequantize_value, tensor_params)
//     c    = sum_j p'[j] * v[j]
//     out  = fq(c)                             context quantizer, written in the merged [batch, 1, heads * head_dim] layout
//
// Launch shape: one 256-thread workgroup per (batch, head).  LPR = head_dim / 4 lanes cover a row of K or V with one
// float4 each, so a wave takes R = 64 / LPR rows per load and the four waves 4 R rows per trip; kTripsInFlight trips are
// loaded before the first is reduced.  Scores, then exps, then fake-quantised probabilities live in LDS (kv_len floats,
// 16 KB at the limit of 4096) and pass between the three phases through two barriers; the second product's four per-wave
// partial vectors meet in LDS (4 x head_dim floats) and are added in wave order.  Traffic per (b, h): 2 * kv_len *
// head_dim * 4 B of K and V, head_dim * 4 B of q, kv_len * 4 B of mask, head_dim * 4 B written.
//
// Summation order, fixed by (head_dim, kv_len) alone -- not by cap, alignment or placement; no float atomics:
//   a score      four products of a lane added left to right, then an xor butterfly over the row's LPR lanes
//                (strides 1, 2, 4, ... : both partners of a step hold the same sum bit for bit);
//   the softmax  denominator: thread t adds exps t, t + 256, ... in order, wave_sum_f32, then (w0 + w1) + (w2 + w3);
//   a context    element: lane (wave w, row r) adds its positions (4 i + w) R + r for i = 0, 1, ... in order, an xor
//                butterfly over the wave's R row groups (strides LPR, 2 LPR, ... 32), then ((w0 + w1) + w2) + w3.
#include <math.h>
#include <hip/hip_runtime.h>
#include "osq_device.h"
#include "osq_host.h"

namespace osq {

constexpr int kDecThreads = 256;
constexpr int kDecWaves = kDecThreads / OSQ_WAVE;
constexpr int kDecMaxKv = 4096;          // the row of scores / probabilities in LDS: 16 KB
constexpr int kTripsInFlight = 4;        // loads issued per lane before the first reduction

struct DecQuant {              // one quantizer of the site; scale == nullptr: no quantizer, values pass through
    float* scale;              // written only under OSQ_PARAM_SANITIZE
    void* zero_point;
    int zp_type, mode;
    float grad_factor, qmin, qmax;
};

struct DecArgs {
    const float* q;            // [batch, heads, 1, head_dim] dense
    const float* k;            // [batch, heads, k_cap, head_dim], positions [0, kv_len) read
    const float* v;            // [batch, heads, v_cap, head_dim]
    const float* mask;         // nullable, [batch, 1, 1, kv_len] dense, additive
    float* out;                // [batch, 1, heads * head_dim] dense
    float* probs_out;          // nullable, [batch, heads, 1, kv_len] dense
    int64_t heads, k_cap, v_cap;
    int kv_len;
    DecQuant probs, ctx;
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

template <int LPR>
__global__ __launch_bounds__(kDecThreads) void decode_attention_fq_kernel(DecArgs a) {
    constexpr int R = OSQ_WAVE / LPR;              // rows of K / V one wave load covers
    constexpr int kTrip = kDecWaves * R;           // positions one trip of the workgroup covers
    __shared__ float s_p[kDecMaxKv];               // scores -> exps -> fake-quantised probabilities
    __shared__ float4 s_part[kDecWaves][LPR];      // per-wave partial context vectors
    __shared__ float s_red[2][kDecWaves];          // per-wave maxima and sums of exps

    const int lane = threadIdx.x & (OSQ_WAVE - 1), w = threadIdx.x / OSQ_WAVE;
    const int r = lane / LPR, c = lane % LPR;
    const int64_t bh = blockIdx.x;
    const int n = a.kv_len;
    const int trips = (n + kTrip - 1) / kTrip;
    const QParams pq = dec_params(a.probs), cq = dec_params(a.ctx);

    // ---- scores
    const float4 q4 = reinterpret_cast<const float4*>(a.q)[bh * LPR + c];
    const float4* kb = reinterpret_cast<const float4*>(a.k) + bh * a.k_cap * LPR + c;
    const float* mrow = a.mask ? a.mask + (bh / a.heads) * n : nullptr;
    for (int t0 = 0; t0 < trips; t0 += kTripsInFlight) {
        float4 kk[kTripsInFlight];
#pragma unroll
        for (int u = 0; u < kTripsInFlight; ++u) {
            const int j = ((t0 + u) * kDecWaves + w) * R + r;
            kk[u] = load_stream(kb + static_cast<int64_t>(j < n ? j : n - 1) * LPR);     // past the end: the last row again, unused
        }
#pragma unroll
        for (int u = 0; u < kTripsInFlight; ++u) {
            const int j = ((t0 + u) * kDecWaves + w) * R + r;
            float d = q4.x * kk[u].x;
            d = d + q4.y * kk[u].y;
            d = d + q4.z * kk[u].z;
            d = d + q4.w * kk[u].w;
            d = row_lanes_sum<LPR>(d);
            if (c == 0 && j < n) s_p[j] = mrow ? d + mrow[j] : d;
        }
    }
    __syncthreads();

    // ---- softmax and the probabilities quantizer: thread t owns positions t, t + 256, ...
    float mx = -INFINITY;
    for (int j = threadIdx.x; j < n; j += kDecThreads) mx = fmaxf(mx, s_p[j]);     // fmaxf drops a NaN: its exp makes the sum NaN
    mx = wave_max(mx);
    if (lane == 0) s_red[0][w] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(s_red[0][0], s_red[0][1]), fmaxf(s_red[0][2], s_red[0][3]));
    float sum = 0.f;
    for (int j = threadIdx.x; j < n; j += kDecThreads) {
        const float e = expf(s_p[j] - mx);
        s_p[j] = e;
        sum += e;
    }
    sum = wave_sum_f32(sum);
    if (lane == 0) s_red[1][w] = sum;
    __syncthreads();
    const float rcp = 1.0f / ((s_red[1][0] + s_red[1][1]) + (s_red[1][2] + s_red[1][3]));
    float* prow = a.probs_out ? a.probs_out + bh * n : nullptr;
    for (int j = threadIdx.x; j < n; j += kDecThreads) {
        const float p = dec_fq(s_p[j] * rcp, a.probs, pq);
        s_p[j] = p;
        if (prow) prow[j] = p;
    }
    __syncthreads();

    // ---- context
    const float4* vb = reinterpret_cast<const float4*>(a.v) + bh * a.v_cap * LPR + c;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int t0 = 0; t0 < trips; t0 += kTripsInFlight) {
        float4 vv[kTripsInFlight];
#pragma unroll
        for (int u = 0; u < kTripsInFlight; ++u) {
            const int j = ((t0 + u) * kDecWaves + w) * R + r;
            vv[u] = load_stream(vb + static_cast<int64_t>(j < n ? j : n - 1) * LPR);
        }
#pragma unroll
        for (int u = 0; u < kTripsInFlight; ++u) {
            const int j = ((t0 + u) * kDecWaves + w) * R + r;
            if (j < n) {
                const float p = s_p[j];
                acc.x = acc.x + p * vv[u].x;
                acc.y = acc.y + p * vv[u].y;
                acc.z = acc.z + p * vv[u].z;
                acc.w = acc.w + p * vv[u].w;
            }
        }
    }
    acc.x = row_groups_sum<LPR>(acc.x);
    acc.y = row_groups_sum<LPR>(acc.y);
    acc.z = row_groups_sum<LPR>(acc.z);
    acc.w = row_groups_sum<LPR>(acc.w);
    if (r == 0) s_part[w][c] = acc;
    __syncthreads();
    if (threadIdx.x < LPR) {
        float4 o = s_part[0][c];
#pragma unroll
        for (int k = 1; k < kDecWaves; ++k) {
            const float4 t = s_part[k][c];
            o.x = o.x + t.x; o.y = o.y + t.y; o.z = o.z + t.z; o.w = o.w + t.w;
        }
        o = make_float4(dec_fq(o.x, a.ctx, cq), dec_fq(o.y, a.ctx, cq), dec_fq(o.z, a.ctx, cq), dec_fq(o.w, a.ctx, cq));
        reinterpret_cast<float4*>(a.out)[bh * LPR + c] = o;      // [batch, 1, heads * head_dim]: row b, columns of head h
    }
}

static bool dec_mode_ok(int mode) {
    return (mode & ~(OSQ_PARAM_MODE_MASK | OSQ_PARAM_SANITIZE)) == 0 && (mode & OSQ_PARAM_MODE_MASK) <= OSQ_PARAM_LSQPLUS;
}

}  // namespace osq

using namespace osq;

extern "C" int osq_decode_attention_fake_quant(const float* q, const float* k, const float* v, const float* mask, float* out,
                                               float* probs_out, int64_t batch, int64_t heads, int64_t head_dim,
                                               int64_t kv_len, int64_t k_cap, int64_t v_cap,
                                               float* probs_scale, void* probs_zero_point, int probs_zp_type, int probs_mode,
                                               float probs_grad_factor, int probs_quant_min, int probs_quant_max,
                                               float* ctx_scale, void* ctx_zero_point, int ctx_zp_type, int ctx_mode,
                                               float ctx_grad_factor, int ctx_quant_min, int ctx_quant_max,
                                               osq_stream stream) {
    OSQ_REQUIRE(batch >= 0 && heads >= 0 && head_dim > 0 && batch * heads <= INT32_MAX, "decode_attention_fake_quant: bad shape");
    OSQ_REQUIRE(!probs_scale || probs_zero_point, "decode_attention_fake_quant: probs scale without zero_point");
    OSQ_REQUIRE(!ctx_scale || ctx_zero_point, "decode_attention_fake_quant: ctx scale without zero_point");
    OSQ_REQUIRE(!probs_scale || dec_mode_ok(probs_mode), "decode_attention_fake_quant: bad probs mode");
    OSQ_REQUIRE(!ctx_scale || dec_mode_ok(ctx_mode), "decode_attention_fake_quant: bad ctx mode");
    if (kv_len < 1 || kv_len > kDecMaxKv) return OSQ_ERR_UNSUPPORTED;
    const int64_t lpr = head_dim / 4;
    if (head_dim % 4 || lpr > OSQ_WAVE || (lpr & (lpr - 1))) return OSQ_ERR_UNSUPPORTED;
    OSQ_REQUIRE(k_cap >= kv_len && v_cap >= kv_len, "decode_attention_fake_quant: cap below kv_len");
    if (batch * heads == 0) return OSQ_OK;
    OSQ_REQUIRE(q && k && v && out, "decode_attention_fake_quant: null tensor");
    if (!aligned16(q) || !aligned16(k) || !aligned16(v) || !aligned16(out) || !aligned16(mask) || !aligned16(probs_out))
        return OSQ_ERR_UNSUPPORTED;
    DecArgs a{q, k, v, mask, out, probs_out, heads, k_cap, v_cap, static_cast<int>(kv_len),
              DecQuant{probs_scale, probs_zero_point, probs_zp_type, probs_mode, probs_grad_factor,
                       static_cast<float>(probs_quant_min), static_cast<float>(probs_quant_max)},
              DecQuant{ctx_scale, ctx_zero_point, ctx_zp_type, ctx_mode, ctx_grad_factor,
                       static_cast<float>(ctx_quant_min), static_cast<float>(ctx_quant_max)}};
    const dim3 grid(static_cast<unsigned>(batch * heads));
    hipStream_t st = static_cast<hipStream_t>(stream);
#define OSQ_DEC(LPR) hipLaunchKernelGGL((decode_attention_fq_kernel<LPR>), grid, dim3(kDecThreads), 0, st, a)
    switch (lpr) {
        case 1: OSQ_DEC(1); break;
        case 2: OSQ_DEC(2); break;
        case 4: OSQ_DEC(4); break;
        case 8: OSQ_DEC(8); break;
        case 16: OSQ_DEC(16); break;
        case 32: OSQ_DEC(32); break;
        default: OSQ_DEC(64); break;
    }
#undef OSQ_DEC
    return check_launch("decode_attention_fake_quant");
}

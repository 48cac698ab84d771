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
// K and V are the cache's fp32 buffers, or its byte buffers of integer codes (osq_decode_attention_codes; kv_codes.hip
// writes them): the same kernel body with the same lane map, a lane then loading its four elements of a row as ONE 32-bit
// word of four codes instead of a float4 and turning each into float(u + quant_min), then (q - zp_eff) * scale_eff
// (dequantize_value) -- the word the fp32 cache holds -- before the arithmetic below.  A quarter of the bytes per load,
// so four times the loads are issued before the first is reduced (KvCodes::kInFlight): the bytes in flight per CU stay.
// Traffic per (b, h) over codes: 2 * kv_len * head_dim bytes of K and V.
//
// Summation order, fixed by (head_dim, kv_len) alone -- not by cap, alignment or placement, nor by the cache's storage
// format (the loads in flight do not enter it: every position's products are formed and added as listed); no float atomics:
//   a score      four products of a lane added left to right, then an xor butterfly over the row's LPR lanes
//                (strides 1, 2, 4, ... : both partners of a step hold the same sum bit for bit);
//   the softmax  denominator: thread t adds exps t, t + 256, ... in order, wave_sum_f32, then (w0 + w1) + (w2 + w3);
//   a context    element: lane (wave w, row r) adds its positions (4 i + w) R + r for i = 0, 1, ... in order, an xor
//                butterfly over the wave's R row groups (strides LPR, 2 LPR, ... 32), then ((w0 + w1) + w2) + w3.
//
// The _at forms (osq_decode_attention_fake_quant_at / _codes_at) are the same kernel with the length read by the launch:
// kv_len = *kv_len_dev + kv_len_add, one scalar read per workgroup before anything else, so that a captured graph of a
// decoding step serves every position.  What the host derived from the length either holds for every length up to kv_max
// (caps, row strides of mask and probs_out) or comes from device memory indexed by it (the probabilities quantizer's grad
// factor: a table of the host's own words).  The trip loops do not change: n is an SGPR either way.
#include <math.h>
#include <hip/hip_runtime.h>
#include "decode_attention.h"

namespace osq {

constexpr int kDecMaxKv = 4096;          // the row of scores / probabilities in LDS: 16 KB

struct DecArgs {
    const float* q;            // [batch, heads, 1, head_dim] dense
    const void* k;             // [batch, heads, k_cap, head_dim] fp32 words or code bytes, positions [0, kv_len) read
    const void* v;             // [batch, heads, v_cap, head_dim]
    const float* mask;         // nullable, [batch, 1, 1, :] additive, rows mask_stride floats apart (static form: kv_len)
    float* out;                // [batch, 1, heads * head_dim] dense
    float* probs_out;          // nullable, [batch, heads, 1, :], rows probs_stride floats apart (static form: kv_len)
    int64_t heads, k_cap, v_cap, mask_stride, probs_stride;
    int kv_len;
    // the _at forms: kv_len = *kv_len_dev + kv_len_add, read by the launch; outside [1, kv_max] -> out is NaN, nothing read
    const int32_t* kv_len_dev; // nullptr: the static forms, kv_len above
    int kv_len_add, kv_max;
    const float* grad_table;   // nullable: probs.grad_factor = grad_table[kv_len], the host's own words
    DecQuant probs, ctx;
    DecCode kc, vc;            // coded form only
    const int32_t* rejected;   // coded form only: the cache's counter; non-zero: the cache holds elements without a code
};

template <int LPR, typename KV>
__global__ __launch_bounds__(kDecThreads) void decode_attention_fq_kernel(DecArgs a) {
    constexpr int kTripsInFlight = KV::kInFlight;
    constexpr int R = OSQ_WAVE / LPR;              // rows of K / V one wave load covers
    constexpr int kTrip = kDecWaves * R;           // positions one trip of the workgroup covers
    __shared__ float s_p[kDecMaxKv];               // scores -> exps -> fake-quantised probabilities
    __shared__ float4 s_part[kDecWaves][LPR];      // per-wave partial context vectors
    __shared__ float s_red[2][kDecWaves];          // per-wave maxima and sums of exps

    const int lane = threadIdx.x & (OSQ_WAVE - 1), w = threadIdx.x / OSQ_WAVE;
    const int r = lane / LPR, c = lane % LPR;
    const int64_t bh = blockIdx.x;
    int n = a.kv_len;
    DecQuant probs = a.probs;
    if (a.kv_len_dev) {                            // workgroup-uniform: the length is a device word, read once into an SGPR
        n = __builtin_amdgcn_readfirstlane(*a.kv_len_dev) + a.kv_len_add;
        if (n < 1 || n > a.kv_max) {               // a length no address may be formed from
            const float nan = __builtin_nanf("");
            if (threadIdx.x < LPR) reinterpret_cast<float4*>(a.out)[bh * LPR + c] = make_float4(nan, nan, nan, nan);
            return;
        }
        if (a.grad_table) probs.grad_factor = a.grad_table[n];
    }
    const int trips = (n + kTrip - 1) / kTrip;
    const QParams pq = dec_params(probs), cq = dec_params(a.ctx);      // first: the parameter repair rides here

    if (a.rejected && *a.rejected != 0) {          // workgroup-uniform: a cache with an uncodable element never yields numbers
        const float nan = __builtin_nanf("");
        if (a.probs_out)
            for (int j = threadIdx.x; j < n; j += kDecThreads) a.probs_out[bh * a.probs_stride + j] = nan;
        if (threadIdx.x < LPR) reinterpret_cast<float4*>(a.out)[bh * LPR + c] = make_float4(nan, nan, nan, nan);
        return;
    }
    const typename KV::Params kp = KV::params(a.kc), vp = KV::params(a.vc);

    // ---- scores
    const float4 q4 = reinterpret_cast<const float4*>(a.q)[bh * LPR + c];
    const int64_t kb = bh * a.k_cap * LPR + c;           // in words of four elements
    const float* mrow = a.mask ? a.mask + (bh / a.heads) * a.mask_stride : nullptr;
    for (int t0 = 0; t0 < trips; t0 += kTripsInFlight) {
        typename KV::Word kw[kTripsInFlight];
#pragma unroll
        for (int u = 0; u < kTripsInFlight; ++u) {
            const int j = ((t0 + u) * kDecWaves + w) * R + r;
            kw[u] = KV::load(a.k, kb + static_cast<int64_t>(j < n ? j : n - 1) * LPR);     // past the end: the last row again, unused
        }
#pragma unroll
        for (int u = 0; u < kTripsInFlight; ++u) {
            const int j = ((t0 + u) * kDecWaves + w) * R + r;
            const float4 kk = KV::values(kw[u], kp);
            float d = q4.x * kk.x;
            d = d + q4.y * kk.y;
            d = d + q4.z * kk.z;
            d = d + q4.w * kk.w;
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
    float* prow = a.probs_out ? a.probs_out + bh * a.probs_stride : nullptr;
    for (int j = threadIdx.x; j < n; j += kDecThreads) {
        const float p = dec_fq(s_p[j] * rcp, probs, pq);
        s_p[j] = p;
        if (prow) prow[j] = p;
    }
    __syncthreads();

    // ---- context
    const int64_t vb = bh * a.v_cap * LPR + c;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int t0 = 0; t0 < trips; t0 += kTripsInFlight) {
        typename KV::Word vw[kTripsInFlight];
#pragma unroll
        for (int u = 0; u < kTripsInFlight; ++u) {
            const int j = ((t0 + u) * kDecWaves + w) * R + r;
            vw[u] = KV::load(a.v, vb + static_cast<int64_t>(j < n ? j : n - 1) * LPR);
        }
#pragma unroll
        for (int u = 0; u < kTripsInFlight; ++u) {
            const int j = ((t0 + u) * kDecWaves + w) * R + r;
            if (j < n) {
                const float p = s_p[j];
                const float4 vv = KV::values(vw[u], vp);
                acc.x = acc.x + p * vv.x;
                acc.y = acc.y + p * vv.y;
                acc.z = acc.z + p * vv.z;
                acc.w = acc.w + p * vv.w;
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


// What the _at forms add: the device word of the length, the constant added to it, and the row strides of mask / probs_out.
struct DecAt {
    const int32_t* kv_len_dev;
    int64_t kv_len_add, mask_stride, probs_stride;
    const float* grad_table;
};

// checks and launch shared by the two storage formats; kv_align: what K and V must be aligned to.  at == nullptr: the static
// forms.  Otherwise kv_len is kv_max, the largest length the launch may meet: every host check holds for all lengths up to it.
template <typename KV>
static int launch_decode_attention(const char* what, const float* q, const void* k, const void* v, const float* mask, float* out,
                                   float* probs_out, int64_t batch, int64_t heads, int64_t head_dim, int64_t kv_len,
                                   int64_t k_cap, int64_t v_cap, const DecCode& kc, const DecCode& vc, const int32_t* rejected,
                                   const DecQuant& probs, const DecQuant& ctx, uintptr_t kv_align, osq_stream stream,
                                   const DecAt* at = nullptr) {
    OSQ_REQUIRE(batch >= 0 && heads >= 0 && head_dim > 0 && batch * heads <= INT32_MAX, "decode_attention: bad shape");
    OSQ_REQUIRE(!probs.scale || probs.zero_point, "decode_attention: probs scale without zero_point");
    OSQ_REQUIRE(!ctx.scale || ctx.zero_point, "decode_attention: ctx scale without zero_point");
    OSQ_REQUIRE(!probs.scale || dec_mode_ok(probs.mode), "decode_attention: bad probs mode");
    OSQ_REQUIRE(!ctx.scale || dec_mode_ok(ctx.mode), "decode_attention: bad ctx mode");
    if (kv_len < 1 || kv_len > kDecMaxKv) return OSQ_ERR_UNSUPPORTED;
    const int64_t lpr = head_dim / 4;
    if (head_dim % 4 || lpr > OSQ_WAVE || (lpr & (lpr - 1))) return OSQ_ERR_UNSUPPORTED;
    OSQ_REQUIRE(k_cap >= kv_len && v_cap >= kv_len, "decode_attention: cap below kv_len");
    if (at) {
        OSQ_REQUIRE(at->kv_len_dev, "decode_attention: null kv_len word");
        OSQ_REQUIRE(at->kv_len_add >= 0 && at->kv_len_add <= kDecMaxKv, "decode_attention: bad kv_len_add");
        OSQ_REQUIRE((!mask || at->mask_stride >= kv_len) && (!probs_out || at->probs_stride >= kv_len),
                    "decode_attention: row stride below kv_max");
    }
    if (batch * heads == 0) return OSQ_OK;
    OSQ_REQUIRE(q && k && v && out, "decode_attention: null tensor");
    if (!aligned16(q) || !aligned16(out) || !aligned16(mask) || !aligned16(probs_out)) return OSQ_ERR_UNSUPPORTED;
    if ((reinterpret_cast<uintptr_t>(k) | reinterpret_cast<uintptr_t>(v)) & (kv_align - 1u)) return OSQ_ERR_UNSUPPORTED;
    DecArgs a{q, k, v, mask, out, probs_out, heads, k_cap, v_cap, at ? at->mask_stride : kv_len, at ? at->probs_stride : kv_len,
              static_cast<int>(kv_len), at ? at->kv_len_dev : nullptr, at ? static_cast<int>(at->kv_len_add) : 0,
              static_cast<int>(kv_len), at ? at->grad_table : nullptr, probs, ctx, kc, vc, rejected};
    const dim3 grid(static_cast<unsigned>(batch * heads));
    hipStream_t st = static_cast<hipStream_t>(stream);
#define OSQ_DEC(LPR) hipLaunchKernelGGL((decode_attention_fq_kernel<LPR, KV>), grid, dim3(kDecThreads), 0, st, a)
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
    return check_launch(what);
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
    return launch_decode_attention<KvWords>(
        "decode_attention_fake_quant", q, k, v, mask, out, probs_out, batch, heads, head_dim, kv_len, k_cap, v_cap, DecCode{}, DecCode{},
        nullptr, dec_quant(probs_scale, probs_zero_point, probs_zp_type, probs_mode, probs_grad_factor, probs_quant_min, probs_quant_max),
        dec_quant(ctx_scale, ctx_zero_point, ctx_zp_type, ctx_mode, ctx_grad_factor, ctx_quant_min, ctx_quant_max), 16u, stream);
}

extern "C" int osq_decode_attention_codes(const float* q, const uint8_t* k, const uint8_t* v, const float* mask, float* out,
                                          float* probs_out, int64_t batch, int64_t heads, int64_t head_dim, int64_t kv_len,
                                          int64_t k_cap, int64_t v_cap,
                                          const float* k_scale_eff, const float* k_zp_eff, int k_quant_min,
                                          const float* v_scale_eff, const float* v_zp_eff, int v_quant_min, const int32_t* rejected,
                                          float* probs_scale, void* probs_zero_point, int probs_zp_type, int probs_mode,
                                          float probs_grad_factor, int probs_quant_min, int probs_quant_max,
                                          float* ctx_scale, void* ctx_zero_point, int ctx_zp_type, int ctx_mode,
                                          float ctx_grad_factor, int ctx_quant_min, int ctx_quant_max,
                                          osq_stream stream) {
    OSQ_REQUIRE(k_scale_eff && k_zp_eff && v_scale_eff && v_zp_eff && rejected, "decode_attention_codes: null record or rejected counter");
    return launch_decode_attention<KvCodes>(
        "decode_attention_codes", q, k, v, mask, out, probs_out, batch, heads, head_dim, kv_len, k_cap, v_cap,
        DecCode{k_scale_eff, k_zp_eff, k_quant_min}, DecCode{v_scale_eff, v_zp_eff, v_quant_min}, rejected,
        dec_quant(probs_scale, probs_zero_point, probs_zp_type, probs_mode, probs_grad_factor, probs_quant_min, probs_quant_max),
        dec_quant(ctx_scale, ctx_zero_point, ctx_zp_type, ctx_mode, ctx_grad_factor, ctx_quant_min, ctx_quant_max), 4u, stream);
}

extern "C" int osq_decode_attention_fake_quant_at(const float* q, const float* k, const float* v, const float* mask,
                                                  int64_t mask_stride, float* out, float* probs_out, int64_t probs_stride,
                                                  int64_t batch, int64_t heads, int64_t head_dim,
                                                  const int32_t* kv_len_dev, int64_t kv_len_add, int64_t kv_max,
                                                  int64_t k_cap, int64_t v_cap, const float* probs_grad_table,
                                                  float* probs_scale, void* probs_zero_point, int probs_zp_type, int probs_mode,
                                                  float probs_grad_factor, int probs_quant_min, int probs_quant_max,
                                                  float* ctx_scale, void* ctx_zero_point, int ctx_zp_type, int ctx_mode,
                                                  float ctx_grad_factor, int ctx_quant_min, int ctx_quant_max,
                                                  osq_stream stream) {
    const DecAt at{kv_len_dev, kv_len_add, mask_stride, probs_stride, probs_grad_table};
    return launch_decode_attention<KvWords>(
        "decode_attention_fake_quant_at", q, k, v, mask, out, probs_out, batch, heads, head_dim, kv_max, k_cap, v_cap, DecCode{},
        DecCode{}, nullptr, dec_quant(probs_scale, probs_zero_point, probs_zp_type, probs_mode, probs_grad_factor, probs_quant_min, probs_quant_max),
        dec_quant(ctx_scale, ctx_zero_point, ctx_zp_type, ctx_mode, ctx_grad_factor, ctx_quant_min, ctx_quant_max), 16u, stream, &at);
}

extern "C" int osq_decode_attention_codes_at(const float* q, const uint8_t* k, const uint8_t* v, const float* mask,
                                             int64_t mask_stride, float* out, float* probs_out, int64_t probs_stride,
                                             int64_t batch, int64_t heads, int64_t head_dim,
                                             const int32_t* kv_len_dev, int64_t kv_len_add, int64_t kv_max,
                                             int64_t k_cap, int64_t v_cap, const float* probs_grad_table,
                                             const float* k_scale_eff, const float* k_zp_eff, int k_quant_min,
                                             const float* v_scale_eff, const float* v_zp_eff, int v_quant_min, const int32_t* rejected,
                                             float* probs_scale, void* probs_zero_point, int probs_zp_type, int probs_mode,
                                             float probs_grad_factor, int probs_quant_min, int probs_quant_max,
                                             float* ctx_scale, void* ctx_zero_point, int ctx_zp_type, int ctx_mode,
                                             float ctx_grad_factor, int ctx_quant_min, int ctx_quant_max,
                                             osq_stream stream) {
    OSQ_REQUIRE(k_scale_eff && k_zp_eff && v_scale_eff && v_zp_eff && rejected, "decode_attention_codes_at: null record or rejected counter");
    const DecAt at{kv_len_dev, kv_len_add, mask_stride, probs_stride, probs_grad_table};
    return launch_decode_attention<KvCodes>(
        "decode_attention_codes_at", q, k, v, mask, out, probs_out, batch, heads, head_dim, kv_max, k_cap, v_cap,
        DecCode{k_scale_eff, k_zp_eff, k_quant_min}, DecCode{v_scale_eff, v_zp_eff, v_quant_min}, rejected,
        dec_quant(probs_scale, probs_zero_point, probs_zp_type, probs_mode, probs_grad_factor, probs_quant_min, probs_quant_max),
        dec_quant(ctx_scale, ctx_zero_point, ctx_zp_type, ctx_mode, ctx_grad_factor, ctx_quant_min, ctx_quant_max), 4u, stream, &at);
}

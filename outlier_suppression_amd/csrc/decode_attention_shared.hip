// Attention of ONE decoding step over keys and values that several query rows share: beam search's cross-attention, where the
// `group` beams of a batch row attend to the same encoder keys / values.  decode_attention.hip serves one query row per
// workgroup and so reads K and V of a batch row once per beam; here one workgroup serves up to kShChunk = 8 query rows of a
// (batch row, head) from a SINGLE pass over K and a single pass over V.
//
//     q [batch * group, heads, 1, d]     query row b * group + g attends to K / V row b and mask row b
//     k, v [batch, heads, cap, d]        fp32 words or code bytes (KvWords / KvCodes of decode_attention.h)
//     mask [batch, 1, 1, kv_len]         nullable
//     out [batch * group, 1, heads * d], probs_out [batch * group, heads, 1, kv_len] (nullable)
//
// Launch shape: one 256-thread workgroup per (batch row, head, chunk of at most 8 query rows); ceil(group / 8) chunks per
// (row, head), the last one ragged, neighbours in the grid so that the second chunk finds K and V in L2.  The lane map is
// decode_attention.hip's: LPR = head_dim / 4 lanes cover a row with one word each, a wave R = 64 / LPR rows per load, the four
// waves 4 R rows per trip, KV::kInFlight trips loaded before the first is reduced.  A loaded word of K is decoded once and
// multiplied into each of the chunk's queries (their q4 in registers); the chunk's score rows live in LDS, 8 x kv_len floats
// (32 KiB at the limit of 1024: BART's source positions); softmax and the probabilities quantizer run per query row; the pass
// over V holds one context accumulator per query.  The per-wave partial vectors (4 x 8 x head_dim floats) reuse the score
// rows' LDS after a barrier.  Traffic per (b, h): 2 * kv_len * head_dim words of K and V whatever the group.
//
// Summation order: for every query row each score, the softmax denominator and every context element are formed and added
// exactly as the header comment of decode_attention.hip lists them (the chunk loop only repeats that arithmetic per query).
// out and probs_out are therefore WORD-EQUAL to decode_attention.hip run on k / v / mask repeated `group` times along the
// batch, for both storage formats.  No atomics.  The parameter repair under OSQ_PARAM_SANITIZE rides in every workgroup (all
// compute the same repaired words); a non-zero `rejected` counter of a coded cache yields NaN.  Static length only:
// cross-attention's length does not change between steps, a captured step replays the same launch.
#include <math.h>
#include <hip/hip_runtime.h>
#include "decode_attention.h"

namespace osq {

constexpr int kShChunk = 8;              // query rows one workgroup serves
constexpr int kShMaxKv = 1024;           // the chunk's score rows in LDS: 8 x 4 KiB
constexpr int kShMaxGroup = 64;

struct ShArgs {
    const float* q;            // [batch * group, heads, 1, head_dim] dense
    const void* k;             // [batch, heads, k_cap, head_dim]
    const void* v;             // [batch, heads, v_cap, head_dim]
    const float* mask;         // nullable, [batch, 1, 1, kv_len]
    float* out;                // [batch * group, 1, heads * head_dim] dense
    float* probs_out;          // nullable, [batch * group, heads, 1, kv_len]
    int64_t heads, k_cap, v_cap;
    int kv_len, group, chunks;
    DecQuant probs, ctx;
    DecCode kc, vc;            // coded form only
    const int32_t* rejected;   // coded form only
};

template <int LPR, typename KV>
__global__ __launch_bounds__(kDecThreads) void decode_attention_shared_kernel(ShArgs a) {
    constexpr int kTripsInFlight = KV::kInFlight;
    constexpr int R = OSQ_WAVE / LPR;
    constexpr int kTrip = kDecWaves * R;
    static_assert(kDecWaves * kShChunk * LPR * 4 <= kShChunk * kShMaxKv, "the partial vectors reuse the score rows");
    __shared__ __attribute__((aligned(16))) float s_p[kShChunk * kShMaxKv];   // per query: scores -> exps -> probabilities
    __shared__ float s_red[2][kShChunk][kDecWaves];                           // per query: per-wave maxima and sums of exps

    const int lane = threadIdx.x & (OSQ_WAVE - 1), w = threadIdx.x / OSQ_WAVE;
    const int r = lane / LPR, c = lane % LPR;
    const int64_t bh = blockIdx.x / a.chunks;            // K / V row (b, h)
    const int g0 = static_cast<int>(blockIdx.x % a.chunks) * kShChunk;
    const int gn = min(kShChunk, a.group - g0);          // workgroup-uniform: the chunk's query rows, 1..8
    const int64_t b = bh / a.heads, h = bh % a.heads;
    const int64_t qh0 = (b * a.group + g0) * a.heads + h;      // (query row, head) of the chunk's first query; + g * heads
    const int n = a.kv_len;
    const int trips = (n + kTrip - 1) / kTrip;
    const QParams pq = dec_params(a.probs), cq = dec_params(a.ctx);     // first: the parameter repair rides here

    if (a.rejected && *a.rejected != 0) {                // workgroup-uniform
        const float nan = __builtin_nanf("");
        for (int g = 0; g < gn; ++g) {
            const int64_t qh = qh0 + g * a.heads;
            if (a.probs_out)
                for (int j = threadIdx.x; j < n; j += kDecThreads) a.probs_out[qh * n + j] = nan;
            if (threadIdx.x < LPR) reinterpret_cast<float4*>(a.out)[qh * LPR + c] = make_float4(nan, nan, nan, nan);
        }
        return;
    }
    const typename KV::Params kp = KV::params(a.kc), vp = KV::params(a.vc);

    // ---- scores: every word of K loaded once, used by the chunk's queries
    {
        float4 q4[kShChunk];
#pragma unroll
        for (int g = 0; g < kShChunk; ++g)
            q4[g] = reinterpret_cast<const float4*>(a.q)[(qh0 + (g < gn ? g : 0) * a.heads) * LPR + c];
        const int64_t kb = bh * a.k_cap * LPR + c;
        const float* mrow = a.mask ? a.mask + b * n : nullptr;
        for (int t0 = 0; t0 < trips; t0 += kTripsInFlight) {
            typename KV::Word kw[kTripsInFlight];
#pragma unroll
            for (int u = 0; u < kTripsInFlight; ++u) {
                const int j = ((t0 + u) * kDecWaves + w) * R + r;
                kw[u] = KV::load(a.k, kb + static_cast<int64_t>(j < n ? j : n - 1) * LPR);   // past the end: the last row again, unused
            }
#pragma unroll
            for (int u = 0; u < kTripsInFlight; ++u) {
                const int j = ((t0 + u) * kDecWaves + w) * R + r;
                const float4 kk = KV::values(kw[u], kp);
                const bool store = c == 0 && j < n;
                const float m = (store && mrow) ? mrow[j] : 0.f;
#pragma unroll
                for (int g = 0; g < kShChunk; ++g) {
                    if (g < gn) {                            // uniform; all 64 lanes reach the lane sums
                        float d = q4[g].x * kk.x;
                        d = d + q4[g].y * kk.y;
                        d = d + q4[g].z * kk.z;
                        d = d + q4[g].w * kk.w;
                        d = row_lanes_sum<LPR>(d);
                        if (store) s_p[g * kShMaxKv + j] = mrow ? d + m : d;
                    }
                }
            }
        }
    }
    __syncthreads();

    // ---- softmax and the probabilities quantizer, per query: thread t owns positions t, t + 256, ...
    for (int g = 0; g < gn; ++g) {
        const float* sp = s_p + g * kShMaxKv;
        float mx = -INFINITY;
        for (int j = threadIdx.x; j < n; j += kDecThreads) mx = fmaxf(mx, sp[j]);
        mx = wave_max(mx);
        if (lane == 0) s_red[0][g][w] = mx;
    }
    __syncthreads();
    for (int g = 0; g < gn; ++g) {
        float* sp = s_p + g * kShMaxKv;
        const float mx = fmaxf(fmaxf(s_red[0][g][0], s_red[0][g][1]), fmaxf(s_red[0][g][2], s_red[0][g][3]));
        float sum = 0.f;
        for (int j = threadIdx.x; j < n; j += kDecThreads) {
            const float e = expf(sp[j] - mx);
            sp[j] = e;
            sum += e;
        }
        sum = wave_sum_f32(sum);
        if (lane == 0) s_red[1][g][w] = sum;
    }
    __syncthreads();
    for (int g = 0; g < gn; ++g) {
        float* sp = s_p + g * kShMaxKv;
        const float rcp = 1.0f / ((s_red[1][g][0] + s_red[1][g][1]) + (s_red[1][g][2] + s_red[1][g][3]));
        float* prow = a.probs_out ? a.probs_out + (qh0 + g * a.heads) * n : nullptr;
        for (int j = threadIdx.x; j < n; j += kDecThreads) {
            const float p = dec_fq(sp[j] * rcp, a.probs, pq);
            sp[j] = p;
            if (prow) prow[j] = p;
        }
    }
    __syncthreads();

    // ---- context: every word of V loaded once, one accumulator per query
    float4 acc[kShChunk];
#pragma unroll
    for (int g = 0; g < kShChunk; ++g) acc[g] = make_float4(0.f, 0.f, 0.f, 0.f);
    const int64_t vb = bh * a.v_cap * LPR + c;
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
                const float4 vv = KV::values(vw[u], vp);
#pragma unroll
                for (int g = 0; g < kShChunk; ++g) {
                    if (g < gn) {
                        const float p = s_p[g * kShMaxKv + j];
                        acc[g].x = acc[g].x + p * vv.x;
                        acc[g].y = acc[g].y + p * vv.y;
                        acc[g].z = acc[g].z + p * vv.z;
                        acc[g].w = acc[g].w + p * vv.w;
                    }
                }
            }
        }
    }
    __syncthreads();                                     // every wave is done with the probabilities: their LDS is reused
    float4* s_part = reinterpret_cast<float4*>(s_p);     // [kDecWaves][kShChunk][LPR] per-wave partial context vectors
#pragma unroll
    for (int g = 0; g < kShChunk; ++g) {
        if (g < gn) {
            acc[g].x = row_groups_sum<LPR>(acc[g].x);
            acc[g].y = row_groups_sum<LPR>(acc[g].y);
            acc[g].z = row_groups_sum<LPR>(acc[g].z);
            acc[g].w = row_groups_sum<LPR>(acc[g].w);
            if (r == 0) s_part[(w * kShChunk + g) * LPR + c] = acc[g];
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < gn * LPR; i += kDecThreads) {
        const int g = i / LPR, cc = i % LPR;
        float4 o = s_part[g * LPR + cc];
#pragma unroll
        for (int k = 1; k < kDecWaves; ++k) {
            const float4 t = s_part[(k * kShChunk + g) * LPR + cc];
            o.x = o.x + t.x; o.y = o.y + t.y; o.z = o.z + t.z; o.w = o.w + t.w;
        }
        o = make_float4(dec_fq(o.x, a.ctx, cq), dec_fq(o.y, a.ctx, cq), dec_fq(o.z, a.ctx, cq), dec_fq(o.w, a.ctx, cq));
        reinterpret_cast<float4*>(a.out)[(qh0 + g * a.heads) * LPR + cc] = o;     // row b * group + g0 + g, columns of head h
    }
}

// checks and launch shared by the two storage formats; kv_align: what K and V must be aligned to
template <typename KV>
static int launch_decode_attention_shared(const char* what, const float* q, const void* k, const void* v, const float* mask,
                                          float* out, float* probs_out, int64_t batch, int64_t group, int64_t heads,
                                          int64_t head_dim, int64_t kv_len, int64_t k_cap, int64_t v_cap, const DecCode& kc,
                                          const DecCode& vc, const int32_t* rejected, const DecQuant& probs, const DecQuant& ctx,
                                          uintptr_t kv_align, osq_stream stream) {
    OSQ_REQUIRE(batch >= 0 && heads >= 0 && head_dim > 0 && group >= 1, "decode_attention_shared: bad shape");
    OSQ_REQUIRE(!probs.scale || probs.zero_point, "decode_attention_shared: probs scale without zero_point");
    OSQ_REQUIRE(!ctx.scale || ctx.zero_point, "decode_attention_shared: ctx scale without zero_point");
    OSQ_REQUIRE(!probs.scale || dec_mode_ok(probs.mode), "decode_attention_shared: bad probs mode");
    OSQ_REQUIRE(!ctx.scale || dec_mode_ok(ctx.mode), "decode_attention_shared: bad ctx mode");
    if (group > kShMaxGroup || kv_len < 1 || kv_len > kShMaxKv) return OSQ_ERR_UNSUPPORTED;
    const int64_t lpr = head_dim / 4;
    if (head_dim % 4 || lpr > OSQ_WAVE || (lpr & (lpr - 1))) return OSQ_ERR_UNSUPPORTED;
    const int64_t chunks = (group + kShChunk - 1) / kShChunk;
    OSQ_REQUIRE(batch <= INT32_MAX && heads <= INT32_MAX && batch * heads <= INT32_MAX / kShMaxGroup,
                "decode_attention_shared: bad shape");
    OSQ_REQUIRE(k_cap >= kv_len && v_cap >= kv_len, "decode_attention_shared: cap below kv_len");
    if (batch * heads == 0) return OSQ_OK;
    OSQ_REQUIRE(q && k && v && out, "decode_attention_shared: null tensor");
    if (!aligned16(q) || !aligned16(out) || !aligned16(mask) || !aligned16(probs_out)) return OSQ_ERR_UNSUPPORTED;
    if ((reinterpret_cast<uintptr_t>(k) | reinterpret_cast<uintptr_t>(v)) & (kv_align - 1u)) return OSQ_ERR_UNSUPPORTED;
    ShArgs a{q, k, v, mask, out, probs_out, heads, k_cap, v_cap, static_cast<int>(kv_len), static_cast<int>(group),
             static_cast<int>(chunks), probs, ctx, kc, vc, rejected};
    const dim3 grid(static_cast<unsigned>(batch * heads * chunks));
    hipStream_t st = static_cast<hipStream_t>(stream);
#define OSQ_DEC(LPR) hipLaunchKernelGGL((decode_attention_shared_kernel<LPR, KV>), grid, dim3(kDecThreads), 0, st, a)
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

extern "C" int osq_decode_attention_shared(const float* q, const float* k, const float* v, const float* mask, float* out,
                                           float* probs_out, int64_t batch, int64_t group, int64_t heads, int64_t head_dim,
                                           int64_t kv_len, int64_t k_cap, int64_t v_cap,
                                           float* probs_scale, void* probs_zero_point, int probs_zp_type, int probs_mode,
                                           float probs_grad_factor, int probs_quant_min, int probs_quant_max,
                                           float* ctx_scale, void* ctx_zero_point, int ctx_zp_type, int ctx_mode,
                                           float ctx_grad_factor, int ctx_quant_min, int ctx_quant_max,
                                           osq_stream stream) {
    return launch_decode_attention_shared<KvWords>(
        "decode_attention_shared", q, k, v, mask, out, probs_out, batch, group, heads, head_dim, kv_len, k_cap, v_cap, DecCode{},
        DecCode{}, nullptr, dec_quant(probs_scale, probs_zero_point, probs_zp_type, probs_mode, probs_grad_factor, probs_quant_min, probs_quant_max),
        dec_quant(ctx_scale, ctx_zero_point, ctx_zp_type, ctx_mode, ctx_grad_factor, ctx_quant_min, ctx_quant_max), 16u, stream);
}

extern "C" int osq_decode_attention_shared_codes(const float* q, const uint8_t* k, const uint8_t* v, const float* mask, float* out,
                                                 float* probs_out, int64_t batch, int64_t group, int64_t heads,
                                                 int64_t head_dim, int64_t kv_len, int64_t k_cap, int64_t v_cap,
                                                 const float* k_scale_eff, const float* k_zp_eff, int k_quant_min,
                                                 const float* v_scale_eff, const float* v_zp_eff, int v_quant_min,
                                                 const int32_t* rejected,
                                                 float* probs_scale, void* probs_zero_point, int probs_zp_type, int probs_mode,
                                                 float probs_grad_factor, int probs_quant_min, int probs_quant_max,
                                                 float* ctx_scale, void* ctx_zero_point, int ctx_zp_type, int ctx_mode,
                                                 float ctx_grad_factor, int ctx_quant_min, int ctx_quant_max,
                                                 osq_stream stream) {
    OSQ_REQUIRE(k_scale_eff && k_zp_eff && v_scale_eff && v_zp_eff && rejected,
                "decode_attention_shared_codes: null record or rejected counter");
    return launch_decode_attention_shared<KvCodes>(
        "decode_attention_shared_codes", q, k, v, mask, out, probs_out, batch, group, heads, head_dim, kv_len, k_cap, v_cap,
        DecCode{k_scale_eff, k_zp_eff, k_quant_min}, DecCode{v_scale_eff, v_zp_eff, v_quant_min}, rejected,
        dec_quant(probs_scale, probs_zero_point, probs_zp_type, probs_mode, probs_grad_factor, probs_quant_min, probs_quant_max),
        dec_quant(ctx_scale, ctx_zero_point, ctx_zp_type, ctx_mode, ctx_grad_factor, ctx_quant_min, ctx_quant_max), 4u, stream);
}

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
// ONE kernel, decode_attention_kernel<LPR, KV, CH>, in two chunk sizes.  CH = 1: one query row per workgroup, a 256-thread
// workgroup per (batch, head).  CH = 8 (osq_decode_attention_shared / _codes): query rows that share their keys and values --
// beam search's cross-attention, where the `group` beams of a batch row attend to the same encoder keys / values -- and one
// workgroup serves up to 8 query rows of a (batch row, head) from a SINGLE pass over K and a single pass over V:
//
//     q [batch * group, heads, 1, d]     query row b * group + g attends to K / V row b and mask row b
//     k, v [batch, heads, cap, d]        fp32 words or code bytes
//     mask [batch, 1, 1, :]              nullable
//     out [batch * group, 1, heads * d], probs_out [batch * group, heads, 1, :] (nullable)
//
// ceil(group / 8) chunks per (row, head), the last one ragged, neighbours in the grid so that the second chunk finds K and V
// in L2.  A loaded word of K is decoded once and multiplied into each of the chunk's queries (their q4 in registers);
// softmax and the probabilities quantizer run per query row; the pass over V holds one context accumulator per query.  With
// CH = 1 the chunk is the constant 1 and every loop over it folds away.
//
// Lane map: LPR = head_dim / 4 lanes cover a row of K or V with one float4 each, so a wave takes R = 64 / LPR rows per load
// and the four waves 4 R rows per trip; kTripsInFlight trips are loaded before the first is reduced.  Scores, then exps, then
// fake-quantised probabilities live in LDS, CH rows of kMaxKv<CH> floats (16 KB at CH = 1 and its limit of 4096; 32 KB at
// CH = 8 and its limit of 1024: BART's source positions), and pass between the three phases through two barriers; the second
// product's per-wave partial vectors (4 x CH x head_dim floats) meet in LDS -- their own at CH = 1, the score rows' after one
// more barrier at CH = 8 -- and are added in wave order.  Traffic per (b, h): 2 * kv_len * head_dim * 4 B of K and V whatever the group, per query row
// head_dim * 4 B of q and head_dim * 4 B written, kv_len * 4 B of mask.
//
// K and V are the cache's fp32 buffers, or its byte buffers of integer codes (osq_decode_attention_codes; kv_codes.hip
// writes them): the same kernel body with the same lane map, a lane then loading its four elements of a row as ONE 32-bit
// word of four codes instead of a float4 and turning each into float(u + quant_min), then (q - zp_eff) * scale_eff
// (dequantize_value) -- the word the fp32 cache holds -- before the arithmetic below.  A quarter of the bytes per load,
// so four times the loads are issued before the first is reduced (KvCodes::kInFlight): the bytes in flight per CU stay.
// Traffic per (b, h) over codes: 2 * kv_len * head_dim bytes of K and V.
//
// Summation order, fixed by (head_dim, kv_len) alone -- not by cap, alignment or placement, nor by the cache's storage
// format (the loads in flight do not enter it: every position's products are formed and added as listed), nor by the chunk
// (its loop only repeats the arithmetic per query row: the shared form's out and probs_out are WORD-EQUAL to the one-query
// form run on k / v / mask repeated `group` times along the batch); no float atomics:
//   a score      four products of a lane added left to right, then an xor butterfly over the row's LPR lanes
//                (strides 1, 2, 4, ... : both partners of a step hold the same sum bit for bit);
//   the softmax  denominator: thread t adds exps t, t + 256, ... in order, wave_sum_f32, then (w0 + w1) + (w2 + w3);
//   a context    element: lane (wave w, row r) adds its positions (4 i + w) R + r for i = 0, 1, ... in order, an xor
//                butterfly over the wave's R row groups (strides LPR, 2 LPR, ... 32), then ((w0 + w1) + w2) + w3.
// The parameter repair under OSQ_PARAM_SANITIZE rides in every workgroup (all compute the same repaired words); a non-zero
// `rejected` counter of a coded cache yields NaN.
//
// The _at forms (osq_decode_attention_fake_quant_at / _codes_at) are the same kernel with the length read by the launch:
// kv_len = *kv_len_dev + kv_len_add, one scalar read per workgroup before anything else, so that a captured graph of a
// decoding step serves every position.  What the host derived from the length either holds for every length up to kv_max
// (caps, row strides of mask and probs_out) or comes from device memory indexed by it (the probabilities quantizer's grad
// factor: a table of the host's own words).  The trip loops do not change: n is an SGPR either way.  One query row only:
// cross-attention's length does not change between steps, a captured step replays the same shared launch.
#include <math.h>
#include <hip/hip_runtime.h>
#include "attention_quant.h"
#include "codes_device.h"
#include "osq_host.h"

namespace osq {

constexpr int kDecThreads = 256;
constexpr int kDecWaves = kDecThreads / OSQ_WAVE;
constexpr int kDecMaxGroup = 64;
template <int CH> constexpr int kMaxKv = CH == 1 ? 4096 : 1024;     // a score row in LDS: CH rows are 16 KB / 32 KB

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

struct DecArgs {
    const float* q;            // [batch * group, heads, 1, head_dim] dense
    const void* k;             // [batch, heads, k_cap, head_dim] fp32 words or code bytes, positions [0, kv_len) read
    const void* v;             // [batch, heads, v_cap, head_dim]
    const float* mask;         // nullable, [batch, 1, 1, :] additive, rows mask_stride floats apart (CH = 8: kv_len)
    float* out;                // [batch * group, 1, heads * head_dim] dense
    float* probs_out;          // nullable, [batch * group, heads, 1, :], rows probs_stride floats apart (CH = 8: kv_len)
    int64_t heads, k_cap, v_cap;
    int64_t mask_stride, probs_stride;    // read at CH = 1 only; the static forms pass kv_len
    int kv_len;
    int group, chunks;         // query rows per K / V row and workgroups they take, ceil(group / CH); 1 and 1 at CH = 1
    // the _at forms (CH = 1 only): kv_len = *kv_len_dev + kv_len_add, read by the launch; outside [1, kv_max] -> out is NaN, nothing read
    const int32_t* kv_len_dev; // nullptr: the static forms, kv_len above
    int kv_len_add, kv_max;
    const float* grad_table;   // nullable: probs.grad_factor = grad_table[kv_len], the host's own words
    DecQuant probs, ctx;
    DecCode kc, vc;            // coded form only
    const int32_t* rejected;   // coded form only: the cache's counter; non-zero: the cache holds elements without a code
};

template <int LPR, typename KV, int CH>
__global__ __launch_bounds__(kDecThreads) void decode_attention_kernel(DecArgs a) {
    constexpr int kTripsInFlight = KV::kInFlight;
    constexpr int R = OSQ_WAVE / LPR;              // rows of K / V one wave load covers
    constexpr int kTrip = kDecWaves * R;           // positions one trip of the workgroup covers
    constexpr int kRow = kMaxKv<CH>;
    static_assert(kDecWaves * CH * LPR * 4 <= CH * kRow, "the partial vectors reuse the score rows");
    __shared__ __attribute__((aligned(16))) float s_p[CH * kRow];   // per query: scores -> exps -> fake-quantised probabilities
    __shared__ float s_red[2][CH][kDecWaves];                       // per query: per-wave maxima and sums of exps

    const int lane = threadIdx.x & (OSQ_WAVE - 1), w = threadIdx.x / OSQ_WAVE;
    const int r = lane / LPR, c = lane % LPR;
    const int64_t bh = CH == 1 ? blockIdx.x : blockIdx.x / a.chunks;             // K / V row (b, h)
    const int g0 = CH == 1 ? 0 : static_cast<int>(blockIdx.x % a.chunks) * CH;
    const int gn = CH == 1 ? 1 : min(CH, a.group - g0);     // workgroup-uniform: the chunk's query rows, 1..CH
    const int64_t b = bh / a.heads, h = bh % a.heads;
    const int64_t qh0 = CH == 1 ? bh : (b * a.group + g0) * a.heads + h;   // (query row, head) of the chunk's first query; + g * heads
    int n = a.kv_len;
    DecQuant probs = a.probs;
    if constexpr (CH == 1) {                       // the _at forms exist for one query row only: compiled out of the shared form
        if (a.kv_len_dev) {                        // workgroup-uniform: the length is a device word, read once into an SGPR
            n = __builtin_amdgcn_readfirstlane(*a.kv_len_dev) + a.kv_len_add;
            if (n < 1 || n > a.kv_max) {           // a length no address may be formed from
                const float nan = __builtin_nanf("");
                if (threadIdx.x < LPR) reinterpret_cast<float4*>(a.out)[bh * LPR + c] = make_float4(nan, nan, nan, nan);
                return;
            }
            if (a.grad_table) probs.grad_factor = a.grad_table[n];
        }
    }
    // rows of mask and probs_out: the shared forms are static, their rows lie kv_len apart
    const int64_t mask_stride = CH == 1 ? a.mask_stride : n, probs_stride = CH == 1 ? a.probs_stride : n;
    const int trips = (n + kTrip - 1) / kTrip;
    const QParams pq = dec_params(probs), cq = dec_params(a.ctx);      // first: the parameter repair rides here

    if (a.rejected && *a.rejected != 0) {          // workgroup-uniform: a cache with an uncodable element never yields numbers
        const float nan = __builtin_nanf("");
        for (int g = 0; g < gn; ++g) {
            const int64_t qh = qh0 + g * a.heads;
            if (a.probs_out)
                for (int j = threadIdx.x; j < n; j += kDecThreads) a.probs_out[qh * probs_stride + j] = nan;
            if (threadIdx.x < LPR) reinterpret_cast<float4*>(a.out)[qh * LPR + c] = make_float4(nan, nan, nan, nan);
        }
        return;
    }
    const typename KV::Params kp = KV::params(a.kc), vp = KV::params(a.vc);

    // ---- scores: every word of K loaded once, used by the chunk's queries
    {
        float4 q4[CH];
#pragma unroll
        for (int g = 0; g < CH; ++g)
            q4[g] = reinterpret_cast<const float4*>(a.q)[(qh0 + (g < gn ? g : 0) * a.heads) * LPR + c];
        const int64_t kb = bh * a.k_cap * LPR + c;           // in words of four elements
        const float* mrow = a.mask ? a.mask + b * mask_stride : nullptr;
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
                // a chunk's rows share the mask word: loaded once ahead of them (CH loads in the loop are not merged), and
                // where it is added at CH = 1 (ahead it costs 5 VGPRs at LPR 1 over codes: 67, a wave per SIMD)
                const float m = (CH > 1 && store && mrow) ? mrow[j] : 0.f;
#pragma unroll
                for (int g = 0; g < CH; ++g) {
                    if (g < gn) {                            // uniform; all 64 lanes reach the lane sums
                        float d = q4[g].x * kk.x;
                        d = d + q4[g].y * kk.y;
                        d = d + q4[g].z * kk.z;
                        d = d + q4[g].w * kk.w;
                        d = row_lanes_sum<LPR>(d);
                        if (store) s_p[g * kRow + j] = mrow ? d + (CH > 1 ? m : mrow[j]) : d;
                    }
                }
            }
        }
    }
    __syncthreads();

    // ---- softmax and the probabilities quantizer, per query: thread t owns positions t, t + 256, ...
    for (int g = 0; g < gn; ++g) {
        const float* sp = s_p + g * kRow;
        float mx = -INFINITY;
        for (int j = threadIdx.x; j < n; j += kDecThreads) mx = fmaxf(mx, sp[j]);     // fmaxf drops a NaN: its exp makes the sum NaN
        mx = wave_max(mx);
        if (lane == 0) s_red[0][g][w] = mx;
    }
    __syncthreads();
    for (int g = 0; g < gn; ++g) {
        float* sp = s_p + g * kRow;
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
        float* sp = s_p + g * kRow;
        const float rcp = 1.0f / ((s_red[1][g][0] + s_red[1][g][1]) + (s_red[1][g][2] + s_red[1][g][3]));
        float* prow = a.probs_out ? a.probs_out + (qh0 + g * a.heads) * probs_stride : nullptr;
        for (int j = threadIdx.x; j < n; j += kDecThreads) {
            const float p = dec_fq(sp[j] * rcp, probs, pq);
            sp[j] = p;
            if (prow) prow[j] = p;
        }
    }
    __syncthreads();

    // ---- context: every word of V loaded once, one accumulator per query
    float4 acc[CH];
#pragma unroll
    for (int g = 0; g < CH; ++g) acc[g] = make_float4(0.f, 0.f, 0.f, 0.f);
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
                for (int g = 0; g < CH; ++g) {
                    if (g < gn) {
                        const float p = s_p[g * kRow + j];
                        acc[g].x = acc[g].x + p * vv.x;
                        acc[g].y = acc[g].y + p * vv.y;
                        acc[g].z = acc[g].z + p * vv.z;
                        acc[g].w = acc[g].w + p * vv.w;
                    }
                }
            }
        }
    }
    // [kDecWaves][CH][LPR] per-wave partial context vectors.  At CH = 8 they reuse the score rows once every wave is done with
    // the probabilities; at CH = 1 they keep LDS of their own (4 x head_dim floats): the barrier the reuse costs showed in the
    // coded one-query launch (profiles/decode_attention_fold.txt)
    __shared__ float4 s_own[CH == 1 ? kDecWaves * LPR : 1];
    if constexpr (CH > 1) __syncthreads();
    float4* s_part = CH == 1 ? s_own : reinterpret_cast<float4*>(s_p);
#pragma unroll
    for (int g = 0; g < CH; ++g) {
        if (g < gn) {
            acc[g].x = row_groups_sum<LPR>(acc[g].x);
            acc[g].y = row_groups_sum<LPR>(acc[g].y);
            acc[g].z = row_groups_sum<LPR>(acc[g].z);
            acc[g].w = row_groups_sum<LPR>(acc[g].w);
            if (r == 0) s_part[(w * CH + g) * LPR + c] = acc[g];
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < gn * LPR; i += kDecThreads) {
        const int g = i / LPR, cc = i % LPR;
        float4 o = s_part[g * LPR + cc];
#pragma unroll
        for (int k = 1; k < kDecWaves; ++k) {
            const float4 t = s_part[(k * CH + g) * LPR + cc];
            o.x = o.x + t.x; o.y = o.y + t.y; o.z = o.z + t.z; o.w = o.w + t.w;
        }
        o = make_float4(dec_fq(o.x, a.ctx, cq), dec_fq(o.y, a.ctx, cq), dec_fq(o.z, a.ctx, cq), dec_fq(o.w, a.ctx, cq));
        reinterpret_cast<float4*>(a.out)[(qh0 + g * a.heads) * LPR + cc] = o;     // row b * group + g0 + g, columns of head h
    }
}

// What the _at forms add: the device word of the length, the constant added to it, and the row strides of mask / probs_out.
struct DecAt {
    const int32_t* kv_len_dev;
    int64_t kv_len_add, mask_stride, probs_stride;
    const float* grad_table;
};

// OSQ_REQUIRE with the message's prefix by the chunk size: the texts of the two launchers this one replaces
#define OSQ_DEC_REQUIRE(cond, msg)                                                                \
    do {                                                                                          \
        if (!(cond)) {                                                                            \
            set_error("%s: %s", CH == 1 ? "decode_attention" : "decode_attention_shared", msg);   \
            return OSQ_ERR_INVALID_ARGUMENT;                                                      \
        }                                                                                         \
    } while (0)

// checks and launch shared by the two chunk sizes and the two storage formats; kv_align: what K and V must be aligned to.
// The limits go by CH: kv_len up to kMaxKv<CH>; one query row per K / V row at CH = 1, up to 64 at CH = 8; the grid within
// INT32_MAX, which the one-query forms ask with the shape and the shared forms after their refusals, as each always has.
// at == nullptr: the static forms.  Otherwise (CH = 1 only: the kernel holds the length word's block for one query row) kv_len
// is kv_max, the largest length the launch may meet: every host check holds for all lengths up to it.
template <typename KV, int CH>
static int launch_decode_attention(const char* what, const float* q, const void* k, const void* v, const float* mask, float* out,
                                   float* probs_out, int64_t batch, int64_t group, int64_t heads, int64_t head_dim,
                                   int64_t kv_len, int64_t k_cap, int64_t v_cap, const DecCode& kc, const DecCode& vc,
                                   const int32_t* rejected, const DecQuant& probs, const DecQuant& ctx, uintptr_t kv_align,
                                   osq_stream stream, const DecAt* at = nullptr) {
    const auto grid_fits = [&] {
        return CH == 1 ? batch * heads <= INT32_MAX
                       : batch <= INT32_MAX && heads <= INT32_MAX && batch * heads <= INT32_MAX / kDecMaxGroup;
    };
    OSQ_DEC_REQUIRE(!at || CH == 1, "no _at form");
    OSQ_DEC_REQUIRE(batch >= 0 && heads >= 0 && head_dim > 0 && group >= 1 && (CH != 1 || grid_fits()), "bad shape");
    OSQ_DEC_REQUIRE(!probs.scale || probs.zero_point, "probs scale without zero_point");
    OSQ_DEC_REQUIRE(!ctx.scale || ctx.zero_point, "ctx scale without zero_point");
    OSQ_DEC_REQUIRE(!probs.scale || dec_mode_ok(probs.mode), "bad probs mode");
    OSQ_DEC_REQUIRE(!ctx.scale || dec_mode_ok(ctx.mode), "bad ctx mode");
    if (group > (CH == 1 ? 1 : kDecMaxGroup) || kv_len < 1 || kv_len > kMaxKv<CH>) return OSQ_ERR_UNSUPPORTED;
    const int64_t lpr = head_dim / 4;
    if (head_dim % 4 || lpr > OSQ_WAVE || (lpr & (lpr - 1))) return OSQ_ERR_UNSUPPORTED;
    const int64_t chunks = (group + CH - 1) / CH;
    OSQ_DEC_REQUIRE(grid_fits(), "bad shape");      // asked again at CH = 1, where it cannot fail: only the shared forms ask it here
    OSQ_DEC_REQUIRE(k_cap >= kv_len && v_cap >= kv_len, "cap below kv_len");
    if (at) {
        OSQ_DEC_REQUIRE(at->kv_len_dev, "null kv_len word");
        OSQ_DEC_REQUIRE(at->kv_len_add >= 0 && at->kv_len_add <= kMaxKv<CH>, "bad kv_len_add");
        OSQ_DEC_REQUIRE((!mask || at->mask_stride >= kv_len) && (!probs_out || at->probs_stride >= kv_len), "row stride below kv_max");
    }
    if (batch * heads == 0) return OSQ_OK;
    OSQ_DEC_REQUIRE(q && k && v && out, "null tensor");
    if (!aligned16(q) || !aligned16(out) || !aligned16(mask) || !aligned16(probs_out)) return OSQ_ERR_UNSUPPORTED;
    if ((reinterpret_cast<uintptr_t>(k) | reinterpret_cast<uintptr_t>(v)) & (kv_align - 1u)) return OSQ_ERR_UNSUPPORTED;
    DecArgs a{q, k, v, mask, out, probs_out, heads, k_cap, v_cap, at ? at->mask_stride : kv_len, at ? at->probs_stride : kv_len,
              static_cast<int>(kv_len), static_cast<int>(group), static_cast<int>(chunks), at ? at->kv_len_dev : nullptr,
              at ? static_cast<int>(at->kv_len_add) : 0, static_cast<int>(kv_len), at ? at->grad_table : nullptr, probs, ctx, kc, vc,
              rejected};
    const dim3 grid(static_cast<unsigned>(batch * heads * chunks));
    hipStream_t st = static_cast<hipStream_t>(stream);
#define OSQ_DEC(LPR) hipLaunchKernelGGL((decode_attention_kernel<LPR, KV, CH>), grid, dim3(kDecThreads), 0, st, a)
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
#undef OSQ_DEC_REQUIRE

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
    return launch_decode_attention<KvWords, 1>(
        "decode_attention_fake_quant", q, k, v, mask, out, probs_out, batch, 1, heads, head_dim, kv_len, k_cap, v_cap,
        DecCode{}, DecCode{}, nullptr, OSQ_DEC_QUANT(probs), OSQ_DEC_QUANT(ctx), 16u, stream);
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
    return launch_decode_attention<KvCodes, 1>(
        "decode_attention_codes", q, k, v, mask, out, probs_out, batch, 1, heads, head_dim, kv_len, k_cap, v_cap,
        DecCode{k_scale_eff, k_zp_eff, k_quant_min}, DecCode{v_scale_eff, v_zp_eff, v_quant_min}, rejected,
        OSQ_DEC_QUANT(probs), OSQ_DEC_QUANT(ctx), 4u, stream);
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
    return launch_decode_attention<KvWords, 1>(
        "decode_attention_fake_quant_at", q, k, v, mask, out, probs_out, batch, 1, heads, head_dim, kv_max, k_cap, v_cap,
        DecCode{}, DecCode{}, nullptr, OSQ_DEC_QUANT(probs), OSQ_DEC_QUANT(ctx), 16u, stream, &at);
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
    return launch_decode_attention<KvCodes, 1>(
        "decode_attention_codes_at", q, k, v, mask, out, probs_out, batch, 1, heads, head_dim, kv_max, k_cap, v_cap,
        DecCode{k_scale_eff, k_zp_eff, k_quant_min}, DecCode{v_scale_eff, v_zp_eff, v_quant_min}, rejected,
        OSQ_DEC_QUANT(probs), OSQ_DEC_QUANT(ctx), 4u, stream, &at);
}

extern "C" int osq_decode_attention_shared(const float* q, const float* k, const float* v, const float* mask, float* out,
                                           float* probs_out, int64_t batch, int64_t group, int64_t heads, int64_t head_dim,
                                           int64_t kv_len, int64_t k_cap, int64_t v_cap,
                                           float* probs_scale, void* probs_zero_point, int probs_zp_type, int probs_mode,
                                           float probs_grad_factor, int probs_quant_min, int probs_quant_max,
                                           float* ctx_scale, void* ctx_zero_point, int ctx_zp_type, int ctx_mode,
                                           float ctx_grad_factor, int ctx_quant_min, int ctx_quant_max,
                                           osq_stream stream) {
    return launch_decode_attention<KvWords, 8>(
        "decode_attention_shared", q, k, v, mask, out, probs_out, batch, group, heads, head_dim, kv_len, k_cap, v_cap,
        DecCode{}, DecCode{}, nullptr, OSQ_DEC_QUANT(probs), OSQ_DEC_QUANT(ctx), 16u, stream);
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
    OSQ_REQUIRE(k_scale_eff && k_zp_eff && v_scale_eff && v_zp_eff && rejected, "decode_attention_shared_codes: null record or rejected counter");
    return launch_decode_attention<KvCodes, 8>(
        "decode_attention_shared_codes", q, k, v, mask, out, probs_out, batch, group, heads, head_dim, kv_len, k_cap, v_cap,
        DecCode{k_scale_eff, k_zp_eff, k_quant_min}, DecCode{v_scale_eff, v_zp_eff, v_quant_min}, rejected,
        OSQ_DEC_QUANT(probs), OSQ_DEC_QUANT(ctx), 4u, stream);
}

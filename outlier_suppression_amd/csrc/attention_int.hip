// Attention over a WHOLE sequence on the quantizers' INTEGER CODES: the one launch of attention_block.hip with both products on
// the bf16 matrix instruction v_mfma_f32_32x32x16_bf16 -- and exact.
//
// Every operand of both products is the output of a per-tensor quantizer the attention module owns: s * n with an integer
// |n| <= 255.  Such integers are exact in bf16 (8 significant bits), their products (< 2**16) are exact in fp32, and fp32
// sums that stay below 2**24 are exact in ANY order.  So the products are computed on the integers, the scales are applied
// once to the exact sum, and the kernel may tile as it likes: no S-sized LDS, no limit at 1024 keys, no order contract for
// the products.  For every (b, head, t), with (s_x, zp_x, qmin_x, qmax_x) the repaired parameters of site x (dec_params):
//
//     n_q[t][i] = clamp(rint(q[t][i] / s_q) + zp_q, qmin_q, qmax_q) - zp_q     likewise n_k[j][i], n_v[j][i]: the site's
//                 quantizer once more -- on the quantizers' own outputs this is their integer, exactly
//     N[j]  = sum_i n_q[t][i] * n_k[j][i]                 EXACT integer, |N| < 2**24
//     sc[j] = float(N[j]) * (s_q * s_k)                   s_q * s_k rounded once
//     x[j]  = pre(sc[j]) + mask[b, h, t, j]               the pre-softmax rule (attention_seq.h): one rounding per operation
//     p     = softmax(x)                                  row max exact; e = expf(x - max) (ocml); the denominator: per half h
//                                                         of a key tile's rows (below) the chain from +0 over the tiles in
//                                                         order and the half's 16 keys of a tile in register order, then
//                                                         half 0 + half 1; p = e * (1 / sum).  A row with a NaN, a +inf or
//                                                         only -inf is NaN (that row only)
//     n_p[j] = clamp(rint(p[j] / s_p) + zp_p, qmin_p, qmax_p) - zp_p            probs_out gets n_p * s_p (dec_fq's word)
//     C[i]  = sum_j n_p[j] * n_v[j][i]                    EXACT integer (up to 2**30): fp32 over at most kIntChunk = 128 keys
//                                                         (< 2**23), the chunks added as int32
//     c[i]  = float(C[i]) * (s_p * s_v)                   int -> float round-to-nearest-even, one product
//     out   = fq_ctx(c), or c without a context quantizer, merged [B, T, h * d]
//
// Work split: one 256-thread workgroup per (b, head, tile of kIntTQ = 128 queries), a wave per 32 queries.  The keys go by in
// tiles of kIntTK = 32: the workgroup converts a tile of K (and, in the last pass, of V) to integers ONCE and shares it through
// LDS as bf16; the next tile's loads are in flight while this one is computed.  A wave computes the score tile as K_tile . Q^T
// (A = K from LDS, B = its 32 queries, held in registers for the whole kernel): the query then sits on the lane (lane & 31)
// and the keys in the 16 result registers (key row (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)), a row's max and sum are a
// reduction over registers plus one exchange with lane ^ 32, and the tile of probability codes is, packed to bf16, already the
// B operand of V^T . P^T (registers 8s .. 8s + 7 are k-step s; A = V^T from a transposed LDS image, read in that same k
// order).  Three passes over the keys -- max; denominator; codes and context -- each recomputing the score tile: the
// products are the cheap part and nothing of S's size is kept.
//
// LDS: the K tile (32 rows of D + 8 bf16) and the V^T tile (max(D, 32) rows of 36 bf16): 17920 B = 17.5 KiB at head_dim 128.
//
// What the host cannot see the workgroups check themselves: a repaired zero point of q, k, v or the probabilities that is
// not an integer inside [qmin, qmax] (|n| could exceed 255, or not be an integer) makes the launch write NaN to all of out
// and probs_out.  A non-finite element of q, k or v makes n NaN (quantize_value), and a NaN reaches exactly the outputs the
// eager sequence would hand it to: a chunk sum that is not a finite integer below 2**24 is caught BEFORE the float -> int
// conversion and marks its output NaN.
//
// The words of a query row depend on that row of q alone (a column of an MFMA result depends on that column of B alone):
// not on T, on where the row sits in its tile, on B or h, or on strides.  Rows beyond T repeat row T - 1 (dropped); keys
// beyond S carry code 0 in P and V and are neither reduced nor stored.  Addresses are clamped to [0, T) and [0, S).
// So a GROUP of G decoder rows that share one row of k, v and mask (osq_attention_fake_quant_int_shared) is the row map of
// attention_seq.h and nothing else: a workgroup's 128 queries are virtual rows of [0, G * T), and out and probs_out are word for
// word those of the unshared entry point on k, v and mask repeated G times.
// Inference only; no allocation, no host sync, no workspace, no atomics: legal inside a stream capture.
#include <math.h>
#include <hip/hip_runtime.h>
#include "attention_seq.h"

namespace osq {

constexpr int kIntThreads = 256;
constexpr int kIntWaves = kIntThreads / OSQ_WAVE;
constexpr int kIntTQ = 32 * kIntWaves;   // query rows of a workgroup
constexpr int kIntTK = 32;               // keys of a tile: the M of the score product, two k-steps of the context product
constexpr int kIntChunk = 128;           // keys whose context terms are summed in fp32 before they join the int32 sum
constexpr int kIntMaxS = 16384;          // C <= 255 * 255 * S < 2**30
constexpr int kIntVtStride = 36;         // bf16 per row of the V^T image: 72 B, 8-byte aligned reads, rows 18 banks apart

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));
typedef unsigned short u16x4 __attribute__((ext_vector_type(4)));

struct IntArgs : SeqArgs {     // tiles of kIntTQ queries
    DecQuant qq, kq, vq, probs, ctx;
};

// the bf16 word of an integer |n| <= 256 (exact: the low 16 bits are zero) or of a NaN
__device__ __forceinline__ unsigned short int_bf16(float n) {
    return n != n ? static_cast<unsigned short>(0x7FC0u) : static_cast<unsigned short>(__float_as_uint(n) >> 16);
}

// the integer of the rule: the site's quantizer, minus the zero point (NaN for a non-finite x)
__device__ __forceinline__ float int_code(float x, const DecQuant& d, const QParams& p) {
    return quantize_value(x, p.scale, p.zp, d.qmin, d.qmax) - p.zp;
}

__device__ __forceinline__ bool int_zp_ok(const DecQuant& d, const QParams& p) {
    return p.zp >= d.qmin && p.zp <= d.qmax && rintf(p.zp) == p.zp;
}

template <int D>
__global__ __launch_bounds__(kIntThreads) void attention_int_kernel(IntArgs a) {
    constexpr int KSTEPS = D / 16;                    // k-steps of the score product
    constexpr int KP = D + 8;                         // bf16 per row of the K tile: 16-byte aligned rows, 4 banks apart
    constexpr int NCH = D >= 32 ? D / 32 : 1;         // 32-row chunks of the context (head_dim 16: half a chunk)
    constexpr int VROWS = NCH * 32;
    constexpr int NV = D >= 32 ? D / 32 : 1;          // float4 a thread loads of a 32 x D tile
    constexpr int F4ROW = D / 4;                      // float4 per row
    __shared__ __attribute__((aligned(16))) unsigned short s_k[kIntTK * KP];
    __shared__ __attribute__((aligned(16))) unsigned short s_vt[VROWS * kIntVtStride];

    const int lane = threadIdx.x & (OSQ_WAVE - 1), w = threadIdx.x / OSQ_WAVE;
    const int l31 = lane & 31, half = lane >> 5;
    const int64_t bh = blockIdx.x / a.tiles;
    const int t0 = static_cast<int>(blockIdx.x % a.tiles) * kIntTQ;
    const int64_t b = bh / a.heads, h = bh % a.heads;
    const int R = a.rows, S = a.kv_len;               // virtual query rows of this (b, head): the row map of attention_seq.h
    const int nrows = min(kIntTQ, R - t0);            // 1..128 query rows of this workgroup
    const QParams qp = dec_params(a.qq), kp = dec_params(a.kq), vp = dec_params(a.vq);   // first: the parameter repair rides here
    const QParams pq = dec_params(a.probs), cq = dec_params(a.ctx);

    if (!(int_zp_ok(a.qq, qp) && int_zp_ok(a.kq, kp) && int_zp_ok(a.vq, vp) && int_zp_ok(a.probs, pq))) {   // uniform
        const float nan = __builtin_nanf("");
        for (int i = threadIdx.x; i < nrows * D; i += kIntThreads) seq_out_row<D>(a, b, h, t0 + i / D)[i % D] = nan;
        if (a.probs_out) {
            for (int row = 0; row < nrows; ++row) {
                float* p = seq_probs_row(a, b, h, t0 + row);
                for (int i = threadIdx.x; i < S; i += kIntThreads) p[i] = nan;
            }
        }
        return;
    }

    const bool active = t0 + 32 * w < R;              // a wave whose 32 queries all lie beyond R only helps with the tiles
    const int tq = min(t0 + 32 * w + l31, R - 1);     // this lane's query: a virtual row
    const float sqk = qp.scale * kp.scale, spv = pq.scale * vp.scale;

    // ---- this lane's share of Q as the B operand: k-step s holds q[tq][16 s + 8 half + 0..7]
    bf16x8 qf[KSTEPS];
    {
        const float4* qrow = reinterpret_cast<const float4*>(seq_q_row(a, b, h, tq));
#pragma unroll
        for (int s = 0; s < KSTEPS; ++s) {
            const float4 x = qrow[4 * s + 2 * half], y = qrow[4 * s + 2 * half + 1];
            u16x8 u;
            u[0] = int_bf16(int_code(x.x, a.qq, qp)); u[1] = int_bf16(int_code(x.y, a.qq, qp));
            u[2] = int_bf16(int_code(x.z, a.qq, qp)); u[3] = int_bf16(int_code(x.w, a.qq, qp));
            u[4] = int_bf16(int_code(y.x, a.qq, qp)); u[5] = int_bf16(int_code(y.y, a.qq, qp));
            u[6] = int_bf16(int_code(y.z, a.qq, qp)); u[7] = int_bf16(int_code(y.w, a.qq, qp));
            qf[s] = __builtin_bit_cast(bf16x8, u);
        }
    }
    if constexpr (VROWS > D) {                        // head_dim 16: rows 16 .. 31 of the V^T image stay zero
        for (int i = threadIdx.x; i < (VROWS - D) * kIntVtStride; i += kIntThreads) s_vt[D * kIntVtStride + i] = 0;
    }

    const float* kbase = a.k + b * a.k_sb + h * a.k_sh;
    const float* vbase = a.v + b * a.v_sb + h * a.v_sh;
    const float* mbase = a.mask ? seq_mask_row(a, b, h, tq) : nullptr;
    const int ktiles = (S + kIntTK - 1) / kIntTK;

    // a thread's float4s of tile jt of K or V: float4 number threadIdx.x + 256 u is row idx / F4ROW, elements 4 (idx % F4ROW)..
    const auto load_tile = [&](const float* base, int64_t stride, int jt, float4* x) {
#pragma unroll
        for (int u = 0; u < NV; ++u) {
            const int idx = threadIdx.x + kIntThreads * u;
            if (idx < kIntTK * F4ROW) {
                const int key = min(jt * kIntTK + idx / F4ROW, S - 1);
                x[u] = reinterpret_cast<const float4*>(base + static_cast<int64_t>(key) * stride)[idx % F4ROW];
            }
        }
    };
    const auto store_k = [&](const float4* x) {
#pragma unroll
        for (int u = 0; u < NV; ++u) {
            const int idx = threadIdx.x + kIntThreads * u;
            if (idx < kIntTK * F4ROW) {
                u16x4 c;
                c[0] = int_bf16(int_code(x[u].x, a.kq, kp)); c[1] = int_bf16(int_code(x[u].y, a.kq, kp));
                c[2] = int_bf16(int_code(x[u].z, a.kq, kp)); c[3] = int_bf16(int_code(x[u].w, a.kq, kp));
                *reinterpret_cast<u16x4*>(&s_k[(idx / F4ROW) * KP + 4 * (idx % F4ROW)]) = c;
            }
        }
    };
    const auto store_vt = [&](const float4* x, int jt) {      // transposed: [element][key]; a key beyond S is code 0
#pragma unroll
        for (int u = 0; u < NV; ++u) {
            const int idx = threadIdx.x + kIntThreads * u;
            if (idx < kIntTK * F4ROW) {
                const int key = idx / F4ROW, e = 4 * (idx % F4ROW);
                const bool ok = jt * kIntTK + key < S;
                s_vt[(e + 0) * kIntVtStride + key] = ok ? int_bf16(int_code(x[u].x, a.vq, vp)) : 0;
                s_vt[(e + 1) * kIntVtStride + key] = ok ? int_bf16(int_code(x[u].y, a.vq, vp)) : 0;
                s_vt[(e + 2) * kIntVtStride + key] = ok ? int_bf16(int_code(x[u].z, a.vq, vp)) : 0;
                s_vt[(e + 3) * kIntVtStride + key] = ok ? int_bf16(int_code(x[u].w, a.vq, vp)) : 0;
            }
        }
    };
    // x[r] of the rule for the tile in LDS: key jt * 32 + mfma32_row(r, half), query tq (keys beyond S: whatever, never used)
    const auto score_tile = [&](int jt, float* x) {
        f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < KSTEPS; ++s) {
            const u16x8 kf = *reinterpret_cast<const u16x8*>(&s_k[l31 * KP + 16 * s + 8 * half]);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, kf), qf[s], acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float y = pre_softmax(a.pre, acc[r] * sqk, a.alpha, a.divisor);
            if (mbase) y = y + mbase[min(jt * kIntTK + mfma32_row(r, half), S - 1)];
            x[r] = y;
        }
    };
    // every tile of the keys in turn through LDS, the next tile's loads issued before this one's work; f(jt) by the active waves
    const auto for_tiles = [&](bool with_v, auto&& f) {
        float4 kx[NV], vx[NV];
        load_tile(kbase, a.k_st, 0, kx);
        if (with_v) load_tile(vbase, a.v_st, 0, vx);
        for (int jt = 0; jt < ktiles; ++jt) {
            __syncthreads();                          // the last tile's readers are done
            store_k(kx);
            if (with_v) store_vt(vx, jt);
            __syncthreads();
            if (jt + 1 < ktiles) {
                load_tile(kbase, a.k_st, jt + 1, kx);
                if (with_v) load_tile(vbase, a.v_st, jt + 1, vx);
            }
            if (active) f(jt);
        }
    };

    // ---- pass 1: the row maximum (fmaxf drops a NaN: its exp makes the sum NaN)
    float mx = -INFINITY;
    for_tiles(false, [&](int jt) {
        float x[16];
        score_tile(jt, x);
#pragma unroll
        for (int r = 0; r < 16; ++r)
            if (jt * kIntTK + mfma32_row(r, half) < S) mx = fmaxf(mx, x[r]);
    });
    mx = fmaxf(mx, __shfl_xor(mx, 32, OSQ_WAVE));

    // ---- pass 2: the denominator
    float sum = 0.f;
    for_tiles(false, [&](int jt) {
        float x[16];
        score_tile(jt, x);
#pragma unroll
        for (int r = 0; r < 16; ++r)
            if (jt * kIntTK + mfma32_row(r, half) < S) sum = sum + expf(x[r] - mx);
    });
    {
        const float other = __shfl_xor(sum, 32, OSQ_WAVE);
        sum = half ? other + sum : sum + other;       // half 0 + half 1 in both lanes
    }
    const float rcp = 1.0f / sum;

    // ---- pass 3: probability codes and the context  C^T[i][t] = sum_j V^T[i][j] * P^T[j][t]
    f32x16 cacc[NCH];
    int cint[NCH][16];
    unsigned bad[NCH];                                // bit r: a chunk sum of register r was no finite integer below 2**24
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        bad[c] = 0;
#pragma unroll
        for (int r = 0; r < 16; ++r) { cacc[c][r] = 0.f; cint[c][r] = 0; }
    }
    const auto flush = [&]() {
#pragma unroll
        for (int c = 0; c < NCH; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float f = cacc[c][r];
                if (fabsf(f) < 16777216.f) cint[c][r] += static_cast<int>(f);    // false for a NaN and an infinity
                else bad[c] |= 1u << r;
                cacc[c][r] = 0.f;
            }
    };
    float* prow = a.probs_out ? seq_probs_row(a, b, h, tq) : nullptr;
    const bool row_ok = t0 + 32 * w + l31 < R;
    for_tiles(true, [&](int jt) {
        float x[16];
        score_tile(jt, x);
        u16x8 pf[2];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int key = jt * kIntTK + mfma32_row(r, half);
            float n = 0.f;
            if (key < S) {
                const float p = expf(x[r] - mx) * rcp;
                n = int_code(p, a.probs, pq);
                if (prow && row_ok) prow[key] = n * pq.scale;
            }
            pf[r >> 3][r & 7] = int_bf16(n);
        }
#pragma unroll
        for (int c = 0; c < NCH; ++c)
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                // element j of half h is key 16 s + 8 (j >> 2) + 4 h + (j & 3) on both operands
                const unsigned short* vrow = &s_vt[(32 * c + l31) * kIntVtStride + 16 * s + 4 * half];
                const u16x4 lo = *reinterpret_cast<const u16x4*>(vrow), hi = *reinterpret_cast<const u16x4*>(vrow + 8);
                const u16x8 vf = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                cacc[c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, vf), __builtin_bit_cast(bf16x8, pf[s]),
                                                                  cacc[c], 0, 0, 0);
            }
        if ((jt + 1) % (kIntChunk / kIntTK) == 0) flush();
    });
    flush();

    if (row_ok) {
        float* orow = seq_out_row<D>(a, b, h, tq);
#pragma unroll
        for (int c = 0; c < NCH; ++c)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int i = 32 * c + 8 * g + 4 * half;                    // elements i .. i + 3: registers 4 g .. 4 g + 3
                if (i < D) {
                    float y[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int r = 4 * g + e;
                        const float cf = static_cast<float>(cint[c][r]) * spv;
                        y[e] = (bad[c] >> r) & 1u ? __builtin_nanf("") : dec_fq(cf, a.ctx, cq);
                    }
                    *reinterpret_cast<float4*>(orow + i) = make_float4(y[0], y[1], y[2], y[3]);
                }
            }
    }
}

static bool int_site_ok(const float* scale, const void* zero_point, int mode, int quant_min, int quant_max) {
    return scale && zero_point && dec_mode_ok(mode) && quant_min <= quant_max &&
           static_cast<int64_t>(quant_max) - quant_min <= 255;
}

}  // namespace osq

using namespace osq;

// batch counts the rows of k / v; q, out and probs_out have batch * group
extern "C" int osq_attention_fake_quant_int_shared(const float* q, const float* k, const float* v, const float* mask, float* out,
                                            float* probs_out, int64_t batch, int64_t group, int64_t heads, int64_t tokens,
                                            int64_t kv_len, int64_t head_dim,
                                            int64_t q_stride_b, int64_t q_stride_h, int64_t q_stride_t,
                                            int64_t k_stride_b, int64_t k_stride_h, int64_t k_stride_t,
                                            int64_t v_stride_b, int64_t v_stride_h, int64_t v_stride_t,
                                            int64_t mask_stride_b, int64_t mask_stride_h, int64_t mask_stride_t,
                                            float alpha, float divisor,
                                            float* q_scale, void* q_zero_point, int q_zp_type, int q_mode,
                                            float q_grad_factor, int q_quant_min, int q_quant_max,
                                            float* k_scale, void* k_zero_point, int k_zp_type, int k_mode,
                                            float k_grad_factor, int k_quant_min, int k_quant_max,
                                            float* v_scale, void* v_zero_point, int v_zp_type, int v_mode,
                                            float v_grad_factor, int v_quant_min, int v_quant_max,
                                            float* probs_scale, void* probs_zero_point, int probs_zp_type, int probs_mode,
                                            float probs_grad_factor, int probs_quant_min, int probs_quant_max,
                                            float* ctx_scale, void* ctx_zero_point, int ctx_zp_type, int ctx_mode,
                                            float ctx_grad_factor, int ctx_quant_min, int ctx_quant_max,
                                            osq_stream stream) {
    const char* what = "attention_fake_quant_int";
    IntArgs a{{q, k, v, mask, out, probs_out, q_stride_b, q_stride_h, q_stride_t, k_stride_b, k_stride_h, k_stride_t,
               v_stride_b, v_stride_h, v_stride_t, mask_stride_b, mask_stride_h, mask_stride_t, heads, 0, 0, 0, 0, 0, 0, alpha,
               divisor},
              OSQ_DEC_QUANT(q), OSQ_DEC_QUANT(k), OSQ_DEC_QUANT(v), OSQ_DEC_QUANT(probs), OSQ_DEC_QUANT(ctx)};
    if (const int rc = seq_check_shape(what, a, batch, group, tokens, head_dim)) return rc;
    OSQ_SEQ_REQUIRE(!ctx_scale || ctx_zero_point, "ctx scale without zero_point");
    OSQ_SEQ_REQUIRE(!ctx_scale || dec_mode_ok(ctx_mode), "bad ctx mode");
    // the four quantizers of the products: all there, per-tensor records, at most 256 codes
    if (!int_site_ok(q_scale, q_zero_point, q_mode, q_quant_min, q_quant_max) ||
        !int_site_ok(k_scale, k_zero_point, k_mode, k_quant_min, k_quant_max) ||
        !int_site_ok(v_scale, v_zero_point, v_mode, v_quant_min, v_quant_max) ||
        !int_site_ok(probs_scale, probs_zero_point, probs_mode, probs_quant_min, probs_quant_max))
        return OSQ_ERR_UNSUPPORTED;
    int64_t blocks;
    if (const int rc = seq_check_launch(what, a, batch, tokens, kv_len, head_dim, kIntTQ, kIntMaxS, &blocks); rc || !blocks) return rc;
    const dim3 grid(static_cast<unsigned>(blocks));
    hipStream_t st = static_cast<hipStream_t>(stream);
    OSQ_HEAD_DIM_DISPATCH(head_dim, hipLaunchKernelGGL((attention_int_kernel<D>), grid, dim3(kIntThreads), 0, st, a));
    return check_launch(what);
}

extern "C" int osq_attention_fake_quant_int(const float* q, const float* k, const float* v, const float* mask, float* out,
                                            float* probs_out, int64_t batch, int64_t heads, int64_t tokens, int64_t kv_len,
                                            int64_t head_dim,
                                            int64_t q_stride_b, int64_t q_stride_h, int64_t q_stride_t,
                                            int64_t k_stride_b, int64_t k_stride_h, int64_t k_stride_t,
                                            int64_t v_stride_b, int64_t v_stride_h, int64_t v_stride_t,
                                            int64_t mask_stride_b, int64_t mask_stride_h, int64_t mask_stride_t,
                                            float alpha, float divisor,
                                            float* q_scale, void* q_zero_point, int q_zp_type, int q_mode,
                                            float q_grad_factor, int q_quant_min, int q_quant_max,
                                            float* k_scale, void* k_zero_point, int k_zp_type, int k_mode,
                                            float k_grad_factor, int k_quant_min, int k_quant_max,
                                            float* v_scale, void* v_zero_point, int v_zp_type, int v_mode,
                                            float v_grad_factor, int v_quant_min, int v_quant_max,
                                            float* probs_scale, void* probs_zero_point, int probs_zp_type, int probs_mode,
                                            float probs_grad_factor, int probs_quant_min, int probs_quant_max,
                                            float* ctx_scale, void* ctx_zero_point, int ctx_zp_type, int ctx_mode,
                                            float ctx_grad_factor, int ctx_quant_min, int ctx_quant_max,
                                            osq_stream stream) {
    return osq_attention_fake_quant_int_shared(q, k, v, mask, out, probs_out, batch, 1, heads, tokens, kv_len, head_dim, q_stride_b,
                                q_stride_h, q_stride_t, k_stride_b, k_stride_h, k_stride_t, v_stride_b, v_stride_h,
                                v_stride_t, mask_stride_b, mask_stride_h, mask_stride_t, alpha, divisor, q_scale,
                                q_zero_point, q_zp_type, q_mode, q_grad_factor, q_quant_min, q_quant_max, k_scale,
                                k_zero_point, k_zp_type, k_mode, k_grad_factor, k_quant_min, k_quant_max, v_scale,
                                v_zero_point, v_zp_type, v_mode, v_grad_factor, v_quant_min, v_quant_max, probs_scale,
                                probs_zero_point, probs_zp_type, probs_mode, probs_grad_factor, probs_quant_min,
                                probs_quant_max, ctx_scale, ctx_zero_point, ctx_zp_type, ctx_mode, ctx_grad_factor,
                                ctx_quant_min, ctx_quant_max, stream);
}

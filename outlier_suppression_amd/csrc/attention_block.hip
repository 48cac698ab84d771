// Attention over a WHOLE sequence: scores, pre-softmax scaling, mask, softmax, probabilities quantizer, context, merge-heads
// context quantizer in ONE launch -- the T > 1 counterpart of decode_attention.hip.
//
// QuantizedBertSelfAttention.forward (model/quant_bert.py) and QuantizedBartAttention._attend (model/quant_bart.py) run
//     bmm -> (scale, mask add, softmax, probs quantizer) -> bmm -> merge heads + context quantizer
// and the [B, h, T, S] scores tensor crosses HBM four times.  Here a workgroup keeps the score rows of a tile of queries in
// LDS: it reads Q, K, V and the mask and writes the context.  For every (b, head, query t):
//
//     s[j] = dot(q[t], k[j])                    j < S
//     v[j] = pre(s[j]) + mask[b, h, t, j]       the pre-softmax rule (attention_seq.h)
//     p    = softmax(v)                         row max subtracted, ocml's accurate expf, fp32 sum, p = e * (1 / sum); a row
//                                               with a NaN, a +inf or only -inf is NaN (that row only)
//     p'   = fq(p)                              attention_probs quantizer (dec_fq, attention_quant.h)
//     c    = sum_j p'[j] * V[j];  out = fq(c)   context quantizer, written in the merged [B, T, h * d] layout
//
// Work split: one 256-thread workgroup per (b, head, tile of kBlkTQ = 32 queries); the tiles of a (b, head) are neighbours in
// the grid, so the second finds K and V in L2.  Both products run on the fp32-input matrix instruction
// v_mfma_f32_32x32x2_f32 (__builtin_amdgcn_mfma_f32_32x32x2f32): its result is bit for bit a k-ordered chain of fmaf, one
// rounding per product, whatever -ffp-contract says, so the order of every sum stays defined.
//
//   scores   key tiles of kBlkTK = 32 go round the four waves.  A lane holds half a row of Q (row t0 + (lane & 31), elements
//            [half * d/2, (half + 1) * d/2), half = lane >> 5) in d/2 registers, loads the same half of a row of K, and
//            d/2 instructions give the 32 x 32 tile.  pre(s) + mask goes to the tile's score rows in LDS.
//   softmax  a wave per row, rows going round the waves: max, exps, sum, p' -- in place, as in the decode kernel -- and
//            p' to probs_out.
//   context  A = the rows of p' from LDS, B = V from memory (a lane loads ONE float per step; 32 lanes cover 128 B of a
//            row); wave w takes the 32 columns w % (d / 32) of the context and segment w / (d / 32) of the steps; the
//            segments' partial tiles meet in LDS, over the score rows after one more barrier.
//
// LDS: 32 score rows of SMAX + 1 floats, SMAX the kernel's class of S (128 / 256 / 512 / 1024: 16.1 / 32.1 / 64.1 /
// 128.1 KiB of the CU's 160: 9 / 4 / 2 / 1 workgroups per CU by LDS); the 16 KiB of partial context tiles reuse them.
//
// ORDER CONTRACT.  Every sum is in an order fixed by (head_dim, S) alone; no float atomics.
//   a score      fma chain from +0 over k = 0, d/2, 1, d/2 + 1, ..., d/2 - 1, d - 1;
//   the softmax  max: exact.  denominator: lane l adds exps l, l + 64, ... in order, then wave_sum_f32;
//   a context    element: with n = ceil(S / 2) steps in 128 / d segments (d = 16: 4) of ceil(n / segments) steps, segment g
//                is the fma chain from +0 over j = 2 * first(g), 2 * first(g) + 1, ... in order; then ((g0 + g1) + g2) + g3.
// A row of an MFMA result depends on that row of A alone, and each query row is reduced by one wave on its own: the words of
// a query row do not depend on T, on where the row sits in its tile, on B or h, or on strides.  Padding: rows beyond T repeat
// row T - 1 (their results are dropped); key columns beyond S are neither stored nor reduced; a step beyond S (odd S) or
// beyond a wave's segment multiplies +0 by +0 -- and a chain that starts at +0 never holds -0, so adding +0 changes no
// word, signed zeros included.  Addresses are clamped to [0, T) and [0, S): memory beyond them is never read.
// So a GROUP of G decoder rows that share one row of k, v and mask (osq_attention_fake_quant_shared) is the row map of
// attention_seq.h and nothing else: a tile's 32 queries are virtual rows of [0, G * T), and out and probs_out are word for word
// those of the unshared entry point on k, v and mask repeated G times.
//
// Inference only; no allocation, no host sync, no workspace: legal inside a stream capture.  The parameter repair under
// OSQ_PARAM_SANITIZE rides in every workgroup (all compute the same repaired words).
#include <math.h>
#include <hip/hip_runtime.h>
#include "attention_seq.h"

namespace osq {

constexpr int kBlkThreads = 256;
constexpr int kBlkWaves = kBlkThreads / OSQ_WAVE;
constexpr int kBlkTQ = 32;          // query rows of a workgroup: the M of the matrix instruction
constexpr int kBlkTK = 32;          // key columns of a score tile: its N
constexpr int kBlkMaxS = 1024;
constexpr int kBlkInFlight = 16;    // steps of the context a lane loads at once (a word of V, a probability), one batch ahead

struct BlkArgs : SeqArgs {     // tiles of kBlkTQ queries
    DecQuant probs, ctx;
};

template <int D, int SMAX>
__global__ __launch_bounds__(kBlkThreads) void attention_block_kernel(BlkArgs a) {
    constexpr int SP = SMAX + 1;                      // odd row stride: the 32 rows of a column lie in 32 banks
    constexpr int HALF = D / 2;                       // elements of a row of Q / K a lane holds
    constexpr int NCH = D >= 32 ? D / 32 : 1;         // 32-column chunks of the context
    constexpr int NSEG = kBlkWaves / NCH;             // segments of the steps over j
    static_assert(kBlkWaves * kBlkTQ * 32 <= kBlkTQ * SP, "the partial context tiles reuse the score rows");
    __shared__ float s_p[kBlkTQ * SP];                // per query: scores -> exps -> fake-quantised probabilities
    // per wave: its partial 32 x 32 tile of the context, over the score rows once every wave is done with the probabilities
    // (16 KiB of their own would leave S = 512 at 80.1 KiB: one workgroup per CU where two fit)
    float (*s_part)[kBlkTQ][32] = reinterpret_cast<float (*)[kBlkTQ][32]>(s_p);

    const int lane = threadIdx.x & (OSQ_WAVE - 1), w = threadIdx.x / OSQ_WAVE;
    const int l31 = lane & 31, half = lane >> 5;
    const int64_t bh = blockIdx.x / a.tiles;
    const int t0 = static_cast<int>(blockIdx.x % a.tiles) * kBlkTQ;
    const int64_t b = bh / a.heads, h = bh % a.heads;
    const int R = a.rows, S = a.kv_len;               // virtual query rows of this (b, head): the row map of attention_seq.h
    const int nrows = min(kBlkTQ, R - t0);            // 1..32 query rows of this tile
    const QParams pq = dec_params(a.probs), cq = dec_params(a.ctx);      // first: the parameter repair rides here

    // ---- scores
    {
        float qf[HALF];
        const float4* qrow = reinterpret_cast<const float4*>(seq_q_row(a, b, h, min(t0 + l31, R - 1)) + half * HALF);
#pragma unroll
        for (int c = 0; c < HALF / 4; ++c) {
            const float4 x = qrow[c];
            qf[4 * c] = x.x; qf[4 * c + 1] = x.y; qf[4 * c + 2] = x.z; qf[4 * c + 3] = x.w;
        }
        const float* kbase = a.k + b * a.k_sb + h * a.k_sh + half * HALF;
        const int ktiles = (S + kBlkTK - 1) / kBlkTK;
        // half a row of K of key tile jt; the next tile's loads are issued before this tile's products
        const auto load_k = [&](int jt, float* kf) {
            const float4* krow = reinterpret_cast<const float4*>(kbase + static_cast<int64_t>(min(jt * kBlkTK + l31, S - 1)) * a.k_st);
#pragma unroll
            for (int c = 0; c < HALF / 4; ++c) {
                const float4 x = krow[c];
                kf[4 * c] = x.x; kf[4 * c + 1] = x.y; kf[4 * c + 2] = x.z; kf[4 * c + 3] = x.w;
            }
        };
        // (head_dim 128 loads each tile as it comes: a second half row of 64 registers leaves one wave per SIMD)
        constexpr bool kAhead = HALF <= 32;
        float kf[HALF], kn[kAhead ? HALF : 1];
        if (kAhead && w < ktiles) load_k(w, kf);
        for (int jt = w; jt < ktiles; jt += kBlkWaves) {
            const int col = jt * kBlkTK + l31;
            if constexpr (!kAhead) load_k(jt, kf);
            else if (jt + kBlkWaves < ktiles) load_k(jt + kBlkWaves, kn);
            f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kk = 0; kk < HALF; ++kk) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(qf[kk], kf[kk], acc, 0, 0, 0);
            if (col < S) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = mfma32_row(r, half);
                    float x = pre_softmax(a.pre, acc[r], a.alpha, a.divisor);
                    if (a.mask) x = x + seq_mask_row(a, b, h, min(t0 + row, R - 1))[col];
                    s_p[row * SP + col] = x;
                }
            }
            if constexpr (kAhead) {
#pragma unroll
                for (int kk = 0; kk < HALF; ++kk) kf[kk] = kn[kk];
            }
        }
    }
    __syncthreads();

    // ---- softmax and the probabilities quantizer: a wave per row, lane l owns positions l, l + 64, ...
    for (int row = w; row < nrows; row += kBlkWaves) {
        float* sp = s_p + row * SP;
        float mx = -INFINITY;
        for (int j = lane; j < S; j += OSQ_WAVE) mx = fmaxf(mx, sp[j]);     // fmaxf drops a NaN: its exp makes the sum NaN
        mx = wave_max(mx);
        float sum = 0.f;
        for (int j = lane; j < S; j += OSQ_WAVE) {
            const float e = expf(sp[j] - mx);
            sp[j] = e;
            sum += e;
        }
        const float rcp = 1.0f / wave_sum_f32(sum);
        float* prow = a.probs_out ? seq_probs_row(a, b, h, t0 + row) : nullptr;
        for (int j = lane; j < S; j += OSQ_WAVE) {
            const float p = dec_fq(sp[j] * rcp, a.probs, pq);
            sp[j] = p;
            if (prow) prow[j] = p;
        }
        if (lane == 0) sp[S] = 0.f;       // the partner of position S - 1 in the last step of an odd S (SP = SMAX + 1: in the row)
    }
    __syncthreads();

    // ---- context: wave w takes column chunk w % NCH and segment w / NCH of the steps
    {
        const int chunk = w % NCH, seg = w / NCH;
        const int nsteps = (S + 1) / 2, per = (nsteps + NSEG - 1) / NSEG;
        const int st0 = seg * per, st1 = min(nsteps, st0 + per);
        const int vcol = chunk * 32 + l31;
        const bool col_ok = vcol < D;                  // head_dim 16: half a chunk
        const float* vbase = a.v + b * a.v_sb + h * a.v_sh + (col_ok ? vcol : 0);
        const float* arow = s_p + l31 * SP;
        f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        // kBlkInFlight steps from st on: a word of V and a probability each; the next batch is issued before this one's products
        const auto load_v = [&](int st, float* vb, float* pa) {
#pragma unroll
            for (int u = 0; u < kBlkInFlight; ++u) {
                const int j = 2 * (st + u) + half;
                const bool ok = st + u < st1 && j < S;
                const float x = vbase[static_cast<int64_t>(ok ? j : S - 1) * a.v_st];
                vb[u] = ok && col_ok ? x : 0.f;
                pa[u] = arow[min(j, S)];               // position S holds +0
            }
        };
        float vb[kBlkInFlight], pa[kBlkInFlight], vn[kBlkInFlight], pn[kBlkInFlight];
        if (st0 < st1) load_v(st0, vb, pa);
        for (int st = st0; st < st1; st += kBlkInFlight) {
            if (st + kBlkInFlight < st1) load_v(st + kBlkInFlight, vn, pn);
#pragma unroll
            for (int u = 0; u < kBlkInFlight; ++u)
                if (st + u < st1) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[u], vb[u], acc, 0, 0, 0);     // wave-uniform
#pragma unroll
            for (int u = 0; u < kBlkInFlight; ++u) { vb[u] = vn[u]; pa[u] = pn[u]; }
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 16; ++r) s_part[w][mfma32_row(r, half)][l31] = acc[r];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nrows * D; i += kBlkThreads) {
        const int row = i / D, col = i % D;
        const int chunk = col / 32, cc = col % 32;
        float o = s_part[chunk][row][cc];
#pragma unroll
        for (int g = 1; g < NSEG; ++g) o = o + s_part[g * NCH + chunk][row][cc];
        seq_out_row<D>(a, b, h, t0 + row)[col] = dec_fq(o, a.ctx, cq);
    }
}

template <int D>
static void launch_block(const BlkArgs& a, dim3 grid, hipStream_t st) {
    if (a.kv_len <= 128) hipLaunchKernelGGL((attention_block_kernel<D, 128>), grid, dim3(kBlkThreads), 0, st, a);
    else if (a.kv_len <= 256) hipLaunchKernelGGL((attention_block_kernel<D, 256>), grid, dim3(kBlkThreads), 0, st, a);
    else if (a.kv_len <= 512) hipLaunchKernelGGL((attention_block_kernel<D, 512>), grid, dim3(kBlkThreads), 0, st, a);
    else hipLaunchKernelGGL((attention_block_kernel<D, kBlkMaxS>), grid, dim3(kBlkThreads), 0, st, a);
}

}  // namespace osq

using namespace osq;

// batch counts the rows of k / v; q, out and probs_out have batch * group
extern "C" int osq_attention_fake_quant_shared(const float* q, const float* k, const float* v, const float* mask, float* out,
                                        float* probs_out, int64_t batch, int64_t group, int64_t heads, int64_t tokens,
                                        int64_t kv_len, int64_t head_dim,
                                        int64_t q_stride_b, int64_t q_stride_h, int64_t q_stride_t,
                                        int64_t k_stride_b, int64_t k_stride_h, int64_t k_stride_t,
                                        int64_t v_stride_b, int64_t v_stride_h, int64_t v_stride_t,
                                        int64_t mask_stride_b, int64_t mask_stride_h, int64_t mask_stride_t,
                                        float alpha, float divisor,
                                        float* probs_scale, void* probs_zero_point, int probs_zp_type, int probs_mode,
                                        float probs_grad_factor, int probs_quant_min, int probs_quant_max,
                                        float* ctx_scale, void* ctx_zero_point, int ctx_zp_type, int ctx_mode,
                                        float ctx_grad_factor, int ctx_quant_min, int ctx_quant_max,
                                        osq_stream stream) {
    const char* what = "attention_fake_quant";
    BlkArgs a{{q, k, v, mask, out, probs_out, q_stride_b, q_stride_h, q_stride_t, k_stride_b, k_stride_h, k_stride_t,
               v_stride_b, v_stride_h, v_stride_t, mask_stride_b, mask_stride_h, mask_stride_t, heads, 0, 0, 0, 0, 0, 0, alpha,
               divisor},
              OSQ_DEC_QUANT(probs), OSQ_DEC_QUANT(ctx)};
    if (const int rc = seq_check_shape(what, a, batch, group, tokens, head_dim)) return rc;
    OSQ_SEQ_REQUIRE(!probs_scale || probs_zero_point, "probs scale without zero_point");
    OSQ_SEQ_REQUIRE(!ctx_scale || ctx_zero_point, "ctx scale without zero_point");
    OSQ_SEQ_REQUIRE(!probs_scale || dec_mode_ok(probs_mode), "bad probs mode");
    OSQ_SEQ_REQUIRE(!ctx_scale || dec_mode_ok(ctx_mode), "bad ctx mode");
    int64_t blocks;
    if (const int rc = seq_check_launch(what, a, batch, tokens, kv_len, head_dim, kBlkTQ, kBlkMaxS, &blocks); rc || !blocks) return rc;
    const dim3 grid(static_cast<unsigned>(blocks));
    hipStream_t st = static_cast<hipStream_t>(stream);
    OSQ_HEAD_DIM_DISPATCH(head_dim, launch_block<D>(a, grid, st));
    return check_launch(what);
}

extern "C" int osq_attention_fake_quant(const float* q, const float* k, const float* v, const float* mask, float* out,
                                        float* probs_out, int64_t batch, int64_t heads, int64_t tokens, int64_t kv_len,
                                        int64_t head_dim,
                                        int64_t q_stride_b, int64_t q_stride_h, int64_t q_stride_t,
                                        int64_t k_stride_b, int64_t k_stride_h, int64_t k_stride_t,
                                        int64_t v_stride_b, int64_t v_stride_h, int64_t v_stride_t,
                                        int64_t mask_stride_b, int64_t mask_stride_h, int64_t mask_stride_t,
                                        float alpha, float divisor,
                                        float* probs_scale, void* probs_zero_point, int probs_zp_type, int probs_mode,
                                        float probs_grad_factor, int probs_quant_min, int probs_quant_max,
                                        float* ctx_scale, void* ctx_zero_point, int ctx_zp_type, int ctx_mode,
                                        float ctx_grad_factor, int ctx_quant_min, int ctx_quant_max,
                                        osq_stream stream) {
    return osq_attention_fake_quant_shared(q, k, v, mask, out, probs_out, batch, 1, heads, tokens, kv_len, head_dim,
                                           q_stride_b, q_stride_h, q_stride_t, k_stride_b, k_stride_h, k_stride_t,
                                           v_stride_b, v_stride_h, v_stride_t, mask_stride_b, mask_stride_h, mask_stride_t,
                                           alpha, divisor, probs_scale, probs_zero_point, probs_zp_type, probs_mode,
                                           probs_grad_factor, probs_quant_min, probs_quant_max, ctx_scale, ctx_zero_point,
                                           ctx_zp_type, ctx_mode, ctx_grad_factor, ctx_quant_min, ctx_quant_max, stream);
}

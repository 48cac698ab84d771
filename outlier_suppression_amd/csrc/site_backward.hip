// Backward of the one-launch GELU and attention-probabilities sites (fake_quant.hip: fq_tensor_vec_kernel<.., GELU>;
// attention.hip), for the one stage that trains through them: learn_scale's Adam loop over the LSQ / LSQ+ parameters.
//
// Eager autograd runs, per site and step, the quantizer's backward (one pass: osq_lsq_backward_per_tensor) and then torch's
// backward of what stands in front of it, over tensors the forward had to keep:
//     GELU site [B, T, 4H]       forward  gelu (r x, w g) + fake-quant (r g, w y)             16 B, g kept besides x
//                                backward LSQ (r g, r gy, w dg) + GELU (r x, r dg, w dx)      24 B       = 40 B per element
//     probabilities [B, h, T, S] forward  scale / mask (r s, w v) + softmax (r v, w p) + fake-quant (r p, w y)   24 B, p kept
//                                backward LSQ (r p, r gy, w dp) + softmax (r p, r dp, w dv) + scaling (r dv, w ds)   32 B
// Here the forward is the site's one launch (8 B) and keeps only its INPUT; the backward is one launch that recomputes the
// quantizer's input in registers -- the same device functions, hence the words the forward quantised -- and reads x, gy,
// writes dx: 12 B.  20 B per element for the pair.
//
// The parameter gradients are the sums of lsq_backward.h's bwd_elem terms, reduced by lsq_bwd_finish: fp32 per lane over a
// short run, float64 from there, workgroup partials combined in block order by the workgroup that arrives last.  No atomics
// on floating-point data: the same inputs give the same words on every run.  Both kernels own workspace family
// kFamSiteBackward: a site's backward may overlap a plain quantizer's backward (kFamLsqBackward) of another graph branch.
#include <hip/hip_ext.h>
#include "lsq_backward.h"
#include "attention_row.h"

namespace osq {

// ---------------------------------------------------------------- GELU site

// lsq_bwd_tensor_kernel<GeluProducer> (lsq_backward.h): g = gelu_erf(x) made per element, dg and the sum terms are
// bwd_elem(g, gy, ..), dx = dg * (Phi(x) + x phi(x)).  On the grid osq_lsq_backward_per_tensor takes for n, dscale / dzp are
// word-equal to that call on F.gelu(x): the same terms meet in the same order.

// ---------------------------------------------------------------- attention-probabilities site

struct AttnBwdArgs {
    AttnArgs f;               // the forward's record: scores, mask, geometry, alpha / divisor (y and quant unused)
    const float* gy;          // [rows, cols], the gradient of the fake-quantised probabilities
    float* dscores;           // [rows, cols]
    const float* scale;       // the probabilities quantizer, read only: the parameter repair is the forward's
    const void* zero_point;
    int zp_type, mode;
    float grad_factor, qmin, qmax;
    float* dscale;            // nullable
    float* dzp;               // nullable
    double* partials;
    unsigned int* counter;
    int wt;                   // dscores through write-through stores (rows * cols / 4 < 2^28)
};

// One wave per row, the row in registers as in the forward: R float4 of scores (then e, then p), of the mask and of gy (then
// dp) per lane; the next row's scores / mask / gy are on their way before this row's first reduction.  Three wave reductions
// per row: the forward's max and sum in fp32, and dot = sum_j dp_j p_j in float64 (exact products), rounded to fp32 once.
//     p_j  = e_j * r                               softmax_row: the forward's words
//     dp_j = bwd_elem(p_j, gy_j, ..)               and its three sum terms, fp32 per lane over the row
//     dscores_j = pre' * (p_j * (dp_j - dot))      pre' = alpha | 1 / divisor (one fp32 division per launch) | nothing
// The mask is an additive constant: no gradient.  A key masked with -inf has p = 0 and so dscores = 0.
template <int R, int PRE, bool MASK>
__global__ __launch_bounds__(kAttnThreads) void attention_softmax_fq_bwd_kernel(AttnBwdArgs a) {
    static_assert(kAttnThreads == kBwdThreads, "lsq_bwd_finish: one workgroup size");
    const int lane = threadIdx.x & (OSQ_WAVE - 1);
    const int64_t wave0 = (static_cast<int64_t>(blockIdx.x) * kAttnThreads + threadIdx.x) / OSQ_WAVE;
    const int64_t nwaves = static_cast<int64_t>(gridDim.x) * kAttnWaves;
    const int cols4 = a.f.cols >> 2;
    const QParams q = effective_params(a.scale[0], load_zp(a.zero_point, a.zp_type), a.mode, a.grad_factor);
    const float s = q.scale, z = q.zp;
    const float pd = PRE == kPreDivide ? 1.0f / a.f.divisor : a.f.alpha;
    float4* d4 = reinterpret_cast<float4*>(a.dscores);
    const WtStore dwt(d4, a.wt ? a.f.rows * cols4 : 0);
    double t_ds = 0.0, t_dz = 0.0;
    float4 v[R], m[R], g[R];
    if (wave0 < a.f.rows) {
        load_attn_row<R, MASK>(a.f, wave0, lane, cols4, v, m);
        load_row<R>(a.gy, wave0, lane, cols4, g);
    }
    for (int64_t row = wave0; row < a.f.rows; row += nwaves) {
        float4 vn[R], mn[R], gn[R];
        if (row + nwaves < a.f.rows) {
            load_attn_row<R, MASK>(a.f, row + nwaves, lane, cols4, vn, mn);
            load_row<R>(a.gy, row + nwaves, lane, cols4, gn);
        }
        const float r = softmax_row<R, PRE, MASK>(a.f, lane, cols4, v, m);
        BwdAcc acc = {0.f, 0.f, 0.f};
        double dot64 = 0.0;        // the products are exact in float64: dot is the row's sum rounded once
#pragma unroll
        for (int k = 0; k < R; ++k) {
            if (lane + k * OSQ_WAVE < cols4) {         // the float4s repeated beyond the row's end join no sum
                const float4 p = make_float4(v[k].x * r, v[k].y * r, v[k].z * r, v[k].w * r);
                const float4 dp = bwd_elem4(PlainProducer(), p, g[k], s, z, a.qmin, a.qmax, acc);
                dot64 += (static_cast<double>(dp.x) * p.x + static_cast<double>(dp.y) * p.y) +
                         (static_cast<double>(dp.z) * p.z + static_cast<double>(dp.w) * p.w);
                v[k] = p;
                g[k] = dp;
            }
        }
        const float dot = static_cast<float>(wave_sum(dot64));
        const int64_t base = row * cols4;
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const int c = lane + k * OSQ_WAVE;
            if (c < cols4) {
                float4 o = make_float4(v[k].x * (g[k].x - dot), v[k].y * (g[k].y - dot), v[k].z * (g[k].z - dot),
                                       v[k].w * (g[k].w - dot));
                if (PRE != kPrePlain) o = make_float4(pd * o.x, pd * o.y, pd * o.z, pd * o.w);
                if (a.wt) dwt.put(base + c, o); else store_stream(d4 + base + c, o);
            }
        }
        t_ds += static_cast<double>(acc.ds_mul) + static_cast<double>(acc.ds_div);
        t_dz += static_cast<double>(acc.dz);
#pragma unroll
        for (int k = 0; k < R; ++k) {
            v[k] = vn[k];
            g[k] = gn[k];
            if (MASK) m[k] = mn[k];
        }
    }
    lsq_bwd_finish(t_ds, t_dz, a.mode, a.grad_factor, a.dscale, a.dzp, a.partials, a.counter);
}

static bool bwd_mode_ok(int mode) { return mode >= OSQ_PARAM_FIXED && mode <= OSQ_PARAM_LSQPLUS; }

}  // namespace osq

using namespace osq;

extern "C" int osq_gelu_fake_quant_backward(const float* x, const float* grad_out, float* grad_x, int64_t n,
                                            const float* scale, const void* zero_point, int zp_type,
                                            int mode, float grad_factor, int quant_min, int quant_max,
                                            float* grad_scale, float* grad_zero_point,
                                            void* workspace, osq_stream stream) {
    OSQ_REQUIRE(n >= 0 && scale && zero_point && workspace, "gelu_fake_quant_backward: null pointer or n < 0");
    OSQ_REQUIRE(n == 0 || (x && grad_out && grad_x), "gelu_fake_quant_backward: null tensor");
    OSQ_REQUIRE(bwd_mode_ok(mode), "gelu_fake_quant_backward: bad mode (the parameter repair is forward-only)");
    OSQ_REQUIRE(zp_type == OSQ_ZP_INT32 || zp_type == OSQ_ZP_FLOAT32, "gelu_fake_quant_backward: bad zp_type");
    if (!aligned16(x) || !aligned16(grad_out) || !aligned16(grad_x)) {
        osq::set_error("gelu_fake_quant_backward: needs 16-byte aligned tensors");
        return OSQ_ERR_UNSUPPORTED;
    }
    const int64_t n4 = n / 4;
    const int tail = static_cast<int>(n - n4 * 4);
    const int grid = lsq_backward_grid(n4);          // the plain backward's grid for n: the sums meet in its order
    Workspace ws(workspace);
    hipLaunchKernelGGL(lsq_bwd_tensor_kernel<GeluProducer>, dim3(grid), dim3(kBwdThreads), 0, static_cast<hipStream_t>(stream),
                       reinterpret_cast<const float4*>(x), reinterpret_cast<const float4*>(grad_out),
                       reinterpret_cast<float4*>(grad_x), n4, x + n4 * 4, grad_out + n4 * 4, grad_x + n4 * 4, tail, scale,
                       zero_point, zp_type, mode, grad_factor, static_cast<float>(quant_min), static_cast<float>(quant_max),
                       grad_scale, grad_zero_point, ws.doubles(kFamSiteBackward), ws.counter(kFamSiteBackward),
                       (stream_write_through() && n4 <= kWtMaxFloat4) ? 1 : 0);
    return check_launch("gelu_fake_quant_backward");
}

extern "C" int osq_attention_softmax_fake_quant_backward(const float* scores, const float* mask, int64_t batch, int64_t heads,
                                                         int64_t tokens, int64_t cols, int64_t mask_stride_b,
                                                         int64_t mask_stride_h, int64_t mask_stride_t, float alpha,
                                                         float divisor, const float* grad_out, float* grad_scores,
                                                         const float* scale, const void* zero_point, int zp_type,
                                                         int mode, float grad_factor, int quant_min, int quant_max,
                                                         float* grad_scale, float* grad_zero_point,
                                                         void* workspace, osq_stream stream) {
    OSQ_REQUIRE(batch >= 0 && heads >= 0 && tokens >= 0 && cols > 0 && cols <= INT32_MAX,
                "attention_softmax_fake_quant_backward: bad shape");
    OSQ_REQUIRE(scale && zero_point && workspace, "attention_softmax_fake_quant_backward: null parameter or workspace");
    OSQ_REQUIRE(bwd_mode_ok(mode), "attention_softmax_fake_quant_backward: bad mode (the parameter repair is forward-only)");
    OSQ_REQUIRE(zp_type == OSQ_ZP_INT32 || zp_type == OSQ_ZP_FLOAT32, "attention_softmax_fake_quant_backward: bad zp_type");
    OSQ_REQUIRE(!mask || (mask_stride_b >= 0 && mask_stride_h >= 0 && mask_stride_t >= 0),
                "attention_softmax_fake_quant_backward: negative mask stride");
    OSQ_REQUIRE(alpha == 1.0f || divisor == 1.0f, "attention_softmax_fake_quant_backward: give alpha or divisor, not both");
    const int64_t rows = batch * heads * tokens;
    OSQ_REQUIRE(rows == 0 || (scores && grad_out && grad_scores), "attention_softmax_fake_quant_backward: null tensor");
    // the geometry of the forward's register-resident kernel; anything else keeps the eager chain
    if (!attn_row_geometry(scores, mask, cols, mask_stride_b, mask_stride_h, mask_stride_t) || !aligned16(grad_out) ||
        !aligned16(grad_scores)) {
        osq::set_error("attention_softmax_fake_quant_backward: needs cols %% 4 == 0, cols <= 2048 and 16-byte aligned rows");
        return OSQ_ERR_UNSUPPORTED;
    }
    Workspace ws(workspace);
    AttnBwdArgs a{};
    a.f = AttnArgs{scores, nullptr, mask, mask_stride_b, mask_stride_h, mask_stride_t, heads, tokens, rows,
                   static_cast<int>(cols), alpha, divisor, DecQuant{}};
    a.gy = grad_out;
    a.dscores = grad_scores;
    a.scale = scale;
    a.zero_point = zero_point;
    a.zp_type = zp_type;
    a.mode = mode;
    a.grad_factor = grad_factor;
    a.qmin = static_cast<float>(quant_min);
    a.qmax = static_cast<float>(quant_max);
    a.dscale = grad_scale;
    a.dzp = grad_zero_point;
    a.partials = ws.doubles(kFamSiteBackward);
    a.counter = ws.counter(kFamSiteBackward);
    a.wt = rows * (cols / 4) <= kWtMaxFloat4 ? 1 : 0;
    // an empty tensor still launches one workgroup: the sums over no rows are zeros, written like any other
    const dim3 grid(static_cast<unsigned>(grid_for(rows, kAttnWaves, kMaxBlocks)));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int pre = pre_of(alpha, divisor);
    const int per_lane = static_cast<int>((cols / 4 + OSQ_WAVE - 1) / OSQ_WAVE);
#define OSQ_ATTN_B(R, PRE, MASK) \
    hipLaunchKernelGGL((attention_softmax_fq_bwd_kernel<R, PRE, MASK>), grid, dim3(kAttnThreads), 0, st, a)
#define OSQ_ATTN_BM(R, PRE) do { if (mask) OSQ_ATTN_B(R, PRE, true); else OSQ_ATTN_B(R, PRE, false); } while (0)
#define OSQ_ATTN_BR(PRE)                                 \
    do {                                                 \
        if (per_lane <= 1) OSQ_ATTN_BM(1, PRE);          \
        else if (per_lane <= 2) OSQ_ATTN_BM(2, PRE);     \
        else if (per_lane <= 4) OSQ_ATTN_BM(4, PRE);     \
        else OSQ_ATTN_BM(8, PRE);                        \
    } while (0)
    if (pre == kPreDivide) OSQ_ATTN_BR(kPreDivide);
    else if (pre == kPreScale) OSQ_ATTN_BR(kPreScale);
    else OSQ_ATTN_BR(kPrePlain);
#undef OSQ_ATTN_BR
#undef OSQ_ATTN_BM
#undef OSQ_ATTN_B
    return check_launch("attention_softmax_fake_quant_backward");
}

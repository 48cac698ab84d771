// Backward of the one-launch residual + LayerNorm + fake-quant site (layernorm.hip), for the one stage that trains through
// it: learn_scale's Adam loop over the LSQ / LSQ+ parameters, with every other parameter frozen.
//
// Eager autograd runs, per site and step, over [B, T, H] tensors:
//     forward   GammaResidual (r x, r hidden, w r) + LayerNorm (r r, w n) [+ bias (r n, w n)] + fake-quant (r n, w y)   28-36 B
//     backward  LSQ (r n, r gy, w dn) + LayerNorm (r r, r dn, w dr) + residual (r dr, w dx)                             28-32 B
// with r and n kept between the two.  Here the forward is the site's one launch (12 B with a residual) and keeps only its
// INPUTS; the backward is one launch that recomputes r, the moments and the quantizer's input in registers -- layernorm_row.h,
// the device code of the forward, hence the words it quantised -- reads x, hidden, gy and writes dx, dhidden: 20 B, 16 B when
// gamma is absent (dx and dhidden are then the same words, stored once).  28-32 B per element for the pair.
//
// The parameter gradients are the sums of lsq_backward.h's bwd_elem terms, reduced by lsq_bwd_finish as in site_backward.hip:
// fp32 per lane over a row, float64 per lane across rows, workgroup partials combined in block order by the workgroup that
// arrives last.  No atomics on floating-point data: the same inputs give the same words on every run.  Workspace family
// kFamSiteBackward.  No gradients for gamma / weight / bias: the callers keep the eager lines when one of them learns.
#include <hip/hip_ext.h>
#include "lsq_backward.h"
#include "layernorm_row.h"

namespace osq {

constexpr int kLnBwdMaxCols = 4 * 8 * OSQ_WAVE;     // 2048: eight float4 per lane
constexpr int kLnBwdBlocks = 1024;                  // grid cap, the forward's (g_ln_blocks); rows are grid-strided above it

struct LnBwdArgs {
    LnArgs f;                 // the forward's record: x, hidden, gamma, weight, bias, geometry, eps (y and the quantizer unused)
    const float4* gy;         // [rows, cols], the gradient of the fake-quantised output
    float4* dx;               // nullable: dr * gamma, or dr
    float4* dh;               // nullable: dr (only with hidden)
    const float* scale;       // the site's quantizer, read only: the parameter repair is the forward's; nullable: no fake-quant
    const void* zero_point;
    int zp_type, mode;
    float grad_factor, qmin, qmax;
    double inv_cols, eps;     // 1 / cols and eps in float64, for the gradient's own statistics
    float* dscale;            // nullable
    float* dzp;               // nullable
    double* partials;
    unsigned int* counter;
    int wt;                   // dx / dh through write-through stores (rows * cols / 4 < 2^28)
};

template <int R>
__device__ __forceinline__ void ln_load_gy(const LnBwdArgs& a, int64_t row, int lane, float4* g) {
    const float4* gr = a.gy + row * a.f.cols4;
#pragma unroll
    for (int k = 0; k < R; ++k) {
        const int c = lane + k * OSQ_WAVE, cc = c < a.f.cols4 ? c : a.f.cols4 - 1;
        g[k] = load_stream(gr + cc);
    }
}

// One wave per row, the row in registers as in the forward.  HID: the site has a residual (hidden; gamma rides on it).
//     r, mean, rstd                    ln_row_moments: the forward's words, two fp32 wave reductions
//     n_j = ((r_j - mean) * rstd) * w_j + b_j                           ln_xhat / ln_affine: the words the forward quantised
//     dn_j = bwd_elem(n_j, gy_j, ..)                                    and its three sum terms, fp32 per lane over the row
//     dxhat_j = dn_j * w_j                                              fp32
// The LayerNorm backward itself runs on float64 statistics of the fp32 row r, all from ONE more wave round of four values --
// with dev_j = r_j - mean (exact in float64):
//     C1 = sum dxhat_j ;  P = sum dxhat_j dev_j ;  S1 = sum dev_j ;  S2 = sum dev_j^2
//     delta = S1 / cols  (what the fp32 mean missed) ;  rstd' = 1 / sqrt(S2 / cols - delta^2 + eps)
//     xhat'_j = (dev_j - delta) * rstd' ;  c1 = C1 ;  c2 = sum dxhat_j xhat'_j = rstd' (P - delta C1)
//     dr_j = rstd' ((dxhat_j - c1 / cols) - xhat'_j (c2 / cols))        float64, rounded to fp32 once
//     dhidden_j = dr_j ;  dx_j = dr_j * gamma_j (HID with gamma), else dr_j
// fp32 xhat with float64 c1 / c2 does not meet the tests' bar at 4 columns (7.3e-7 against 5.4e-7: the fp32 mean and rstd carry
// roundings of their own, as torch's do, and twice the eager chain's error is no margin between two such sets over 4 elements);
// the quantizer still sees the forward's fp32 words, which decide what is clipped.
// Registers: once r is formed hidden is dead, so two operands stay live per element -- v (x, then r) and y (gy, then dxhat):
// 2 R float4 per lane -- besides the next row's x / hidden / gy, which leave before this row's first reduction, and the kept
// per-column operands (R <= 4).
template <int R, bool HID>
__global__ __launch_bounds__(kLnThreads) void residual_layernorm_fq_bwd_kernel(LnBwdArgs a) {
    static_assert(kLnThreads == kBwdThreads, "lsq_bwd_finish: one workgroup size");
    const int lane = threadIdx.x & (OSQ_WAVE - 1);
    const int64_t wave0 = (static_cast<int64_t>(blockIdx.x) * kLnThreads + threadIdx.x) / OSQ_WAVE;
    const int64_t nwaves = static_cast<int64_t>(gridDim.x) * kLnWaves;
    const int cols4 = a.f.cols4;
    const bool fq = a.scale != nullptr;          // a site without an output quantizer: dn = gy, no parameter sums
    const QParams q = fq ? effective_params(a.scale[0], load_zp(a.zero_point, a.zp_type), a.mode, a.grad_factor) : QParams{1.f, 0.f};
    const float s = q.scale, z = q.zp;
    const bool by_gamma = HID && a.f.gamma;
    const bool want_dr = a.dx || a.dh;           // neither tensor gradient wanted: the parameter sums alone, no third reduction
    const int64_t n4 = a.wt ? a.f.rows * cols4 : 0;
    const WtStore xwt(a.dx, a.dx ? n4 : 0), hwt(a.dh, a.dh ? n4 : 0);
    constexpr int RK = LnKeep<R>::regs;
    float4 g[RK], w[RK], b[RK];
    ln_load_cols<R>(a.f, lane, g, w, b);
    double t_ds = 0.0, t_dz = 0.0;
    float4 v[R], h[HID ? R : 1], y[R];
    if (wave0 < a.f.rows) {
        ln_load_row<R>(a.f, HID, wave0, lane, v, h);
        ln_load_gy<R>(a, wave0, lane, y);
    }
    for (int64_t row = wave0; row < a.f.rows; row += nwaves) {
        float4 vn[R], hn[HID ? R : 1], yn[R];
        if (row + nwaves < a.f.rows) {
            ln_load_row<R>(a.f, HID, row + nwaves, lane, vn, hn);
            ln_load_gy<R>(a, row + nwaves, lane, yn);
        }
        float mean, rstd;
        ln_row_moments<R>(a.f, HID, lane, v, h, g, mean, rstd);
        BwdAcc acc = {0.f, 0.f, 0.f};
        const double mean64 = static_cast<double>(mean);
        double c1 = 0.0, pd = 0.0, s1 = 0.0, s2 = 0.0;
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const int c = lane + k * OSQ_WAVE;
            if (c < cols4) {                      // the float4s repeated beyond the row's end join no sum
                const float4 wk = ln_row_weight<R>(a.f, w, k, c);
                const float4 bk = ln_row_bias<R>(a.f, b, k, c);
                const float ww[4] = {wk.x, wk.y, wk.z, wk.w}, bb[4] = {bk.x, bk.y, bk.z, bk.w};
                const float t[4] = {v[k].x, v[k].y, v[k].z, v[k].w};
                float d[4] = {y[k].x, y[k].y, y[k].z, y[k].w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (fq) d[e] = bwd_elem(ln_affine(a.f, ln_xhat(t[e], mean, rstd), ww[e], bb[e]), d[e], s, z, a.qmin, a.qmax, acc);
                    if (a.f.weight) d[e] = d[e] * ww[e];
                    const double dev = static_cast<double>(t[e]) - mean64;       // exact
                    c1 += static_cast<double>(d[e]);
                    pd += static_cast<double>(d[e]) * dev;
                    s1 += dev;
                    s2 += dev * dev;
                }
                y[k] = make_float4(d[0], d[1], d[2], d[3]);
            }
        }
        if (want_dr) {
            // ONE round, four float64 values; from them the row's moments and both projections of the LayerNorm backward
            c1 = wave_sum(c1);
            pd = wave_sum(pd);
            s1 = wave_sum(s1);
            s2 = wave_sum(s2);
            const double delta = s1 * a.inv_cols;                                  // the true mean of r less the forward's fp32 mean
            const double rstd64 = 1.0 / sqrt((s2 * a.inv_cols - delta * delta) + a.eps);
            const double m1 = c1 * a.inv_cols;                                     // c1 / cols
            const double m2 = rstd64 * (pd - delta * c1) * a.inv_cols;             // c2 / cols, c2 = sum_j dxhat_j xhat_j
            const double shift = mean64 + delta;
            const int64_t base = row * cols4;
#pragma unroll
            for (int k = 0; k < R; ++k) {
                const int c = lane + k * OSQ_WAVE;
                if (c < cols4) {
                    const float t[4] = {v[k].x, v[k].y, v[k].z, v[k].w}, d[4] = {y[k].x, y[k].y, y[k].z, y[k].w};
                    float o[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const double xh = (static_cast<double>(t[e]) - shift) * rstd64;
                        o[e] = static_cast<float>(rstd64 * ((static_cast<double>(d[e]) - m1) - xh * m2));
                    }
                    const float4 dr = make_float4(o[0], o[1], o[2], o[3]);
                    if (a.dh) {
                        if (a.wt) hwt.put(base + c, dr); else store_stream(a.dh + base + c, dr);
                    }
                    if (a.dx) {
                        float4 ox = dr;
                        if (by_gamma) {
                            const float4 gk = LnKeep<R>::keep ? g[LnKeep<R>::keep ? k : 0] : a.f.gamma[c];
                            ox = make_float4(dr.x * gk.x, dr.y * gk.y, dr.z * gk.z, dr.w * gk.w);
                        }
                        if (a.wt) xwt.put(base + c, ox); else store_stream(a.dx + base + c, ox);
                    }
                }
            }
        }
        t_ds += static_cast<double>(acc.ds_mul) + static_cast<double>(acc.ds_div);
        t_dz += static_cast<double>(acc.dz);
#pragma unroll
        for (int k = 0; k < R; ++k) {
            v[k] = vn[k];
            y[k] = yn[k];
            if (HID) h[k] = hn[k];
        }
    }
    lsq_bwd_finish(t_ds, t_dz, a.mode, a.grad_factor, a.dscale, a.dzp, a.partials, a.counter);
}

}  // namespace osq

using namespace osq;

extern "C" int osq_residual_layernorm_fake_quant_backward(const float* x, const float* hidden, const float* gamma,
                                                          const float* weight, const float* bias, double eps,
                                                          int64_t rows, int64_t cols, const float* grad_out,
                                                          float* grad_x, float* grad_hidden,
                                                          const float* scale, const void* zero_point, int zp_type,
                                                          int mode, float grad_factor, int quant_min, int quant_max,
                                                          float* grad_scale, float* grad_zero_point,
                                                          void* workspace, osq_stream stream) {
    OSQ_REQUIRE(rows >= 0 && cols > 0, "residual_layernorm_fake_quant_backward: bad shape");
    OSQ_REQUIRE(workspace && (scale ? zero_point != nullptr : (!zero_point && !grad_scale && !grad_zero_point)),
                "residual_layernorm_fake_quant_backward: null workspace, or scale and zero_point not given together");
    OSQ_REQUIRE(mode >= OSQ_PARAM_FIXED && mode <= OSQ_PARAM_LSQPLUS,
                "residual_layernorm_fake_quant_backward: bad mode (the parameter repair is forward-only)");
    OSQ_REQUIRE(zp_type == OSQ_ZP_INT32 || zp_type == OSQ_ZP_FLOAT32, "residual_layernorm_fake_quant_backward: bad zp_type");
    OSQ_REQUIRE(rows == 0 || (x && grad_out), "residual_layernorm_fake_quant_backward: null tensor");
    OSQ_REQUIRE(hidden || !grad_hidden, "residual_layernorm_fake_quant_backward: grad_hidden without hidden");
    OSQ_REQUIRE(!(hidden && gamma) || !grad_x || grad_x != grad_hidden,
                "residual_layernorm_fake_quant_backward: with gamma, grad_x and grad_hidden are different words");
    // the geometry of the register-resident kernel; anything else keeps the eager lines
    if (cols % 4 != 0 || cols > kLnBwdMaxCols || !aligned16(x) || !aligned16(grad_out) || !aligned16(grad_x) ||
        !aligned16(grad_hidden) || !aligned16(hidden) || !aligned16(gamma) || !aligned16(weight) || !aligned16(bias)) {
        osq::set_error("residual_layernorm_fake_quant_backward: needs cols %% 4 == 0, cols <= 2048 and 16-byte aligned operands");
        return OSQ_ERR_UNSUPPORTED;
    }
    if (!(hidden && gamma) && grad_hidden == grad_x) grad_hidden = nullptr;     // the same words: stored once
    Workspace ws(workspace);
    LnBwdArgs a{};
    a.f = LnArgs{reinterpret_cast<const float4*>(x), reinterpret_cast<const float4*>(hidden),
                 reinterpret_cast<const float4*>(gamma), reinterpret_cast<const float4*>(weight),
                 reinterpret_cast<const float4*>(bias), nullptr, rows, static_cast<int>(cols / 4),
                 static_cast<float>(1.0 / static_cast<double>(cols)), static_cast<float>(eps), nullptr, nullptr, zp_type, mode,
                 grad_factor, static_cast<float>(quant_min), static_cast<float>(quant_max)};
    a.gy = reinterpret_cast<const float4*>(grad_out);
    a.dx = reinterpret_cast<float4*>(grad_x);
    a.dh = reinterpret_cast<float4*>(grad_hidden);
    a.scale = scale;
    a.zero_point = zero_point;
    a.zp_type = zp_type;
    a.mode = mode;
    a.grad_factor = grad_factor;
    a.qmin = static_cast<float>(quant_min);
    a.qmax = static_cast<float>(quant_max);
    a.inv_cols = 1.0 / static_cast<double>(cols);
    a.eps = eps;
    a.dscale = grad_scale;
    a.dzp = grad_zero_point;
    a.partials = ws.doubles(kFamSiteBackward);
    a.counter = ws.counter(kFamSiteBackward);
    a.wt = (stream_write_through() && rows * (cols / 4) <= kWtMaxFloat4) ? 1 : 0;
    // an empty tensor still launches one workgroup: the sums over no rows are zeros, written like any other
    const dim3 grid(static_cast<unsigned>(grid_for(rows, kLnWaves, kLnBwdBlocks)));
    static_assert(kLnBwdBlocks <= kMaxBlocks, "lsq_bwd_finish: gridDim.x <= kMaxBlocks");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int per_lane = (a.f.cols4 + OSQ_WAVE - 1) / OSQ_WAVE;
#define OSQ_LNB(R) \
    do { \
        if (hidden) hipLaunchKernelGGL((residual_layernorm_fq_bwd_kernel<R, true>), grid, dim3(kLnThreads), 0, st, a); \
        else hipLaunchKernelGGL((residual_layernorm_fq_bwd_kernel<R, false>), grid, dim3(kLnThreads), 0, st, a); \
    } while (0)
    if (per_lane <= 1) OSQ_LNB(1);
    else if (per_lane <= 2) OSQ_LNB(2);
    else if (per_lane <= 3) OSQ_LNB(3);
    else if (per_lane <= 4) OSQ_LNB(4);
    else OSQ_LNB(8);
#undef OSQ_LNB
    return check_launch("residual_layernorm_fake_quant_backward");
}

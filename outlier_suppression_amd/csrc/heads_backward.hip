// Backward of the head-split sites of an attention block -- the query / key / value sites (fake_quant.hip:
// fq_headsplit_multi_kernel) and the context site (the strided fake-quant on the permuted context) -- for the one stage that
// trains through them: learn_scale's Adam loop over the LSQ / LSQ+ parameters.
//
// Each of these sites is a per-tensor fake-quant BETWEEN two layouts of one tensor: [B, T, h*d] (token-major: what a Linear
// writes and reads) and [B, h, T, d] (head-major: what the batched matmuls read and write).  Eager autograd keeps the two
// apart: the quantizer's backward runs on one layout (after making the saved view contiguous and copying the gradient into
// that layout) and a separate copy carries dx into the other, about four passes over the tensor.  Here one launch reads x in
// the layout the forward read it in, reads dy in the layout the forward wrote, and writes dx where x lives: 12 B per element.
//
//     split  (q / k / v)   x, dx token-major      dy head-major, or the TRANSPOSED head-major form below
//     merge  (context)     x, dx head-major       dy token-major
//
// One body serves both (template parameter MERGE): it walks the TOKEN-MAJOR float4 index e, maps it to the head-major index
// with fq_headsplit_multi_kernel's two multiply-shift divisions (osq_device.h: head_major_index), and takes x / dx at one of
// the two and dy at the other.  A wave's access is then 1 KiB of consecutive bytes on the token-major side and 64 / (d / 4)
// runs of d floats -- whole rows, one per head -- on the other; sixteen tokens of a workgroup's trip land 16 d floats in a row
// in each head's plane.  Two float4 of x and of dy in flight per lane and trip, as in the dense backward.
//
// Transposed dy (split only).  The key is used as k^T: torch.matmul's backward hands back a dense [B, h, d, T] tensor, seen
// as [B, h, T, d] through strides (h*d*T, d*T, 1, T).  Read along d it would be 4-byte accesses T floats apart.  A site
// flagged `transposed` is walked in tiles instead: a workgroup takes (b, head, chunk of up to 64 floats of d, 64 tokens),
// loads the [d-chunk][64 tokens] tile with one wave per d row -- 256 consecutive bytes per wave-load, scalar loads, so T needs
// no alignment and the last tile of a row is simply short -- stores it to LDS row by row, and after one barrier every lane
// reads its float4 ALONG d (four LDS words one pitch apart) next to the float4 of x it already has in registers.  Lanes are
// assigned d-fastest, so the x / dx accesses stay runs of whole d-float rows.  The LDS pitch is 64 + 16 / (d-chunk / 4) words:
// a wave's read (d / 4 quads x 64 / (d / 4) tokens) then touches 64 different banks (pitch 65 at d >= 64: bank = 4 q + t + j),
// and the row-wise stores are conflict-free at any pitch.  64 tokens = one wave per tile row: the widest coalesced load a wave
// can make, and with a 64-float chunk the tile is 16.25 KiB -- seven workgroups of a CU hold theirs together.  The x loads are
// issued before the barrier, so they travel with the tile's.
//
// The parameter gradients are the sums of lsq_backward.h's bwd_elem terms, ended by lsq_bwd_finish per SITE: blockIdx.y = site
// (1..4 sites of one geometry, a table as in fq_headsplit_multi_kernel), each site with its own partials and ticket counters
// in the workspace (osq_host.h: Workspace::heads_*), so the four reductions of a launch never meet.  fp32 per lane over a
// trip, float64 from there, workgroup partials combined in block order by the workgroup that arrives last: no atomics on
// floating-point data, the same words on every run.  dx is a per-element function of (x, dy): word-equal to
// osq_lsq_backward_per_tensor on the same elements in any layout.
#include <hip/hip_ext.h>
#include "lsq_backward.h"

namespace osq {

constexpr int kHeadsTokTile = OSQ_HEADS_TOKEN_TILE;     // tokens of a transposed tile: one wave per tile row
constexpr int kHeadsChunkQuads = 16;                    // float4s of d per tile at most (64 floats)
constexpr int kHeadsTileWords = kHeadsChunkQuads * 4 * (kHeadsTokTile + 1);    // 4 dvc * (64 + 16 / dvc) <= this for dvc <= 16
constexpr int kHeadsBwdBlocks = 1792;                   // workgroups of a launch over all its sites: the dense backward's cap (7 per CU)
static_assert(kHeadsTokTile == OSQ_WAVE, "a wave loads one row of the tile");
static_assert(kBwdThreads * 4 == kHeadsChunkQuads * kHeadsTokTile, "four float4 of x per lane and tile");

struct HeadsBwdSites {
    const float4* x[kWsHeadsSites];
    const float* gy[kWsHeadsSites];
    float4* dx[kWsHeadsSites];              // nullable: the sums are still formed
    const float* scale[kWsHeadsSites];
    const void* zp[kWsHeadsSites];
    float* dscale[kWsHeadsSites];           // nullable
    float* dzp[kWsHeadsSites];              // nullable
    double* partials[kWsHeadsSites];
    unsigned int* counter[kWsHeadsSites];
    int zp_type[kWsHeadsSites], mode[kWsHeadsSites], transposed[kWsHeadsSites];
    float g[kWsHeadsSites], qmin[kWsHeadsSites], qmax[kWsHeadsSites];
};

__device__ __forceinline__ float load_stream_f32(const float* p) { return __builtin_nontemporal_load(p); }

template <bool MERGE>
__global__ __launch_bounds__(kBwdThreads) void heads_bwd_kernel(HeadsBwdSites s, HeadSplit d, unsigned int batch,
                                                                unsigned int n4, int wt) {
    __shared__ float tile[kHeadsTileWords];
    const int site = blockIdx.y;
    const float4* __restrict__ x = s.x[site];
    const float* __restrict__ gy = s.gy[site];
    float4* __restrict__ dx = s.dx[site];
    const float qmin = s.qmin[site], qmax = s.qmax[site];
    const int mode = s.mode[site];
    const float g = s.g[site];
    const QParams p = effective_params(s.scale[site][0], load_zp(s.zp[site], s.zp_type[site]), mode, g);
    const float sc = p.scale, z = p.zp;
    const PlainProducer f;
    const WtStore dwt(dx, wt ? n4 : 0);                      // wt: dx leaves through write-through stores (n4 < 2^28)
    auto put = [&](unsigned int i, const float4& o) {
        if (!dx) return;
        if (wt) dwt.put(i, o); else store_stream(&dx[i], o);
    };
    double t_ds = 0.0, t_dz = 0.0;
    if (!MERGE && s.transposed[site]) {                      // workgroup-uniform
        const unsigned int dv = 1u << d.dv_shift, dvc = dv < kHeadsChunkQuads ? dv : kHeadsChunkQuads;
        const unsigned int dvc_shift = d.dv_shift < 4u ? d.dv_shift : 4u;
        const unsigned int chunks = dv >> dvc_shift, dc = 4u * dvc, pitch = kHeadsTokTile + kHeadsChunkQuads / dvc;
        const unsigned int ttiles = (d.T + kHeadsTokTile - 1) / kHeadsTokTile;
        const unsigned int n_tiles = batch * d.h * chunks * ttiles;          // <= n4 / 4 + batch * h * chunks < 2^31
        const unsigned int row0 = threadIdx.x / OSQ_WAVE, tl_load = threadIdx.x & (OSQ_WAVE - 1);
        for (unsigned int id = blockIdx.x; id < n_tiles; id += gridDim.x) {
            unsigned int r = id;
            const unsigned int tt = r % ttiles; r /= ttiles;
            const unsigned int ch = r % chunks; r /= chunks;
            const unsigned int head = r % d.h, b = r / d.h;
            const unsigned int t0 = tt * kHeadsTokTile;
            // dy[b, head, ch * dc + dd, t0 + tl]: row dd by wave (row0 + 4 k), 64 consecutive tokens per wave-load
            const size_t grow = (static_cast<size_t>(b * d.h + head) * (4u * dv) + ch * dc) * d.T + t0;
            float gl[kHeadsChunkQuads];
#pragma unroll
            for (int k = 0; k < kHeadsChunkQuads; ++k) {
                const unsigned int dd = row0 + 4u * k;
                gl[k] = (dd < dc && t0 + tl_load < d.T) ? load_stream_f32(&gy[grow + static_cast<size_t>(dd) * d.T + tl_load]) : 0.0f;
            }
            // x[b, t0 + tl, head, ch * dvc + q]: lanes d-fastest, four float4 per lane
            float4 xa[4];
            unsigned int xi[4];
            bool ok[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const unsigned int idx = threadIdx.x + k * kBwdThreads, q = idx & (dvc - 1u), tl = idx >> dvc_shift;
                ok[k] = tl < static_cast<unsigned int>(kHeadsTokTile) && t0 + tl < d.T;
                xi[k] = ok[k] ? ((((b * d.T + t0 + tl) * d.h + head) << d.dv_shift) + ch * dvc + q) : 0u;
                xa[k] = ok[k] ? load_stream(&x[xi[k]]) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int k = 0; k < kHeadsChunkQuads; ++k) {
                const unsigned int dd = row0 + 4u * k;
                if (dd < dc) tile[dd * pitch + tl_load] = gl[k];
            }
            __syncthreads();
            BwdAcc acc = {0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (ok[k]) {
                    const unsigned int idx = threadIdx.x + k * kBwdThreads, q = idx & (dvc - 1u), tl = idx >> dvc_shift;
                    const float* col = &tile[4u * q * pitch + tl];
                    const float4 gq = make_float4(col[0], col[pitch], col[2u * pitch], col[3u * pitch]);
                    put(xi[k], bwd_elem4(f, xa[k], gq, sc, z, qmin, qmax, acc));
                }
            }
            t_ds += static_cast<double>(acc.ds_mul) + static_cast<double>(acc.ds_div);
            t_dz += static_cast<double>(acc.dz);
            __syncthreads();                                 // the next tile overwrites the one just read
        }
    } else {
        const float4* __restrict__ gy4 = reinterpret_cast<const float4*>(gy);
        const unsigned int stride = gridDim.x * kBwdThreads;                 // n4 + 2 * stride < 2^32 (launcher)
        for (unsigned int i = blockIdx.x * kBwdThreads + threadIdx.x; i < n4; i += 2u * stride) {
            const bool two = (i + stride) < n4;
            const unsigned int j = two ? i + stride : i;
            const unsigned int h0 = head_major_index(i, d), h1 = head_major_index(j, d);
            const unsigned int x0 = MERGE ? h0 : i, x1 = MERGE ? h1 : j;     // where x and dx live
            const unsigned int g0 = MERGE ? i : h0, g1 = MERGE ? j : h1;     // where dy lives
            const float4 a0 = load_stream(&x[x0]);
            const float4 b0 = load_stream(&gy4[g0]);
            float4 a1 = a0, b1 = b0;
            if (two) {
                a1 = load_stream(&x[x1]);
                b1 = load_stream(&gy4[g1]);
            }
            BwdAcc acc = {0.f, 0.f, 0.f};
            put(x0, bwd_elem4(f, a0, b0, sc, z, qmin, qmax, acc));
            if (two) put(x1, bwd_elem4(f, a1, b1, sc, z, qmin, qmax, acc));
            t_ds += static_cast<double>(acc.ds_mul) + static_cast<double>(acc.ds_div);
            t_dz += static_cast<double>(acc.dz);
        }
    }
    lsq_bwd_finish(t_ds, t_dz, mode, g, s.dscale[site], s.dzp[site], s.partials[site], s.counter[site]);
}

}  // namespace osq

using namespace osq;

extern "C" int osq_fake_quant_heads_backward(const osq_heads_backward_site* sites, int n_sites, int64_t batch, int64_t tokens,
                                             int64_t heads, int64_t head_dim, int direction, void* workspace,
                                             osq_stream stream) {
    OSQ_REQUIRE(sites && n_sites >= 1 && n_sites <= kWsHeadsSites, "fake_quant_heads_backward: 1..4 sites");
    OSQ_REQUIRE(batch >= 1 && tokens >= 1 && heads >= 1 && head_dim >= 1, "fake_quant_heads_backward: bad geometry");
    OSQ_REQUIRE(direction == OSQ_HEADS_SPLIT || direction == OSQ_HEADS_MERGE, "fake_quant_heads_backward: bad direction");
    OSQ_REQUIRE(workspace, "fake_quant_heads_backward: null workspace");
    // the geometry of fq_headsplit_multi_kernel: every index of the kernel in 32 bits, the multiply-shift divisions exact
    const int64_t dvv = head_dim / 4;
    if (head_dim % 4 != 0 || (dvv & (dvv - 1)) != 0 || dvv > 64 || batch >= (1ll << 30) || tokens >= (1ll << 31) ||
        heads * dvv >= (1ll << 31) || batch * tokens >= (1ll << 30) / (heads * dvv)) {
        osq::set_error("fake_quant_heads_backward: needs head_dim %% 4 == 0, head_dim / 4 a power of two <= 64 and fewer than 2^30 float4s");
        return OSQ_ERR_UNSUPPORTED;
    }
    const int64_t n4 = batch * tokens * heads * dvv;
    Workspace ws(workspace);
    HeadsBwdSites hs{};
    for (int i = 0; i < n_sites; ++i) {
        const osq_heads_backward_site& t = sites[i];
        OSQ_REQUIRE(t.x && t.grad_out && t.scale && t.zero_point, "fake_quant_heads_backward: null pointer in a site");
        OSQ_REQUIRE(t.mode >= OSQ_PARAM_FIXED && t.mode <= OSQ_PARAM_LSQPLUS,
                    "fake_quant_heads_backward: bad mode (the parameter repair is forward-only)");
        OSQ_REQUIRE(t.zp_type == OSQ_ZP_INT32 || t.zp_type == OSQ_ZP_FLOAT32, "fake_quant_heads_backward: bad zp_type");
        OSQ_REQUIRE(!(t.grad_out_transposed && direction == OSQ_HEADS_MERGE),
                    "fake_quant_heads_backward: the transposed gradient is a head-major layout (split direction only)");
        // the transposed gradient is read word by word: 4-byte alignment, which a float pointer has
        if (!aligned16(t.x) || (t.grad_x && !aligned16(t.grad_x)) || (!t.grad_out_transposed && !aligned16(t.grad_out))) {
            osq::set_error("fake_quant_heads_backward: needs 16-byte aligned tensors");
            return OSQ_ERR_UNSUPPORTED;
        }
        hs.x[i] = reinterpret_cast<const float4*>(t.x);
        hs.gy[i] = t.grad_out;
        hs.dx[i] = reinterpret_cast<float4*>(t.grad_x);
        hs.scale[i] = t.scale;
        hs.zp[i] = t.zero_point;
        hs.dscale[i] = t.grad_scale;
        hs.dzp[i] = t.grad_zero_point;
        hs.partials[i] = ws.heads_partials(i);
        hs.counter[i] = ws.heads_counter(i);
        hs.zp_type[i] = t.zp_type;
        hs.mode[i] = t.mode;
        hs.transposed[i] = t.grad_out_transposed ? 1 : 0;
        hs.g[i] = t.grad_factor;
        hs.qmin[i] = static_cast<float>(t.quant_min);
        hs.qmax[i] = static_cast<float>(t.quant_max);
    }
    const HeadSplit d = make_head_split(heads, dvv, tokens);
    // per site: two float4 per lane and trip, the launch's workgroups shared among its sites; <= kMaxBlocks (lsq_bwd_finish)
    const int per_site = grid_for(n4, kBwdThreads * 2, kHeadsBwdBlocks / n_sites);
    const dim3 grid(static_cast<unsigned>(per_site), static_cast<unsigned>(n_sites));
    const int wt = (stream_write_through() && n4 <= kWtMaxFloat4) ? 1 : 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (direction == OSQ_HEADS_MERGE)
        hipLaunchKernelGGL(heads_bwd_kernel<true>, grid, dim3(kBwdThreads), 0, st, hs, d, static_cast<unsigned int>(batch),
                           static_cast<unsigned int>(n4), wt);
    else
        hipLaunchKernelGGL(heads_bwd_kernel<false>, grid, dim3(kBwdThreads), 0, st, hs, d, static_cast<unsigned int>(batch),
                           static_cast<unsigned int>(n4), wt);
    return check_launch("fake_quant_heads_backward");
}

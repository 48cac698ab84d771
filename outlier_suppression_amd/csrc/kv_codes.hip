// The KV cache of incremental decoding held as integer codes: the append of one decoder step.
//
// fq_kv_append_kernel (fake_quant.hip) writes a step's fake-quantised keys / values as fp32 words, every one of them
// (x_quant - zp_eff) * scale_eff with x_quant an integer of a 6- or 8-bit range.  Here a site's destination may instead be a
// BYTE buffer of the same [B, h, cap, d] geometry holding u = x_quant - quant_min (codes_device.h: the code of codes.hip),
// with the effective parameters kept once per cached tensor (the record) -- a quarter of the cache's bytes and of what the
// step's attention reads (decode_attention.hip).  The quantising arithmetic is tensor_params / quantize_value, the chain
// of the fp32 append, so the dequantised code is that launch's word, bit for bit.
//
// One launch, blockIdx.y = site.  The unit of work is a WORD of four elements: a float4 of x gives one 32-bit store of codes
// (one float4 store at an fp32 site); the kept prefix is copied a word per lane, or four words (16 bytes) per lane at a
// coded site whose prefix, caps and pointers are multiples of 16 bytes.  No lane writes a byte another lane writes.
//
// osq_fake_quant_kv_append_codes_at: the same kernel with the offset of the flagged sites read from a device word by the
// launch (kv_append_position, osq_device.h), for a captured graph of a decoding step; the copy count and the copy width are
// then formed from that word, the grid from the capacity.
#include <algorithm>
#include "codes_device.h"
#include "osq_host.h"

namespace osq {

constexpr int kKvSites = 4;
constexpr int kKvCoded = 1, kKvWriteRecord = 2;

struct KvCodesSites {
    const float4* x[kKvSites];
    void* y[kKvSites];
    const void* src[kKvSites];               // nullptr: nothing to copy
    const int64_t* rows[kKvSites];           // nullptr: row b of src
    float* scale[kKvSites];
    void* zp[kKvSites];
    float* scale_eff[kKvSites];
    float* zp_eff[kKvSites];
    int zp_type[kKvSites], mode[kKvSites], flags[kKvSites];
    float g[kKvSites], qmin[kKvSites], qmax[kKvSites];
    unsigned int tokens[kKvSites], cap[kKvSites], offset[kKvSites];
    unsigned int src_cap[kKvSites], src_batch[kKvSites];
    unsigned int copy_words[kKvSites];       // words one lane copies: 1, or 4 at a coded site (16 bytes)
    unsigned int n_copy[kKvSites], n_total[kKvSites];   // work items: copy units, then the words of x
    // osq_fake_quant_kv_append_codes_at: the offset of the sites flagged in `at` is the device word *pos, read by the launch.
    // Their n_copy is formed from it, n_total holds the words of x alone, and copy_words says what the host could decide (4:
    // caps and pointers allow 16 bytes per lane); the launch goes back to a word per lane for a prefix that is no multiple of it.
    const int32_t* pos;                      // nullptr: the static form, every offset above
    int at[kKvSites];
    unsigned int batch_heads, any_coded;
};

__global__ __launch_bounds__(kCodeThreads) void fq_kv_append_codes_kernel(KvCodesSites s, unsigned int heads, unsigned int dv,
                                                                          int32_t* __restrict__ rejected) {
    const int site = blockIdx.y;
    const float4* __restrict__ x = s.x[site];
    const float qmin = s.qmin[site], qmax = s.qmax[site];
    const bool coded = s.flags[site] & kKvCoded;
    const unsigned int cap = s.cap[site], tokens = s.tokens[site];
    unsigned int offset = s.offset[site], n_copy = s.n_copy[site], n_total = s.n_total[site], cw = s.copy_words[site];
    if (s.pos) {                                       // workgroup-uniform
        const int pos = kv_append_position(s);
        if (pos < 0) {                                 // refused: nothing written, counted once where a cache of codes is at stake
            if (s.any_coded && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) atomicAdd(rejected, 1);
            return;
        }
        if (s.at[site]) {
            offset = static_cast<unsigned int>(pos);
            if ((offset * dv) % cw) cw = 1u;
            n_copy = s.src[site] ? s.batch_heads * (offset * dv / cw) : 0u;
            n_total += n_copy;
        }
    }
    const QParams p = tensor_params(s.scale[site], s.zp[site], s.zp_type[site], s.mode[site], s.g[site], qmin, qmax);
    const unsigned int stride = gridDim.x * kCodeThreads;
    const unsigned int head_row = heads * dv, past_units = offset * dv / cw;
    unsigned int rej = 0;
    if (coded && blockIdx.x == 0 && threadIdx.x == 0) {
        // the record: written by the tensor's first append, compared bit for bit by every later one
        if (s.flags[site] & kKvWriteRecord) {
            s.scale_eff[site][0] = p.scale;
            s.zp_eff[site][0] = p.zp;
        } else if (__float_as_uint(s.scale_eff[site][0]) != __float_as_uint(p.scale) ||
                   __float_as_uint(s.zp_eff[site][0]) != __float_as_uint(p.zp)) {
            rej += 1u;
        }
    }
    for (unsigned int i = blockIdx.x * kCodeThreads + threadIdx.x; i < n_total; i += stride) {
        if (i < n_copy) {
            // y[b, head, :offset] = src[rows[b], head, :offset], unit r of the prefix
            const unsigned int bh = i / past_units, r = i - bh * past_units;
            const unsigned int b = bh / heads, head = bh - b * heads;
            const int64_t row = s.rows[site] ? s.rows[site][b] : static_cast<int64_t>(b);
            const bool ok = row >= 0 && row < static_cast<int64_t>(s.src_batch[site]);
            const unsigned int from = ((static_cast<unsigned int>(row) * heads + head) * s.src_cap[site]) * dv + r * cw;
            const unsigned int to = bh * cap * dv + r * cw;
            if (!coded) {
                float4 v;
                if (ok) v = static_cast<const float4*>(s.src[site])[from];
                else v.x = v.y = v.z = v.w = __builtin_nanf("");             // an index out of range: NaN, no read
                static_cast<float4*>(s.y[site])[to] = v;
            } else if (cw == 4) {
                osq_v4u32 v = {0u, 0u, 0u, 0u};                              // an index out of range: code 0, counted, no read
                if (ok) v = *reinterpret_cast<const osq_v4u32*>(static_cast<const unsigned int*>(s.src[site]) + from);
                else rej += 16u;
                *reinterpret_cast<osq_v4u32*>(static_cast<unsigned int*>(s.y[site]) + to) = v;
            } else {
                unsigned int v = 0u;
                if (ok) v = static_cast<const unsigned int*>(s.src[site])[from];
                else rej += 4u;
                static_cast<unsigned int*>(s.y[site])[to] = v;
            }
        } else {
            // y[b, head, offset + j, :] = fake_quant(x[b, j, head * d:(head + 1) * d]), or its codes
            const unsigned int e = i - n_copy;
            const unsigned int bt = e / head_row, c = e - bt * head_row;
            const unsigned int b = bt / tokens, j = bt - b * tokens;
            const unsigned int head = c / dv, dd = c - head * dv;
            const unsigned int to = ((b * heads + head) * cap + offset + j) * dv + dd;
            const float4 v = x[e];
            if (coded) {
                static_cast<unsigned int*>(s.y[site])[to] = code_of(v.x, p, qmin, qmax, rej) | (code_of(v.y, p, qmin, qmax, rej) << 8) |
                                                            (code_of(v.z, p, qmin, qmax, rej) << 16) | (code_of(v.w, p, qmin, qmax, rej) << 24);
            } else {
                float4 o, q;
                fq4_plain(v, o, q, p.scale, p.zp, qmin, qmax);
                static_cast<float4*>(s.y[site])[to] = o;
            }
        }
    }
    add_rejected(rejected, rej);
}

static bool aligned_to(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1u)) == 0; }

}  // namespace osq

using namespace osq;

// pos == nullptr: the static form.  Otherwise site i with at[i] != 0 takes its offset from the device word *pos: whatever
// the static form decides from the offset holds here for every offset the capacity admits, or is left to the launch.
static int kv_append_codes_launch(const osq_kv_codes_site* sites, int n_sites, int64_t batch, int64_t heads, int64_t head_dim,
                                  int32_t* rejected, const int32_t* pos, const int32_t* at, osq_stream stream) {
    OSQ_REQUIRE(sites && n_sites >= 1 && n_sites <= kKvSites, "fake_quant_kv_append_codes: 1..4 sites");
    OSQ_REQUIRE(batch >= 0 && heads >= 1 && head_dim >= 1, "fake_quant_kv_append_codes: bad geometry");
    if (head_dim % 4 != 0) return OSQ_ERR_UNSUPPORTED;
    const int64_t dv = head_dim / 4;
    const int64_t kLimit = 1ll << 31;                  // every index of the kernel in 32 bits
    KvCodesSites ks{};
    int64_t most = 0;
    for (int i = 0; i < n_sites; ++i) {
        const osq_kv_codes_site& t = sites[i];
        const bool coded = t.coded != 0;
        const bool from_pos = pos && at[i];
        const int64_t offset = from_pos ? 0 : t.offset;
        const int64_t word = coded ? 4 : 16;           // bytes of four elements; the alignment asked of y and src
        OSQ_REQUIRE(t.scale && t.zero_point, "fake_quant_kv_append_codes: null parameter pointer in a site");
        OSQ_REQUIRE(t.tokens >= 0 && offset >= 0 && t.cap >= offset + t.tokens,
                    "fake_quant_kv_append_codes: need 0 <= offset, offset + tokens <= cap");
        if (coded) {
            OSQ_REQUIRE(rejected && t.scale_eff && t.zp_eff, "fake_quant_kv_append_codes: a coded site needs its record and the rejected counter");
            OSQ_REQUIRE(static_cast<int64_t>(t.quant_max) - t.quant_min >= 0 && static_cast<int64_t>(t.quant_max) - t.quant_min <= 255,
                        "fake_quant_kv_append_codes: quant_max - quant_min does not fit a byte");
        }
        const int64_t n_app = batch * t.tokens * heads * dv;
        OSQ_REQUIRE(n_app == 0 || (t.x && t.y), "fake_quant_kv_append_codes: null tensor in a site");
        const bool copy = t.src && (from_pos || offset > 0) && batch > 0 && !(t.src == t.y && !t.src_rows);
        int64_t n_copy = 0, copy_words = 1;            // from_pos: the longest prefix, a word per lane: the grid and the limit go by it
        if (copy) {
            OSQ_REQUIRE(t.y && t.src_cap >= offset && t.src_batch >= 1, "fake_quant_kv_append_codes: source smaller than offset");
            OSQ_REQUIRE(t.src_rows || t.src_batch == batch, "fake_quant_kv_append_codes: source batch differs, no row index");
            // the copy must not read what the launch writes: the same buffer with a row index, or overlapping ranges
            const char *s0 = static_cast<const char*>(t.src), *s1 = s0 + t.src_batch * heads * t.src_cap * dv * word;
            const char *y0 = static_cast<const char*>(t.y), *y1 = y0 + batch * heads * t.cap * dv * word;
            if (s0 < y1 && y0 < s1) return OSQ_ERR_UNSUPPORTED;
            if (!aligned_to(t.src, word) || t.src_batch * heads * t.src_cap * dv >= kLimit) return OSQ_ERR_UNSUPPORTED;
            if (coded && aligned16(t.src) && aligned16(t.y) && (offset * dv) % 4 == 0 && (t.cap * dv) % 4 == 0 && (t.src_cap * dv) % 4 == 0)
                copy_words = 4;
            n_copy = from_pos ? batch * heads * std::min(t.cap - t.tokens, t.src_cap) * dv : batch * heads * (offset * dv / copy_words);
        }
        if ((t.x && !aligned16(t.x)) || (t.y && !aligned_to(t.y, word))) return OSQ_ERR_UNSUPPORTED;
        if (batch * heads * t.cap * dv >= kLimit || n_copy + n_app >= kLimit) return OSQ_ERR_UNSUPPORTED;
        ks.x[i] = reinterpret_cast<const float4*>(t.x);
        ks.y[i] = t.y;
        ks.src[i] = copy ? t.src : nullptr;
        ks.rows[i] = copy ? t.src_rows : nullptr;
        ks.scale[i] = t.scale;
        ks.zp[i] = t.zero_point;
        ks.scale_eff[i] = t.scale_eff;
        ks.zp_eff[i] = t.zp_eff;
        ks.zp_type[i] = t.zp_type;
        ks.mode[i] = t.mode;
        ks.flags[i] = coded ? (kKvCoded | (t.write_record ? kKvWriteRecord : 0)) : 0;
        ks.g[i] = t.grad_factor;
        ks.qmin[i] = static_cast<float>(t.quant_min);
        ks.qmax[i] = static_cast<float>(t.quant_max);
        ks.tokens[i] = static_cast<unsigned int>(t.tokens);
        ks.cap[i] = static_cast<unsigned int>(t.cap);
        ks.offset[i] = static_cast<unsigned int>(offset);
        ks.at[i] = from_pos;
        ks.any_coded |= coded ? 1u : 0u;
        ks.src_cap[i] = copy ? static_cast<unsigned int>(t.src_cap) : 0u;
        ks.src_batch[i] = copy ? static_cast<unsigned int>(t.src_batch) : 0u;
        ks.copy_words[i] = static_cast<unsigned int>(copy_words);
        ks.n_copy[i] = from_pos ? 0u : static_cast<unsigned int>(n_copy);
        ks.n_total[i] = static_cast<unsigned int>((from_pos ? 0 : n_copy) + n_app);
        most = std::max(most, n_copy + n_app);
    }
    if (most == 0) return OSQ_OK;
    ks.pos = pos;
    ks.batch_heads = static_cast<unsigned int>(batch * heads);
    const dim3 grid(static_cast<unsigned>(grid_for(most, kCodeThreads, kMaxBlocks)), static_cast<unsigned>(n_sites));
    hipLaunchKernelGGL(fq_kv_append_codes_kernel, grid, dim3(kCodeThreads), 0, static_cast<hipStream_t>(stream), ks,
                       static_cast<unsigned int>(heads), static_cast<unsigned int>(dv), rejected);
    return check_launch(pos ? "fake_quant_kv_append_codes_at" : "fake_quant_kv_append_codes");
}

extern "C" int osq_fake_quant_kv_append_codes(const osq_kv_codes_site* sites, int n_sites, int64_t batch, int64_t heads,
                                              int64_t head_dim, int32_t* rejected, osq_stream stream) {
    return kv_append_codes_launch(sites, n_sites, batch, heads, head_dim, rejected, nullptr, nullptr, stream);
}

extern "C" int osq_fake_quant_kv_append_codes_at(const osq_kv_codes_site* sites, int n_sites, int64_t batch, int64_t heads,
                                                 int64_t head_dim, int32_t* rejected, const int32_t* pos, const int32_t* site_at,
                                                 osq_stream stream) {
    OSQ_REQUIRE(pos && site_at, "fake_quant_kv_append_codes_at: null position word or site flags");
    return kv_append_codes_launch(sites, n_sites, batch, heads, head_dim, rejected, pos, site_at, stream);
}

// What the attention sites over WHOLE sequences share (attention.hip: the probabilities site on given scores;
// attention_block.hip: the block in fp32; attention_int.hip: the block on integer codes): the pre-softmax rule, the argument
// record and the launch check of the two block kernels, and the small pieces both of those are built from.  The kernels are
// different algorithms; what surrounds them is stated here once.
#pragma once
#include "attention_quant.h"

namespace osq {

// THE PRE-SOFTMAX RULE, each form in the bits of the eager code it stands for (-ffp-contract=off: one rounding per operation):
//     kPrePlain    v = s + mask                   neither alpha nor divisor given (BART: q is scaled before the product)
//     kPreScale    v = mask + s * alpha           alpha != 1 (BERT: torch.add(mask, s, alpha=1/sqrt(d)), alpha a power of two)
//     kPreDivide   v = s / divisor + mask         divisor != 1 (BERT, other head sizes: IEEE division, not a reciprocal)
// Without a mask there is no add.  The entry points refuse a call that gives both alpha and divisor.
enum { kPrePlain = 0, kPreScale = 1, kPreDivide = 2 };

static int pre_of(float alpha, float divisor) { return divisor != 1.0f ? kPreDivide : (alpha != 1.0f ? kPreScale : kPrePlain); }

// pre(s); the caller then adds the mask's element, a rounding of its own
__device__ __forceinline__ float pre_softmax(int pre, float s, float alpha, float divisor) {
    if (pre == kPreScale) return s * alpha;
    if (pre == kPreDivide) return s / divisor;
    return s;
}

typedef float f32x16 __attribute__((ext_vector_type(16)));     // the 32 x 32 result of a matrix instruction, 16 words per lane

// row of a 32 x 32 result a lane holds in register r, half = lane >> 5 (its column is lane & 31)
__device__ __forceinline__ int mfma32_row(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

// CALL with D = head_dim as a constant; seq_check_launch has refused every other head size
#define OSQ_HEAD_DIM_DISPATCH(head_dim, CALL)                   \
    switch (head_dim) {                                         \
        case 16: { constexpr int D = 16; CALL; break; }         \
        case 32: { constexpr int D = 32; CALL; break; }         \
        case 64: { constexpr int D = 64; CALL; break; }         \
        default: { constexpr int D = 128; CALL; break; }        \
    }

// The arguments the two block kernels share; each kernel's record is this one followed by its quantizers.  With group = G > 1
// the G decoder rows b * G .. b * G + G - 1 of q, out and probs_out share row b of k, v and mask (the layout of
// decode_attention.hip's shared form); batch counts the rows of k / v.
struct SeqArgs {
    const float* q;            // [B * G, h, T, d]: row (bd, h, t) at bd * q_sb + h * q_sh + t * q_st, head_dim contiguous floats
    const float* k;            // [B, h, S, d]
    const float* v;
    const float* mask;         // nullable; row (b, h, t) at b * m_sb + h * m_sh + t * m_st, S contiguous floats
    float* out;                // dense [B * G, T, heads * head_dim]
    float* probs_out;          // nullable, dense [B * G, heads, T, S]
    int64_t q_sb, q_sh, q_st, k_sb, k_sh, k_st, v_sb, v_sh, v_st, m_sb, m_sh, m_st;
    int64_t heads;
    int group;                 // G
    int tokens, kv_len;        // T, S
    int rows, tiles;           // G * T virtual query rows of a (b, head); ceil(rows / the query rows of a workgroup)
    int pre;
    float alpha, divisor;
};

// THE ROW MAP.  A workgroup serves one (b, head) and a tile of VIRTUAL query rows r in [0, rows): the T rows of decoder row
// b * G, then those of b * G + 1, ...  Every address of a query row in either kernel goes through here; with G == 1 each is
// what it was without a group (j == 0, t == r, bd == b).  Rows beyond `rows` repeat row rows - 1 and are dropped: the caller
// clamps r.
struct SeqRow {
    int64_t bd;                // decoder row b * G + j, j = r / T
    int t;                     // r - j * T
};

__device__ __forceinline__ SeqRow seq_row(const SeqArgs& a, int64_t b, int r) {
    const int j = r / a.tokens;
    return {b * a.group + j, r - j * a.tokens};          // (b is 64-bit: b * G fits whatever it is multiplied by next)
}

__device__ __forceinline__ const float* seq_q_row(const SeqArgs& a, int64_t b, int64_t h, int r) {
    const SeqRow x = seq_row(a, b, r);
    return a.q + x.bd * a.q_sb + h * a.q_sh + static_cast<int64_t>(x.t) * a.q_st;
}

// the mask goes by the SHARED row b, not by the decoder row (a.mask is not null)
__device__ __forceinline__ const float* seq_mask_row(const SeqArgs& a, int64_t b, int64_t h, int r) {
    return a.mask + b * a.m_sb + h * a.m_sh + static_cast<int64_t>(seq_row(a, b, r).t) * a.m_st;
}

// row ((bd * T + t) * heads + h) * D of the dense merged out; bd * T + t == b * rows + r, so this one needs no division
template <int D>
__device__ __forceinline__ float* seq_out_row(const SeqArgs& a, int64_t b, int64_t h, int r) {
    return a.out + ((b * a.rows + r) * a.heads + h) * D;
}

// (a.probs_out is not null)
__device__ __forceinline__ float* seq_probs_row(const SeqArgs& a, int64_t b, int64_t h, int r) {
    const SeqRow x = seq_row(a, b, r);
    return a.probs_out + ((x.bd * a.heads + h) * a.tokens + x.t) * static_cast<int64_t>(a.kv_len);
}

// OSQ_REQUIRE with the entry point's name in front of the message
#define OSQ_SEQ_REQUIRE(cond, msg)                   \
    do {                                             \
        if (!(cond)) {                               \
            set_error("%s: %s", what, msg);          \
            return OSQ_ERR_INVALID_ARGUMENT;         \
        }                                            \
    } while (0)

// The launch check of the block kernels comes in two parts, an entry point's checks of its own quantizers between them -- the
// order in which a call with several faults is refused.  First part: what is wrong whatever the kernel.  `a` holds the
// pointers, strides, heads, alpha and divisor as given; the lengths and the group come as the ABI's int64.  Fills group of `a`.
static int seq_check_shape(const char* what, SeqArgs& a, int64_t batch, int64_t group, int64_t tokens, int64_t head_dim) {
    OSQ_SEQ_REQUIRE(batch >= 0 && a.heads >= 0 && tokens >= 0 && tokens <= INT32_MAX && head_dim > 0 && group >= 1 &&
                    group <= INT32_MAX && group * tokens <= INT32_MAX, "bad shape");
    a.group = static_cast<int>(group);
    OSQ_SEQ_REQUIRE(a.q_sb >= 0 && a.q_sh >= 0 && a.q_st >= 0 && a.k_sb >= 0 && a.k_sh >= 0 && a.k_st >= 0 &&
                    a.v_sb >= 0 && a.v_sh >= 0 && a.v_st >= 0, "negative stride");
    OSQ_SEQ_REQUIRE(!a.mask || (a.m_sb >= 0 && a.m_sh >= 0 && a.m_st >= 0), "negative mask stride");
    OSQ_SEQ_REQUIRE(a.alpha == 1.0f || a.divisor == 1.0f, "give alpha or divisor, not both");
    return OSQ_OK;
}

// Second part: what this kernel -- workgroups of tile_q query rows, at most max_kv keys -- does not take (OSQ_ERR_UNSUPPORTED:
// the caller runs its other path), the grid bound, the empty call and the pointers.  Fills tokens, kv_len, rows, tiles and pre
// of `a` and gives the workgroups to launch, 0 for an empty call (OSQ_OK, nothing to do).
static int seq_check_launch(const char* what, SeqArgs& a, int64_t batch, int64_t tokens, int64_t kv_len, int64_t head_dim,
                            int tile_q, int max_kv, int64_t* blocks) {
    *blocks = 0;
    if (head_dim != 16 && head_dim != 32 && head_dim != 64 && head_dim != 128) return OSQ_ERR_UNSUPPORTED;
    if (kv_len < 1 || kv_len > max_kv) return OSQ_ERR_UNSUPPORTED;
    // float4 loads of (half) rows of q and k; v is held to the same rule where it is read by the float
    if ((a.q_sb | a.q_sh | a.q_st | a.k_sb | a.k_sh | a.k_st | a.v_sb | a.v_sh | a.v_st) & 3) return OSQ_ERR_UNSUPPORTED;
    const int64_t group = a.group, rows = group * tokens, tiles = (rows + tile_q - 1) / tile_q;
    OSQ_SEQ_REQUIRE(batch <= INT32_MAX && batch * group <= INT32_MAX && a.heads <= INT32_MAX &&
                    batch * a.heads <= INT32_MAX / (tiles > 0 ? tiles : 1), "bad shape");
    if (batch * a.heads * tokens == 0) return OSQ_OK;
    OSQ_SEQ_REQUIRE(a.q && a.k && a.v && a.out, "null tensor");
    if (!aligned16(a.q) || !aligned16(a.k) || !aligned16(a.v) || !aligned16(a.out)) return OSQ_ERR_UNSUPPORTED;
    if ((reinterpret_cast<uintptr_t>(a.mask) | reinterpret_cast<uintptr_t>(a.probs_out)) & 3u) return OSQ_ERR_UNSUPPORTED;
    a.tokens = static_cast<int>(tokens);
    a.kv_len = static_cast<int>(kv_len);
    a.rows = static_cast<int>(rows);
    a.tiles = static_cast<int>(tiles);
    a.pre = pre_of(a.alpha, a.divisor);
    *blocks = batch * a.heads * tiles;
    return OSQ_OK;
}

}  // namespace osq

// Linear layers of a frozen model on the quantizers' INTEGER CODES: out = x . W^T + bias on the int8 matrix instruction
// v_mfma_i32_32x32x32_i8 -- int32 accumulation, exact by construction.
//
// In a frozen model both operands of a QLinear are codes times a scale: the weight is its quantizer's output (the bytes
// export_codes stores), the input is the output of a per-tensor activation quantizer.  For input row r, output channel c
// and reduction length K (include/osq_hip.h, "integer linear"):
//
//     ux = clamp(rint(x[r,k] / s_x) + zp_x, qmin_x, qmax_x) - qmin_x      the producer's quantizer once more: exact on its own outputs
//     uw = clamp(rint(w[c,k] / s_w[c]) + zp_w[c], qmin_w, qmax_w) - qmin_w the weight's exported code byte
//     a = ux - 128, b = uw - 128                                           int8
//     zx = (zp_x - qmin_x) - 128,  zw[c] = (zp_w[c] - qmin_w) - 128        integers, or the launch writes NaN everywhere
//     N[r,c] = sum_k a*b - zw[c] * sum_k a[r,k] - zx * sum_k b[c,k] + K * zx * zw[c]        int32, exact: |N| <= 255*255*K
//     out[r,c] = (float)N[r,c] * (s_x * s_w[c]) + bias[c]                  one rounding per operation, in this order
//
// Three launches:
//   activation_codes_kernel  x [M,K] fp32 -> a [M,K] bytes + rowsum [M] int32: once per producer output, shared by its consumers.
//                            A wave per row, 16-byte loads, four codes to a 4-byte store, the row sum by wave shuffles.  A row
//                            with a non-finite element has no codes: its row sum is kLinNoRow and exactly that row of out is NaN.
//   weight_codes_kernel      w [N,K] fp32 -> b [N,K] bytes + colsum, s_w, zw [N] + one `bad` word: once per frozen weight.
//   linear_int_kernel        one 256-thread workgroup per 128 x 128 tile of out, a wave per 64 x 64 part: 2 x 2 tiles of the
//                            32 x 32 x 32 instruction, 64 accumulator registers.  K goes by in steps of 64 bytes: the code tiles
//                            of W and X (128 rows each) are fetched with 16-byte loads into double-buffered LDS, the next step's
//                            loads issued before this step's products, one barrier per step.  A row of a tile is 64 + 16 bytes:
//                            row i starts at bank 20 i mod 64, so the 16 lanes of a 16-byte read phase hit 16 disjoint groups of
//                            four banks.  LDS: 2 x 2 x 128 x 80 B = 40 KiB.
//   linear_int_rows_kernel   M <= 32 (a decoding step, the pooler, the classifier): a 128-row tile would leave all but N / 128
//                            CUs idle.  One workgroup per 32 channels, its four waves split K in chunks of 128 bytes per row and
//                            read their operands straight from memory (every weight byte once, by one wave; x stays in cache);
//                            the four partial tiles are added through LDS (int32: any order) and wave 0 finishes.
// A = W, B = X in both: a lane holds ONE row of x (lane & 31) and, in register r of a 32 x 32 result, channel
// (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5) -- the map csrc/attention_int.hip documents -- so registers 4 g .. 4 g + 3 are four
// consecutive channels: their colsum / zw / s_w / bias come with one 16-byte load each and leave as one 16-byte store where
// N % 4 == 0.  Both operands read their 16 bytes of a k-step from the same place of their row, so the k order inside the
// instruction does not matter.  Rows beyond M and channels beyond N are clamped at the load and dropped at the store; bytes
// beyond K (K % 64 != 0) are zero in both operands.
//
// PACKED 4-BIT WEIGHTS (osq_weight_codes_sums_w4, osq_linear_int_w4; a weight quantizer of at most 16 codes).  N[r,c] does not
// depend on the offset taken off the codes, so the packed path takes none: b = uw in 0..15, zw[c] = zp_w[c] - qmin_w, colsum[c]
// = sum_k uw -- the same integer, every term below 2**31 at K = 16384, the same epilogue.  W is [N, K / 2] bytes in the
// `code_bits 4` layout of include/osq_hip.h (byte j: element 2 j low, 2 j + 1 high); K % 16 == 0 keeps a row whole bytes, 8-byte
// aligned.  x is the shared, unpermuted activation_codes output.
//   weight_codes_w4_kernel   encode_row's loop with two 16-byte loads per lane and trip: eight codes to one 4-byte store.
//   linear_int_rows_kernel_w4  the weight stream is half as long, so a lane's 16-byte weight load now spans 32 k: in a step of
//                            64 k half h of the wave holds packed bytes for k0 + 64 s + 32 h .. + 31 of its channel, unpacks them
//                            in registers (p & 0x0F0F0F0F: even elements, (p >> 4) & 0x0F0F0F0F: odd ones, two v_perm_b32 put
//                            them back in k order) and feeds k .. + 15 to one instruction and k + 16 .. + 31 to the next, x loaded
//                            at the same two places.  A wave's chunk is 128 k = 64 packed bytes of a row; the NEXT chunk's six
//                            loads leave before this chunk's four products (two register sets), so a wave with two or more
//                            chunks always has weight bytes in flight.  The loop over whole chunks has no branch in it -- the
//                            wait before a product then counts exactly the six younger loads -- and K's partial last chunk, which
//                            one wave has, is read after it with predicated loads.  K split over four waves and the LDS add as above.
//                            K % 32 == 16: rows are 8-byte, not 16-byte aligned -- the 16-byte load is typed 8-byte aligned --
//                            and the row's last 16 k are 8 packed bytes: the half that owns them issues ONE 8-byte load and
//                            zeroes the rest, so no lane reads past its row and the last row's reads end with the tensor.
//   linear_int_kernel<true>  the tile kernel's body with one change: a granule of W is fetched as 8 packed bytes (8-byte
//                            aligned) and unpacked into its 16 bytes just before the stash, so LDS holds what the 8-bit kernel's
//                            does: same layout, bank note, product loop and epilogue, four registers fewer in flight.
// No allocation, no host sync, no workspace, no atomics: legal inside a stream capture.  Inference only.
//
// CODES FOR THE NEXT LINEAR (osq_linear_int_codes; a feed-forward block's fc1).  The three product kernels take one more
// template argument, kCodes: same K loop, another epilogue.  It writes no out; per element u = code_of(gelu_erf(lin_value(..)))
// under the NEXT linear's quantizer (gelu_erf only where the launch asks for it), codes [M, N] bytes u - 128 and rowsum [M] =
// sum_c (u - 128): what activation_codes would make of the fake-quantised out -- re-encoding a fake-quantised value gives
// back its code -- word for word.  N % 16 == 0.
//   a lane's granule         per row the 32 bytes of a 32 x 32 result are A0 B0 A1 B1 A2 B2 A3 B3, A in lanes 0..31 and B in their
//                            partners (lane ^ 32): each lane sends the two words its partner needs and keeps its own two, and
//                            holds 16 contiguous bytes of its row (lin_code_granule).
//   tile kernel              the 128 x 128 code bytes are staged in the operand LDS, free after the K loop, at a pitch of 144
//                            (the bank note is at the code) and leave 16 bytes per lane, 8 consecutive lanes to a 128-byte line.
//   rows kernels             a workgroup owns 32 bytes of a row, two lanes' granules: wave 0 stores them from registers.
//   row sums                 a workgroup's partial per row comes from the granules and is added into the ZEROED rowsum with one
//                            vector int32 atomic add per row (order-free: deterministic).  kLinNoRow cannot be made by adding:
//                            a lane that meets an element without a code ORs its row's flag; every workgroup fences and takes a
//                            ticket of its row tile, and whoever draws the last one exchanges kLinNoRow into the flagged rows
//                            and into those that came in without codes.  Nobody waits.  A bad launch (*w_bad, zp_x or the out
//                            zero point no integer in range) is uniform: the first channel tile's workgroups store kLinNoRow
//                            into every row and nobody adds.  The caller zeroes rowsum, flags [M] and tickets [row tiles]: one
//                            buffer, one clear, before every launch.
#include <math.h>
#include <hip/hip_runtime.h>
#include "attention_quant.h"
#include "codes_device.h"
#include "lsq_backward.h"

namespace osq {

constexpr int kLinThreads = 256;
constexpr int kLinTile = 128;            // rows of x and channels of a workgroup's tile
constexpr int kLinKStep = 64;            // code bytes of a row per step: two k-steps of the instruction
constexpr int kLinPitch = kLinKStep + 16;    // bytes of a tile row in LDS
constexpr int kLinMaxK = 16384;          // |N| <= 255 * 255 * K < 2**30
constexpr int kLinRowsM = 32;            // up to here: linear_int_rows_kernel
constexpr int kLinRowsChunk = 128;       // bytes of a row a wave of linear_int_rows_kernel takes at a time
constexpr int kLinW4Chunk = 128;         // k of a row a wave of linear_int_rows_kernel_w4 takes at a time: 64 packed bytes
constexpr int kLinNoRow = INT32_MIN;     // rowsum of a row without codes (a real one is at most 128 * K = 2**21)

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));
typedef int i32x2 __attribute__((ext_vector_type(2)));
typedef int i32x4_a8 __attribute__((ext_vector_type(4), aligned(8)));       // a packed row starts on 8 bytes where K % 32 == 16

// Eight 4-bit codes of one word, element 2 j in the low nibble of byte j, as two words of bytes in element order.
__device__ __forceinline__ i32x2 unpack_w4(int p) {
    const unsigned int even = static_cast<unsigned int>(p) & 0x0F0F0F0Fu, odd = (static_cast<unsigned int>(p) >> 4) & 0x0F0F0F0Fu;
    return i32x2{static_cast<int>(__builtin_amdgcn_perm(odd, even, 0x05010400u)),       // e0 o0 e1 o1
                 static_cast<int>(__builtin_amdgcn_perm(odd, even, 0x07030602u))};      // e2 o2 e3 o3
}

// sixteen codes of two words
__device__ __forceinline__ i32x4 unpack_w4(int p0, int p1) {
    const i32x2 a = unpack_w4(p0), b = unpack_w4(p1);
    return i32x4{a.x, a.y, b.x, b.y};
}

__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
    for (int d = OSQ_WAVE / 2; d; d >>= 1) v += __shfl_xor(v, d, OSQ_WAVE);
    return v;
}

// One wave, one row of n4 float4: the bytes (u ^ 0x80 = u - 128 as int8) four to a word.  Returns the row's sum of u - 128 in
// every lane; `rej` counts this lane's elements without a code (code_of).
__device__ __forceinline__ int encode_row(const float4* __restrict__ xr, unsigned int* __restrict__ cr, int n4, int lane,
                                          const QParams& p, float qmin, float qmax, unsigned int& rej) {
    constexpr int kTrip = 4;             // 16-byte loads in flight per lane
    int sum = 0;
    for (int j0 = lane; j0 < n4; j0 += kTrip * OSQ_WAVE) {
        float4 v[kTrip];
#pragma unroll
        for (int u = 0; u < kTrip; ++u)
            if (j0 + u * OSQ_WAVE < n4) v[u] = xr[j0 + u * OSQ_WAVE];
#pragma unroll
        for (int u = 0; u < kTrip; ++u)
            if (j0 + u * OSQ_WAVE < n4) {
                const unsigned int u0 = code_of(v[u].x, p, qmin, qmax, rej), u1 = code_of(v[u].y, p, qmin, qmax, rej);
                const unsigned int u2 = code_of(v[u].z, p, qmin, qmax, rej), u3 = code_of(v[u].w, p, qmin, qmax, rej);
                sum += static_cast<int>(u0 + u1 + u2 + u3) - 512;
                cr[j0 + u * OSQ_WAVE] = (u0 | (u1 << 8) | (u2 << 16) | (u3 << 24)) ^ 0x80808080u;
            }
    }
    return wave_sum_i32(sum);
}

// The packed twin: n8 pairs of float4, eight codes u (no offset: 0 .. 15) to a word in the `code_bits 4` layout.  Returns the
// row's sum of u.
__device__ __forceinline__ int encode_row_w4(const float4* __restrict__ xr, unsigned int* __restrict__ cr, int n8, int lane,
                                             const QParams& p, float qmin, float qmax, unsigned int& rej) {
    constexpr int kTrip = 2;             // pairs of 16-byte loads in flight per lane
    int sum = 0;
    for (int j0 = lane; j0 < n8; j0 += kTrip * OSQ_WAVE) {
        float4 v[kTrip][2];
#pragma unroll
        for (int u = 0; u < kTrip; ++u)
            if (j0 + u * OSQ_WAVE < n8) {
                v[u][0] = xr[2 * (j0 + u * OSQ_WAVE)];
                v[u][1] = xr[2 * (j0 + u * OSQ_WAVE) + 1];
            }
#pragma unroll
        for (int u = 0; u < kTrip; ++u)
            if (j0 + u * OSQ_WAVE < n8) {
                unsigned int word = 0;
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const unsigned int u0 = code_of(v[u][h].x, p, qmin, qmax, rej), u1 = code_of(v[u][h].y, p, qmin, qmax, rej);
                    const unsigned int u2 = code_of(v[u][h].z, p, qmin, qmax, rej), u3 = code_of(v[u][h].w, p, qmin, qmax, rej);
                    sum += static_cast<int>(u0 + u1 + u2 + u3);
                    word |= (u0 | (u1 << 4) | (u2 << 8) | (u3 << 12)) << (16 * h);
                }
                cr[j0 + u * OSQ_WAVE] = word;
            }
    }
    return wave_sum_i32(sum);
}

__device__ __forceinline__ bool lin_zp_ok(float zp, float qmin, float qmax) {
    return zp >= qmin && zp <= qmax && rintf(zp) == zp;       // false for a NaN
}

__global__ __launch_bounds__(kLinThreads) void activation_codes_kernel(const float* __restrict__ x, int64_t ldx,
                                                                       uint8_t* __restrict__ codes, int32_t* __restrict__ rowsum,
                                                                       int64_t rows, int cols, DecQuant q) {
    const QParams p = dec_params(q);                  // first: the parameter repair rides here
    const int lane = threadIdx.x & (OSQ_WAVE - 1);
    const int64_t wave = (static_cast<int64_t>(blockIdx.x) * kLinThreads + threadIdx.x) / OSQ_WAVE;
    const int64_t nwaves = static_cast<int64_t>(gridDim.x) * (kLinThreads / OSQ_WAVE);
    for (int64_t r = wave; r < rows; r += nwaves) {
        unsigned int rej = 0;
        const int sum = encode_row(reinterpret_cast<const float4*>(x + r * ldx), reinterpret_cast<unsigned int*>(codes + r * cols),
                                   cols / 4, lane, p, q.qmin, q.qmax, rej);
        const int bad = wave_sum_i32(static_cast<int>(rej));
        if (lane == 0) rowsum[r] = bad ? kLinNoRow : sum;
    }
}

// rows = output channels; channels: rows (a scale per row) or 1.  kW4: packed codes [rows, cols / 2] without the offset of 128
template <bool kW4>
__global__ __launch_bounds__(kLinThreads) void weight_codes_kernel(const float* __restrict__ w, uint8_t* __restrict__ codes,
                                                                   int32_t* __restrict__ colsum, float* __restrict__ scale_eff,
                                                                   int32_t* __restrict__ zw, int32_t* __restrict__ bad,
                                                                   int64_t rows, int64_t channels, int cols,
                                                                   const float* __restrict__ scale_p, const void* __restrict__ zp_p,
                                                                   int zp_type, int mode, float g, float qmin, float qmax) {
    const int lane = threadIdx.x & (OSQ_WAVE - 1);
    const int64_t wave = (static_cast<int64_t>(blockIdx.x) * kLinThreads + threadIdx.x) / OSQ_WAVE;
    const int64_t nwaves = static_cast<int64_t>(gridDim.x) * (kLinThreads / OSQ_WAVE);
    for (int64_t r = wave; r < rows; r += nwaves) {
        const int64_t c = channels == 1 ? 0 : r;
        const QParams p = effective_params(scale_p[c], load_zp(zp_p, zp_type, c), mode, g);
        unsigned int rej = 0;
        const float4* wr = reinterpret_cast<const float4*>(w + r * cols);
        const int sum = kW4 ? encode_row_w4(wr, reinterpret_cast<unsigned int*>(codes + r * (cols / 2)), cols / 8, lane, p, qmin, qmax, rej)
                            : encode_row(wr, reinterpret_cast<unsigned int*>(codes + r * cols), cols / 4, lane, p, qmin, qmax, rej);
        const int nbad = wave_sum_i32(static_cast<int>(rej));
        if (lane == 0) {
            const bool ok = lin_zp_ok(p.zp, qmin, qmax);
            colsum[r] = sum;
            scale_eff[r] = p.scale;
            zw[r] = ok ? static_cast<int>(p.zp - qmin) - (kW4 ? 0 : 128) : 0;
            if (!ok || nbad) *bad = 1;                // every writer writes the same word
        }
    }
}

struct LinArgs {
    const uint8_t *xc, *wc;            // a [M, K], b [N, K] (packed: [N, K / 2])
    const int32_t *xrs, *wcs, *wz, *wbad;
    const float *ws, *bias;
    float* out;                        // [M, N]
    int M, N, K;
    int vec;                           // N % 4 == 0 and out, wcs, wz, ws, bias 16-byte aligned: 16-byte epilogue accesses
    DecQuant xq;
    // the kCodes epilogue only (out is null): codes [M, N] bytes, rowsum [M] zeroed, flags [M] and tickets [row tiles] zeroed
    uint8_t* codes;
    int32_t *rowsum, *flags, *tickets;
    DecQuant oq;                       // the quantizer of the NEXT linear's input
    int gelu;                          // 1: gelu_erf between the linear's word and the code
};

// zx and s_x of the launch; false (uniform): the launch writes NaN everywhere
__device__ __forceinline__ bool lin_prologue(const LinArgs& a, int& zx, float& sx) {
    const QParams xp = dec_params(a.xq);
    sx = xp.scale;
    const bool ok = lin_zp_ok(xp.zp, a.xq.qmin, a.xq.qmax) && *a.wbad == 0;
    zx = ok ? static_cast<int>(xp.zp - a.xq.qmin) - 128 : 0;
    return ok;
}

__device__ __forceinline__ void lin_fill_nan(const LinArgs& a, int m0, int n0, int tm, int tn) {
    const float nan = __builtin_nanf("");
    for (int i = threadIdx.x; i < tm * tn; i += kLinThreads) {
        const int r = m0 + i / tn, c = n0 + i % tn;
        if (r < a.M && c < a.N) a.out[static_cast<int64_t>(r) * a.N + c] = nan;
    }
}

__device__ __forceinline__ float lin_value(int acc, int rs, int cs, int zw, int zx, int kzx, float sx, float sw, bool has_bias,
                                           float bias, bool row_nan) {
    const int n = acc - zw * rs - zx * cs + kzx * zw;
    float y = static_cast<float>(n) * (sx * sw);
    if (has_bias) y = y + bias;
    return row_nan ? __builtin_nanf("") : y;
}

// the 16 registers of one 32 x 32 result: row `row` of x, channels c0 + (r & 3) + 8 * (r >> 2) + 4 * half
__device__ __forceinline__ void lin_store_tile(const LinArgs& a, const i32x16& acc, int row, int c0, int half, int zx, float sx) {
    if (row >= a.M) return;
    const int rs_raw = a.xrs[row];
    const bool row_nan = rs_raw == kLinNoRow;
    const int rs = row_nan ? 0 : rs_raw, kzx = a.K * zx;
    const bool has_bias = a.bias != nullptr;
    float* orow = a.out + static_cast<int64_t>(row) * a.N;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int c = c0 + 8 * g + 4 * half;
        if (c >= a.N) continue;
        if (a.vec) {
            const i32x4 cs = *reinterpret_cast<const i32x4*>(a.wcs + c), zw = *reinterpret_cast<const i32x4*>(a.wz + c);
            const float4 sw = *reinterpret_cast<const float4*>(a.ws + c);
            const float4 b = has_bias ? *reinterpret_cast<const float4*>(a.bias + c) : make_float4(0.f, 0.f, 0.f, 0.f);
            *reinterpret_cast<float4*>(orow + c) =
                make_float4(lin_value(acc[4 * g + 0], rs, cs.x, zw.x, zx, kzx, sx, sw.x, has_bias, b.x, row_nan),
                            lin_value(acc[4 * g + 1], rs, cs.y, zw.y, zx, kzx, sx, sw.y, has_bias, b.y, row_nan),
                            lin_value(acc[4 * g + 2], rs, cs.z, zw.z, zx, kzx, sx, sw.z, has_bias, b.z, row_nan),
                            lin_value(acc[4 * g + 3], rs, cs.w, zw.w, zx, kzx, sx, sw.w, has_bias, b.w, row_nan));
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (c + e < a.N)
                    orow[c + e] = lin_value(acc[4 * g + e], rs, a.wcs[c + e], a.wz[c + e], zx, kzx, sx, a.ws[c + e], has_bias,
                                            has_bias ? a.bias[c + e] : 0.f, row_nan);
        }
    }
}

// ---- the kCodes epilogue: the next linear's activation codes instead of out (header, "CODES FOR THE NEXT LINEAR") ----------

// out quantizer's parameters; false (uniform): its zero point is no integer in range, the launch is bad
__device__ __forceinline__ bool lin_out_params(const LinArgs& a, QParams& op) {
    op = dec_params(a.oq);
    return lin_zp_ok(op.zp, a.oq.qmin, a.oq.qmax);
}

// a bad launch: every row sum is kLinNoRow, written by the workgroups of the first channel tile; nobody adds
__device__ __forceinline__ void lin_poison_rows(const LinArgs& a, int m0, int tm, bool first_channel_tile) {
    if (!first_channel_tile) return;
    for (int r = threadIdx.x; r < tm; r += kLinThreads)
        if (m0 + r < a.M) a.rowsum[m0 + r] = kLinNoRow;
}

// The 16 registers of one 32 x 32 result as this lane's 16 CONTIGUOUS code bytes of row `row`: channels c0 + 16 * half .. + 15.
// In the register map the lane owns 4 g .. 4 g + 3 -> channels 8 g + 4 half ..: words A0..A3 in half 0 and B0..B3 in half 1
// of a row whose 32 bytes are A0 B0 A1 B1 A2 B2 A3 B3.  Each lane sends the two words its partner (lane ^ 32) needs and keeps
// the two it needs itself: half 0 ends with A0 B0 A1 B1, half 1 with A2 B2 A3 B3.  Every lane of the wave calls (the exchange
// is wave-wide); a row beyond M or a granule beyond N gives zero words.  `rej`: elements of this lane without a code.
__device__ __forceinline__ i32x4 lin_code_granule(const LinArgs& a, const i32x16& acc, int row, int c0, int half, int zx, float sx,
                                                  const QParams& op, unsigned int& rej) {
    const bool live = row < a.M;
    const int rs_raw = a.xrs[min(row, a.M - 1)];
    const bool row_nan = rs_raw == kLinNoRow;
    const int rs = row_nan ? 0 : rs_raw, kzx = a.K * zx;
    const bool has_bias = a.bias != nullptr;
    unsigned int w[4], bad = 0;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int c = c0 + 8 * g + 4 * half;           // N % 16 == 0: c < N takes c .. c + 3 with it
        w[g] = 0;
        if (!live || c >= a.N) continue;
        i32x4 cs, zw;
        float sw[4], b[4] = {0.f, 0.f, 0.f, 0.f};
        if (a.vec) {
            cs = *reinterpret_cast<const i32x4*>(a.wcs + c);
            zw = *reinterpret_cast<const i32x4*>(a.wz + c);
            const float4 s4 = *reinterpret_cast<const float4*>(a.ws + c);
            sw[0] = s4.x, sw[1] = s4.y, sw[2] = s4.z, sw[3] = s4.w;
            if (has_bias) {
                const float4 b4 = *reinterpret_cast<const float4*>(a.bias + c);
                b[0] = b4.x, b[1] = b4.y, b[2] = b4.z, b[3] = b4.w;
            }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                cs[e] = a.wcs[c + e];
                zw[e] = a.wz[c + e];
                sw[e] = a.ws[c + e];
                if (has_bias) b[e] = a.bias[c + e];
            }
        }
        unsigned int u[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float v = lin_value(acc[4 * g + e], rs, cs[e], zw[e], zx, kzx, sx, sw[e], has_bias, b[e], row_nan);
            u[e] = code_of(a.gelu ? gelu_erf(v) : v, op, a.oq.qmin, a.oq.qmax, bad);
        }
        w[g] = (u[0] | (u[1] << 8) | (u[2] << 16) | (u[3] << 24)) ^ 0x80808080u;
    }
    rej += bad;
    const int r0 = __shfl_xor(static_cast<int>(half ? w[0] : w[2]), 32, OSQ_WAVE);
    const int r1 = __shfl_xor(static_cast<int>(half ? w[1] : w[3]), 32, OSQ_WAVE);
    return half ? i32x4{r0, static_cast<int>(w[2]), r1, static_cast<int>(w[3])}
                : i32x4{static_cast<int>(w[0]), r0, static_cast<int>(w[1]), r1};
}

// sum of the 16 bytes of a granule as int8
__device__ __forceinline__ int lin_granule_sum(const i32x4& v) {
    int s = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int b = 0; b < 4; ++b) s += static_cast<int>(static_cast<int8_t>(static_cast<unsigned int>(v[e]) >> (8 * b)));
    return s;
}

// The end of a kCodes workgroup, after its adds and flags: take a ticket of row tile `tile`; whoever draws the last of `total`
// sees every other workgroup's adds and flags (their fence came before their ticket) and overwrites the flagged rows, and the
// rows that came in without codes, with kLinNoRow.  Nobody waits.  `s_last`: one word of LDS.
__device__ __forceinline__ void lin_finish_rows(const LinArgs& a, int tile, int total, int m0, int tm, int* s_last) {
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) *s_last = atomicAdd(a.tickets + tile, 1) == total - 1;
    __syncthreads();
    if (!*s_last) return;
    __threadfence();
    for (int r = threadIdx.x; r < tm; r += kLinThreads) {
        const int row = m0 + r;
        if (row < a.M && (a.xrs[row] == kLinNoRow || __hip_atomic_load(a.flags + row, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)))
            atomicExch(a.rowsum + row, kLinNoRow);
    }
}

// a row's flag: some element of it has no code (a row that came in without codes needs none: everyone reads that from xrs)
__device__ __forceinline__ void lin_flag_row(const LinArgs& a, int row, unsigned int rej) {
    if (rej && row < a.M && a.xrs[row] != kLinNoRow) atomicOr(a.flags + row, 1);
}

// The rows kernels' end, wave 0 alone (the workgroup's other waves have left: no barrier from here on): a lane's granule goes
// straight to memory -- a workgroup owns 32 bytes of a row, two lanes' worth, there is nothing to gather -- the row's partial
// sum is the two lanes', one add per row.
__device__ __forceinline__ void lin_codes_rows(const LinArgs& a, const i32x16& acc, int l31, int n0, int half, int zx, float sx,
                                               const QParams& op) {
    unsigned int rej = 0;
    const i32x4 v = lin_code_granule(a, acc, l31, n0, half, zx, sx, op, rej);
    const int c = n0 + 16 * half;
    const bool live = l31 < a.M && c < a.N;
    if (live) *reinterpret_cast<i32x4*>(a.codes + static_cast<int64_t>(l31) * a.N + c) = v;
    int sum = lin_granule_sum(v);                     // zero words where the granule is not there
    sum += __shfl_xor(sum, 32, OSQ_WAVE);
    if (half == 0 && l31 < a.M && a.xrs[l31] != kLinNoRow) atomicAdd(a.rowsum + l31, sum);
    lin_flag_row(a, l31, rej);
    __threadfence();                                  // the wave's adds and flags, then lane 0's ticket
    int last = 0;
    if (threadIdx.x == 0) last = atomicAdd(a.tickets, 1) == static_cast<int>(gridDim.x) - 1;
    if (!__shfl(last, 0, OSQ_WAVE)) return;
    __threadfence();
    if (threadIdx.x < a.M && (a.xrs[threadIdx.x] == kLinNoRow ||
                              __hip_atomic_load(a.flags + threadIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)))
        atomicExch(a.rowsum + threadIdx.x, kLinNoRow);
}

constexpr int kLinCodePitch = kLinTile + 16;          // bytes of a staged row of codes: 9 granules, see linear_int_kernel

// kW4: a.wc is packed [N, K / 2]; a granule of W is in flight as its 8 packed bytes (gw[u].x, .y) and unpacked at the stash.
// kCodes: the epilogue writes the next linear's codes and row sums instead of out.
template <bool kW4, bool kCodes = false>
__global__ __launch_bounds__(kLinThreads) void linear_int_kernel(LinArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t s_w[2][kLinTile * kLinPitch];
    __shared__ __attribute__((aligned(16))) uint8_t s_x[2][kLinTile * kLinPitch];
    const int lane = threadIdx.x & (OSQ_WAVE - 1), w = threadIdx.x / OSQ_WAVE;
    const int l31 = lane & 31, half = lane >> 5;
    const int mtiles = (a.M + kLinTile - 1) / kLinTile;
    const int m0 = static_cast<int>(blockIdx.x % mtiles) * kLinTile, n0 = static_cast<int>(blockIdx.x / mtiles) * kLinTile;
    int zx;
    float sx;
    QParams op{1.f, 0.f};
    bool ok = lin_prologue(a, zx, sx);
    if constexpr (kCodes) ok = lin_out_params(a, op) && ok;      // both repairs ride, whatever the other says
    if (!ok) {                                        // uniform
        if constexpr (kCodes) lin_poison_rows(a, m0, kLinTile, n0 == 0);
        else lin_fill_nan(a, m0, n0, kLinTile, kLinTile);
        return;
    }
    const int wm = w & 1, wn = w >> 1;                // this wave's 64 x 64 part

    // a thread's two 16-byte granules of each tile: granule threadIdx.x + 256 u is row idx / 4, bytes 16 (idx % 4) ..
    osq_v4u32 gw[2], gx[2];
    const auto load = [&](int k0) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int idx = threadIdx.x + kLinThreads * u, row = idx >> 2, k = k0 + 16 * (idx & 3);
            const osq_v4u32 zero = {0u, 0u, 0u, 0u};
            gw[u] = gx[u] = zero;
            if (k < a.K) {
                const int64_t wrow = min(n0 + row, a.N - 1);
                if constexpr (kW4) {
                    const i32x2 p = *reinterpret_cast<const i32x2*>(a.wc + wrow * (a.K / 2) + k / 2);
                    gw[u].x = static_cast<unsigned int>(p.x);
                    gw[u].y = static_cast<unsigned int>(p.y);
                } else {
                    gw[u] = *reinterpret_cast<const osq_v4u32*>(a.wc + wrow * a.K + k);
                }
                gx[u] = *reinterpret_cast<const osq_v4u32*>(a.xc + static_cast<int64_t>(min(m0 + row, a.M - 1)) * a.K + k);
            }
        }
    };
    const auto stash = [&](int buf) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int idx = threadIdx.x + kLinThreads * u, at = (idx >> 2) * kLinPitch + 16 * (idx & 3);
            if constexpr (kW4) {
                *reinterpret_cast<i32x4*>(&s_w[buf][at]) = unpack_w4(static_cast<int>(gw[u].x), static_cast<int>(gw[u].y));
            } else {
                *reinterpret_cast<osq_v4u32*>(&s_w[buf][at]) = gw[u];
            }
            *reinterpret_cast<osq_v4u32*>(&s_x[buf][at]) = gx[u];
        }
    };

    i32x16 acc[2][2];                                 // [x part][channel part]
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0;

    load(0);
    stash(0);
    __syncthreads();
    const int steps = (a.K + kLinKStep - 1) / kLinKStep;
    for (int s = 0; s < steps; ++s) {
        const int buf = s & 1, k0 = s * kLinKStep;
        if (s + 1 < steps) load(k0 + kLinKStep);      // in flight during this step's products
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            if (k0 + 32 * ks >= a.K) break;           // uniform: the half step beyond K is zeros
            i32x4 fw[2], fx[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                fw[t] = *reinterpret_cast<const i32x4*>(&s_w[buf][(64 * wn + 32 * t + l31) * kLinPitch + 32 * ks + 16 * half]);
                fx[t] = *reinterpret_cast<const i32x4*>(&s_x[buf][(64 * wm + 32 * t + l31) * kLinPitch + 32 * ks + 16 * half]);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fw[j], fx[i], acc[i][j], 0, 0, 0);
        }
        if (s + 1 < steps) stash(buf ^ 1);            // last read in step s - 1: every wave has passed that step's barrier
        __syncthreads();
    }

    if constexpr (!kCodes) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
                lin_store_tile(a, acc[i][j], m0 + 64 * wm + 32 * i + l31, n0 + 64 * wn + 32 * j, half, zx, sx);
    } else {
        // The operand LDS is free (every wave is past the last step's barrier): the tile's 128 x 128 code bytes are staged in
        // s_w at a pitch of 128 + 16 bytes, so that a row leaves as whole 128-byte lines.  Both sides move 16 bytes per lane, 16
        // lanes to a phase over 16 groups of four banks; a granule at (row, g) lies in group (9 row + g) mod 16.  Staging: the
        // 16 lanes of a phase hold 16 consecutive rows at one g -- 9 is odd, 16 groups.  Read-out: a phase takes the 8 granules
        // of row R and of row R + 8 -- groups 9 R + 0 .. 7 and 9 R + 72 + 0 .. 7 = 9 R + 8 .. 15 -- and 8 consecutive lanes write
        // one 128-byte line of a row to memory.
        uint8_t* s_c = &s_w[0][0];                    // 128 x 144 B = 18 KiB of its 20
        int* s_last = reinterpret_cast<int*>(&s_x[0][0]);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int rl = 64 * wm + 32 * i + l31;
            unsigned int rej = 0;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int cl = 64 * wn + 32 * j;
                *reinterpret_cast<i32x4*>(&s_c[rl * kLinCodePitch + cl + 16 * half]) =
                    lin_code_granule(a, acc[i][j], m0 + rl, n0 + cl, half, zx, sx, op, rej);
            }
            lin_flag_row(a, m0 + rl, rej);
        }
        __syncthreads();
        const int g = threadIdx.x & 7, c = n0 + 16 * g;
#pragma unroll
        for (int p = 0; p < kLinTile / 32; ++p) {
            const int rl = 32 * p + 16 * (threadIdx.x >> 7) + 8 * ((threadIdx.x >> 3) & 1) + ((threadIdx.x >> 4) & 7);
            const int row = m0 + rl;
            const bool live = row < a.M && c < a.N;
            i32x4 v = {0, 0, 0, 0};
            if (live) {
                v = *reinterpret_cast<const i32x4*>(&s_c[rl * kLinCodePitch + 16 * g]);
                *reinterpret_cast<i32x4*>(a.codes + static_cast<int64_t>(row) * a.N + c) = v;
            }
            int sum = lin_granule_sum(v);             // the row's 8 granules are 8 consecutive lanes
            sum += __shfl_xor(sum, 1, OSQ_WAVE);
            sum += __shfl_xor(sum, 2, OSQ_WAVE);
            sum += __shfl_xor(sum, 4, OSQ_WAVE);
            if (g == 0 && row < a.M && a.xrs[row] != kLinNoRow) atomicAdd(a.rowsum + row, sum);
        }
        lin_finish_rows(a, m0 / kLinTile, (a.N + kLinTile - 1) / kLinTile, m0, kLinTile, s_last);
    }
}

template <bool kCodes>
__global__ __launch_bounds__(kLinThreads) void linear_int_rows_kernel(LinArgs a) {
    constexpr int kWaves = kLinThreads / OSQ_WAVE;
    __shared__ int s_part[kWaves - 1][16][OSQ_WAVE];
    const int lane = threadIdx.x & (OSQ_WAVE - 1), w = threadIdx.x / OSQ_WAVE;
    const int l31 = lane & 31, half = lane >> 5;
    const int n0 = static_cast<int>(blockIdx.x) * 32;
    int zx;
    float sx;
    QParams op{1.f, 0.f};
    bool ok = lin_prologue(a, zx, sx);
    if constexpr (kCodes) ok = lin_out_params(a, op) && ok;
    if (!ok) {                                        // uniform
        if constexpr (kCodes) lin_poison_rows(a, 0, kLinRowsM, n0 == 0);
        else lin_fill_nan(a, 0, n0, kLinRowsM, 32);
        return;
    }
    const uint8_t* wrow = a.wc + static_cast<int64_t>(min(n0 + l31, a.N - 1)) * a.K + 16 * half;
    const uint8_t* xrow = a.xc + static_cast<int64_t>(min(l31, a.M - 1)) * a.K + 16 * half;
    i32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0;
    for (int k0 = kLinRowsChunk * w; k0 < a.K; k0 += kLinRowsChunk * kWaves) {
        i32x4 fw[4], fx[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {                 // all eight loads leave before the first product
            const i32x4 zero = {0, 0, 0, 0};
            fw[s] = fx[s] = zero;
            if (k0 + 32 * s + 16 * half < a.K) {
                fw[s] = *reinterpret_cast<const i32x4*>(wrow + k0 + 32 * s);
                fx[s] = *reinterpret_cast<const i32x4*>(xrow + k0 + 32 * s);
            }
        }
#pragma unroll
        for (int s = 0; s < 4; ++s)
            if (k0 + 32 * s < a.K) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(fw[s], fx[s], acc, 0, 0, 0);      // uniform
    }
    if (w) {
#pragma unroll
        for (int r = 0; r < 16; ++r) s_part[w - 1][r][lane] = acc[r];
    }
    __syncthreads();
    if (w) return;
#pragma unroll
    for (int v = 0; v < kWaves - 1; ++v)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] += s_part[v][r][lane];
    if constexpr (kCodes) lin_codes_rows(a, acc, l31, n0, half, zx, sx, op);
    else lin_store_tile(a, acc, l31, n0, half, zx, sx);
}

// One chunk of a lane of linear_int_rows_kernel_w4: per 64-k step its channel's 16 packed bytes (32 k) and its x row's 2 x 16.
struct W4Chunk {
    i32x4 w[2], x[2][2];
};

template <bool kCodes>
__global__ __launch_bounds__(kLinThreads) void linear_int_rows_kernel_w4(LinArgs a) {
    constexpr int kWaves = kLinThreads / OSQ_WAVE;
    __shared__ int s_part[kWaves - 1][16][OSQ_WAVE];
    const int lane = threadIdx.x & (OSQ_WAVE - 1);
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x / OSQ_WAVE);      // a scalar: the K loop's branches are the wave's
    const int l31 = lane & 31, half = lane >> 5;
    const int n0 = static_cast<int>(blockIdx.x) * 32;
    int zx;
    float sx;
    QParams op{1.f, 0.f};
    bool ok = lin_prologue(a, zx, sx);
    if constexpr (kCodes) ok = lin_out_params(a, op) && ok;
    if (!ok) {                                        // uniform
        if constexpr (kCodes) lin_poison_rows(a, 0, kLinRowsM, n0 == 0);
        else lin_fill_nan(a, 0, n0, kLinRowsM, 32);
        return;
    }
    const uint8_t* wrow = a.wc + static_cast<int64_t>(min(n0 + l31, a.N - 1)) * (a.K / 2);
    const uint8_t* xrow = a.xc + static_cast<int64_t>(min(l31, a.M - 1)) * a.K;

    // A whole chunk (k0 + 128 <= K): six loads and no branch, so the wait before a product counts exactly the loads behind it.
    const auto load_whole = [&](int k0, W4Chunk& c) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int k = k0 + 64 * s + 32 * half;
            c.w[s] = *reinterpret_cast<const i32x4_a8*>(wrow + k / 2);
            c.x[s][0] = *reinterpret_cast<const i32x4*>(xrow + k);
            c.x[s][1] = *reinterpret_cast<const i32x4*>(xrow + k + 16);
        }
    };
    // K's last, partial chunk (one wave has it): nothing is read at or beyond K, what is not read is zero.
    const auto load_part = [&](int k0, W4Chunk& c) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const i32x4 zero = {0, 0, 0, 0};
            c.w[s] = c.x[s][0] = c.x[s][1] = zero;
            const int k = k0 + 64 * s + 32 * half, left = a.K - k;      // a multiple of 16
            if (left >= 32) {
                c.w[s] = *reinterpret_cast<const i32x4_a8*>(wrow + k / 2);
                c.x[s][0] = *reinterpret_cast<const i32x4*>(xrow + k);
                c.x[s][1] = *reinterpret_cast<const i32x4*>(xrow + k + 16);
            } else if (left == 16) {                  // the row's last 8 packed bytes
                const i32x2 p = *reinterpret_cast<const i32x2*>(wrow + k / 2);
                c.w[s].x = p.x;
                c.w[s].y = p.y;
                c.x[s][0] = *reinterpret_cast<const i32x4*>(xrow + k);
            }
        }
    };

    i32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0;
    // the products of a chunk of which `left` k exist (uniform; 128: folded)
    const auto products = [&](const W4Chunk& c, int left) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            if (64 * s >= left) break;
            // k .. + 15 and k + 16 .. + 31 of this half's 32
            const i32x4 lo = unpack_w4(c.w[s].x, c.w[s].y), hi = unpack_w4(c.w[s].z, c.w[s].w);
            acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(lo, c.x[s][0], acc, 0, 0, 0);
            if (64 * s + 16 < left) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(hi, c.x[s][1], acc, 0, 0, 0);
        }
    };
    // This wave's whole chunks are k0 + kRound * i, i < n; two register sets take them in turn, each loaded while the other's
    // products run.
    constexpr int kRound = kLinW4Chunk * kWaves;
    const int k0 = kLinW4Chunk * w;
    const int n = a.K - k0 >= kLinW4Chunk ? (a.K - k0 - kLinW4Chunk) / kRound + 1 : 0;
    W4Chunk ca, cb;
    if (n) {
        load_whole(k0, ca);
        int i = 1;
        for (; i + 1 < n; i += 2) {
            load_whole(k0 + kRound * i, cb);
            products(ca, kLinW4Chunk);
            load_whole(k0 + kRound * (i + 1), ca);
            products(cb, kLinW4Chunk);
        }
        if (i < n) {                                  // K = 1024: every wave's two chunks
            load_whole(k0 + kRound * i, cb);
            products(ca, kLinW4Chunk);
            products(cb, kLinW4Chunk);
        } else {
            products(ca, kLinW4Chunk);
        }
    }
    if (k0 + kRound * n < a.K) {
        load_part(k0 + kRound * n, ca);
        products(ca, a.K - (k0 + kRound * n));
    }
    if (w) {
#pragma unroll
        for (int r = 0; r < 16; ++r) s_part[w - 1][r][lane] = acc[r];
    }
    __syncthreads();
    if (w) return;
#pragma unroll
    for (int v = 0; v < kWaves - 1; ++v)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] += s_part[v][r][lane];
    if constexpr (kCodes) lin_codes_rows(a, acc, l31, n0, half, zx, sx, op);
    else lin_store_tile(a, acc, l31, n0, half, zx, sx);
}

static bool lin_quant_ok(int mode, int quant_min, int quant_max) {
    return dec_mode_ok(mode) && quant_min <= quant_max && static_cast<int64_t>(quant_max) - quant_min <= 255;
}

static bool lin_k_ok(int64_t cols) { return cols >= 16 && cols <= kLinMaxK && cols % 16 == 0; }

}  // namespace osq

using namespace osq;

extern "C" int osq_activation_codes(const float* x, int64_t rows, int64_t cols, int64_t row_stride, uint8_t* codes,
                                    int32_t* rowsum, float* x_scale, void* x_zero_point, int x_zp_type, int x_mode,
                                    float x_grad_factor, int x_quant_min, int x_quant_max, osq_stream stream) {
    OSQ_REQUIRE(rows >= 0 && rows <= INT32_MAX, "activation_codes: bad row count");
    OSQ_REQUIRE(lin_k_ok(cols), "activation_codes: the row length must be a multiple of 16 in [16, 16384]");
    OSQ_REQUIRE(x_scale && x_zero_point, "activation_codes: null scale or zero_point");
    OSQ_REQUIRE(x_zp_type == OSQ_ZP_INT32 || x_zp_type == OSQ_ZP_FLOAT32, "activation_codes: bad zp_type");
    OSQ_REQUIRE(lin_quant_ok(x_mode, x_quant_min, x_quant_max), "activation_codes: bad mode, or more than 256 codes");
    if (rows == 0) return OSQ_OK;
    OSQ_REQUIRE(x && codes && rowsum, "activation_codes: null tensor");
    OSQ_REQUIRE(row_stride >= cols && row_stride % 4 == 0 && aligned16(x), "activation_codes: x rows are not 16-byte aligned");
    OSQ_REQUIRE((reinterpret_cast<uintptr_t>(codes) & 3u) == 0 && (reinterpret_cast<uintptr_t>(rowsum) & 3u) == 0,
                "activation_codes: codes / rowsum not 4-byte aligned");
    const int grid = grid_for(rows, kLinThreads / OSQ_WAVE, kMaxBlocks * 2);
    hipLaunchKernelGGL(activation_codes_kernel, dim3(grid), dim3(kLinThreads), 0, static_cast<hipStream_t>(stream), x, row_stride,
                       codes, rowsum, rows, static_cast<int>(cols), OSQ_DEC_QUANT(x));
    return check_launch("activation_codes");
}

// osq_weight_codes_sums and its packed twin
static int lin_weight_codes(bool w4, const float* w, int64_t rows, int64_t cols, int64_t channels, uint8_t* codes,
                            int32_t* colsum, float* scale_eff, int32_t* zw, int32_t* bad, const float* scale,
                            const void* zero_point, int zp_type, int mode, float grad_factor, int quant_min,
                            int quant_max, osq_stream stream) {
    OSQ_REQUIRE(rows >= 0 && rows <= INT32_MAX, "weight_codes_sums: bad row count");
    OSQ_REQUIRE(lin_k_ok(cols), "weight_codes_sums: the row length must be a multiple of 16 in [16, 16384]");
    OSQ_REQUIRE(channels == 1 || channels == rows, "weight_codes_sums: one scale, or one per row");
    OSQ_REQUIRE(scale && zero_point, "weight_codes_sums: null scale or zero_point");
    OSQ_REQUIRE(zp_type == OSQ_ZP_INT32 || zp_type == OSQ_ZP_FLOAT32, "weight_codes_sums: bad zp_type");
    OSQ_REQUIRE(mode >= OSQ_PARAM_FIXED && mode <= OSQ_PARAM_LSQPLUS, "weight_codes_sums: bad mode");
    OSQ_REQUIRE(quant_min <= quant_max && static_cast<int64_t>(quant_max) - quant_min <= 255, "weight_codes_sums: more than 256 codes");
    OSQ_REQUIRE(!w4 || quant_max - quant_min <= 15, "weight_codes_sums_w4: more than 16 codes");
    if (rows == 0) return OSQ_OK;
    OSQ_REQUIRE(w && codes && colsum && scale_eff && zw && bad, "weight_codes_sums: null tensor");
    OSQ_REQUIRE(aligned16(w) && (reinterpret_cast<uintptr_t>(codes) & 3u) == 0, "weight_codes_sums: w not 16-byte or codes not 4-byte aligned");
    const int grid = grid_for(rows, kLinThreads / OSQ_WAVE, kMaxBlocks * 2);
    hipLaunchKernelGGL(w4 ? weight_codes_kernel<true> : weight_codes_kernel<false>, dim3(grid), dim3(kLinThreads), 0,
                       static_cast<hipStream_t>(stream), w, codes, colsum, scale_eff, zw, bad, rows, channels, static_cast<int>(cols),
                       scale, zero_point, zp_type, mode, grad_factor, static_cast<float>(quant_min), static_cast<float>(quant_max));
    return check_launch(w4 ? "weight_codes_sums_w4" : "weight_codes_sums");
}

extern "C" int osq_weight_codes_sums(const float* w, int64_t rows, int64_t cols, int64_t channels, uint8_t* codes,
                                     int32_t* colsum, float* scale_eff, int32_t* zw, int32_t* bad, const float* scale,
                                     const void* zero_point, int zp_type, int mode, float grad_factor, int quant_min,
                                     int quant_max, osq_stream stream) {
    return lin_weight_codes(false, w, rows, cols, channels, codes, colsum, scale_eff, zw, bad, scale, zero_point, zp_type, mode,
                            grad_factor, quant_min, quant_max, stream);
}

extern "C" int osq_weight_codes_sums_w4(const float* w, int64_t rows, int64_t cols, int64_t channels, uint8_t* codes,
                                        int32_t* colsum, float* scale_eff, int32_t* zw, int32_t* bad, const float* scale,
                                        const void* zero_point, int zp_type, int mode, float grad_factor, int quant_min,
                                        int quant_max, osq_stream stream) {
    return lin_weight_codes(true, w, rows, cols, channels, codes, colsum, scale_eff, zw, bad, scale, zero_point, zp_type, mode,
                            grad_factor, quant_min, quant_max, stream);
}

// what osq_linear_int_codes writes instead of out, and how: null for osq_linear_int and its packed twin
struct LinCodesOut {
    uint8_t* codes;
    int32_t *rowsum, *scratch;
    DecQuant oq;
    int gelu;
};

// osq_linear_int, its packed twin and osq_linear_int_codes: w_codes [channels, cols] or [channels, cols / 2]
static int lin_launch(bool w4, const uint8_t* x_codes, const int32_t* x_rowsum, const uint8_t* w_codes, const int32_t* w_colsum,
                      const float* w_scale, const int32_t* w_zw, const int32_t* w_bad, const float* bias, float* out,
                      int64_t rows, int64_t channels, int64_t cols, float* x_scale, void* x_zero_point, int x_zp_type,
                      int x_mode, float x_grad_factor, int x_quant_min, int x_quant_max, osq_stream stream,
                      const LinCodesOut* co = nullptr) {
    OSQ_REQUIRE(rows >= 0 && rows <= INT32_MAX && channels >= 0 && channels <= INT32_MAX, "linear_int: bad shape");
    OSQ_REQUIRE(lin_k_ok(cols), "linear_int: K must be a multiple of 16 in [16, 16384]");
    OSQ_REQUIRE(x_scale && x_zero_point, "linear_int: null scale or zero_point");
    OSQ_REQUIRE(x_zp_type == OSQ_ZP_INT32 || x_zp_type == OSQ_ZP_FLOAT32, "linear_int: bad zp_type");
    OSQ_REQUIRE(lin_quant_ok(x_mode, x_quant_min, x_quant_max), "linear_int: bad mode, or more than 256 codes");
    OSQ_REQUIRE(!co || channels == 0 || lin_k_ok(channels), "linear_int_codes: N must be a multiple of 16 in [16, 16384]");
    if (rows == 0 || channels == 0) return OSQ_OK;
    OSQ_REQUIRE(x_codes && x_rowsum && w_codes && w_colsum && w_scale && w_zw && w_bad && (co ? co->codes && co->rowsum && co->scratch : out != nullptr),
                "linear_int: null tensor");
    OSQ_REQUIRE(aligned16(x_codes) && aligned16(w_codes) && (!co || aligned16(co->codes)), "linear_int: codes not 16-byte aligned");
    OSQ_REQUIRE(((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(bias) | reinterpret_cast<uintptr_t>(x_rowsum) |
                  reinterpret_cast<uintptr_t>(w_colsum) | reinterpret_cast<uintptr_t>(w_scale) | reinterpret_cast<uintptr_t>(w_zw) |
                  reinterpret_cast<uintptr_t>(co ? co->rowsum : nullptr) | reinterpret_cast<uintptr_t>(co ? co->scratch : nullptr)) & 3u) == 0,
                "linear_int: a tensor is not 4-byte aligned");
    const int vec = channels % 4 == 0 && aligned16(out) && aligned16(w_colsum) && aligned16(w_scale) && aligned16(w_zw) && aligned16(bias);
    LinArgs a{x_codes, w_codes, x_rowsum, w_colsum, w_zw, w_bad, w_scale, bias, out, static_cast<int>(rows),
              static_cast<int>(channels), static_cast<int>(cols), vec, OSQ_DEC_QUANT(x)};
    if (co) {                                         // scratch: a flag per row, then a ticket per row tile
        a.codes = co->codes;
        a.rowsum = co->rowsum;
        a.flags = co->scratch;
        a.tickets = co->scratch + rows;
        a.oq = co->oq;
        a.gelu = co->gelu;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (rows <= kLinRowsM) {
        const auto kernel = co ? (w4 ? linear_int_rows_kernel_w4<true> : linear_int_rows_kernel<true>)
                               : (w4 ? linear_int_rows_kernel_w4<false> : linear_int_rows_kernel<false>);
        hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>((channels + 31) / 32)), dim3(kLinThreads), 0, st, a);
    } else {
        const int64_t blocks = ((rows + kLinTile - 1) / kLinTile) * ((channels + kLinTile - 1) / kLinTile);
        OSQ_REQUIRE(blocks <= INT32_MAX, "linear_int: too many tiles");
        const auto kernel = co ? (w4 ? linear_int_kernel<true, true> : linear_int_kernel<false, true>)
                               : (w4 ? linear_int_kernel<true, false> : linear_int_kernel<false, false>);
        hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(blocks)), dim3(kLinThreads), 0, st, a);
    }
    return check_launch(co ? "linear_int_codes" : w4 ? "linear_int_w4" : "linear_int");
}

extern "C" int osq_linear_int(const uint8_t* x_codes, const int32_t* x_rowsum, const uint8_t* w_codes, const int32_t* w_colsum,
                              const float* w_scale, const int32_t* w_zw, const int32_t* w_bad, const float* bias, float* out,
                              int64_t rows, int64_t channels, int64_t cols, float* x_scale, void* x_zero_point, int x_zp_type,
                              int x_mode, float x_grad_factor, int x_quant_min, int x_quant_max, osq_stream stream) {
    return lin_launch(false, x_codes, x_rowsum, w_codes, w_colsum, w_scale, w_zw, w_bad, bias, out, rows, channels, cols, x_scale,
                      x_zero_point, x_zp_type, x_mode, x_grad_factor, x_quant_min, x_quant_max, stream);
}

extern "C" int osq_linear_int_w4(const uint8_t* x_codes, const int32_t* x_rowsum, const uint8_t* w_codes, const int32_t* w_colsum,
                                 const float* w_scale, const int32_t* w_zw, const int32_t* w_bad, const float* bias, float* out,
                                 int64_t rows, int64_t channels, int64_t cols, float* x_scale, void* x_zero_point, int x_zp_type,
                                 int x_mode, float x_grad_factor, int x_quant_min, int x_quant_max, osq_stream stream) {
    return lin_launch(true, x_codes, x_rowsum, w_codes, w_colsum, w_scale, w_zw, w_bad, bias, out, rows, channels, cols, x_scale,
                      x_zero_point, x_zp_type, x_mode, x_grad_factor, x_quant_min, x_quant_max, stream);
}

extern "C" int osq_linear_int_codes(const uint8_t* x_codes, const int32_t* x_rowsum, const uint8_t* w_codes, const int32_t* w_colsum,
                                    const float* w_scale, const int32_t* w_zw, const int32_t* w_bad, const float* bias,
                                    uint8_t* codes, int32_t* rowsum, int32_t* scratch, int64_t rows, int64_t channels, int64_t cols,
                                    float* x_scale, void* x_zero_point, int x_zp_type, int x_mode, float x_grad_factor,
                                    int x_quant_min, int x_quant_max, float* out_scale, void* out_zero_point, int out_zp_type,
                                    int out_mode, float out_grad_factor, int out_quant_min, int out_quant_max, int activation,
                                    int w_bits, osq_stream stream) {
    OSQ_REQUIRE(w_bits == 8 || w_bits == 4, "linear_int_codes: w_bits is 8 or 4");
    OSQ_REQUIRE(activation == 0 || activation == 1, "linear_int_codes: activation is 0 (none) or 1 (exact GELU)");
    OSQ_REQUIRE(out_scale && out_zero_point, "linear_int_codes: null out scale or zero_point");
    OSQ_REQUIRE(out_zp_type == OSQ_ZP_INT32 || out_zp_type == OSQ_ZP_FLOAT32, "linear_int_codes: bad out zp_type");
    OSQ_REQUIRE(lin_quant_ok(out_mode, out_quant_min, out_quant_max), "linear_int_codes: bad out mode, or more than 256 codes");
    const LinCodesOut co{codes, rowsum, scratch, OSQ_DEC_QUANT(out), activation};
    return lin_launch(w_bits == 4, x_codes, x_rowsum, w_codes, w_colsum, w_scale, w_zw, w_bad, bias, nullptr, rows, channels, cols,
                      x_scale, x_zero_point, x_zp_type, x_mode, x_grad_factor, x_quant_min, x_quant_max, stream, &co);
}

/*
 * osq_hip.h -- C ABI of the MI355X (gfx950) fake-quant / observer hot path.
 *
 * The reference (wimh966/outlier_suppression) has no FFI: its hot path is a chain
 * of eager PyTorch ops inside quant_transformer/quantization/ (the .py files).  Each entry
 * point below replaces one such chain; the comment above it cites the reference
 * lines it stands in for.  INTEGRATION.md shows the ctypes stub a maintainer of
 * the reference would add to call them.
 *
 * Conventions
 *   - all tensor pointers are DEVICE pointers to fp32 unless stated otherwise;
 *   - `stream` is a hipStream_t passed as void*; every call is asynchronous on
 *     that stream and never synchronises with the host;
 *   - scalars that the reference reads with `.item()` (scale, zero_point,
 *     min_val, max_val) stay on the device and are passed by pointer;
 *   - return value: 0 on success, a negative osq_status otherwise;
 *     osq_last_error() returns a thread-local description;
 *   - `workspace` is caller-owned device scratch of at least
 *     osq_workspace_bytes() bytes, zero-initialised ONCE by the caller and then
 *     reused (kernels leave it zeroed where they need it zeroed).  One
 *     workspace per stream in flight.
 */
#ifndef OSQ_HIP_H
#define OSQ_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* osq_stream;

/* Bumped whenever a signature or the workspace layout changes; the Python host refuses a library whose
 * osq_abi_version() differs from the number it was written against (a stale libosq_hip.so must be rebuilt).
 * 5: the LSQ / LSQ+ backward takes its summation order as an argument (`lanes` / `sum_lanes`).
 * 8: osq_attention_softmax_fake_quant, OSQ_TIME_ATTENTION_SOFTMAX.
 * 10: osq_observe_flat / _channels, osq_token_minmax, osq_observe_tokens and osq_fake_quant_per_channel take `dtype` first;
 *     their separate 16-bit twins are gone.
 *     Added within 10 (no existing signature changed): osq_quantize_codes, osq_dequantize_codes, osq_dequantize_codes_multi,
 *     osq_decode_attention_fake_quant, osq_fake_quant_kv_append_codes, osq_decode_attention_codes,
 *     osq_fake_quant_kv_append_at, osq_fake_quant_kv_append_codes_at, osq_decode_attention_fake_quant_at,
 *     osq_decode_attention_codes_at, osq_beam_select_workspace_bytes, osq_beam_select, osq_beam_advance,
 *     osq_beam_select_at, osq_beam_advance_at, osq_greedy_advance_workspace_bytes, osq_greedy_advance,
 *     osq_greedy_advance_at, osq_sample_advance_workspace_bytes, osq_sample_advance, osq_sample_advance_at,
 *     osq_sample_uniforms, osq_sample_nucleus_workspace_bytes, osq_sample_nucleus, osq_sample_nucleus_at,
 *     osq_decode_attention_shared, osq_decode_attention_shared_codes, osq_sample_advance_group, osq_sample_advance_group_at,
 *     osq_sample_nucleus_group, osq_sample_nucleus_group_at, osq_sample_uniforms_group, osq_token_logprob_workspace_bytes,
 *     osq_token_logprob, osq_token_logprob_backward, osq_attention_fake_quant, osq_attention_fake_quant_int,
 *     osq_attention_fake_quant_shared, osq_attention_fake_quant_int_shared. */
#define OSQ_ABI_VERSION 10

typedef enum osq_status {
    OSQ_OK = 0,
    OSQ_ERR_INVALID_ARGUMENT = -1,
    OSQ_ERR_HIP = -2,
    OSQ_ERR_UNSUPPORTED = -3
} osq_status;

/* zero-point storage: FixedFakeQuantize keeps int32 (fake_quant.py:105),
 * LSQPlusFakeQuantize an fp32 Parameter (fake_quant.py:174). */
typedef enum osq_zp_type { OSQ_ZP_INT32 = 0, OSQ_ZP_FLOAT32 = 1 } osq_zp_type;

/* how the learnable variants post-process (scale, zero_point) before quantising */
typedef enum osq_param_mode {
    OSQ_PARAM_FIXED = 0,   /* util_quant.py:11-26   use as is                                  */
    OSQ_PARAM_LSQ = 1,     /* util_quant.py:29-45   scale <- grad_scale(scale, g)              */
    OSQ_PARAM_LSQPLUS = 2, /* util_quant.py:48-67   zp <- round_ste(zp); both <- grad_scale()  */
    OSQ_PARAM_MODE_MASK = 3,
    /* flag for the per-tensor forward entry points, OR-ed into `mode`: first repair the parameters
     * IN PLACE the way LSQFakeQuantize / LSQPlusFakeQuantize.forward do while their observer is off
     * (fake_quant.py:152-153, 188-191: scale.abs_(); scale.clamp_(min=finfo(float32).eps); LSQ+ also
     * zero_point.clamp_(quant_min, quant_max)), then quantise with the repaired values -- the same
     * result as osq_lsq_sanitize followed by the plain call, in one launch.  These entry points therefore take
     * `scale` / `zero_point` without a const qualifier; without the flag they only read them. */
    OSQ_PARAM_SANITIZE = 16,
    /* flag for osq_observe_tokens_fake_quant, OR-ed into `mode`: this call must not use the one-launch PERSISTENT form
     * (a grid of one workgroup per CU whose workgroups wait for each other: it needs the whole device) --
     * three ordinary launches instead, same results.  The per-call counterpart of osq_set_tuning("fused_step", 0). */
    OSQ_PARAM_NO_PERSISTENT = 32
} osq_param_mode;

/* running-statistic rule applied after a batch's (min, max) is known */
typedef enum osq_update_rule {
    OSQ_UPDATE_NONE = 0,     /* only report the batch's (min, max)                      */
    OSQ_UPDATE_RUNNING = 1,  /* observer.py:143-144  min_val = min(min_val, cur) ...    */
    OSQ_UPDATE_AVERAGE = 2   /* observer.py:194-202  (m*cnt + cur) / (cnt+1)            */
} osq_update_rule;

/* Element type of the `const void*` / `void*` tensor data of the entry points with a `dtype` argument; any other value
 * is rejected (-1) before anything else is looked at.  The 16-bit types are read as they lie and widened in registers
 * (the reference widens first: x_orig.to(min_val.dtype), observer.py:134; torch promotes bf16 / fp16 x with fp32
 * parameters to fp32): statistics, scale, zero point and fp32 outputs are word-equal to the fp32 call on x widened. */
typedef enum osq_dtype { OSQ_DTYPE_F32 = 0, OSQ_DTYPE_BF16 = 1, OSQ_DTYPE_F16 = 2 } osq_dtype;

/*
 * Logical [batch, tokens, feat_outer, feat_inner] view of an activation, i.e. the
 * tensor observer.py:72-80 builds with permute+reshape, described by element
 * strides instead of being materialised.  feat_inner is the fastest feature axis.
 *   [B,T,H]            seq_pos=1: outer=1,  inner=H
 *   [B,h,T,d]          seq_pos=2: outer=h,  inner=d
 *   [B,h,d,T]          seq_pos=3: outer=h,  inner=d  (strides of the view)
 *   [B,h,T,S]          seq_pos=2: outer=h,  inner=S
 */
typedef struct osq_token_view {
    int64_t batch, tokens, feat_outer, feat_inner;
    int64_t stride_batch, stride_token, stride_outer, stride_inner;
} osq_token_view;

const char* osq_last_error(void);
int         osq_abi_version(void);
size_t      osq_workspace_bytes(void);

/* Process-wide switches.  The RELEASE library accepts exactly these keys (atomic words, each read once per launch):
 *   summation order (picks WHICH rounding of a whole-tensor sum is returned):
 *     "mse_sum_order" 0 | 8 | 16 | 64   MSEFast losses: 8 / 16 = ATen's one-thread CPU order for 8- / 16-lane SIMD
 *                                       (oracle/aten_sum.py; bit-equal to the reference run on a one-thread host), 64 = double-doubles
 *                                       (order-independent; test mode), 0 = order-free.  The C library starts at 0; the Python
 *                                       host sets 8 when it loads the library (its default tier; OSQ_STRICT=0 keeps 0).  With the
 *                                       order set, per-tensor searches go through osq_msefast_tensor_evals_ordered (one launch per
 *                                       evaluation) or osq_msefast_ordered_multi_* (rounds).
 *     "mse_rows_order" 0 | 8 | 16       the per-channel rows' losses likewise (default 8).
 *     (The other whole-tensor sum of the path, the parameter gradients of the LSQ / LSQ+ backward, takes its order as an
 *     ARGUMENT: osq_lsq_backward_per_tensor_ordered(lanes), osq_lsq_backward_per_channel(sum_lanes).)
 *   path selection (results equal; tests drive every implementation through them):
 *     "fused_step" 0     osq_observe_tokens_fake_quant never uses its one-launch persistent form (per call:
 *                        OSQ_PARAM_NO_PERSISTENT in `mode`; per process also OSQ_FUSED_STEP=0 in the environment);
 *     "mse_resident" 0   per-tensor MSEFast searches of the order-free tier run one launch per evaluation instead of the
 *                        persistent resident form;
 *     "final_fast" 0     the token range finaliser without the two-workgroup kernel; "select_shortcut" 0: that kernel always
 *                        runs its register threshold pass;
 *     "mse_memo" 0       every loss evaluation of a per-tensor MSEFast search streams its tensor, also one whose (scale, zero
 *                        point) pair the search has evaluated before (default 1: answered from the search's memo, see
 *                        osq_msefast_tensor_stats; same results, iterates and nfev either way);
 *   robustness:
 *     "fused_spin_limit" / "mse_spin_limit" n   bound of the cross-workgroup waits of the two persistent launch families
 *                        (0 = the default, ~2 s; n > 0 = n - 1 polls, so 1 makes every wait give up at once: tests force the
 *                        time-out path).
 * Performance A/B knobs -- "fq_unroll", "fq_max_blocks", "fq_nt", "fq_headsplit", "stream_wt", "bwd_blocks", "bwd_order_chunks",
 * "ln_blocks", "attn_blocks", "obs_blocks", "tok_nt", "fused_gate", "fused_grid", "select_hint", "mse_round_groups" (8), "mse_lean" (1),
 * "mse_grid_all" -- are compile-time constants (the measured winners) in the release library, which answers
 * OSQ_ERR_INVALID_ARGUMENT for them; only the -DOSQ_TUNABLE development build (`make dbg`: libosq_hip_dbg.so) keeps them as
 * variables.  osq_build_flags(): bit 0 = that build, bit 1 = phase timestamps compiled in (-DOSQ_FINAL_TIMING). */
#define OSQ_BUILD_TUNABLE 1
#define OSQ_BUILD_FINAL_TIMING 2
int osq_build_flags(void);
int osq_set_tuning(const char* key, int value);

/* Measurement aid (bench.py).  The events given to osq_time_next_launch ride on the dispatch packet of the
 * NEXT launch of kernel family `which` issued by the calling thread (other launches pass untouched), so
 * osq_timing_elapsed_us(start, stop) is that kernel's own run time on its stream -- the duration
 * rocprofv3 --kernel-trace reports -- not the stream-order interval between two recorded events. */
typedef enum osq_timed_kernel {
    OSQ_TIME_NONE = 0,
    OSQ_TIME_FAKE_QUANT = 1,     /* dense osq_fake_quant_per_tensor                      */
    OSQ_TIME_LSQ_BACKWARD = 2,   /* osq_lsq_backward_per_tensor                          */
    OSQ_TIME_OBSERVE_FLAT = 3,   /* osq_observe_flat (aligned input)                     */
    OSQ_TIME_TOKEN_MINMAX = 4,   /* osq_token_minmax / first launch of osq_observe_tokens */
    OSQ_TIME_TOKEN_SELECT = 5,   /* two-workgroup launch of osq_token_range_finalize      */
    OSQ_TIME_LAYERNORM = 6,      /* osq_residual_layernorm_fake_quant                     */
    OSQ_TIME_FUSED_STEP = 7,     /* one-launch form of osq_observe_tokens_fake_quant      */
    OSQ_TIME_FAKE_QUANT_STRIDED = 8,  /* 16-byte form of osq_fake_quant_per_tensor_strided (head-split views) */
    OSQ_TIME_FAKE_QUANT_CHANNEL = 9,  /* row form of osq_fake_quant_per_channel (weights, ch_axis 0)          */
    OSQ_TIME_OBSERVE_CHANNELS = 10,   /* osq_observe_channels                                                */
    OSQ_TIME_TOKEN_MINMAX_MULTI = 11, /* osq_token_minmax_multi                                              */
    OSQ_TIME_MSEFAST_ROWS = 12,       /* osq_msefast_rows (the per-row search launch)                        */
    OSQ_TIME_OBSERVE_TOKENS = 13,     /* one-launch form of osq_observe_tokens                               */
    OSQ_TIME_ATTENTION_SOFTMAX = 14   /* osq_attention_softmax_fake_quant                                    */
} osq_timed_kernel;
int osq_timing_events_create(void** start, void** stop);
int osq_timing_events_destroy(void* start, void* stop);
int osq_time_next_launch(int which, void* start, void* stop);
int osq_timing_elapsed_us(void* start, void* stop, float* us);

/* ------------------------------------------------------------------ fake-quant forward */

/* util_quant.py:11-15 fake_quantize_per_tensor_affine, as called by
 * FixedFakeQuantize.forward fake_quant.py:123-125 (scale/zero_point stay on device
 * instead of .item()); with mode=LSQ/LSQPLUS also util_quant.py:29-34 / 48-55 forward
 * (LSQFakeQuantize / LSQPlusFakeQuantize.forward, fake_quant.py:159-167 / 199-208).
 * x, y: n contiguous fp32.  x_quant (nullable): the clamped integer tensor, fp32 storage (as packed integers:
 * osq_quantize_codes). */
int osq_fake_quant_per_tensor(const float* x, float* y, float* x_quant, int64_t n,
                              float* scale, void* zero_point, int zp_type,
                              int mode, float grad_factor, int quant_min, int quant_max,
                              osq_stream stream);

/* The intermediate-activation site of a transformer block in one pass (model/quant_bert.py:277-280,
 * quant_bart.py:347-348: fc1 / dense -> GELU -> *_act_fn_post_act_fake_quantize): y = fake_quantize(gelu(x))
 * with torch's exact (erf) GELU, bit-identical to F.gelu followed by osq_fake_quant_per_tensor.  x, y: n
 * contiguous fp32, 16-byte aligned (else OSQ_ERR_UNSUPPORTED).  Inference only. */
int osq_gelu_fake_quant_per_tensor(const float* x, float* y, int64_t n,
                                   float* scale, void* zero_point, int zp_type,
                                   int mode, float grad_factor, int quant_min, int quant_max,
                                   osq_stream stream);

/* Same arithmetic for a non-dense tensor of up to 4 dims (e.g. hidden_states[:, 0],
 * quant_bert.py:445): explicit sizes and element strides for input and output. */
int osq_fake_quant_per_tensor_strided(const float* x, float* y, float* x_quant,
                                      const int64_t sizes[4], const int64_t x_strides[4],
                                      const int64_t y_strides[4],
                                      float* scale, void* zero_point, int zp_type,
                                      int mode, float grad_factor, int quant_min, int quant_max,
                                      osq_stream stream);

/* The query / key / value sites of one attention block (model/quant_bert.py:148-155: three Quantizer calls on the
 * head-split views of three [B, T, h*d] projections) as ONE launch.  Site i reads x = [batch, tokens, heads, head_dim]
 * memory (contiguous) and writes y = the dense [batch, heads, tokens, head_dim] tensor the batched matmul wants, with
 * its own (scale, zero_point) -- the same arithmetic, parameter modes (incl. OSQ_PARAM_SANITIZE) and bits as
 * osq_fake_quant_per_tensor_strided on each site.  1..4 sites of ONE geometry; head_dim / 4 a power of two <= 64,
 * 16-byte aligned tensors, else OSQ_ERR_UNSUPPORTED (nothing launched: the caller runs the sites one by one). */
typedef struct osq_headsplit_site {
    const float* x;
    float* y;
    float* scale;
    void* zero_point;
    int32_t zp_type, mode;
    float grad_factor;
    int32_t quant_min, quant_max, pad;
} osq_headsplit_site;
int osq_fake_quant_headsplit_multi(const osq_headsplit_site* sites, int n_sites, int64_t batch, int64_t tokens,
                                   int64_t heads, int64_t head_dim, osq_stream stream);

/* Incremental decoding (model/quant_bart.py, QuantizedBartCache): the attention sites of one decoder step as ONE launch.
 * Site i reads the contiguous [batch, tokens, heads * head_dim] projection x and writes
 *     y[b, head, offset + j, :] = fake_quant(x[b, j, head * head_dim:(head + 1) * head_dim])
 * into y = a dense [batch, heads, cap, head_dim] buffer, with its own (scale, zero_point), zp_type, mode (incl.
 * OSQ_PARAM_SANITIZE) and grad_factor: the arithmetic and bits of osq_fake_quant_headsplit_multi.  A query site is
 * cap = tokens, offset = 0.  With src set (and offset > 0) the same launch also copies the first offset positions,
 *     y[b, :, :offset, :] = src[src_rows[b], :, :offset, :]      (src_rows NULL: row b; src = [src_batch, heads, src_cap, head_dim])
 * -- the beam reorder of a KV cache folded into the next append.  src == y without a row index copies nothing (an
 * in-place append).  src_rows lives on the device (int64); a row outside [0, src_batch) yields NaN and reads nothing.
 * OSQ_ERR_UNSUPPORTED, nothing launched: head_dim % 4, a tensor not 16-byte aligned, src overlapping y (src == y with a
 * row index included), or a site of 2^31 float4s or more.  The caller then runs the eager form. */
typedef struct osq_kv_append_site {
    const float* x;
    float* y;
    const float* src;
    const int64_t* src_rows;
    float* scale;
    void* zero_point;
    int64_t tokens, cap, offset, src_batch, src_cap;
    int32_t zp_type, mode;
    float grad_factor;
    int32_t quant_min, quant_max, pad;
} osq_kv_append_site;
int osq_fake_quant_kv_append(const osq_kv_append_site* sites, int n_sites, int64_t batch, int64_t heads,
                             int64_t head_dim, osq_stream stream);

/* osq_fake_quant_kv_append with the position read by the launch, so that a captured graph of a decoding step can be
 * replayed at every position.  pos: one device int32.  site_at: n_sites host flags; site i with site_at[i] != 0 appends at
 * [*pos, *pos + tokens) and copies [0, *pos) from src through src_rows (its `offset` field is not read); the other sites
 * keep their own offset (a query site: 0).  src set means "copy the prefix", whatever *pos turns out to be (0: nothing);
 * src == y without a row index still copies nothing.  The grid is sized from cap.  For every position the destination
 * holds, byte for byte, what osq_fake_quant_kv_append writes when called with offset = that position.
 * A position that fits no flagged site -- *pos < 0, *pos + tokens > cap, or, where a prefix is copied, *pos > src_cap --
 * is refused by the launch itself: no address is formed from it and NO site writes anything (the parameter repair of
 * OSQ_PARAM_SANITIZE included).  OSQ_ERR_UNSUPPORTED as for the static form, decided for the longest prefix cap admits. */
int osq_fake_quant_kv_append_at(const osq_kv_append_site* sites, int n_sites, int64_t batch, int64_t heads,
                                int64_t head_dim, const int32_t* pos, const int32_t* site_at, osq_stream stream);

/* util_quant.py:18-26 fake_quantize_per_channel_affine (and the per-channel learnable
 * forwards :37-45, :58-67).  x is contiguous `dtype` data viewed as [outer, channels, inner]
 * with ch_axis in the middle; scale/zero_point have `channels` entries; y is fp32.  x_quant (nullable, the
 * integers before dequantisation) exists for fp32 x only: non-NULL with a 16-bit dtype is an invalid argument. */
int osq_fake_quant_per_channel(int dtype, const void* x, float* y, float* x_quant,
                               int64_t outer, int64_t channels, int64_t inner,
                               const float* scale, const void* zero_point, int zp_type,
                               int mode, float grad_factor, int quant_min, int quant_max,
                               osq_stream stream);

/* ------------------------------------------------------------------ LSQ / LSQ+ backward */

/* What autograd produces for util_quant.py:48-55 (per-tensor): dx (elementwise, same
 * fp32 operations as autograd), dscale[1], dzero_point[1] (nullable for LSQ).
 * Needed by learn_scale, token_wise_clipping.py:89-107. */
int osq_lsq_backward_per_tensor(const float* x, const float* grad_out, float* grad_x, int64_t n,
                                const float* scale, const void* zero_point, int zp_type,
                                int mode, float grad_factor, int quant_min, int quant_max,
                                float* grad_scale, float* grad_zero_point,
                                void* workspace, osq_stream stream);

/* The same backward in the REFERENCE's summation order: grad_scale / grad_zero_point are the FOUR fp32 reductions autograd
 * forms on the reference's CPU (mul + div backward, add + sub backward; util_quant.py:48-55,70-71), each added in the order
 * of torch.sum on a one-thread host with `lanes` (8 | 16) fp32 SIMD lanes (csrc/aten_order.h), for any n.  The plain entry point above
 * accumulates in float64 and rounds once (order-free; 2e-5 from autograd's fp32 sums) and is ~1.3x faster.  scratch: osq_ordered_sum_scratch_bytes(n, 4) bytes of
 * device memory, contents irrelevant.  x, grad_out, grad_x: contiguous, no alignment requirement. */
size_t osq_ordered_sum_scratch_bytes(int64_t n, int n_sums);
int osq_lsq_backward_per_tensor_ordered(const float* x, const float* grad_out, float* grad_x, int64_t n,
                                        const float* scale, const void* zero_point, int zp_type,
                                        int mode, float grad_factor, int quant_min, int quant_max,
                                        float* grad_scale, float* grad_zero_point, int lanes,
                                        void* scratch, size_t scratch_bytes, void* workspace, osq_stream stream);

/* Per-channel form (util_quant.py:58-67), x viewed as [outer, channels, inner].  sum_lanes 8 | 16: weights
 * (outer == 1, inner <= 3072) take every row's four reductions in torch's one-thread order on that many SIMD lanes (bit-equal to
 * the reference's autograd run); 0 (and every other layout): float64 sums rounded once.  An empty x (outer, channels or inner 0)
 * launches nothing and sets the `channels` gradients to zero. */
int osq_lsq_backward_per_channel(const float* x, const float* grad_out, float* grad_x,
                                 int64_t outer, int64_t channels, int64_t inner,
                                 const float* scale, const void* zero_point, int zp_type,
                                 int mode, float grad_factor, int quant_min, int quant_max,
                                 float* grad_scale, float* grad_zero_point,
                                 int sum_lanes, osq_stream stream);

/* fake_quant.py:152-153 / 188-191: what LSQFakeQuantize / LSQPlusFakeQuantize do to their
 * parameters on every forward while the observer is off:
 *   scale.abs_(); scale.clamp_(min=eps); zero_point.clamp_(quant_min, quant_max)  (fp32 zp only)
 * n entries, in place, one launch.  zero_point may be NULL (LSQ keeps an int32 buffer). */
int osq_lsq_sanitize(float* scale, float* zero_point, int64_t n, float eps,
                     int quant_min, int quant_max, osq_stream stream);

/* ------------------------------------------------------------------ observers */

/* observer.py:101-119 ObserverBase.calculate_qparams over n entries.
 * zero_point_out is int32 or fp32 storage according to zp_type. */
int osq_calculate_qparams(const float* min_val, const float* max_val, int64_t n,
                          int quant_min, int quant_max, int symmetric,
                          float* scale_out, void* zero_point_out, int zp_type,
                          osq_stream stream);

/* observer.py:139 torch._aminmax(x) over n contiguous values of `dtype`, followed by the
 * running-statistic rule of the observer (MinMaxObserver :143-144, Avg* :194-202)
 * and, when scale_out != NULL, calculate_qparams (:101-119) -- what
 * QuantizeBase.forward does after observer(...) at fake_quant.py:108-116.
 * cur_minmax (nullable): the batch's own (min, max), 2 floats.  `cnt` is the
 * observer's batch counter BEFORE this call (host int, observer.py:198). */
int osq_observe_flat(int dtype, const void* x, int64_t n,
                     int update_rule, int64_t cnt, float* min_val, float* max_val,
                     float* cur_minmax,
                     int quant_min, int quant_max, int symmetric,
                     float* scale_out, void* zero_point_out, int zp_type,
                     void* workspace, osq_stream stream);

/* observer.py:141-144 per-channel min/max: _transform_to_ch_axis + _aminmax(y, 1) +
 * running min/max, x contiguous `dtype` data viewed as [outer, channels, inner]; optional
 * qparams per channel.  min_val/max_val hold `channels` entries. */
int osq_observe_channels(int dtype, const void* x, int64_t outer, int64_t channels, int64_t inner,
                         int update_rule, int64_t cnt, float* min_val, float* max_val,
                         int quant_min, int quant_max, int symmetric,
                         float* scale_out, void* zero_point_out, int zp_type,
                         osq_stream stream);

/* observer.py:64-65 after observer.py:72-84: per-token min and max over the feature
 * axes of `dtype` data, for the tokens t < lengths[b] only (lengths == NULL: every token,
 * observer.py:86-98).  token_min/token_max have batch*tokens slots, slot b*T+t;
 * slots of padded tokens are left untouched. */
int osq_token_minmax(int dtype, const void* x, const osq_token_view* view, const int64_t* lengths,
                     float* token_min, float* token_max, osq_stream stream);

/* osq_token_minmax for MANY tensors in ONE launch (the observer passes of a calibration forward call ~100 sites of 6-50 MB
 * each, token_wise_clipping.py:29-47: launch-bound one by one).  descs / tok_end: DEVICE arrays of n_sites entries; site i
 * is `x` seen through `view`, valid tokens t < lengths[b] (NULL: all), extrema written to token_min / token_max[batch*tokens]
 * (padded slots untouched); vec != 0 promises what osq_token_minmax checks for its 16-byte path (stride_inner == 1,
 * feat_inner % 4 == 0, every other stride % 4 == 0, x 16-byte aligned); tok_end[i] = token slots of sites 0..i. */
typedef struct osq_site_desc {
    const float* x;
    const int64_t* lengths;
    float* token_min;
    float* token_max;
    osq_token_view view;
    int32_t vec;
    int32_t pad;
} osq_site_desc;
int osq_token_minmax_multi(const osq_site_desc* descs, const int64_t* tok_end, int n_sites, int64_t total_tokens,
                           osq_stream stream);

/* Everything after the per-token extrema in AvgPruneMinMaxObserver.forward /
 * AvgMinMaxObserver.forward / MinMaxObserver.forward with a mask:
 *   prune != 0: cac_thres + prune_token (observer.py:50-70) with `percentile`;
 *   prune == 0: plain min/max over the valid tokens (observer.py:193), also used
 *               when 'attention_probs' is in the observer's name (observer.py:62-63);
 * then the update rule (observer.py:194-202 or 143-144) and optional qparams.
 * Up to 32768 token slots, 16-byte aligned arrays, batch*tokens % 4 == 0, tokens >= 4 and a
 * `workspace`: one launch of TWO workgroups, one per side of the statistic (token_max / -token_min),
 * that meet through an 8-byte exchange in the workspace.  Other layouts: one launch, one workgroup.
 * Above 32768 slots, when `workspace` and `list_scratch` (2 * batch * tokens uint32, caller-owned,
 * contents irrelevant) are given: three multi-workgroup launches.  osq_set_wide_min_slots() moves that
 * switch point; osq_set_tuning("final_fast", 0) disables the two-workgroup kernel (tests). */
int osq_token_range_finalize(const float* token_min, const float* token_max,
                             int64_t batch, int64_t tokens, const int64_t* lengths,
                             int prune, double percentile,
                             int update_rule, int64_t cnt, float* min_val, float* max_val,
                             float* cur_minmax,
                             int quant_min, int quant_max, int symmetric,
                             float* scale_out, void* zero_point_out, int zp_type,
                             void* workspace, void* list_scratch, osq_stream stream);

/* osq_token_minmax followed by osq_token_range_finalize on the same stream: a whole masked
 * observation (AvgPruneMinMaxObserver / AvgMinMaxObserver / MinMaxObserver.forward with a mask,
 * observer.py:130-145, 184-203, 214-237) behind one call of the host binding.  token_min/token_max:
 * caller-owned scratch of batch*tokens floats each (their contents are the per-token extrema afterwards). */
int osq_observe_tokens(int dtype, const void* x, const osq_token_view* view, const int64_t* lengths,
                       float* token_min, float* token_max,
                       int prune, double percentile,
                       int update_rule, int64_t cnt, float* min_val, float* max_val,
                       float* cur_minmax,
                       int quant_min, int quant_max, int symmetric,
                       float* scale_out, void* zero_point_out, int zp_type,
                       void* workspace, void* list_scratch, osq_stream stream);

/* QuantizeBase.forward with observer AND fake-quant enabled (the calibrate-and-quantize state,
 * state.py:22-38; fake_quant.py:107-126 / 178-208) on a masked per-tensor activation, behind one call of the
 * host binding: osq_observe_tokens writing (scale, zero_point), then osq_fake_quant_per_tensor of the same
 * dense x[n] into y with those parameters.  No host sync.  A dense row-major [batch, tokens, features] view
 * with features a multiple of 256 (768, 1024, 3072, 4096), batch <= 1024 and 16-byte aligned buffers runs as ONE
 * persistent launch that keeps the tensor in registers between the reduction and the quantisation (x read from
 * HBM once, fused_step.h; token_min / token_max are scratch whose layout is then private to that launch); anything else, or
 * osq_set_tuning("fused_step", 0), is three launches.  cur_minmax (nullable, 2 floats): also receives THIS batch's
 * (min, max) -- the row a data-parallel calibration exchanges and replays in global batch order (calibration.py; the
 * reference's running mean is sequential, observer.py:194-202) -- while the running statistic moves as usual.
 * osq_fused_step_status reads (and clears) the sticky
 * time-out flags of the one-launch form: 0 = every launch on this workspace completed normally. */
int osq_observe_tokens_fake_quant(const float* x, const osq_token_view* view, const int64_t* lengths,
                                  float* token_min, float* token_max,
                                  int prune, double percentile,
                                  int update_rule, int64_t cnt, float* min_val, float* max_val,
                                  float* cur_minmax,
                                  int quant_min, int quant_max, int symmetric,
                                  float* scale, void* zero_point, int zp_type,
                                  float* y, int64_t n, int mode, float grad_factor,
                                  void* workspace, void* list_scratch, osq_stream stream);

int osq_fused_step_status(void* workspace, int* status_out, osq_stream stream);

/* Sticky time-out flags of BOTH persistent launch families on this workspace -- the one-launch observe + fake-quant step
 * (bit 0: a selector, bit 1: a streaming workgroup waited in vain) and the resident MSEFast searches (bit 0) -- read and
 * cleared after everything enqueued on `stream` has finished (this call synchronises the stream).  Non-zero means some
 * launch since the last call wrote NaN into its outputs because its workgroups were not resident together (another
 * process, or another stream's long kernel, held CUs): the caller must treat every result since the last call as
 * invalid.  reset_on_error != 0 additionally returns both state blocks to their all-zero start, so that the next launch
 * begins clean.  The host binding (outlier_suppression_amd.ops.check_persistent) calls this at its synchronisation
 * points and raises. */
int osq_persistent_status(void* workspace, int* fused_status_out, int* resident_status_out, int reset_on_error,
                          osq_stream stream);

int osq_set_wide_min_slots(int64_t slots);

/* Grid-search form of the same step (token_wise_clipping.py:50-66 calls the observer pass once per
 * candidate percentile although, with fake-quant off, the activations -- hence the per-token
 * extrema -- are identical for every candidate).  The caller keeps the per-token extrema of
 * every (quantizer, batch) pair: problem p = quantizer*n_batches + batch occupies
 * token_min/token_max[p*problem_stride ...], all with the same batch x tokens geometry;
 * lengths is [n_batches, batch] -- or, with lengths_per_quantizer, [n_quantizers, n_batches, batch]: sites of one model
 * may be masked differently (BART's cross-attention keys see the DECODER lengths, quant_bart.py:167,172,472) --;
 * prune_flags[quantizer] == 0 for 'attention_probs'
 * quantizers.  One launch re-thresholds all pairs for `percentile` and writes each pair's
 * (min, max) to cur_table[(batch_index*n_quantizers + quantizer)*2] -- per-batch statistics
 * that are then replayed in batch order with osq_observer_update.  `workspace` (nullable): with it,
 * and the layout rules of osq_token_range_finalize met, every pair gets two workgroups. */
int osq_token_range_finalize_batched(const float* token_min, const float* token_max,
                                     int64_t problem_stride, int n_quantizers, int n_batches,
                                     int64_t batch, int64_t tokens, const int64_t* lengths, int lengths_per_quantizer,
                                     const int32_t* prune_flags, double percentile,
                                     float* cur_table, void* workspace, osq_stream stream);

/* Running statistic for a batch (min, max) that is already known -- the replay step
 * of sharded calibration (gathered per-batch statistics applied in global batch
 * order, observer.py:194-202).  cur_min/cur_max: n entries. */
int osq_observer_update(const float* cur_min, const float* cur_max, int64_t n,
                        int update_rule, int64_t cnt, float* min_val, float* max_val,
                        osq_stream stream);

/* Replay of a whole [n_batches, n_quantizers, 2] table of per-batch (min, max) -- what sharded and cached
 * calibration gather -- in ONE launch: quantizer q folds rows 0..n_batches-1 into its running statistic with
 * rules[q] (OSQ_UPDATE_RUNNING / OSQ_UPDATE_AVERAGE, cnt0 = batches seen before row 0; fresh != 0: start from
 * the untouched (+inf, -inf) state regardless of the buffers), stores it through min_ptrs[q] / max_ptrs[q]
 * (device addresses of 1-element fp32 buffers), and, where scale_ptrs[q] != 0, writes
 * calculate_qparams (observer.py:101-119) through scale_ptrs[q] / zp_ptrs[q] (zp_types[q]).  All arrays live
 * on the device.  Equivalent to n_batches calls of osq_observer_update + n_quantizers of
 * osq_calculate_qparams. */
int osq_replay_statistics(const float* table, int n_batches, int n_quantizers, const int32_t* rules,
                          int64_t cnt0, int fresh, const uint64_t* min_ptrs, const uint64_t* max_ptrs,
                          const int32_t* quant_min, const int32_t* quant_max, const int32_t* symmetric,
                          const uint64_t* scale_ptrs, const uint64_t* zp_ptrs, const int32_t* zp_types,
                          osq_stream stream);

/* Every weight of a model in ONE launch (quantized_module.py:71-72, 97-100 fake-quantise each weight in its own op on
 * every forward).  descs / row_end: DEVICE arrays of n_tensors entries; tensor i is x[rows, inner] (row-major, inner % 4
 * == 0, 16-byte aligned) -> y, quantised per row with scale[row % channels] / zero_point[row % channels] (channels == 1:
 * per-tensor); row_end[i] = rows of tensors 0..i.  mode / grad_factor as in osq_fake_quant_per_channel (no
 * OSQ_PARAM_SANITIZE).  Same arithmetic as the per-tensor calls: bit-identical outputs. */
typedef struct osq_weight_desc {
    const float* x;
    float* y;
    const float* scale;
    const void* zero_point;
    int64_t rows, channels, inner;
    int32_t zp_type, mode;
    float grad_factor;
    int32_t quant_min, quant_max;
    int32_t pad;
} osq_weight_desc;
int osq_fake_quant_weights_multi(const osq_weight_desc* descs, const int64_t* row_end, int n_tensors,
                                 int64_t total_rows, osq_stream stream);

/* ------------------------------------------------------------------ integer codes (csrc/codes.hip) */

/* The result of PTQ as integers: what a W8 / W4 checkpoint stores instead of fp32 weights.
 *
 * Code format.  u = x_quant - quant_min, x_quant the clamped integer tensor of util_quant.py:12-13: an unsigned integer in
 * [0, quant_max - quant_min].
 *   code_bits 8: one byte per element, in x's contiguous order; n bytes.
 *   code_bits 4: only when quant_max - quant_min <= 15.  Packed over the FLATTENED tensor: byte k holds element 2k in its low
 *                nibble and element 2k + 1 in its high nibble; with an odd n the last high nibble is 0; ceil(n / 2) bytes.
 *   A 6-bit quantizer uses code_bits 8 (no three-byte packing).
 * (float(u + quant_min) - zp_eff) * scale_eff is the fake-quant y of the same call word for word.
 *
 * osq_quantize_codes: x is contiguous `dtype` data viewed as [outer, channels, inner] as in osq_fake_quant_per_channel
 * (channels == 1: per-tensor; pass the tensor's rows as `outer`, a wave walks a row); scale / zero_point / zp_type / mode /
 * grad_factor as there (no OSQ_PARAM_SANITIZE).  scale_eff / zp_eff (nullable, `channels` fp32 entries): the EFFECTIVE
 * parameters that reached the quantiser, written once per channel -- in the LSQ modes grad_scale's value can differ from
 * the stored parameter by an ulp, and the dequantiser must use what the quantiser used.  rejected (nullable, device int32,
 * only ever added to -- the caller zeroes it): the number of elements whose x_quant is NaN or not an integer (a NaN or
 * infinite x, a NaN parameter, a fractional zero point); such an element has no code and 0 is written for it.
 * x and codes 16-byte aligned with inner a multiple of 4 elements (8 for bf16 / fp16, 8 at code_bits 4): 16-byte loads,
 * codes stored 4 bytes per lane (16 where a row's code bytes are a multiple of 16).  Every other layout -- odd inner, a
 * channel axis with inner 1, pointers off alignment, an odd n -- runs a generic kernel with the same results (never
 * OSQ_ERR_UNSUPPORTED).  An empty x launches nothing and writes nothing.
 *
 * osq_dequantize_codes: y[outer, channels, inner] fp32 = (float(u + quant_min) - zp_eff[c]) * scale_eff[c], the operation
 * order of util_quant.py:14.  y 16-byte aligned, inner % 4 == 0 and codes 4-byte (code_bits 4: 2-byte) aligned: one wave per
 * row, float4 stores; otherwise the generic kernel. */
int osq_quantize_codes(int dtype, const void* x, uint8_t* codes,
                       int64_t outer, int64_t channels, int64_t inner,
                       const float* scale, const void* zero_point, int zp_type,
                       int mode, float grad_factor,
                       int quant_min, int quant_max, int code_bits,
                       float* scale_eff, float* zp_eff,
                       int32_t* rejected, osq_stream stream);
int osq_dequantize_codes(const uint8_t* codes, float* y,
                         int64_t outer, int64_t channels, int64_t inner,
                         const float* scale_eff, const float* zp_eff,
                         int quant_min, int code_bits, osq_stream stream);

/* Every coded weight of a checkpoint in ONE launch (load time), the table scheme of osq_fake_quant_weights_multi.  descs /
 * row_end: DEVICE arrays of n_tensors entries; tensor i is codes -> y[rows, inner] (row-major, inner % 4 == 0, y 16-byte
 * aligned, codes 4-byte aligned -- 2-byte at code_bits 4, where inner % 4 == 0 also makes every row start on a byte),
 * row r dequantised with scale_eff[r % channels] / zp_eff[r % channels] (channels == 1: per-tensor); row_end[i] = rows of
 * tensors 0..i.  Entries of both code widths may share a table.  Same arithmetic as osq_dequantize_codes: the same words. */
typedef struct osq_codes_desc {
    const uint8_t* codes;
    float* y;
    const float* scale_eff;
    const float* zp_eff;
    int64_t rows, channels, inner;
    int32_t quant_min, code_bits;
} osq_codes_desc;
int osq_dequantize_codes_multi(const osq_codes_desc* descs, const int64_t* row_end, int n_tensors,
                               int64_t total_rows, osq_stream stream);

/* ------------------------------------------------------------------ the KV cache as integer codes (csrc/kv_codes.hip) */

/* A KV cache that holds codes instead of fp32 words: one byte per element, u = x_quant - quant_min (the code format above,
 * code_bits 8; quant_max - quant_min <= 255), in the cache's [batch, heads, cap, head_dim] order.  Per cached tensor a
 * RECORD of two device floats, scale_eff / zp_eff (the effective parameters that reached the quantiser), and one device
 * int32 `rejected` shared by every tensor of a cache, only ever added to.  (float(u + quant_min) - zp_eff) * scale_eff is
 * the word osq_fake_quant_kv_append writes for the same element; osq_dequantize_codes(codes, y, batch * heads * cap, 1,
 * head_dim, scale_eff, zp_eff, quant_min, 8) turns a whole buffer into the fp32 buffer of the same geometry.
 *
 * osq_fake_quant_kv_append_codes is osq_fake_quant_kv_append (same geometry, same parameter handling, OSQ_PARAM_SANITIZE
 * included, same overlap rules) with a destination kind per site:
 *   coded == 0: y (and src) fp32, exactly the fp32 entry point's site -- the query site; scale_eff / zp_eff unused.
 *   coded != 0: y and src are BYTE buffers.  x is quantised with the live parameters (tensor_params / quantize_value: the
 *     x_quant of the fp32 form) and x_quant - quant_min stored, four codes per lane as one 32-bit store.  The kept prefix
 *     is copied as bytes from src through src_rows (16 bytes per lane where prefix, caps and pointers allow, else 4).
 *     write_record != 0: the launch writes the record.  Otherwise it compares its live effective pair with the record bit
 *     for bit and adds 1 to `rejected` on a mismatch (parameters rewritten through raw pointers since the first append).
 *     An element without a code (x_quant NaN or not an integer: a NaN or infinite x, NaN parameters, a fractional
 *     effective zero point) gets code 0 and adds 1 to `rejected`.  A src_rows entry outside [0, src_batch) reads nothing:
 *     the prefix of that batch row gets code 0 and every element of it adds 1 to `rejected` (a byte has no NaN).
 * rejected: device int32, required when a site is coded.  OSQ_ERR_UNSUPPORTED as for the fp32 entry point, with 4-byte
 * alignment asked of byte buffers. */
typedef struct osq_kv_codes_site {
    const float* x;
    void* y;
    const void* src;
    const int64_t* src_rows;
    float* scale;
    void* zero_point;
    float* scale_eff;
    float* zp_eff;
    int64_t tokens, cap, offset, src_batch, src_cap;
    int32_t zp_type, mode;
    float grad_factor;
    int32_t quant_min, quant_max, coded, write_record, pad;
} osq_kv_codes_site;
int osq_fake_quant_kv_append_codes(const osq_kv_codes_site* sites, int n_sites, int64_t batch, int64_t heads,
                                   int64_t head_dim, int32_t* rejected, osq_stream stream);

/* osq_fake_quant_kv_append_codes with the position read by the launch: pos / site_at and the refusal as in
 * osq_fake_quant_kv_append_at.  Whether a coded prefix is copied 16 or 4 bytes per lane is decided by the launch for the
 * position it reads (the bytes written are the same).  A refused position writes nothing -- no record either -- and, when
 * any site is coded, adds exactly 1 to `rejected`.  For every other position the destinations, the records and `rejected`
 * are byte-equal to osq_fake_quant_kv_append_codes called with offset = that position. */
int osq_fake_quant_kv_append_codes_at(const osq_kv_codes_site* sites, int n_sites, int64_t batch, int64_t heads,
                                      int64_t head_dim, int32_t* rejected, const int32_t* pos, const int32_t* site_at,
                                      osq_stream stream);

/* ------------------------------------------------------------------ MSEFast (observer.py:412-567) */

/* one_side: 0 = 'no', 1 = 'pos', 2 = 'neg' (observer.py:528-529, decided once by the caller on
 * the first observed tensor); two_d: 1 for the nested range/shift search (observer.py:458-481),
 * 0 for the 1-D search (observer.py:483-494). */

/* golden_section_{1D,2D}_search with ch_axis = 0 (observer.py:496-517): one bounded-Brent
 * search per row of w[rows, cols] -- the reference's Python loop over channels -- in ONE launch.
 * best_min / best_max: rows fp32 entries (the values assigned at observer.py:504,516);
 * nfev (nullable): loss evaluations spent per row. */
int osq_msefast_rows(const float* w, int64_t rows, int64_t cols, int quant_min, int quant_max,
                     int symmetric, int one_side, int two_d,
                     float* best_min, float* best_max, int32_t* nfev, osq_stream stream);

/* Per-tensor search (observer.py:497-499,510-512).  The Brent state machine lives in `state`
 * (osq_msefast_state_bytes() of device memory).  begin: start from the tensor's (min, max)
 * (2 floats on the device, e.g. cur_minmax of osq_observe_flat / osq_token_range_finalize with
 * OSQ_UPDATE_NONE).  evals_*: enqueue n_evals loss evaluations (loss_fx, observer.py:423-432),
 * each one launch that also advances the state machine; launches after convergence are no-ops.
 * done: copy the converged flag to done_out (device int32).  commit: running min/max
 * (observer.py:535-536) or running mean (observer.py:559-567) of the float64 statistics, then
 * calculate_qparams in float64 into scale_out / zero_point_out (nullable).
 * float64_input: the reference casts x to min_val's dtype (observer.py:524,549), and a per-tensor observer's min_val is
 * float64 after its first call (observer.py:481,494) -- so from the second call on its whole search runs on a float64
 * copy of x (float64 fake-quant, float64 mean, np.float64 function values).  1 selects that arithmetic; x stays the
 * fp32 tensor, the kernels widen as they read. */
size_t osq_msefast_state_bytes(void);
int osq_msefast_tensor_begin(void* state, const float* cur_minmax, int quant_min, int quant_max,
                             int symmetric, int one_side, int two_d, int float64_input, osq_stream stream);
int osq_msefast_tensor_evals_flat(void* state, const float* x, int64_t n, int n_evals,
                                  void* workspace, osq_stream stream);
int osq_msefast_tensor_evals_tokens(void* state, const float* x, const osq_token_view* view,
                                    const int64_t* lengths, int n_evals,
                                    void* workspace, osq_stream stream);
/* Loss evaluations in the REFERENCE's summation order ("mse_sum_order" 8 / 16; observer.py:420-432 on a one-thread host):
 * x_flat holds the observed elements in the order remove_padding / flatten lays them out (observer.py:72-84) -- the tensor
 * itself when it is dense and unmasked, otherwise the copy osq_gather_valid_tokens makes (out: batch * tokens * features
 * floats; count_out: device int64 that receives the number of elements kept).  n: elements (an upper bound when n_device,
 * nullable, points at the device-side count).  scratch: osq_ordered_sum_scratch_bytes(n, 1) bytes.  One launch per
 * evaluation; _evals_flat / _evals_tokens refuse to run while the order is set. */
int osq_gather_valid_tokens(const float* x, const osq_token_view* view, const int64_t* lengths, float* out,
                            int64_t* count_out, osq_stream stream);
int osq_msefast_tensor_evals_ordered(void* state, const float* x_flat, int64_t n, const int64_t* n_device, int n_evals,
                                     void* scratch, size_t scratch_bytes, void* workspace, osq_stream stream);
/* The strict evaluations of SEVERAL searches (the MSEFast observers of one forward: independent while fake-quant is off) as
 * ROUNDS: one launch = one loss evaluation of every unfinished search, each in the reference's order as above.  A launch
 * per evaluation of one site costs ~15 us whatever its size; a round pays that once for up to 128 sites.
 *   table: osq_msefast_ordered_multi_bytes(n_sites) bytes of device memory, ZERO before _prepare (site table + the ticket
 *          counters of every site + the workgroup -> site map of a round); _prepare fills table and map (synchronous on
 *          `stream`), copies the device-side element counts into the table (after the gathers enqueued before it) and returns the grid of a round;
 *   per site: state (between osq_msefast_tensor_begin and _commit), the flat tensor (osq_gather_valid_tokens for a masked
 *          site) with its host-side element bound n[i] and nullable device count n_device[i], and scratch of
 *          osq_ordered_sum_scratch_bytes(n[i], 1) bytes;
 *   _evals: n_evals rounds, then done_out[0] = 1 if every search has converged (nullable). */
size_t osq_msefast_ordered_multi_bytes(int n_sites);
int osq_msefast_ordered_multi_prepare(void* table, size_t table_bytes, void* const* states, const float* const* x_flat,
                                      const int64_t* n, const int64_t* const* n_device, void* const* scratch,
                                      const size_t* scratch_bytes, int n_sites, int* total_blocks_out, osq_stream stream);
int osq_msefast_ordered_multi_evals(const void* table, int n_sites, int total_blocks, int n_evals, int32_t* done_out,
                                    osq_stream stream);
/* The whole per-tensor search in ONE persistent launch (between _begin and _commit; replaces the _evals_* / _done loop):
 * the valid part of the tensor is loaded once into the registers of a one-workgroup-per-CU grid, every loss
 * evaluation is one exchange of per-workgroup partial sums through the workspace.  view == NULL: x is flat, n
 * elements; otherwise a token view with valid lengths (n ignored).  OSQ_ERR_UNSUPPORTED (nothing launched): more
 * than 32 float4 per lane of the grid (512-thread workgroups: 67 MB on 256 CUs), batch > 512, a misaligned flat tensor,
 * or osq_set_tuning("mse_resident", 0) -- the caller then runs the _evals_* loop.  A workgroup that waits in vain for
 * another one's partial sum (the grid was not resident together: another process or stream held CUs) poisons the search
 * with NaN and raises the sticky flag osq_persistent_status reports. */
int osq_msefast_tensor_search(void* state, const float* x, int64_t n, const osq_token_view* view,
                              const int64_t* lengths, void* workspace, osq_stream stream);
/* Several searches in ONE persistent launch (the observers of a forward are independent while fake-quant is off):
 * osq_msefast_resident_slots(elems) = float4 slots per lane of the resident grid a search over `elems` elements takes
 * (1..max_slots; 0 = cannot be resident); a group fits when it has at most max_sites searches whose slots add up to at
 * most max_slots (osq_msefast_resident_limits: 32 and 16).
 * Every round of the launch evaluates the pending candidate of every unfinished search; the exchange of the partial
 * sums and the serial Brent steps of the searches overlap.  Arrays are HOST arrays of n_sites entries; views[i].batch
 * == 0 marks a flat tensor of ns[i] elements.  Each search sits between its own _begin and _commit.
 * OSQ_ERR_UNSUPPORTED: the group does not fit, nothing was launched. */
int osq_msefast_resident_slots(int64_t elems);
int osq_msefast_resident_limits(int* max_slots, int* max_sites);
int osq_msefast_tensor_search_multi(void* const* states, const float* const* xs, const int64_t* ns,
                                    const osq_token_view* views, const int64_t* const* lengths, int n_sites,
                                    void* workspace, osq_stream stream);
int osq_msefast_tensor_done(const void* state, int32_t* done_out, osq_stream stream);
/* The LOSS MEMO of the per-tensor searches (ABI 7).  loss_fx (observer.py:423-432) is a pure function of the tensor and of the
 * pair it hands to the fake-quant -- scale.item(), int(zero_point.item()) -- and scipy's bounded search asks for the same pair
 * many times (the inner search of observer.py:434-446 moves the shift of a fixed range: the scale stays, the integer zero point
 * changes once per quantisation step; the final inner search of observer.py:469-475 repeats an earlier one entirely).  A search
 * keeps the pairs it has streamed (up to 512) in its state; the step after an evaluation advances the state machine for as long
 * as the next candidate's pair is known.  Results, iterates and nfev are those of the search without it, bit for bit; on
 * two-sided data 3/4 of the passes over the tensor go.  osq_set_tuning("mse_memo", 0) switches it off (tests, A/B).
 * The _evals_flat / _evals_tokens / _evals_ordered / _ordered_multi_evals entry points use it; the persistent searches
 * (osq_msefast_tensor_search*: the tensor is in registers, an evaluation costs microseconds) do not.
 * stats_out: 4 device int32 -- nfev so far, pairs kept, evaluations answered from the memo, converged flag. */
int osq_msefast_tensor_stats(const void* state, int32_t* stats_out, osq_stream stream);
/* ObserverBase.calculate_qparams (observer.py:101-119) on float64 statistics -- what a per-tensor MSEFast observer holds:
 * torch computes in the statistics' (promoted) dtype; scale / zero_point are rounded to their fp32 / int32 storage once. */
int osq_calculate_qparams_f64(const double* min_val, const double* max_val, int64_t n, int quant_min, int quant_max,
                              int symmetric, float* scale_out, void* zero_point_out, int zp_type, osq_stream stream);

/* ref_float64 (nullable): int32[2] on the device, zero before the observer's first commit -- whether the REFERENCE's
 * min_val / max_val hold float64 by now.  Its per-tensor results are float64 except the float32 zeros_like of a one-sided
 * search (observer.py:491-492) and the float32 extremum that Python's max / min hand back when the nested search's range
 * reaches beyond the data (observer.py:479-480); while a statistic is float32 its running mean is fp32 arithmetic, while
 * both are, calculate_qparams is, and observer.py:524 / 549 cast the NEXT batch to min_val's dtype: the caller reads
 * ref_float64[0] for osq_msefast_tensor_begin's float64_input.  NULL: float64 throughout. */
int osq_msefast_tensor_commit(const void* state, int update_rule, int64_t cnt,
                              double* min_val, double* max_val,
                              int quant_min, int quant_max, int symmetric,
                              float* scale_out, void* zero_point_out, int zp_type,
                              int32_t* nfev, int32_t* ref_float64, osq_stream stream);

/* ------------------------------------------------------------------ remaining observers of ObserverDict */

/* LSQPlusObserver.forward (observer.py:159-173): min/max = mean -+ 3*std (unbiased) of x viewed as
 * [outer, channels, inner]; channels == 1 is the per-tensor form (needs workspace).  Not accumulated
 * across calls, as in the reference.  Optional qparams. */
int osq_observe_moments(const float* x, int64_t outer, int64_t channels, int64_t inner,
                        float* min_val, float* max_val, int quant_min, int quant_max, int symmetric,
                        float* scale_out, void* zero_point_out, int zp_type,
                        void* workspace, osq_stream stream);

/* AvgQuantileObserver.forward (observer.py:253-282) after the tensor's own (min, max) is known
 * (cur_minmax, 2 device floats): torch.histc(|x|, 2048, 0, max(-min, max)) with torch's binning
 * (linear estimate + local search against the linspace edges), clip at the bin where the
 * cumulative count reaches threshold * numel, running mean, optional qparams.  x is either flat
 * (view == NULL, n elements) or a token view with valid lengths.  hist_scratch: 2048 uint32,
 * zero on entry, left zeroed. */
int osq_observe_quantile(const float* x, int64_t n, const osq_token_view* view, const int64_t* lengths,
                         const float* cur_minmax, double threshold, uint32_t* hist_scratch,
                         int update_rule, int64_t cnt, float* min_val, float* max_val,
                         int quant_min, int quant_max, int symmetric,
                         float* scale_out, void* zero_point_out, int zp_type, osq_stream stream);

/* MSEObserver / AvgMSEObserver (observer.py:285-409): brute-force grid of 100 clipping ranges
 * (1-D, symmetric or one-sided data) or 100 ranges x (quant_max-quant_min+1) zero-points (2-D);
 * 32 candidates are evaluated per pass over the data.  loss_scratch: scratch_bytes bytes of device memory; with at least
 * osq_mse_grid_scratch_bytes() (13 MB for the 6-bit asymmetric grid: the losses + 256 workgroups' partial sums of every
 * candidate) the whole grid is ONE launch of 1024-thread workgroups + a reduction; with less (>= osq_mse_grid_candidates()
 * floats) it is one launch per 32 candidates.  The first osq_mse_grid_candidates() floats hold the losses afterwards. */
int osq_mse_grid_candidates(int quant_min, int quant_max, int two_d);
size_t osq_mse_grid_scratch_bytes(int quant_min, int quant_max, int two_d);
int osq_mse_grid_tensor(const float* x, int64_t n, const osq_token_view* view, const int64_t* lengths,
                        const float* cur_minmax, int quant_min, int quant_max, int symmetric,
                        int one_side, int two_d, float* loss_scratch, size_t scratch_bytes,
                        int update_rule, int64_t cnt, float* min_val, float* max_val,
                        float* scale_out, void* zero_point_out, int zp_type,
                        void* workspace, osq_stream stream);
/* Test aid: the all-candidates launch replaces x / scale by a reciprocal sequence that is bit-equal to the IEEE division under
 * two guards (csrc/observers_extra.hip, div_by_reciprocal); this counts the admitted pairs (x[i], s[i]) on which the two differ. */
int osq_selftest_division(const float* x, const float* s, int64_t n, int32_t* mismatches, osq_stream stream);
/* per-channel form (observer.py:297-301,316-323): one wave per row of w[rows, cols]. */
int osq_mse_grid_rows(const float* w, int64_t rows, int64_t cols, int quant_min, int quant_max,
                      int symmetric, int one_side, int two_d,
                      float* best_min, float* best_max, osq_stream stream);

/* ------------------------------------------------------------------ gamma migration */

/* gamma_migration.py:70-71  w.weight.data *= gamma  (gamma broadcast over columns). */
int osq_gamma_fold(float* weight, const float* gamma, int64_t rows, int64_t cols,
                   osq_stream stream);

/* util_layernorm.py:27  bias <- beta / gamma. */
int osq_gamma_split_bias(const float* beta, const float* gamma, float* bias_out, int64_t n,
                         osq_stream stream);

/* util_layernorm.py:49-52 GammaResidual.forward: out = input * gamma + hidden
 * (gamma == NULL: input + hidden).  rows x cols contiguous. */
int osq_gamma_residual(const float* input, const float* hidden, const float* gamma,
                       float* out, int64_t rows, int64_t cols, osq_stream stream);

/* ------------------------------------------------------------------ residual + LayerNorm + fake-quant */

/* One pass for what a LayerNorm site of the quantized models runs as four eager steps
 * (model/quant_bert.py:211-216 / 298-303 with model/util_layernorm.py:14-18, 32-37, 49-52):
 *     r = x * gamma + hidden        GammaResidual.forward      (hidden == NULL: r = x; gamma == NULL: x + hidden)
 *     n = layer_norm(r, eps)        over the last axis, cols
 *     n = n * weight + bias         QuantizedLayerNorm: the LayerNorm's affine pair;
 *                                   QuantizedSplitLayerNorm: weight == NULL, bias = beta/gamma
 *     y = fake_quantize(n)          scale == NULL: y = n (observer passes, qoutput == False)
 * rows x cols contiguous fp32, cols % 4 == 0, cols <= 4096, 16-byte aligned operands (else
 * OSQ_ERR_UNSUPPORTED and the caller keeps the eager sequence).  mode / grad_factor / zp_type as in
 * osq_fake_quant_per_tensor, including OSQ_PARAM_SANITIZE.  8 B per element (12 with a residual)
 * instead of 24-32.  Inference only: autograd passes use the eager sequence. */
int osq_residual_layernorm_fake_quant(const float* x, const float* hidden, const float* gamma,
                                      const float* weight, const float* bias, double eps,
                                      float* y, int64_t rows, int64_t cols,
                                      float* scale, void* zero_point, int zp_type,
                                      int mode, float grad_factor, int quant_min, int quant_max,
                                      osq_stream stream);

/* ------------------------------------------------------------------ attention probabilities: mask + softmax + fake-quant */

/* One pass for what the attention-probabilities site of the quantized models runs as three eager steps
 * (model/quant_bert.py:169-185, model/quant_bart.py:232-256), for every row (b, h, t) of a [batch, heads, tokens, cols]
 * scores tensor:
 *     v = pre(scores) + mask        alpha != 1:   mask + scores * alpha    (torch.add(mask, scores, alpha=...): exact
 *                                                                          only for a power-of-two alpha, which callers pass)
 *                                   divisor != 1: scores / divisor + mask  (IEEE division)
 *                                   both 1:       scores + mask
 *                                   (mask == NULL: no addition; at most one of alpha / divisor may differ from 1)
 *     p = softmax(v) over cols      max-subtracted, accurate expf, fp32 sum, p = e * (1 / sum) as torch's CPU kernel;
 *                                   a row with a NaN, a +inf or only -inf entries is NaN
 *     y = fake_quantize(p)          scale == NULL: y = p (observer passes, disabled or per-channel quantizers)
 * scores / y contiguous fp32 (y may be scores).  The mask is fp32 with a contiguous last axis; row (b, h, t) starts at
 * b * mask_stride_b + h * mask_stride_h + t * mask_stride_t elements (0 = broadcast): BERT's [B,1,1,S], BART's [B,1,T,S].
 * mode / grad_factor / zp_type as in osq_fake_quant_per_tensor, including OSQ_PARAM_SANITIZE: for a given p, y is
 * word-equal to osq_fake_quant_per_tensor(p).  cols % 4 == 0, cols <= 2048 with 16-byte aligned scores / y / mask rows
 * run the register-resident kernel (8 B per element); any other shape a generic kernel with the same arithmetic.
 * Inference only: autograd passes use the eager sequence. */
int osq_attention_softmax_fake_quant(const float* scores, const float* mask, int64_t batch, int64_t heads, int64_t tokens,
                                     int64_t cols, int64_t mask_stride_b, int64_t mask_stride_h, int64_t mask_stride_t,
                                     float alpha, float divisor, float* y,
                                     float* scale, void* zero_point, int zp_type,
                                     int mode, float grad_factor, int quant_min, int quant_max,
                                     osq_stream stream);

/* ------------------------------------------------------------------ one decoding step's attention over the KV cache */

/* What QuantizedBartAttention._attend (model/quant_bart.py; the reference's quant_bart.py:232-268) runs for the single
 * query token of a cached decoding step -- bmm, mask add, softmax, attention_probs quantizer, bmm, merge heads, context
 * quantizer -- as ONE launch, one workgroup per (batch, head):
 *     s[j] = dot(q, k[j]) + mask[j]      j < kv_len
 *     p    = softmax(s)                  the arithmetic of osq_attention_softmax_fake_quant: max-subtracted, accurate expf,
 *                                        p = e * (1 / sum)
 *     p'   = fake_quantize(p)            the probs_* group
 *     out  = fake_quantize(sum_j p'[j] * v[j])      the ctx_* group
 * q: dense [batch, heads, 1, head_dim], the already fake-quantised and scaled query.  k / v: [batch, heads, cap, head_dim]
 * buffers with their own cap (row stride cap * head_dim, cap >= kv_len) of which positions [0, kv_len) are read: the cache
 * buffers as they are, or the cross-attention tensors with cap == kv_len.  mask: NULL, or additive dense
 * [batch, 1, 1, kv_len], broadcast over heads.  out: dense [batch, 1, heads * head_dim] (the merged layout).  probs_out:
 * NULL, or dense [batch, heads, 1, kv_len], receives p'.  All fp32.  Each parameter group is (scale, zero_point, zp_type,
 * mode, grad_factor, quant_min, quant_max) as in osq_headsplit_site, OSQ_PARAM_SANITIZE included; a NULL scale means no
 * quantizer: the values pass through.  For given p (given c) the outputs are word-equal to osq_fake_quant_per_tensor.
 * The dot products are fp32 sums in an order fixed by (head_dim, kv_len) alone (csrc/decode_attention.hip) -- not by cap,
 * placement or the cache's storage format (osq_decode_attention_codes), and not rocBLAS's: against the eager sequence the result is equal to a tolerance, not bit for bit; the same inputs give the same
 * words on every run, whatever the caps.
 * OSQ_ERR_UNSUPPORTED, nothing launched (the caller runs the eager sequence): head_dim / 4 not a power of two <= 64, kv_len
 * outside [1, 4096], a pointer not 16-byte aligned.  Inference only. */
int osq_decode_attention_fake_quant(const float* q, const float* k, const float* v, const float* mask, float* out,
                                    float* probs_out, int64_t batch, int64_t heads, int64_t head_dim, int64_t kv_len,
                                    int64_t k_cap, int64_t v_cap,
                                    float* probs_scale, void* probs_zero_point, int probs_zp_type, int probs_mode,
                                    float probs_grad_factor, int probs_quant_min, int probs_quant_max,
                                    float* ctx_scale, void* ctx_zero_point, int ctx_zp_type, int ctx_mode,
                                    float ctx_grad_factor, int ctx_quant_min, int ctx_quant_max,
                                    osq_stream stream);

/* osq_decode_attention_fake_quant over a coded cache: k / v are byte buffers [batch, heads, cap, head_dim] of codes, each
 * with its record (k_scale_eff / k_zp_eff, one device float each) and quant_min.  A lane reads four codes as one 32-bit
 * load, forms float(u + quant_min), then (q - zp_eff) * scale_eff, and goes on as the fp32 form does: out and probs_out
 * are word-equal to osq_decode_attention_fake_quant on the dequantised fp32 k / v, for every shape that takes.  rejected:
 * the cache's counter (device int32, required); non-zero on entry -> every word of out and probs_out is NaN.  Limits and
 * OSQ_ERR_UNSUPPORTED cases as the fp32 form, k / v 4-byte aligned. */
int osq_decode_attention_codes(const float* q, const uint8_t* k, const uint8_t* v, const float* mask, float* out,
                               float* probs_out, int64_t batch, int64_t heads, int64_t head_dim, int64_t kv_len,
                               int64_t k_cap, int64_t v_cap,
                               const float* k_scale_eff, const float* k_zp_eff, int k_quant_min,
                               const float* v_scale_eff, const float* v_zp_eff, int v_quant_min, const int32_t* rejected,
                               float* probs_scale, void* probs_zero_point, int probs_zp_type, int probs_mode,
                               float probs_grad_factor, int probs_quant_min, int probs_quant_max,
                               float* ctx_scale, void* ctx_zero_point, int ctx_zp_type, int ctx_mode,
                               float ctx_grad_factor, int ctx_quant_min, int ctx_quant_max,
                               osq_stream stream);

/* The two entry points above with the length read by the launch: kv_len = *kv_len_dev + kv_len_add (kv_len_dev one device
 * int32; self-attention passes the cache's position word and 1, the step's own token), so that one captured graph serves
 * every step.  kv_max (1..4096, <= k_cap and v_cap) is the largest length the launch may meet; the host checks go by it.
 * mask (nullable) is [batch, 1, 1, >= kv_max] with rows mask_stride floats apart, probs_out (nullable)
 * [batch, heads, 1, >= kv_max] with rows probs_stride floats apart: columns [0, kv_len) are read / written, so buffers
 * laid out for kv_max serve every step.  probs_grad_table: NULL (probs_grad_factor holds), or kv_max + 1 device floats,
 * entry n the grad factor of the probabilities quantizer at kv_len == n as the HOST computed it (the launch reads the
 * word, it does not re-derive it; entry 0 is not read).  For every kv_len in [1, kv_max], out and probs_out[..., :kv_len]
 * are word-equal to the static entry point called with that kv_len; the summation order is fixed by (head_dim, kv_len)
 * alone.  A kv_len outside [1, kv_max]: every word of out is NaN, and q, k, v, mask, the table and the parameters are not
 * read.  OSQ_ERR_UNSUPPORTED as for the static forms, with kv_max in the place of kv_len. */
int osq_decode_attention_fake_quant_at(const float* q, const float* k, const float* v, const float* mask,
                                       int64_t mask_stride, float* out, float* probs_out, int64_t probs_stride,
                                       int64_t batch, int64_t heads, int64_t head_dim,
                                       const int32_t* kv_len_dev, int64_t kv_len_add, int64_t kv_max,
                                       int64_t k_cap, int64_t v_cap, const float* probs_grad_table,
                                       float* probs_scale, void* probs_zero_point, int probs_zp_type, int probs_mode,
                                       float probs_grad_factor, int probs_quant_min, int probs_quant_max,
                                       float* ctx_scale, void* ctx_zero_point, int ctx_zp_type, int ctx_mode,
                                       float ctx_grad_factor, int ctx_quant_min, int ctx_quant_max,
                                       osq_stream stream);
int osq_decode_attention_codes_at(const float* q, const uint8_t* k, const uint8_t* v, const float* mask,
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
                                  osq_stream stream);

/* osq_decode_attention_fake_quant / osq_decode_attention_codes for query rows that share their keys and values
 * (csrc/decode_attention.hip): beam search's cross-attention, where the `group` beams of a batch row attend to the same
 * encoder keys / values.  q: dense [batch * group, heads, 1, head_dim]; query row b * group + g attends to row b of k / v
 * ([batch, heads, cap, head_dim]) and of mask (NULL, or [batch, 1, 1, kv_len]).  out: dense [batch * group, 1, heads *
 * head_dim]; probs_out: NULL, or dense [batch * group, heads, 1, kv_len].  One workgroup serves up to 8 query rows of a
 * (batch row, head) from one pass over K and one over V: K and V are read ceil(group / 8) times, not group times.  For every
 * query row each score, the softmax denominator and every context element are formed and added as
 * osq_decode_attention_fake_quant forms them: out and probs_out are word-equal to that function (to
 * osq_decode_attention_codes) called with k, v and mask repeated `group` times along the batch.  Parameter groups,
 * OSQ_PARAM_SANITIZE, records and the rejected counter as there.  No atomics; no host synchronisation, no allocation: legal
 * inside a stream capture.
 * OSQ_ERR_UNSUPPORTED, nothing launched: group above 64, kv_len outside [1, 1024] (the score rows of 8 queries in 32 KiB of
 * LDS; BART's source positions), head_dim / 4 not a power of two <= 64, a pointer not 16-byte aligned (k / v of the coded
 * form: 4-byte).  group < 1: OSQ_ERR_INVALID_ARGUMENT.  Inference only. */
int osq_decode_attention_shared(const float* q, const float* k, const float* v, const float* mask, float* out,
                                float* probs_out, int64_t batch, int64_t group, int64_t heads, int64_t head_dim,
                                int64_t kv_len, int64_t k_cap, int64_t v_cap,
                                float* probs_scale, void* probs_zero_point, int probs_zp_type, int probs_mode,
                                float probs_grad_factor, int probs_quant_min, int probs_quant_max,
                                float* ctx_scale, void* ctx_zero_point, int ctx_zp_type, int ctx_mode,
                                float ctx_grad_factor, int ctx_quant_min, int ctx_quant_max,
                                osq_stream stream);
int osq_decode_attention_shared_codes(const float* q, const uint8_t* k, const uint8_t* v, const float* mask, float* out,
                                      float* probs_out, int64_t batch, int64_t group, int64_t heads, int64_t head_dim,
                                      int64_t kv_len, int64_t k_cap, int64_t v_cap,
                                      const float* k_scale_eff, const float* k_zp_eff, int k_quant_min,
                                      const float* v_scale_eff, const float* v_zp_eff, int v_quant_min, const int32_t* rejected,
                                      float* probs_scale, void* probs_zero_point, int probs_zp_type, int probs_mode,
                                      float probs_grad_factor, int probs_quant_min, int probs_quant_max,
                                      float* ctx_scale, void* ctx_zero_point, int ctx_zp_type, int ctx_mode,
                                      float ctx_grad_factor, int ctx_quant_min, int ctx_quant_max,
                                      osq_stream stream);

/* ------------------------------------------------------------------ attention over a whole sequence (attention_block.hip) */

/* What QuantizedBertSelfAttention.forward and QuantizedBartAttention._attend run between the q / k / v sites and the output
 * projection -- bmm, (scale, mask add, softmax, attention_probs quantizer), bmm, merge heads + context quantizer -- as ONE
 * launch that never writes the [batch, heads, tokens, kv_len] scores: one workgroup per (batch, head, tile of 32 queries),
 * the tile's score rows in LDS, both products on the fp32-input matrix instruction (v_mfma_f32_32x32x2_f32: a k-ordered
 * chain of fmaf, one rounding per product).  For every (b, h, t):
 *     s[j] = dot(q[t], k[j])                    j < kv_len
 *     v[j] = pre(s[j]) + mask[b, h, t, j]       pre / mask exactly as osq_attention_softmax_fake_quant: alpha != 1:
 *                                               mask + s * alpha; divisor != 1: s / divisor + mask; mask == NULL: no addition
 *     p    = softmax(v)                         max-subtracted, accurate expf, fp32 sum, p = e * (1 / sum); a row with a NaN,
 *                                               a +inf or only -inf entries is NaN (that row only)
 *     p'   = fake_quantize(p)                   the probs_* group
 *     out  = fake_quantize(sum_j p'[j] * v[j])  the ctx_* group, written in the merged layout
 * q: row (b, h, t) starts q_stride_b * b + q_stride_h * h + q_stride_t * t elements into q and holds head_dim contiguous
 * floats; k and v likewise with kv_len rows: dense [B, h, T, d], BERT's permuted views of [B, T, H] and [:, :, :S] views of
 * cache buffers are taken without a copy.  mask: NULL, or additive with a contiguous last axis and element strides
 * mask_stride_b / _h / _t, 0 = broadcast, as in osq_attention_softmax_fake_quant ([B,1,1,S] for BERT, [B,1,T,S] for BART).
 * out: dense [batch, tokens, heads * head_dim].  probs_out: NULL, or dense [batch, heads, tokens, kv_len], receives p'.
 * All fp32.  Each parameter group is (scale, zero_point, zp_type, mode, grad_factor, quant_min, quant_max) as in
 * osq_decode_attention_fake_quant, OSQ_PARAM_SANITIZE included (the repair rides in every workgroup); a NULL scale means no
 * quantizer: the values pass through.  Given p, and given c, the outputs are word-equal to osq_fake_quant_per_tensor.
 * Order contract (csrc/attention_block.hip lists the orders): every sum is in an order fixed by (head_dim, kv_len) alone;
 * no float atomics; the words of a query row do not depend on tokens, on where the row sits in its tile, on batch or
 * heads, or on strides; the columns and rows that pad a ragged tile contribute no term that can change a word, signed
 * zeros included; memory beyond tokens or kv_len is never read.  The order is not rocBLAS's: against the eager sequence the
 * result is equal to a tolerance, not bit for bit.
 * No allocation, no host synchronisation, no workspace: legal inside a stream capture.  Inference only.
 * OSQ_ERR_UNSUPPORTED, nothing launched (the caller runs the eager sequence): head_dim not in {16, 32, 64, 128}; kv_len
 * outside [1, 1024] (32 score rows of 1024 floats are 128 KiB of the CU's 160 KiB of LDS); q / k / v / out not 16-byte
 * aligned, a q / k / v stride that is not a multiple of 4 elements, mask / probs_out not 4-byte aligned.  Both alpha and
 * divisor different from 1: OSQ_ERR_INVALID_ARGUMENT. */
int osq_attention_fake_quant(const float* q, const float* k, const float* v, const float* mask, float* out,
                             float* probs_out, int64_t batch, int64_t heads, int64_t tokens, int64_t kv_len, int64_t head_dim,
                             int64_t q_stride_b, int64_t q_stride_h, int64_t q_stride_t,
                             int64_t k_stride_b, int64_t k_stride_h, int64_t k_stride_t,
                             int64_t v_stride_b, int64_t v_stride_h, int64_t v_stride_t,
                             int64_t mask_stride_b, int64_t mask_stride_h, int64_t mask_stride_t,
                             float alpha, float divisor,
                             float* probs_scale, void* probs_zero_point, int probs_zp_type, int probs_mode,
                             float probs_grad_factor, int probs_quant_min, int probs_quant_max,
                             float* ctx_scale, void* ctx_zero_point, int ctx_zp_type, int ctx_mode,
                             float ctx_grad_factor, int ctx_quant_min, int ctx_quant_max,
                             osq_stream stream);

/* osq_attention_fake_quant for query rows that SHARE their keys and values: `group` = G decoder rows per row of k / v, the
 * layout of osq_decode_attention_shared (several candidates scored against one input).  `batch` counts the rows of k and v.
 * q: [batch * G, heads, tokens, head_dim] by its strides; k / v: [batch, heads, kv_len, head_dim] by theirs; mask: indexed by
 * the SHARED row b (anything broadcastable to [batch, heads, tokens, kv_len]); out: dense [batch * G, tokens, heads *
 * head_dim]; probs_out: NULL or dense [batch * G, heads, tokens, kv_len].  Decoder rows b * G .. b * G + G - 1 attend over
 * row b of k, v and mask.  A workgroup serves one (b, head) and a tile of 32 of the G * tokens query rows of that pair, so
 * every word of k and v is read once per tile of the group, not once per decoder row.
 * CONTRACT: out and probs_out are word for word those of osq_attention_fake_quant on k, v and mask repeated G times along
 * the batch (the words of a query row depend on that row of q alone); with group == 1 this IS osq_attention_fake_quant.
 * Refusals as there, in the same order, with group < 1 "bad shape" (OSQ_ERR_INVALID_ARGUMENT); the INT32_MAX bounds apply
 * to batch * group, to group * tokens and to batch * heads * ceil(group * tokens / 32).  Legal inside a stream capture. */
int osq_attention_fake_quant_shared(const float* q, const float* k, const float* v, const float* mask, float* out,
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
                                    osq_stream stream);

/* ------------------------------------------------------------------ whole-sequence attention on integer codes (attention_int.hip) */

/* osq_attention_fake_quant on the INTEGERS of the q / k / v / probabilities quantizers, both products on the bf16 matrix
 * instruction (v_mfma_f32_32x32x16_bf16) and exact: every operand is s * n with an integer |n| <= 255, exact in bf16; the
 * products are exact in fp32 and fp32 sums below 2**24 are exact in any order.  Inputs, layouts, strides, mask broadcast,
 * alpha / divisor, probs_out and the dense merged out are those of osq_attention_fake_quant; in addition the q_*, k_* and
 * v_* groups are the per-tensor quantizers that produced q, k and v (OSQ_PARAM_SANITIZE included: the repair rides in every
 * workgroup).  The q, k, v and probs groups are required; the ctx group is optional (NULL scale).  For every (b, h, t), with
 * (s_x, zp_x, qmin_x, qmax_x) the repaired, effective parameters of site x:
 *     n_q[t][i] = clamp(rint(q[t][i] / s_q) + zp_q, qmin_q, qmax_q) - zp_q     likewise n_k[j][i], n_v[j][i]: the site's
 *                 quantizer applied once more; on the quantizer's own outputs this is their integer, exactly
 *     N[j]   = sum_i n_q[t][i] * n_k[j][i]            EXACT integer
 *     sc[j]  = float(N[j]) * (s_q * s_k)              s_q * s_k rounded once; |N| < 2**24, so float() is exact
 *     x[j]   = pre(sc[j]) + mask[b, h, t, j]          pre / mask exactly as osq_attention_fake_quant: one rounding per
 *                                                     operation, no contraction into an fma
 *     p      = softmax(x)                             row max exact, ocml expf of x - max, fp32 denominator in an order fixed
 *                                                     by kv_len alone (csrc/attention_int.hip states it), p = e * (1 / sum);
 *                                                     a row with a NaN, a +inf or only -inf is NaN (that row only)
 *     n_p[j] = clamp(rint(p[j] / s_p) + zp_p, qmin_p, qmax_p) - zp_p           probs_out gets float(n_p) * s_p, the word of
 *                                                     osq_fake_quant_per_tensor on p
 *     C[i]   = sum_j n_p[j] * n_v[j][i]               EXACT integer (up to 2**30): fp32 over at most 128 keys at a time, the
 *                                                     chunks added as int32; the chunking is not part of the contract
 *     c[i]   = float(C[i]) * (s_p * s_v)              int -> float round-to-nearest-even, one product
 *     out    = fake_quantize(c) by the ctx group, or c without one; merged [batch, tokens, heads * head_dim]
 * So out is a function of probs_out and v alone, word for word, and the words of a query row do not depend on tokens, on
 * where the row lies, on batch or heads, or on strides.  Memory beyond tokens or kv_len is never read.
 * What the host cannot see the launch checks itself: if the effective zero point of q, k, v or probs is not an integer inside
 * [quant_min, quant_max] (|n| could exceed 255), ALL of out and probs_out is NaN.  A non-finite element of q, k or v makes
 * every output it reaches in the eager sequence NaN and changes no other output.
 * No allocation, no host synchronisation, no workspace, no atomics: legal inside a stream capture.  Inference only.
 * OSQ_ERR_UNSUPPORTED, nothing launched (the caller goes on with osq_attention_fake_quant or the eager sequence): a missing
 * q / k / v / probs group, or one with quant_max - quant_min > 255 or a mode other than FIXED / LSQ / LSQ+ (+ SANITIZE);
 * head_dim not in {16, 32, 64, 128}; kv_len outside [1, 16384]; q / k / v / out not 16-byte aligned, a q / k / v stride
 * that is not a multiple of 4 elements, mask / probs_out not 4-byte aligned.  Both alpha and divisor different from 1:
 * OSQ_ERR_INVALID_ARGUMENT. */
int osq_attention_fake_quant_int(const float* q, const float* k, const float* v, const float* mask, float* out,
                                 float* probs_out, int64_t batch, int64_t heads, int64_t tokens, int64_t kv_len, int64_t head_dim,
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
                                 osq_stream stream);

/* osq_attention_fake_quant_int for query rows that share their keys and values: `group`, `batch`, the layouts of q, k, v,
 * mask, out and probs_out and the row sharing are those of osq_attention_fake_quant_shared; a workgroup serves a tile of 128
 * of the G * tokens query rows of a (b, head).
 * CONTRACT: out and probs_out are word for word those of osq_attention_fake_quant_int on k, v and mask repeated G times along
 * the batch; with group == 1 this IS osq_attention_fake_quant_int.  A bad effective zero point makes ALL of out and
 * probs_out NaN, as there.  Refusals as there, in the same order, with group < 1 "bad shape"; the INT32_MAX bounds apply to
 * batch * group, to group * tokens and to batch * heads * ceil(group * tokens / 128).  Legal inside a stream capture. */
int osq_attention_fake_quant_int_shared(const float* q, const float* k, const float* v, const float* mask, float* out,
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
                                        osq_stream stream);

/* ------------------------------------------------------------------ beam search (beam_select.hip) */

/* The continuations of one beam-search step: what log_softmax, the no-repeat-ngram and min-length logits processors, the add
 * of the running beam scores and torch.topk over [bsz, nb * vocab] compute, without writing anything of the logits' size.
 *     value(b, j, t) = ((x - m) - L) + running_scores[b, j]     x = logits[b * nb + j, t], m = max_t x,
 *                                                               L = log(sum_t exp(x - m)) over the whole row;
 *                      -inf + running_scores[b, j]              when t is banned in row r = b * nb + j
 * each fp32 operation rounded on its own.  The row sum is taken in an order fixed by vocab alone (csrc/beam_select.hip): the
 * same inputs give the same words on every run, wherever the row lies and whatever bsz and nb are.
 * logits: rows = bsz * nb rows of vocab floats, unit stride in a row, rows logits_stride ELEMENTS apart (4-byte aligned is
 * enough).  running_scores: dense [bsz, nb].  seq: int64 token history, rows of at least cur tokens, seq_stride elements
 * apart; read only when ngram > 0 and cur >= ngram.  ban_ids: n_ban <= 16 int64 ids on the device.
 * Banned in row r: every id of ban_ids; and, with n = ngram > 0 and cur >= n, token seq[r, i + n - 1] for every i in
 * [0, cur - n] whose window seq[r, i : i + n - 1] equals the suffix seq[r, cur - n + 1 : cur] (n = 1: every token seen so
 * far).  Ids outside [0, vocab) ban nothing.
 * top_value [bsz, keep] fp32 and top_index [bsz, keep] int64 (the flat index j * vocab + t) receive each batch row's first
 * keep elements in this order: larger value first; equal values by smaller flat index; NaN above every number, NaNs among
 * themselves by flat index (a NaN comes out as the canonical quiet NaN).
 * workspace: at least osq_beam_select_workspace_bytes(bsz, nb, vocab, keep) bytes of device memory, 8-byte aligned, contents
 * arbitrary; one per stream in flight.  Three launches; no host synchronisation, no allocation, nothing read from the host:
 * legal inside a stream capture.
 * OSQ_ERR_INVALID_ARGUMENT, nothing launched: keep > 64, nb > 64, keep > vocab, cur > 4096, n_ban > 16, a workspace that is
 * too small, a row stride below the row's length, a negative or zero extent. */
size_t osq_beam_select_workspace_bytes(int64_t bsz, int64_t nb, int64_t vocab, int64_t keep);
int osq_beam_select(const float* logits, int64_t logits_stride, const float* running_scores, const int64_t* seq,
                    int64_t seq_stride, int64_t cur, int64_t ngram, const int64_t* ban_ids, int64_t n_ban,
                    int64_t bsz, int64_t nb, int64_t vocab, int64_t keep, float* top_value, int64_t* top_index,
                    void* workspace, size_t workspace_bytes, osq_stream stream);

/* osq_beam_select with the position read by the launch: cur = *cur_dev + cur_add (cur_dev one device int32; a captured
 * decoding step passes the KV cache's position word, which after the decoder's increment is the step's cur), so that one
 * captured graph serves every step.  cur_max (0..4096) is the largest position the launch may meet; the host checks go by
 * it: with ngram > 0 and cur_max >= ngram, seq rows hold at least cur_max tokens (seq_stride >= cur_max).  ban_ids apply
 * while cur < ban_below -- the min-length rule, which the host decides for the static form -- and to no step otherwise.
 * The same three kernels; only the second reads the word, once per workgroup.  For every cur in [0, cur_max], top_value
 * and top_index are word-equal to osq_beam_select called with that cur, with ban_ids (cur < ban_below) or with n_ban = 0.
 * A cur outside [0, cur_max]: every word of top_value is the canonical quiet NaN, every top_index is 0, and seq is not
 * read -- no address is formed from a refused position.  Limits, workspace and OSQ_ERR_INVALID_ARGUMENT as for the static
 * form, with cur_max in the place of cur; also a null cur_dev.  No host synchronisation, no allocation. */
int osq_beam_select_at(const float* logits, int64_t logits_stride, const float* running_scores, const int64_t* seq,
                       int64_t seq_stride, const int32_t* cur_dev, int64_t cur_add, int64_t cur_max, int64_t ngram,
                       const int64_t* ban_ids, int64_t n_ban, int64_t ban_below, int64_t bsz, int64_t nb, int64_t vocab,
                       int64_t keep, float* top_value, int64_t* top_index, void* workspace, size_t workspace_bytes,
                       osq_stream stream);

/* ------------------------------------------------------------------ beam search (beam_advance.hip) */

/* The bookkeeping of one beam-search step after the selection, at length cur with a prompt of one token: what
 * model/generation.py::_advance_beams_torch computes from `beam = top_idx // vocab` to `go_on` -- which continuations
 * finished, the nb that go on, the merge into the finished set, the cache rows of the kept beams, the early-stop heuristic
 * and the stopping condition -- in two launches.
 * In: top_value [bsz, keep] fp32 and top_index [bsz, keep] int64 (osq_beam_select's or torch.topk's outputs; an index
 * outside [0, nb * vocab) is taken as the nearest beam: nothing outside the state is read), and the state: running
 * [bsz, nb, max_length] int64, running_scores [bsz, nb] fp32, finished [bsz, nb, max_length] int64, scores [bsz, nb] fp32,
 * finished_len [bsz, nb] int64, done [bsz, nb] bytes (0 / not 0), improvable [bsz] bytes; all dense.  eos_ids: n_eos <= 16
 * int64 ids on the device, or NULL with n_eos = 0.
 * early_stopping: 0 (False), 1 (True), 2 ("never").  len_div = (cur + 1 - 1) ** length_penalty and best_div =
 * best_len ** length_penalty, computed by the host as the Python lines do and handed over as the doubles they are.
 * reciprocal: when set, the division by those scalars is v * (float)(1.0 / div) -- the reciprocal taken in double and rounded
 * to fp32 once: the words of torch's GPU kernel for a division by a host scalar, measured on MI355X; v * (1.0f / (float)div)
 * is NOT that, e.g. for div = 7 ** 0.8 -- and when not set the correctly rounded v / (float)div (torch's CPU kernel).
 * Out, all in buffers of their own (the gathers read the old state: no output may be its input; the host alternates between
 * two sets): the seven state tensors; beam_idx [bsz * nb] int64, the cache row beam + b * nb of every kept beam; next_tokens
 * [bsz * nb] int64 = running_out[:, :, cur]; go_on, one int32 word.  Written as 0 / 1: done_out, improvable_out, go_on.
 * Arithmetic: the torch lines literally -- every fp32 operation rounded on its own, flags multiplied (float(false) * -1e9 is
 * -0.0), the three += on the candidates' scores in the order of the source; hits = cur + 1 >= max_length, or the new token
 * is one of eos_ids.  The two top-k follow osq_beam_select's order: larger value first, equal values by smaller index, NaN
 * above every number.  Token rows are copied over all max_length positions.
 * workspace: at least 4 * bsz bytes of device memory, 4-byte aligned, contents arbitrary; one per stream in flight.  One
 * workgroup per batch row, then one workgroup for go_on; no workgroup waits for another; no host synchronisation, no
 * allocation, nothing read from the host: legal inside a stream capture.
 * OSQ_ERR_INVALID_ARGUMENT, nothing launched: keep > 64, nb > 64, nb > keep, n_eos > 16, max_length > 4096, cur < 1 or
 * cur >= max_length, a non-positive extent, early_stopping outside 0..2, a null tensor, an output pointer equal to its input,
 * a workspace that is too small. */
int osq_beam_advance(const float* top_value, const int64_t* top_index, const int64_t* running, const float* running_scores,
                     const int64_t* finished, const float* scores, const int64_t* finished_len, const uint8_t* done,
                     const uint8_t* improvable, const int64_t* eos_ids, int64_t n_eos, int64_t bsz, int64_t nb, int64_t keep,
                     int64_t vocab, int64_t max_length, int64_t cur, int early_stopping, double len_div, double best_div,
                     int reciprocal, int64_t* running_out, float* running_scores_out, int64_t* finished_out,
                     float* scores_out, int64_t* finished_len_out, uint8_t* done_out, uint8_t* improvable_out,
                     int64_t* beam_idx, int64_t* next_tokens, int32_t* go_on, void* workspace, size_t workspace_bytes,
                     osq_stream stream);

/* osq_beam_advance with the position read by the two launches: cur = *cur_dev + cur_add (cur_dev one device int32), and
 * the two factors read from tables: len_table and best_table hold max_length device floats each, entry c the word the
 * static form derives on the host from len_div / best_div at cur == c -- (float)(1.0 / div) with `reciprocal` set (the
 * kernel multiplies), (float)div without (it divides).  The HOST fills them from the Python expressions of the search; the
 * launch reads the word and re-derives no power.  Entries below 1 are not read.
 * For every cur in [1, max_length), the seven state tensors, beam_idx, next_tokens and go_on are word-equal to
 * osq_beam_advance called with that cur and those divisors.  A cur outside that range: go_on receives -1 and nothing else
 * is written; no address is formed from a refused position.  Limits, workspace and OSQ_ERR_INVALID_ARGUMENT as for the
 * static form (but for cur); also a null cur_dev or table.  No host synchronisation, no allocation. */
int osq_beam_advance_at(const float* top_value, const int64_t* top_index, const int64_t* running,
                        const float* running_scores, const int64_t* finished, const float* scores,
                        const int64_t* finished_len, const uint8_t* done, const uint8_t* improvable, const int64_t* eos_ids,
                        int64_t n_eos, int64_t bsz, int64_t nb, int64_t keep, int64_t vocab, int64_t max_length,
                        const int32_t* cur_dev, int64_t cur_add, int early_stopping, const float* len_table,
                        const float* best_table, int reciprocal, int64_t* running_out, float* running_scores_out,
                        int64_t* finished_out, float* scores_out, int64_t* finished_len_out, uint8_t* done_out,
                        uint8_t* improvable_out, int64_t* beam_idx, int64_t* next_tokens, int32_t* go_on, void* workspace,
                        size_t workspace_bytes, osq_stream stream);

/* ------------------------------------------------------------------ greedy decoding (greedy_advance.hip) */

/* One greedy decoding step after the model, at history length cur: what model/generation.py::_greedy does from
 * `procs(seq, logits)` to its stopping test -- the banned tokens, argmax, the pad / eos lines, the new token into the
 * sequence, the stopping condition -- in three launches that read the logits once.  For every batch row b:
 *     banned (taken as -inf, a NaN included): every id of ban_ids; and the no-repeat-ngram tokens of seq[b, :cur] under
 *         osq_beam_select's rule (window i bans its last token when its first ngram - 1 tokens equal the suffix; nothing when
 *         cur < ngram).  Ids outside [0, vocab) ban nothing.
 *     token = forced, when forced >= 0: every logit is then ignored, NaN included, and none is read
 *             else the arg-max of the banned row: larger value first; equal values by smaller index; -0.0 and +0.0 are equal;
 *             NaN above every number, NaNs among themselves by smaller index -- torch.argmax's and numpy's order.  A row that
 *             is all -inf or all banned gives 0.
 *     with n_eos > 0:  token = unfinished[b] ? token : pad;  unfinished[b] &= token not in eos_ids   (written as 0 / 1)
 *     with n_eos == 0: unfinished is neither read nor written
 *     seq[b, cur] = token (seq may be NULL with ngram == 0: it is then not written), next_tokens[b] = token
 * and go_on (one int32) = (cur + 1 < max_length) && (n_eos == 0 || any row unfinished).  Nothing else of seq is written.
 * logits: bsz rows of vocab floats, unit stride in a row, rows logits_stride ELEMENTS apart (4-byte aligned is enough).
 * seq: int64, rows of max_length tokens, seq_stride elements apart.  ban_ids / eos_ids: n_ban / n_eos <= 16 int64 ids on the
 * device; eos ids are compared, never stored.  unfinished: bsz bytes (0 / not 0).  next_tokens: bsz int64.
 * workspace: at least osq_greedy_advance_workspace_bytes(bsz, vocab) bytes of device memory, 8-byte aligned, contents
 * arbitrary; one per stream in flight.  One workgroup per (row, 4096-token chunk), one per row, one for go_on; no workgroup
 * waits for another; no float atomics: the same inputs give the same words on every run.  No host synchronisation, no
 * allocation, nothing read from the host: legal inside a stream capture.
 * OSQ_ERR_INVALID_ARGUMENT, nothing launched: a non-positive extent, vocab >= 2^31, max_length > 4096, cur < 1 or
 * cur >= max_length, n_ban > 16, n_eos > 16, n_eos > 0 with a null unfinished, forced >= vocab, pad outside [0, vocab) with
 * n_eos > 0 (the tokens that are stored unchecked), a row stride below the row's length, ngram > 0 with a null seq, a
 * workspace that is too small, a null tensor. */
size_t osq_greedy_advance_workspace_bytes(int64_t bsz, int64_t vocab);
int osq_greedy_advance(const float* logits, int64_t logits_stride, int64_t* seq, int64_t seq_stride, int64_t cur,
                       int64_t ngram, const int64_t* ban_ids, int64_t n_ban, int64_t forced, const int64_t* eos_ids,
                       int64_t n_eos, int64_t pad, uint8_t* unfinished, int64_t bsz, int64_t vocab, int64_t max_length,
                       int64_t* next_tokens, int32_t* go_on, void* workspace, size_t workspace_bytes, osq_stream stream);

/* osq_greedy_advance with the position read by the launches: cur = *cur_dev + cur_add (cur_dev one device int32; a captured
 * decoding step passes the KV cache's position word, which after the decoder's increment is the step's cur), so that one
 * captured graph serves every step, forced ones included.  ban_ids apply while cur < ban_below (the min-length rule);
 * forced_bos >= 0 is the token at cur == 1 and forced_eos >= 0 the token at cur == max_length - 1; where both fire, eos wins
 * (the later logits processor).  For every cur in [1, max_length) every output word equals osq_greedy_advance called with
 * that cur and the n_ban / forced the host would have passed.  A cur outside that range: go_on receives -1 and nothing else
 * is written; no address is formed from a refused position.  Limits, workspace and OSQ_ERR_INVALID_ARGUMENT as for the
 * static form (but for cur; forced_bos and forced_eos as forced); also a null cur_dev. */
int osq_greedy_advance_at(const float* logits, int64_t logits_stride, int64_t* seq, int64_t seq_stride,
                          const int32_t* cur_dev, int64_t cur_add, int64_t ngram, const int64_t* ban_ids, int64_t n_ban,
                          int64_t ban_below, int64_t forced_bos, int64_t forced_eos, const int64_t* eos_ids, int64_t n_eos,
                          int64_t pad, uint8_t* unfinished, int64_t bsz, int64_t vocab, int64_t max_length,
                          int64_t* next_tokens, int32_t* go_on, void* workspace, size_t workspace_bytes, osq_stream stream);

/* ------------------------------------------------------------------ seeded sampling (sample_advance.hip) */

/* One sampling step after the model, at history length cur: osq_greedy_advance with a seeded draw in the place of the
 * arg-max.  Bans, the forced token, pad / eos, seq[b, cur], next_tokens, unfinished and go_on are osq_greedy_advance's, word
 * for word; a forced step draws nothing and reads no logit.  Otherwise, for every batch row b:
 *     z = x / temperature (one IEEE fp32 division).  A banned token, a NaN and -inf are out of the draw (weight 0).
 *     top_k >= 1: the survivors are the min(top_k, vocab) largest z left, larger first, equal values by smaller token (-0.0
 *         equals +0.0): exactly top_k of them, ties at the top_k-th value included.  This rank order is their order.
 *     top_k == 0 (with top_p == 1): the survivors are all tokens left, in token order.
 *     weights: m the largest surviving z, w_i = 1 where z_i == m (m = +inf included), else exp(z_i - m)
 *     top_p < 1 (top_k >= 1 only): rank i stays iff sum_{j < i} w_j < top_p * sum_j w_j; rank 0 always stays
 *     u = uniforms[b] when uniforms is given (bsz fp32 values in [0, 1) on the device), else
 *         (word 0 of Philox4x32-10 with key (seed & 0xffffffff, seed >> 32) and counter (b, cur, 0, 0)) >> 8, times 2^-24
 *     token = the first kept survivor with C_i > u * W (C_i the running sum of the kept weights in the survivors' order, W
 *         their total; fp32), the last kept one when rounding leaves none; 0 for a row without a survivor.
 * Every sum has an order fixed by (vocab, top_k) alone, not by the rows' alignment, stride or bsz (sample_advance.hip spells
 * it out); no atomics on device memory: the same inputs give the same words on every run.  The logits are read once with
 * top_k >= 1, once plus one 4096-token chunk per row with top_k == 0.
 * workspace: at least osq_sample_advance_workspace_bytes(bsz, vocab, top_k) bytes of device memory, 8-byte aligned, contents
 * arbitrary; one per stream in flight.  One workgroup per (row, 4096-token chunk), one per row, one for go_on; no workgroup
 * waits for another.  No host synchronisation, no allocation, nothing read from the host: legal inside a stream capture.
 * OSQ_ERR_INVALID_ARGUMENT, nothing launched: what osq_greedy_advance refuses, top_k outside [0, 64], top_p outside (0, 1],
 * a temperature that is not positive and finite.  OSQ_ERR_UNSUPPORTED, nothing launched: top_k == 0 with top_p < 1 (a nucleus
 * over the whole vocabulary: the caller runs its torch lines). */
size_t osq_sample_advance_workspace_bytes(int64_t bsz, int64_t vocab, int64_t top_k);
int osq_sample_advance(const float* logits, int64_t logits_stride, int64_t* seq, int64_t seq_stride, int64_t cur,
                       int64_t ngram, const int64_t* ban_ids, int64_t n_ban, int64_t forced, const int64_t* eos_ids,
                       int64_t n_eos, int64_t pad, uint8_t* unfinished, int64_t bsz, int64_t vocab, int64_t max_length,
                       int64_t* next_tokens, int32_t* go_on, void* workspace, size_t workspace_bytes, uint64_t seed,
                       float temperature, int64_t top_k, float top_p, const float* uniforms, osq_stream stream);

/* osq_sample_advance with the position read by the launches: cur = *cur_dev + cur_add, with ban_below, forced_bos and
 * forced_eos as in osq_greedy_advance_at; the seed is an argument, so one captured graph serves every step of a call.  For
 * every cur in [1, max_length) every output word equals osq_sample_advance called with that cur and the n_ban / forced the
 * host would have passed.  A cur outside that range: go_on receives -1 and nothing else is written; no address is formed
 * from a refused position. */
int osq_sample_advance_at(const float* logits, int64_t logits_stride, int64_t* seq, int64_t seq_stride,
                          const int32_t* cur_dev, int64_t cur_add, int64_t ngram, const int64_t* ban_ids, int64_t n_ban,
                          int64_t ban_below, int64_t forced_bos, int64_t forced_eos, const int64_t* eos_ids, int64_t n_eos,
                          int64_t pad, uint8_t* unfinished, int64_t bsz, int64_t vocab, int64_t max_length,
                          int64_t* next_tokens, int32_t* go_on, void* workspace, size_t workspace_bytes, uint64_t seed,
                          float temperature, int64_t top_k, float top_p, const float* uniforms, osq_stream stream);

/* out[b] = the u osq_sample_advance draws for row b at history length cur with this seed, b in [0, bsz): the same device
 * function as the step's. */
int osq_sample_uniforms(uint64_t seed, int64_t bsz, int64_t cur, float* out, osq_stream stream);

/* Several sequences per input, and the log-probability of every drawn token.  The four _group entry points take the argument
 * list of their namesakes (osq_sample_advance, _at, osq_sample_nucleus, _at) and, before the stream, `group`, `logprobs` and
 * `logprobs_stride`; the namesakes are these with group = 1 and logprobs = NULL.
 *     Rows and groups.  A launch serves bsz = B * G rows; row r is sequence j = r % G of input b = r / G.  G is `group`,
 *         G >= 1 and bsz % G == 0.
 *     The uniform of row r at history length cur is word 0 of Philox4x32-10 with key (seed lo, seed hi) and counter
 *         (b, cur, j, 0), its top 24 bits times 2^-24 (or uniforms[r], bsz values, when given).  With G == 1 this is the
 *         counter (b, cur, 0, 0) above, bit for bit.  A row's draws depend on (seed, b, j, cur) alone: not on G, B or the
 *         launch shape.  Everything else of the step is the namesake's, word for word.
 *     The log-probability: `logprobs` is NULL or fp32, bsz rows logprobs_stride floats apart.  The launch that ends row r
 *         writes the word [r, cur] and no other word of the buffer:
 *             a draw                    lp = (z_tok - m) - logf(W), the first term 0 where z_tok == m (m = +inf included); z, m
 *                                       and W are the fp32 values named above, W the total of the KEPT survivors after top-k /
 *                                       top-p in the kernel's fixed order: the log of the probability with which the rule
 *                                       drew the token
 *             a forced step             0
 *             a row finished before     0 (its token is the pad)
 *             a row without a survivor  -inf
 *         With logprobs == NULL nothing is computed or stored for it; passing a buffer changes no other output word.
 * OSQ_ERR_INVALID_ARGUMENT, nothing launched: what the namesake refuses, group < 1, bsz % group != 0, logprobs given with
 * logprobs_stride < max_length.  osq_sample_uniforms_group: out[r] = the u of row r, r in [0, bsz), under this rule. */
int osq_sample_advance_group(const float* logits, int64_t logits_stride, int64_t* seq, int64_t seq_stride, int64_t cur,
                             int64_t ngram, const int64_t* ban_ids, int64_t n_ban, int64_t forced, const int64_t* eos_ids,
                             int64_t n_eos, int64_t pad, uint8_t* unfinished, int64_t bsz, int64_t vocab, int64_t max_length,
                             int64_t* next_tokens, int32_t* go_on, void* workspace, size_t workspace_bytes, uint64_t seed,
                             float temperature, int64_t top_k, float top_p, const float* uniforms, int64_t group,
                             float* logprobs, int64_t logprobs_stride, osq_stream stream);
int osq_sample_advance_group_at(const float* logits, int64_t logits_stride, int64_t* seq, int64_t seq_stride,
                                const int32_t* cur_dev, int64_t cur_add, int64_t ngram, const int64_t* ban_ids, int64_t n_ban,
                                int64_t ban_below, int64_t forced_bos, int64_t forced_eos, const int64_t* eos_ids,
                                int64_t n_eos, int64_t pad, uint8_t* unfinished, int64_t bsz, int64_t vocab,
                                int64_t max_length, int64_t* next_tokens, int32_t* go_on, void* workspace,
                                size_t workspace_bytes, uint64_t seed, float temperature, int64_t top_k, float top_p,
                                const float* uniforms, int64_t group, float* logprobs, int64_t logprobs_stride,
                                osq_stream stream);
int osq_sample_uniforms_group(uint64_t seed, int64_t bsz, int64_t group, int64_t cur, float* out, osq_stream stream);

/* ------------------------------------------------------------------ a nucleus over the whole vocabulary (sample_nucleus.hip) */

/* One sampling step after the model for top_k == 0 and top_p <= 1, the form osq_sample_advance refuses: every token left is
 * ranked, the nucleus is cut from the ranking and the draw is taken from it -- without a sort.  Bans, the forced token, pad /
 * eos, seq[b, cur], next_tokens, unfinished, go_on and the uniform u (Philox word 0 with key (seed lo, seed hi) and counter
 * (b, cur, 0, 0), or uniforms[b]) are osq_sample_advance's, word for word; a forced step draws nothing and reads no logit.
 * Otherwise, for every batch row b:
 *     z = x / temperature (one IEEE fp32 division), -0.0 taken as +0.0.  A banned token, a NaN and -inf weigh 0.
 *     the survivors rank by larger z first, equal z by smaller token; m the largest z, w_i = 1 where z_i == m (m = +inf
 *         included), else exp(z_i - m)
 *     rank i stays iff the weights ranked above it sum below top_p * total; rank 0 always stays; W = the kept ranks' total
 *     token = the first kept rank whose running sum passes u * W, the last kept rank when rounding leaves none; 0 for a row
 *         without a survivor.
 * top_p == 1 is taken: the plain draw from every token IN RANK ORDER -- not word-equal to osq_sample_advance(top_k = 0,
 * top_p = 1), which walks in token order.
 * How the kernel decides (this fixes the fp32 words; tokens are tolerance-equal to any other summation order).  Let key(z) be
 * the order-preserving 32-bit image of z and S(k) the fp32 sum, in ONE fixed order, of w_i over the tokens with key(z_i) > k;
 * a token not above k adds 0.0f in the same position of the same tree.  Every fp32 add rounds monotonically, so S is
 * non-increasing in k and both searches are bisections over k (at most 32 rounds each), no sort:
 *     the cut:  total = S(0), bound = top_p * total.  k* = the smallest key with S(k*) < bound (a key that is present).  Of the
 *         n tokens with that key, in token order, the j-th (0-based) stays iff S(k*) + float(j) * w(k*) < bound, one multiply
 *         and one add; r >= 1 of them stay, and W = S(k*) + float(r) * w(k*).
 *     the draw: target = u * W.  kv = the smallest key >= k* with S(kv) <= target (present too).  Inside its group the pick is
 *         the first j with S(kv) + float(j + 1) * w(kv) > target, among the r kept ones when kv == k*; the token is the j-th
 *         token with that key, in token order.  When rounding leaves no such j the pick is the group's last eligible token --
 *         for kv == k* the last kept rank.  (key(m) always qualifies as kv: S(key(m)) = 0.)
 * The order of S: the row in 1024 runs of 50 consecutive tokens; a run's tokens 0..24 in order, its tokens 25..49 in order,
 * the two halves added; 64 consecutive runs by four symmetric lane-exchange steps (xor 1, xor 2, mirror of 8, mirror of 16) and
 * then (r0 + r16) + (r32 + r48); the 16 results left to right.  It depends on vocab alone: not on bsz, the rows' stride or
 * alignment.  No atomics on device memory: the same inputs give the same words on every run, and a row's token does not depend
 * on bsz or on its row index but through the Philox counter.  The logits are read once.
 * vocab <= 51200 (what one workgroup holds in registers: 1024 threads of 50 tokens); above it OSQ_ERR_UNSUPPORTED, nothing
 * launched, and osq_sample_nucleus_workspace_bytes returns 0.
 * workspace: at least osq_sample_nucleus_workspace_bytes(bsz, vocab) bytes (the rows' flags: 4 * bsz) of device memory, 8-byte
 * aligned, contents arbitrary; one per stream in flight.  One workgroup per row, then one for go_on; no workgroup waits for
 * another.  No host synchronisation, no allocation, nothing read from the host: legal inside a stream capture.
 * OSQ_ERR_INVALID_ARGUMENT, nothing launched: what osq_sample_advance refuses but for top_k. */
size_t osq_sample_nucleus_workspace_bytes(int64_t bsz, int64_t vocab);
int osq_sample_nucleus(const float* logits, int64_t logits_stride, int64_t* seq, int64_t seq_stride, int64_t cur,
                       int64_t ngram, const int64_t* ban_ids, int64_t n_ban, int64_t forced, const int64_t* eos_ids,
                       int64_t n_eos, int64_t pad, uint8_t* unfinished, int64_t bsz, int64_t vocab, int64_t max_length,
                       int64_t* next_tokens, int32_t* go_on, void* workspace, size_t workspace_bytes, uint64_t seed,
                       float temperature, float top_p, const float* uniforms, osq_stream stream);

/* osq_sample_nucleus with the position read by the launches: cur = *cur_dev + cur_add, with ban_below, forced_bos and
 * forced_eos as in osq_greedy_advance_at.  For every cur in [1, max_length) every output word equals osq_sample_nucleus called
 * with that cur and the n_ban / forced the host would have passed.  A cur outside that range: go_on receives -1 and nothing
 * else is written; no address is formed from a refused position. */
int osq_sample_nucleus_at(const float* logits, int64_t logits_stride, int64_t* seq, int64_t seq_stride,
                          const int32_t* cur_dev, int64_t cur_add, int64_t ngram, const int64_t* ban_ids, int64_t n_ban,
                          int64_t ban_below, int64_t forced_bos, int64_t forced_eos, const int64_t* eos_ids, int64_t n_eos,
                          int64_t pad, uint8_t* unfinished, int64_t bsz, int64_t vocab, int64_t max_length,
                          int64_t* next_tokens, int32_t* go_on, void* workspace, size_t workspace_bytes, uint64_t seed,
                          float temperature, float top_p, const float* uniforms, osq_stream stream);

/* osq_sample_nucleus and osq_sample_nucleus_at for several sequences per input and with the drawn token's log-probability:
 * the rule is stated under "seeded sampling" above.  W is S(k*) + float(r) * w(k*), z_tok the value of the key kv. */
int osq_sample_nucleus_group(const float* logits, int64_t logits_stride, int64_t* seq, int64_t seq_stride, int64_t cur,
                             int64_t ngram, const int64_t* ban_ids, int64_t n_ban, int64_t forced, const int64_t* eos_ids,
                             int64_t n_eos, int64_t pad, uint8_t* unfinished, int64_t bsz, int64_t vocab, int64_t max_length,
                             int64_t* next_tokens, int32_t* go_on, void* workspace, size_t workspace_bytes, uint64_t seed,
                             float temperature, float top_p, const float* uniforms, int64_t group, float* logprobs,
                             int64_t logprobs_stride, osq_stream stream);
int osq_sample_nucleus_group_at(const float* logits, int64_t logits_stride, int64_t* seq, int64_t seq_stride,
                                const int32_t* cur_dev, int64_t cur_add, int64_t ngram, const int64_t* ban_ids, int64_t n_ban,
                                int64_t ban_below, int64_t forced_bos, int64_t forced_eos, const int64_t* eos_ids,
                                int64_t n_eos, int64_t pad, uint8_t* unfinished, int64_t bsz, int64_t vocab,
                                int64_t max_length, int64_t* next_tokens, int32_t* go_on, void* workspace,
                                size_t workspace_bytes, uint64_t seed, float temperature, float top_p, const float* uniforms,
                                int64_t group, float* logprobs, int64_t logprobs_stride, osq_stream stream);

/* ------------------------------------------------------------------ teacher-forced scoring (token_logprob.hip) */

/* The log-probability the model gives a GIVEN token, per row, and the language-model loss over the rows: what
 * -F.cross_entropy(logits, labels, reduction='none' / 'mean', ignore_index) computes, without a tensor of the logits' size.
 * logits: fp32, `rows` rows of `vocab` values `stride` elements apart (stride >= vocab, any parity: a row needs 4-byte
 * alignment only).  labels: int64 [rows].  For row r with label t:
 *     m          the row's maximum (a NaN is no maximum)
 *     W          the sum of expf(z - m) over the row in fp32, -inf logits weighing 0, in an order fixed by vocab alone: the row
 *                in chunks of 4096 tokens; in a chunk, with its own maximum m_c, thread i of 256 adds expf(z - m_c) of the
 *                tokens 4 (i + 256 k) + e in the order k = 0..3, e = 0..3; 64 consecutive threads by four symmetric
 *                lane-exchange steps (xor 1, xor 2, mirror of 8, mirror of 16) and then (r0 + r16) + (r32 + r48); the four
 *                results as (w0 + w1) + (w2 + w3) = W_c; then W = sum over the chunks, in order, of W_c * expf(m_c - m)
 *     lse[r]     = m + logf(W)
 *     logprob[r] = (z_t - m) - logf(W), the first term exactly 0 where z_t == m
 *     t == ignore_index                     logprob[r] = 0; lse[r] is written all the same; the row is not counted as scored
 *     t outside [0, vocab), not ignored     logprob[r] = NaN and the row is counted as bad: no address is formed from such a
 *                                           label, nothing outside the row is read and nothing traps
 *     a row whose maximum is not finite, or that holds a NaN: what the IEEE arithmetic above gives (NaN).  A label on the one
 *     finite value of a row otherwise -inf gives exactly 0, a label on one of its -inf values gives -inf.
 * loss (may be NULL): one fp32, -(sum of the `rows` words of logprob) / scored, the sum in an order fixed by `rows` alone
 *     (thread i of 256 adds the rows i, i + 256, ... in order, then the tree above): NaN where no row was scored, as torch
 *     gives, and NaN where a label was bad.  counts (may be NULL): two int64, {rows scored, rows with a bad label}.
 * A row's words do not depend on rows, on its position or on the grid: one workgroup per (row, chunk) holds the chunk in
 * registers and writes (m_c, W_c) to the workspace; one thread per row merges them and reads z_t; one workgroup forms loss
 * and counts (not launched when both are NULL).  Every logit is read from memory once, nothing of the logits' size is written.
 * No atomics on device memory, no host synchronisation, no allocation: legal inside a stream capture.
 * workspace: at least osq_token_logprob_workspace_bytes(rows, vocab) bytes (8 per row and chunk) of device memory, 8-byte
 * aligned, contents arbitrary; one per stream in flight.  It may be NULL where that size is 0.
 * rows == 0 launches the last kernel alone: loss = NaN, counts = {0, 0}.
 * OSQ_ERR_INVALID_ARGUMENT, nothing launched: with rows > 0 a null logits / labels / logprob / lse / workspace; vocab < 1,
 * vocab > 2^31 - 4097, stride < vocab, rows < 0, more than 2^31 - 1 (row, chunk) pairs (the workspace size is 0 for the last
 * four). */
size_t osq_token_logprob_workspace_bytes(int64_t rows, int64_t vocab);
int osq_token_logprob(const float* logits, int64_t stride, const int64_t* labels, int64_t rows, int64_t vocab,
                      int64_t ignore_index, float* logprob, float* lse, float* loss, int64_t* counts, void* workspace,
                      osq_stream stream);

/* The gradient of the above for the logits, from lse alone: one streaming launch,
 *     dlogits[r, v] = coef_r * (p - [v == t]), p = expf(z - lse[r]),   0 for a row that is ignored or has a bad label
 * and, where vocab <= 4096 (the row is one chunk, one workgroup holds it), p = expf(z - lse[r]) / S with S the fp32 sum of
 * the row's expf(z - lse[r]) in the order of W_c above: S is 1 but for the rounding of lse to one fp32 word, which moves every
 * exponent of the row alike; dividing by it takes that rounding out, so that the dlogits of such a row add up to zero within
 * their own roundings (a short row is where lse's rounding would be large beside them).
 * with coef_r = row_grad[r] where row_grad (fp32 [rows]) is given: the upstream gradient of the row's NEGATIVE log-probability
 * (reduction='none'); else coef_r = scalar_grad[0] / float(counts[0]): the upstream gradient of `loss` over the scored rows
 * the forward counted (reduction='mean'), both read on the device.  dlogits: fp32, rows `dstride` elements apart
 * (dstride >= vocab); the words between the rows are not written.  logits are read once, dlogits written once.
 * OSQ_ERR_INVALID_ARGUMENT, nothing launched: what osq_token_logprob refuses, a null lse / dlogits, dstride < vocab, neither
 * row_grad nor both of scalar_grad and counts.  rows == 0 launches nothing. */
int osq_token_logprob_backward(const float* logits, int64_t stride, const int64_t* labels, const float* lse,
                               const float* row_grad, const float* scalar_grad, const int64_t* counts, int64_t rows,
                               int64_t vocab, int64_t ignore_index, float* dlogits, int64_t dstride, osq_stream stream);

/* ------------------------------------------------------------------ bf16 / fp16 only (lowp.hip) */

/* The three entry points below take OSQ_DTYPE_BF16 / OSQ_DTYPE_F16 only (OSQ_DTYPE_F32 is rejected) and are not folded
 * into the fp32 ones: the in-dtype chain and its backward have no fp32 counterpart (every op is rounded to x's dtype), and
 * the per-tensor widening forward has its own kernel, access pattern and tuning constants. */

/* FixedFakeQuantize per-tensor (util_quant.py:11-15 called with Python numbers or 0-dim tensors) in the input dtype:
 * every op of the chain is rounded to x's dtype, as torch's CPU kernels do --
 *     a = rd(x/s); r = rint(a); b = rd(rd(r - a) + a); c = clamp(rd(b + zp), qmin, qmax); y = rd(rd(c - zp) * s)
 * (rd = round the fp32 result to the dtype, RNE).  scale: 1 fp32 on the device; zero_point: 1 int32 or fp32 (zp_type).
 * x / y: n contiguous elements of `dtype` (16-byte accesses when both are 16-byte aligned, element accesses otherwise). */
int osq_fake_quant_chain_lowp(int dtype, const void* x, void* y, int64_t n, const float* scale, const void* zero_point,
                              int zp_type, int quant_min, int quant_max, osq_stream stream);

/* The autograd backward of the chain above for x: x_int = rd(b + zp) recomputed,
 *     dx = rd(where(qmin <= x_int <= qmax, rd(g * s), +0.0) / s)            (x, grad_out, grad_x: n elements of dtype) */
int osq_fake_quant_chain_backward_lowp(int dtype, const void* x, const void* grad_out, void* grad_x, int64_t n,
                                       const float* scale, const void* zero_point, int zp_type, int quant_min, int quant_max,
                                       osq_stream stream);

/* Per-tensor fake-quant of a bf16 / fp16 x with fp32 [1] parameters (Fixed / LSQ / LSQ+, util_quant.py with >= 1-dim
 * tensors): torch promotes to fp32, so y is fp32 and word-equal to osq_fake_quant_per_tensor on x widened -- the same
 * arguments, OSQ_PARAM_SANITIZE included.  One launch, 2 B read + 4 B written per element. */
int osq_fake_quant_per_tensor_widen(int dtype, const void* x, float* y, int64_t n, float* scale, void* zero_point, int zp_type,
                                    int mode, float grad_factor, int quant_min, int quant_max, osq_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* OSQ_HIP_H */

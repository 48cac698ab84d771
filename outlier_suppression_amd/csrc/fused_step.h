// One launch for a whole quantizer call in the calibrate-and-quantize state (both flags on, fake_quant.py:107-126 /
// 178-208) on a masked [B, T, H] activation: per-token extrema -> token-wise clipping (observer.py:50-70) ->
// running statistic -> calculate_qparams -> fake-quant.  Included by observer.hip after token_select.h.
//
// Why one launch: the scale depends on a reduction over the whole tensor, so a launch-per-stage version reads x
// twice (12 B/elem).  An MI355X holds 128 MiB in its vector register files; a [256,128,768] fp32 tensor is 96 MiB.
// This kernel is a persistent grid of one 1024-thread workgroup per CU in which every wave KEEPS the tokens it
// reduced in registers (24 float4 per lane = 96 VGPRs) until the scale is known, then quantises them from the
// registers: x is read from HBM once, y is written once (8 B/elem of HBM traffic for 12 B/elem of algorithmic
// work), and there are no kernel boundaries inside the call.
//
//   workgroups 0, 1   "selectors", one side each: every wave watches the arrival flags of sixteen streaming workgroups
//                     and pulls a workgroup's per-token extrema into registers as soon as it has published them --
//                     counting and histogramming them on the way (token_select.h, HINT) --, so that when the last
//                     streaming workgroup arrives only its values and the scan are left; then select_from_registers;
//                     each publishes its result as one tagged 8-byte granule;
//   workgroups 2..    "streaming": wave w owns tokens j = w, w + W, w + 2W, ... of an enumeration that lists the valid
//                     tokens first (sample-major) and the padded ones after them.  Phase A1 loads its valid tokens
//                     and reduces them; the extrema go to the workgroup's chunk of the compact arrays with write-through
//                     stores, then the workgroup raises its arrival flag.  Phase A2 loads its padded tokens (they are quantised too:
//                     the reference fake-quantises the whole tensor) while the selectors work.  Phase C: poll the
//                     granules, quantise the held registers, stream y out.  Tokens beyond the register capacity
//                     (24 float4 per lane) are streamed instead: reduced in A1 without being kept, re-read in C.
//
// Hand-offs follow cdna_hip_programming.md G16: payload written with agent-scope (sc1, write-through) stores and
// drained with s_waitcnt vmcnt(0) before the ticket; consumers read it with sc1 loads; every polled word is an
// agent-scope atomic.  No per-launch salt argument (it would be frozen under graph replay): the tag is epoch + 1
// with the epoch counter living in the workspace, read by every workgroup at its start and advanced by the
// finishing selector -- the only launch-to-launch state, and the kernel boundary orders it.  All workgroups must
// be resident together (they spin on each other): the host sizes the grid to min(CUs, occupancy) and every spin
// is bounded -- on a timeout the workgroup raises `status`, writes NaN and leaves.
#pragma once

namespace osq {

constexpr int kFusedThreads = 1024;
constexpr int kFusedWaves = kFusedThreads / OSQ_WAVE;
constexpr int kFusedHoldRegs = 18;        // float4 of activation data a lane keeps in registers across the wait (72 VGPRs)
constexpr int kFusedHoldLds = 9;          // ... and in LDS (9 x 16 B x 1024 threads = 144 KiB of the CU's 160)
constexpr int kFusedMaxBatch = 1024;      // prefix sums of the lengths live in LDS, one entry per thread
constexpr unsigned int kFusedSpinLimit = 1u << 21;

struct FusedState {                       // lives in the caller's workspace; ALL-ZERO before the first launch (or after a reset)
    // Arrival flags: streaming workgroup g stores this launch's tag into flag[(g % 16) * 16 + g / 16] once its extrema
    // have left its CU (selector wave w polls the sixteen words of its own 64-byte line).  A tag is never reused, so
    // nothing has to be reset between launches.  After a TIME-OUT that no longer holds -- a streaming workgroup that
    // becomes resident after workgroup 2 has advanced the epoch computes the next launch's tag -- which is why every
    // reader of a raised status (osq_fused_step_status, osq_persistent_status) wipes this block before the next launch.
    unsigned int flag[256];
    unsigned int epoch, pad0[15];             // launches completed on this workspace
    unsigned long long side[16];              // side[0], side[1]: one granule per selector (tag30 << 34 | empty << 33 | bad << 32 | value bits), adjacent: one 16-byte poll reads both
    unsigned int status, pad3[15];            // sticky: 1 = a selector timed out, 2 = a streaming workgroup timed out
    unsigned int go[2][16];                   // = tag once selector `side` has pulled the per-token extrema into its registers
};

struct FusedArgs {
    const float* x;
    float* y;
    int64_t B, T;                 // rows r = b*T + t at x + r*H, H = 256*NV floats
    const int64_t* lengths;       // NULL: every token is valid
    float* tok_min;               // compact per-token extrema, capacity B*T rounded up to 4 floats each
    float* tok_max;
    int prune;
    float q;
    int shortcut;
    FusedState* st;
    const float* scale_p;         // the module's parameters (also fin.scale_out / fin.zp_out)
    const void* zp_p;
    int zp_type, mode;
    float g, qmin, qmax;
    int gate;                     // 1: padded tokens are loaded only after every workgroup has arrived
    int hint;                     // 1: the selectors histogram a window around the running statistic while the values arrive (token_select.h, HINT)
    unsigned int spin_limit;      // bound of every cross-workgroup wait (kFusedSpinLimit; osq_set_tuning("fused_spin_limit") for tests)
};

__device__ __forceinline__ unsigned long long peek64(const unsigned long long* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned int peek32(const unsigned int* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <typename T>
__device__ __forceinline__ T* uniform_ptr(T* p) {
    const unsigned long long v = reinterpret_cast<unsigned long long>(p);
    const unsigned int lo = uniform(static_cast<unsigned int>(v)), hi = uniform(static_cast<unsigned int>(v >> 32));
    return reinterpret_cast<T*>((static_cast<unsigned long long>(hi) << 32) | lo);
}

__device__ __forceinline__ unsigned long long side_granule(unsigned int tag, const SideResult& r) {
    return (static_cast<unsigned long long>(tag & 0x3fffffffu) << 34) | (r.empty ? (1ull << 33) : 0ull) | (r.bad ? (1ull << 32) : 0ull) |
           __float_as_uint(r.value);
}

// A selector's side of the launch.  The compact arrays hold one CHUNK per streaming workgroup: workgroup g owns the
// tokens j = local * G + g (G streaming workgroups, local = 16 * slot + wave) and writes token j's extremum to
// chunk_start(g) + local; its valid tokens are the first nv(g) = ceil((V - g) / G) of them -- every chunk holds cmax or
// cmax - 1 values.  Selector wave w takes the chunks of workgroups w, w + 16, ...: lane i < 16 polls workgroup
// (w + 16 i)'s flag, and a published chunk is loaded with one dword per lane and absorbed at once (NaN flag, count below
// the hinted window, histogram of the window): the LDS atomics of the first histogram level -- what a CU spends most of
// a selection on -- happen while the streaming workgroups are still arriving.
// One CU retires an instruction of a 16-wave workgroup in ~8 clocks, so the registers are packed: with CH = ceil(cmax/64),
// a chunk's first 64 (CH - 1) values fill CH - 1 registers -- always full --, and the TAILS (cmax - 64 (CH - 1) values or
// one less) of the eight chunks of a group share 1, 2, 4 or 8 registers (tpad = the tail length rounded up to a power of
// two, min(8, 64 / tpad) chunks per register): 18 registers per lane in use instead of 32 at the bench lengths.  noinline: one copy of the selection per CH for the four
// kernel instantiations; the function publishes the side's granule itself, so that what the call costs at its end
// (callee-saved registers coming back from scratch) is behind the hand-off, not in front of it.
template <int CH>
__device__ __attribute__((noinline)) void fused_select(const float* src_, const int side_, const unsigned int total_, const unsigned int V_,
                                                      const int prune_, const float q_, const int shortcut_, const float hint,
                                                      FusedState* st_, const unsigned int tag_, const unsigned int spin_limit_,
                                                      SelShared& S, long long* stamps) {
    constexpr int NC = kFusedWaves;            // chunks per selector wave
    constexpr int NM = NC * (CH - 1);          // registers of full 64-value blocks
    constexpr int R = NM + NC;                 // ... plus at most sixteen tail registers
    // arguments of a called function arrive in VGPRs: tell the compiler they are uniform, or every test below is a vector compare
    const float* const src = uniform_ptr(src_);
    FusedState* const st = uniform_ptr(st_);
    const int side = static_cast<int>(uniform(static_cast<unsigned int>(side_))), prune = static_cast<int>(uniform(static_cast<unsigned int>(prune_)));
    const int shortcut = static_cast<int>(uniform(static_cast<unsigned int>(shortcut_)));
    const unsigned int total = uniform(total_), V = uniform(V_), tag = uniform(tag_), spin_limit = uniform(spin_limit_);
    const float q = __uint_as_float(uniform(__float_as_uint(q_)));
    const int tid = threadIdx.x, lane = tid & (OSQ_WAVE - 1);
    const unsigned int wv = static_cast<unsigned int>(__builtin_amdgcn_readfirstlane(tid / OSQ_WAVE));
    const unsigned int nwg = gridDim.x - 2u;
    const unsigned int qt = total / nwg, rt = total - qt * nwg;      // chunk g starts at g * qt + min(g, rt) ...
    const unsigned int qv = V / nwg, rv = V - qv * nwg;              // ... and holds qv + (g < rv) valid values
    const unsigned int flip = side ? 0x80000000u : 0u;               // side 1 works on -token_min
    const SelWindow win = hint_window(__uint_as_float(uniform(__float_as_uint(hint))), prune);
    const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(src), 0, static_cast<int>(total * 4u), 0x00020000);
    OSQ_SSTAMP(0);

    // A wave's sixteen chunks form GROUPS (chunks GC j .. GC j + GC - 1): a group is loaded and absorbed once all its
    // workgroups have arrived -- one uniform test per group and round: on a 16-wave workgroup every instruction of the
    // polling loop costs ~8 clocks, per-chunk tests made a round longer than the arrivals are apart.  Two groups of eight
    // measured best (bench step kernel 36.9 us; four groups 37.3, eight 38.1, one 37.1; all tokens valid 49.5 / 49.3 / 50.6 /
    // 49.4 -- tools/ab_step.py on one box, -DOSQ_FUSED_GROUPS=n builds).
    // Tails: tlen values (or tlen - 1) per chunk behind its full blocks; the tails of a group share ntg registers.
#ifndef OSQ_FUSED_GROUPS
#define OSQ_FUSED_GROUPS 2
#endif
    constexpr int NG = OSQ_FUSED_GROUPS, GC = NC / NG;               // groups, chunks per group
    constexpr unsigned int kGroupMask = (1u << GC) - 1u;
    const unsigned int cmax = qv + (rv ? 1u : 0u);                   // V > 0: 64 (CH - 1) < cmax <= 64 CH
    const unsigned int tlen = cmax - static_cast<unsigned int>(OSQ_WAVE * (CH - 1));
    const unsigned int lt = tlen <= 1u ? 0u : 32u - static_cast<unsigned int>(__builtin_clz(tlen - 1u));   // tpad = 1 << lt >= tlen
    const unsigned int cpr = (64u >> lt) >= static_cast<unsigned int>(GC) ? static_cast<unsigned int>(GC) : 64u >> lt;   // chunks per tail register: 8, 4, 2, 1
    const unsigned int ntg = static_cast<unsigned int>(GC) / cpr;                                          // tail registers per group: 1, 2, 4, 8
    // registers: [group j: 8 (CH - 1) full blocks][group j: 8 tail registers, ntg of them in use], j = 0, 1
    constexpr int RG = GC * (CH - 1) + GC;                           // per group
    // this lane's place in a tail register: chunk ci of the register's cpr, tail position tl
    const unsigned int ci = static_cast<unsigned int>(lane) >> lt, tl = static_cast<unsigned int>(lane) & ((1u << lt) - 1u);
    const unsigned int lane4 = static_cast<unsigned int>(lane) * 4u;

    for (int k = tid; k < kSelBins; k += kSelThreads) S.hist[k] = 0u;
    if (tid == 0) {
        S.s_fill = 0u; S.s_next = 0xffffffffu; S.s_found[0] = S.s_found[1] = 0xffffffffu; S.s_sel = 0u; S.s_pos = 0u; S.s_late = 0u;
    }
    lds_barrier();
    OSQ_SSTAMP(1);
    const unsigned int limit = spin_limit;

    float v[R];
#pragma unroll
    for (int i = 0; i < R; ++i) v[i] = __builtin_nanf("");
    unsigned int want = 0u;                                           // chunks that exist and hold valid values
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        const unsigned int g = wv + static_cast<unsigned int>(NC * i);
        if (g < nwg && qv + (g < rv ? 1u : 0u) > 0u) want |= 1u << i;
    }
    unsigned int gdone = 0u, below = 0u;                              // groups that are in
#pragma unroll
    for (int j = 0; j < NG; ++j)
        if (((want >> (GC * j)) & kGroupMask) == 0u) gdone |= 1u << j;      // nothing to wait for
    bool bad = false;
    const unsigned int* const flags = &st->flag[wv * NC];
    // One value: sign, NaN flag, and -- hinted -- below-the-window count and the window's histogram.  The range of the
    // keys and the plain maximum are left to select_from_registers (only the paths without a usable window need them).
#define OSQ_ABSORB(reg, okmask)                                                                        \
    do {                                                                                               \
        const float xs = __uint_as_float(__float_as_uint(reg) ^ flip);                                 \
        const bool ok_ = (okmask);                                                                     \
        bad |= ok_ && (xs != xs);                                                                      \
        const float x = ok_ ? xs : __builtin_nanf("");                                                 \
        reg = x;                                                                                       \
        if (win.on) {              /* a poisoned slot's key 0x7fc00000 is neither below nor inside a finite window */ \
            const unsigned int key = abs_key(x), d = key - win.lo;                                     \
            below += key < win.lo ? 1u : 0u;                                                           \
            if (d < win.wd) atomicAdd(&S.hist[d >> win.sh], 1u);                                       \
        }                                                                                              \
    } while (0)
    // Software-pipelined: the poll of round n + 1 is issued right behind the data loads of round n.
    unsigned int f = 0u;
    if (limit && lane < NC) f = peek32(&flags[lane]);
#ifdef OSQ_FINAL_TIMING
    long long dbg_rounds = 0, dbg_empty = 0, dbg_first = 0;
#endif
    constexpr unsigned int kAllGroups = (1u << NG) - 1u;
    for (unsigned int spins = 0; gdone != kAllGroups && spins < limit;) {
        const unsigned int missing = want & ~static_cast<unsigned int>(__ballot(lane < NC && f == tag));   // chunks still awaited
        unsigned int ready = 0u;
#pragma unroll
        for (int j = 0; j < NG; ++j)
            if (((missing >> (GC * j)) & kGroupMask) == 0u) ready |= 1u << j;
        const unsigned int newly = uniform(ready & ~gdone);
#ifdef OSQ_FINAL_TIMING
        if (newly) { if (!dbg_rounds) dbg_first = wall_clock64(); ++dbg_rounds; } else ++dbg_empty;
#endif
        if (!newly) {
            ++spins;
            __builtin_amdgcn_s_sleep(2);
            if (lane < NC) f = peek32(&flags[lane]);
            continue;
        }
        // every load of the round first, then the values
#pragma unroll
        for (int j = 0; j < NG; ++j) {
            if ((newly >> j) & 1u) {
#pragma unroll
                for (int e = 0; e < GC; ++e) {
                    const unsigned int g = wv + static_cast<unsigned int>(NC * (GC * j + e));
                    const unsigned int off = g * qt + (g < rt ? g : rt);
                    // chunk start in the SGPR offset, lane * 4 + c * 256 in the one VGPR / the immediate: no address registers
                    // per load (a chunk that does not exist reads zeros beyond the buffer or a neighbour: masked below)
#pragma unroll
                    for (int c = 0; c < CH - 1; ++c)
                        v[RG * j + e * (CH - 1) + c] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rsrc, lane4 + static_cast<unsigned int>(c * OSQ_WAVE * 4), off * 4u, 16 /* sc1 */));
                }
#pragma unroll
                for (int t = 0; t < GC; ++t) {
                    if (static_cast<unsigned int>(t) < ntg) {
                        const unsigned int i = static_cast<unsigned int>(GC * j) + static_cast<unsigned int>(t) * cpr + ci, g = wv + NC * i;   // per lane
                        const unsigned int off = g * qt + (g < rt ? g : rt) + static_cast<unsigned int>(OSQ_WAVE * (CH - 1)) + tl;
                        v[RG * j + GC * (CH - 1) + t] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rsrc, off * 4u, 0, 16 /* sc1 */));
                    }
                }
            }
        }
        gdone |= newly;
        if (gdone != kAllGroups && lane < NC) f = peek32(&flags[lane]);
#pragma unroll
        for (int j = 0; j < NG; ++j) {
            if ((newly >> j) & 1u) {
#pragma unroll
                for (int e = 0; e < GC; ++e) {
                    const bool exists = (want >> (GC * j + e)) & 1u;                 // uniform
#pragma unroll
                    for (int c = 0; c < CH - 1; ++c) OSQ_ABSORB(v[RG * j + e * (CH - 1) + c], exists);
                }
#pragma unroll
                for (int t = 0; t < GC; ++t) {
                    if (static_cast<unsigned int>(t) < ntg) {
                        const unsigned int i = static_cast<unsigned int>(GC * j) + static_cast<unsigned int>(t) * cpr + ci, g = wv + NC * i;
                        const unsigned int nvg = qv + (g < rv ? 1u : 0u);
                        OSQ_ABSORB(v[RG * j + GC * (CH - 1) + t], ci < cpr && g < nwg && static_cast<unsigned int>(OSQ_WAVE * (CH - 1)) + tl < nvg);
                    }
                }
            }
        }
    }
#undef OSQ_ABSORB
#ifdef OSQ_FINAL_TIMING
    if (lane == 0 && g_osq_dbg) {
        long long* w = g_osq_dbg + 2080 + side * 64 + wv * 4;
        w[0] = wall_clock64(); w[1] = dbg_rounds; w[2] = dbg_empty; w[3] = dbg_first;
    }
#endif
    if (gdone != kAllGroups && lane == 0) S.s_late = 1u;   // a streaming workgroup never arrived
    // the NaN flag and the count below the window: per-wave partials -> LDS -> one barrier -> every thread folds them
    {
        const bool wbad = wave_any(bad);
        below = wave_inclusive_scan_u32(below);
        if (lane == OSQ_WAVE - 1) S.w_below[wv] = below;
        if (lane == 0) S.w_bad[wv] = wbad ? 1u : 0u;
    }
    lds_barrier();
    SelPass0 p0{V, false, 0u, 0u, 0u, false, win, 0u};
    {
        unsigned int nb = 0u, anyb = 0u;
#pragma unroll
        for (int k = 0; k < kSelWaves; k += 4) {
            const uint4 a4 = *reinterpret_cast<const uint4*>(&S.w_below[k]), b4 = *reinterpret_cast<const uint4*>(&S.w_bad[k]);
            nb += a4.x + a4.y + a4.z + a4.w;
            anyb |= b4.x | b4.y | b4.z | b4.w;
        }
        p0.n_below = uniform(nb);
        p0.any_bad = uniform(anyb) != 0u;
    }
    OSQ_SSTAMP(2);
    // the extrema are in registers: the streaming workgroups may use the memory system for their padded tokens
    if (tid == 0) __hip_atomic_store(&st->go[side][0], tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    SideResult r{__builtin_nanf(""), true, false};
    if (S.s_late) {                                        // poison the call instead of hanging
        if (tid == 0) __hip_atomic_fetch_or(&st->status, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
        r = select_from_registers<R, RG, GC * (CH - 1)>(v, p0, prune, q, shortcut, S, stamps, ntg);
    }
    if (tid == 0) __hip_atomic_store(&st->side[side], side_granule(tag, r), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    OSQ_SSTAMP(6);
    OSQ_SDUMP();
}

__device__ __forceinline__ float4 as_float4(const v4u32& w) {
    return make_float4(__uint_as_float(w.x), __uint_as_float(w.y), __uint_as_float(w.z), __uint_as_float(w.w));
}
__device__ __forceinline__ v4u32 as_v4u32(const float4& f) {
    v4u32 w;
    w.x = __float_as_uint(f.x); w.y = __float_as_uint(f.y); w.z = __float_as_uint(f.z); w.w = __float_as_uint(f.w);
    return w;
}

// 16-byte streaming store at (wave-uniform row offset + lane offset).  The offset goes into the VGPR operand, NOT the
// SGPR soffset field: with a register soffset hipcc (ROCm 7.2) pads no wait states between a buffer_store_dwordx4 and
// a following VALU write of its data registers (LLVM's hazard table exempts that form), and on gfx950 the store then
// picks up the NEXT element's v_div_scale result in its first data register for the last four lanes of every row --
// measured here as y.x == scale in ~5 % of the rows, different ones on every run.
__device__ __forceinline__ void store_row16(const v4u32& data, __amdgpu_buffer_rsrc_t rsrc, unsigned int lane_off, unsigned int row_off) {
    // sc1 = write-through: nothing of the 96 MiB of y stays dirty in the L2s for the end of the launch to write back
    // (nt stores: 40.9 us per step, plain 41.5, sc1 or sc0 sc1 38.9, nt sc1 40.5; tools/ab_step.py on one box)
    __builtin_amdgcn_raw_buffer_store_b128(data, rsrc, lane_off + row_off, 0, 16 /* sc1 */);
}

// development aid (-DOSQ_FINAL_TIMING, `make dbg`): thread 0 of every workgroup stamps the 100 MHz wall clock
#ifdef OSQ_FINAL_TIMING
#define OSQ_FSTAMP(k) do { if (threadIdx.x == 0 && g_osq_dbg) g_osq_dbg[blockIdx.x * 8 + (k)] = wall_clock64(); } while (0)
#else
#define OSQ_FSTAMP(k) do { } while (0)
#endif

template <int NV>
__global__ __launch_bounds__(kFusedThreads) void observe_fq_fused_kernel(FusedArgs a, Finish fin) {
    constexpr int SR = kFusedHoldRegs / NV;       // tokens a wave keeps in registers
    constexpr int SL = kFusedHoldLds / NV;        // ... and in LDS
    constexpr int S = SR + SL;
    constexpr int H4 = NV * OSQ_WAVE;             // float4 per token
    constexpr int CH = NV % 4 == 0 ? 4 : 3;       // float4 per lane and trip of the streamed (not held) tokens
    // the selectors' scratch and the streaming workgroups' token slots share the same LDS
    __shared__ union FusedLds {
        SelShared sel;
        v4u32 keep[kFusedWaves * kFusedHoldLds * OSQ_WAVE];
    } lds;
    SelShared& sel_lds = lds.sel;
    v4u32* const keep = lds.keep;
    __shared__ unsigned int pre[kFusedMaxBatch + 1];
    __shared__ unsigned int s_wtot[kFusedWaves];
    __shared__ unsigned int s_word[8];
    __shared__ unsigned int rows[kFusedWaves * 24];

    const int tid = threadIdx.x, lane = tid & (OSQ_WAVE - 1);
    const int wv = __builtin_amdgcn_readfirstlane(tid / OSQ_WAVE);      // wave-uniform, and the compiler knows it
    const unsigned int Bu = static_cast<unsigned int>(a.B), Tu = static_cast<unsigned int>(a.T);
    FusedState* st = a.st;

    OSQ_FSTAMP(0);
    // ---- everybody: epoch of this launch, prefix sums of the clamped lengths
    if (tid == 0) s_word[0] = peek32(&st->epoch);
    {
        unsigned int len = 0u;
        if (static_cast<unsigned int>(tid) < Bu) {
            int64_t l = a.lengths ? a.lengths[tid] : a.T;
            l = l < 0 ? 0 : (l > a.T ? a.T : l);
            len = static_cast<unsigned int>(l);
        }
        const unsigned int incl = wave_inclusive_scan_u32(len);
        if (lane == OSQ_WAVE - 1) s_wtot[wv] = incl;
        __syncthreads();
        unsigned int base = 0u;
#pragma unroll
        for (int k = 0; k < kFusedWaves; ++k) base += (k < wv) ? s_wtot[k] : 0u;
        if (tid == 0) pre[0] = 0u;
        if (static_cast<unsigned int>(tid) < Bu) pre[tid + 1] = base + incl;
        __syncthreads();
    }
    OSQ_FSTAMP(7);
    const unsigned int tag = s_word[0] + 1u;
    const unsigned int V = pre[Bu];                       // valid tokens
    const unsigned int total = Bu * Tu;

    if (blockIdx.x < 2u) {
        // =========================================================== selector (one side)
        const int side = blockIdx.x;
        // the observer's running statistic predicts this batch's threshold (token_select.h, HINT)
        float hint = __builtin_nanf("");
        if (a.hint && fin.rule != OSQ_UPDATE_NONE && fin.min_val && fin.max_val) hint = __builtin_fabsf(side ? fin.min_val[0] : fin.max_val[0]);
        OSQ_FSTAMP(1);
#ifdef OSQ_FINAL_TIMING
        long long* sstamps = g_osq_dbg ? g_osq_dbg + 8 * 256 + 16 * side : nullptr;
#else
        long long* sstamps = nullptr;
#endif
        const float* src = side ? a.tok_min : a.tok_max;
        const unsigned int nwg = gridDim.x - 2u;
        const unsigned int cmax = V ? (V - 1u) / nwg + 1u : 0u;        // valid values of the largest chunk (<= 192: the launcher checks)
#define OSQ_FUSED_SELECT(CH) fused_select<CH>(src, side, total, V, a.prune, a.q, a.shortcut, hint, st, tag, a.spin_limit, sel_lds, sstamps)
        if (cmax <= 1u * OSQ_WAVE) OSQ_FUSED_SELECT(1);
        else if (cmax <= 2u * OSQ_WAVE) OSQ_FUSED_SELECT(2);
        else OSQ_FUSED_SELECT(3);
#undef OSQ_FUSED_SELECT
        OSQ_FSTAMP(3);
        return;
    }

    // =============================================================== streaming workgroup
    const unsigned int nwv = (gridDim.x - 2u) * kFusedWaves;                        // streaming waves
    // what the finishing arithmetic needs, fetched now by the thread that will do it
    float st_min = 0.f, st_max = 0.f, old_s = 0.f, old_z = 0.f;
    const bool have_state = fin.rule != OSQ_UPDATE_NONE && fin.min_val && fin.max_val;
    if (tid == 0) {
        if (have_state) { st_min = fin.min_val[0]; st_max = fin.max_val[0]; }
        old_s = a.scale_p[0];
        old_z = load_zp(a.zp_p, a.zp_type);
    }
    const unsigned int bp = blockIdx.x - 2u;                                         // this workgroup's number among the streaming ones
    // How the W = 16 G tokens of a slot are dealt to the waves (G streaming workgroups): wave w of workgroup bp takes token
    // w * G + bp -- the slot's tokens go round the workgroups one by one -- not 16 * bp + w (16 consecutive tokens per
    // workgroup).  With the latter the same wave of neighbouring workgroups -- they issue their loads and stores at about
    // the same time -- is 16 rows apart, a multiple of 16 KiB at every feature count the kernel takes, and simultaneous
    // requests crowd a few memory channels; and V is rarely a multiple of W: the slot that holds the last valid tokens gave
    // the first (V % W) / 16 workgroups one valid token per wave more than the others (5 against 4 at the bench lengths),
    // and the selection waited for those.  Measured in round 2 (graph replay of the bench step, one box): 44.3 -> 41.5 us
    // ([256,128,768], bench lengths), 55.0 -> 52.8 (all valid), 35.4 -> 33.0 ([32,128,3072]), 21.7 -> 20.0 ([64,128,1024]),
    // 43.6 -> 41.1 ([32,128,4096]); two or four tokens per workgroup, or the workgroups of one XCD on consecutive tokens,
    // measured the same as one; numbering the workgroups in the order they start (a ticket: XCDs receive a launch up to
    // 2 us apart) cost the ticket's round trip, +1.5 us.  So workgroup bp's tokens are j = local * G + bp with
    // local = 16 * slot + wave, and its extrema go to ITS chunk of the compact arrays at position `local`.
    const unsigned int nwg = gridDim.x - 2u;
    const unsigned int gwi = static_cast<unsigned int>(wv) * nwg + bp;
    const unsigned int chunk0 = bp * (total / nwg) + (bp < total % nwg ? bp : total % nwg);       // start of this workgroup's chunk
    // 16 KiB rows (4096 features): workgroup bp starts a token at piece bp % 16, otherwise the workgroups' simultaneous
    // requests are again whole multiples of 16 KiB apart (-1 us of 41 on [32,128,4096]; no effect at 768 / 1024 / 3072)
    const unsigned int prot = NV == 16 ? bp % 16u : 0u;
#define OSQ_FUSED_PIECE(u) ((((static_cast<unsigned int>(u) + prot) >= static_cast<unsigned int>(NV)) ? static_cast<unsigned int>(u) + prot - NV : static_cast<unsigned int>(u) + prot) * 1024u)
#define OSQ_FUSED_TOKEN(k) (static_cast<unsigned int>(k) * nwv + gwi)
    // Rows are addressed as buffer base (SGPR descriptor) + wave-uniform row offset (SGPR) + lane * 16 (one VGPR for
    // every access): no 64-bit address pair per token in flight -- the lanes' registers are for data.
    const unsigned int tensor_bytes = total * static_cast<unsigned int>(H4 * 16);      // < 4 GiB, checked by the launcher
    const auto xrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.x), 0, static_cast<int>(tensor_bytes), 0x00020000);
    const auto yrs = __builtin_amdgcn_make_buffer_rsrc(a.y, 0, static_cast<int>(tensor_bytes), 0x00020000);
    const unsigned int lane_off = static_cast<unsigned int>(lane) * 16u;
    constexpr unsigned int kRowBytes = H4 * 16u;
    constexpr int kNt = 2;                                // aux: non-temporal (streamed once).  Plain, sc0 or sc1 loads instead: 50 us per step against 38.5
    // this wave's LDS slots: float4 (slot s, step u, lane) at keep[((wv * SL + s) * NV + u) * 64 + lane]
    v4u32* const keep_w = keep + static_cast<unsigned int>(wv) * (SL * NV * OSQ_WAVE) + lane;

    // token j of the enumeration -> row b*T + t.  Valid tokens of sample b are j in [pre[b], pre[b+1]); padded ones
    // follow: j - V in [b*T - pre[b], (b+1)*T - pre[b+1]).  b = number of prefix entries (i = 1..B) at or below j:
    // thread (k, w) of the first 16*S threads finds it for slot k of wave w by bisection and leaves the row in LDS.
    // (All sixteen waves counting with ballots, 64 entries at a time, took 3 us: the CU's issue slots, not latency.)
    if (tid < kFusedWaves * S) {
        const unsigned int k = static_cast<unsigned int>(tid) / kFusedWaves, w = static_cast<unsigned int>(tid) % kFusedWaves;
        const unsigned int j = k * nwv + w * nwg + bp;
        unsigned int r = 0u;
        if (j < total) {
            const bool valid = j < V;
            const unsigned int key = valid ? j : j - V;
            unsigned int lo = 0u, hi = Bu;                 // invariant f(lo) <= key < f(hi), f(i) = tokens of this kind before sample i
            while (lo + 1u < hi) {
                const unsigned int mid = (lo + hi) >> 1;   // f(mid) <= key  ->  b >= mid
                const unsigned int f = valid ? pre[mid] : mid * Tu - pre[mid];
                if (f <= key) lo = mid; else hi = mid;
            }
            const unsigned int b = lo;                     // f(b) <= key < f(b + 1); f is monotone, so b is the count
            r = valid ? b * Tu + (key - pre[b]) : b * Tu + (pre[b + 1u] - pre[b]) + (key - (b * Tu - pre[b]));
        }
        rows[tid] = r;
    }
    __syncthreads();
    unsigned int row[S];
#pragma unroll
    for (int k = 0; k < S; ++k) row[k] = uniform(rows[k * kFusedWaves + wv]);
    // A wave's tokens go up with the slot, so its valid slots are the first nval and its slots with a token the first
    // nall: two counts (`k < nval`) instead of a kept condition per slot and phase
    int nval = 0, nall = 0;
#pragma unroll
    for (int k = 0; k < S; ++k) {
        nval += OSQ_FUSED_TOKEN(k) < V ? 1 : 0;
        nall += OSQ_FUSED_TOKEN(k) < total ? 1 : 0;
    }
    OSQ_FSTAMP(1);

    // ---- phase A1: valid tokens -> registers (slots 0..SR-1) / LDS (slots SR..S-1), per-token extrema -> compact arrays
    // hipcc's wait counts cannot see a load behind a branch: with each slot's loads behind their own `j < V`, slot 0 first,
    // the wait in front of every reduction was vmcnt(0) -- no younger load can be ASSUMED issued -- and no reduction
    // overlapped the stream.  So the slots go downwards, slot k inside the `k - 1 < nval` of the slot below it: whoever
    // has issued slot k's loads goes on through slots k - 1 .. 0, on every path their loads are behind slot k's, and the
    // wait in front of slot k's reduction is vmcnt(NV k + NV - 1) .. vmcnt(NV k): its own loads, with everything younger
    // still in flight.  (Loads of ALL slots as straight-line code, through a descriptor of zero records for the slots
    // without a valid token, were countable too, but an out-of-range load still takes its turn in the CU's address and
    // return path: +1.0 us at the bench lengths, +2.1 us on [64,128,1024], tools/ab_step.py on one box.)
    // The extrema stay in the wave -- the pair of the wave's n-th token in lane n % 64, slots and the tokens beyond them
    // alike -- and leave in one masked store pair behind the last reduction (or when 64 are held): vmcnt counts stores
    // too, a publish per token put a write-through round trip in front of the next token's wait.
    static_assert(S <= 9, "OSQ_FUSED_A1_SLOTS lists nine slots");
    v4u32 hold[SR > 0 ? SR : 1][NV];
    float pub_mn = 0.f, pub_mx = 0.f;
    {
        v4u32 tmp[SL > 0 ? SL : 1][NV];
#define OSQ_FUSED_A1_LOAD(k)                                                                                                       \
        if constexpr ((k) < S) {                                                                                                   \
            _Pragma("unroll") for (int u = 0; u < NV; ++u) {                                                                       \
                const v4u32 w = __builtin_amdgcn_raw_buffer_load_b128(xrs, lane_off, row[k] * kRowBytes + OSQ_FUSED_PIECE(u), kNt); \
                if ((k) < SR) hold[(k) < SR ? (k) : 0][u] = w; else tmp[(k) < SR ? 0 : (k) - SR][u] = w;                           \
            }                                                                                                                      \
            __builtin_amdgcn_sched_barrier(0);                /* issued in slot order */                                           \
        }
#define OSQ_FUSED_A1_REDUCE(k)                                                                                                     \
        if constexpr ((k) < S) {                                                                                                   \
            MinMax acc;                                                                                                            \
            acc.init();                                                                                                            \
            _Pragma("unroll") for (int u = 0; u < NV; ++u) {                                                                       \
                const v4u32 w = (k) < SR ? hold[(k) < SR ? (k) : 0][u] : tmp[(k) < SR ? 0 : (k) - SR][u];                          \
                acc.add4(as_float4(w));                                                                                            \
                if ((k) >= SR) keep_w[(((k) - SR) * NV + u) * OSQ_WAVE] = w;                                                       \
            }                                                                                                                      \
            acc.wave_reduce();                                                                                                     \
            acc.poison();                                                                                                          \
            pub_mn = set_lane(pub_mn, acc.mn, (k));                                                                                \
            pub_mx = set_lane(pub_mx, acc.mx, (k));                                                                                \
            __builtin_amdgcn_sched_barrier(0);                /* one token's temporaries at a time: the registers hold data */     \
        }
#define OSQ_FUSED_A1_SLOTS(DO)   /* slots nval - 1 .. 0; nested, not a switch: the structurizer turns a switch that falls through into flag variables */ \
        if (0 < nval) { if (1 < nval) { if (2 < nval) { if (3 < nval) { if (4 < nval) { if (5 < nval) { if (6 < nval) { if (7 < nval) { if (8 < nval) { \
        DO(8) } DO(7) } DO(6) } DO(5) } DO(4) } DO(3) } DO(2) } DO(1) } DO(0) }
        OSQ_FUSED_A1_SLOTS(OSQ_FUSED_A1_LOAD)
        OSQ_FUSED_A1_SLOTS(OSQ_FUSED_A1_REDUCE)
#undef OSQ_FUSED_A1_SLOTS
#undef OSQ_FUSED_A1_REDUCE
#undef OSQ_FUSED_A1_LOAD
    }
    // valid tokens beyond the capacity: reduced now, read again in phase C
    unsigned int npub = static_cast<unsigned int>(nval), pub_local = static_cast<unsigned int>(wv);      // lanes in use; lane 0's place in the chunk
    for (unsigned int j = gwi + static_cast<unsigned int>(S) * nwv; j < V; j += nwv) {
        unsigned int b = 0u;
        for (unsigned int c = 0; c < Bu; c += OSQ_WAVE) {
            const unsigned int i = c + static_cast<unsigned int>(lane) + 1u;
            b += static_cast<unsigned int>(__builtin_popcountll(__ballot(i <= Bu && pre[i <= Bu ? i : Bu] <= j)));
        }
        const unsigned int soff = uniform(b * Tu + (j - pre[b])) * kRowBytes;
        MinMax acc;
        acc.init();
#pragma unroll
        for (int u0 = 0; u0 < NV; u0 += CH) {             // CH float4 in flight per lane: the held tokens keep their registers
            v4u32 v[CH];
#pragma unroll
            for (int u = 0; u < CH; ++u) v[u] = __builtin_amdgcn_raw_buffer_load_b128(xrs, lane_off, soff + (u0 + u) * 1024u, kNt);
#pragma unroll
            for (int u = 0; u < CH; ++u) acc.add4(as_float4(v[u]));
        }
        acc.wave_reduce();
        acc.poison();
        pub_mn = set_lane(pub_mn, acc.mn, static_cast<int>(npub));
        pub_mx = set_lane(pub_mx, acc.mx, static_cast<int>(npub));
        if (++npub == static_cast<unsigned int>(OSQ_WAVE)) {      // (the launcher's limit of 192 values per chunk keeps a wave at 12 today)
            publish_f32(&a.tok_min[chunk0 + pub_local + static_cast<unsigned int>(lane * kFusedWaves)], pub_mn);
            publish_f32(&a.tok_max[chunk0 + pub_local + static_cast<unsigned int>(lane * kFusedWaves)], pub_mx);
            pub_local += OSQ_WAVE * kFusedWaves;
            npub = 0u;
        }
    }
    if (static_cast<unsigned int>(lane) < npub) {
        publish_f32(&a.tok_min[chunk0 + pub_local + static_cast<unsigned int>(lane * kFusedWaves)], pub_mn);
        publish_f32(&a.tok_max[chunk0 + pub_local + static_cast<unsigned int>(lane * kFusedWaves)], pub_mx);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // every publishing wave: its extrema have left this CU
    OSQ_FSTAMP(2);
    __syncthreads();
    if (tid == 0)
        __hip_atomic_store(&st->flag[(bp % kFusedWaves) * kFusedWaves + bp / kFusedWaves], tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    OSQ_FSTAMP(3);

    // ---- phase A2: this wave's padded tokens -> registers / LDS, while the selectors work.  Not before every workgroup
    // has arrived and the selectors hold the extrema (they raise `go`): padded loads issued earlier take bandwidth from the workgroups still in
    // A1 and from the selectors' own loads, and both are what the scale waits for.
    // a.gate: 0 = nothing waits, 1 = every padded load waits, 2 = the register slots' padded tokens are loaded at once
    // (they fill the memory system while the last workgroups finish A1), the LDS slots' after `go`
    if (a.gate != 1) {
#pragma unroll
        for (int k = 0; k < SR; ++k) {
            if (k >= nval && k < nall) {
#pragma unroll
                for (int u = 0; u < NV; ++u)
                    hold[k][u] = __builtin_amdgcn_raw_buffer_load_b128(xrs, lane_off, row[k] * kRowBytes + OSQ_FUSED_PIECE(u), kNt);
            }
        }
        asm volatile("" ::: "memory");
    }
    if (a.gate) {
        if (tid == 0) {
            for (unsigned int spins = 0; spins < a.spin_limit; ++spins) {
                if (peek32(&st->go[0][0]) == tag && peek32(&st->go[1][0]) == tag) break;
                __builtin_amdgcn_s_sleep(2);
            }
        }
        __syncthreads();
    }
    if (a.gate == 1) {
#pragma unroll
        for (int k = 0; k < SR; ++k) {
            if (k >= nval && k < nall) {
#pragma unroll
                for (int u = 0; u < NV; ++u)
                    hold[k][u] = __builtin_amdgcn_raw_buffer_load_b128(xrs, lane_off, row[k] * kRowBytes + OSQ_FUSED_PIECE(u), kNt);
            }
        }
    }
#pragma unroll
    for (int k = SR; k < S; ++k) {
        if (k >= nval && k < nall) {
            v4u32 w[NV];
#pragma unroll
            for (int u = 0; u < NV; ++u) w[u] = __builtin_amdgcn_raw_buffer_load_b128(xrs, lane_off, row[k] * kRowBytes + OSQ_FUSED_PIECE(u), kNt);
#pragma unroll
            for (int u = 0; u < NV; ++u) keep_w[((k - SR) * NV + u) * OSQ_WAVE] = w[u];
        }
    }
    asm volatile("" ::: "memory");

    // ---- wait for the two sides; every workgroup finishes the statistic itself (clip rule, running statistic,
    // calculate_qparams: a few dozen scalar operations) instead of waiting for one finisher to do it and publish again
    if (tid == 0) {
        unsigned long long g0 = 0ull, g1 = 0ull;
        bool ok = false;
        const unsigned long long want = static_cast<unsigned long long>(tag & 0x3fffffffu);
        const auto srs = __builtin_amdgcn_make_buffer_rsrc(st->side, 0, 16, 0x00020000);
        for (unsigned int spins = 0; spins < a.spin_limit; ++spins) {
            const v4u32 w = __builtin_amdgcn_raw_buffer_load_b128(srs, 0, 0, 16);      // sc1: both granules, one request
            g0 = (static_cast<unsigned long long>(w.y) << 32) | w.x;
            g1 = (static_cast<unsigned long long>(w.w) << 32) | w.z;
            ok = (g0 >> 34) == want && (g1 >> 34) == want;
            if (ok) break;
            __builtin_amdgcn_s_sleep(1);
        }
        float s = __builtin_nanf(""), z = s;
        if (!ok) {
            __hip_atomic_fetch_or(&st->status, 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else if ((g0 >> 33) & 1ull) {                    // nothing observed (both sides agree): parameters as they are
            s = old_s;
            z = old_z;
        } else {
            const float up = __uint_as_float(static_cast<unsigned int>(g0)), lo = -__uint_as_float(static_cast<unsigned int>(g1));
            float cur_min = clipped_min(lo, up);           // aminmax(clip(value, lo, up)), observer.py:68,227
            float cur_max = up;
            if (((g0 | g1) >> 32) & 1ull) { cur_min = __builtin_nanf(""); cur_max = cur_min; }
            float mn = cur_min, mx = cur_max;
            if (have_state) {
                mn = st_min;
                mx = st_max;
                apply_update(fin.rule, fin.cnt, cur_min, cur_max, &mn, &mx);
            }
            qparams_from_range(mn, mx, fin.quant_min, fin.quant_max, fin.symmetric, &s, &z);
            if (blockIdx.x == 2u) {                        // ONE workgroup writes the module's buffers
                if (fin.cur) { fin.cur[0] = cur_min; fin.cur[1] = cur_max; }     // this batch's own row (sharded calibration)
                if (have_state) { fin.min_val[0] = mn; fin.max_val[0] = mx; }
                fin.scale_out[0] = s;
                store_zp(fin.zp_out, fin.zp_type, 0, z);
            }
            if (fin.zp_type != OSQ_ZP_FLOAT32) z = static_cast<float>(static_cast<int32_t>(z));   // what a reader of the int32 buffer sees
        }
        if (blockIdx.x == 2u)                              // ... and closes the launch's bookkeeping: the epoch moves on (every workgroup read it at its start -- unless a time-out let one start late: see FusedState)
            __hip_atomic_store(&st->epoch, tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_word[2] = __float_as_uint(s);
        s_word[3] = __float_as_uint(z);
        OSQ_FSTAMP(4);
    }
    __syncthreads();
    OSQ_FSTAMP(5);
    const QParams p = effective_params(__uint_as_float(s_word[2]), __uint_as_float(s_word[3]), a.mode & OSQ_PARAM_MODE_MASK, a.g);
    const float qs = p.scale, qz = p.zp;

    // ---- phase C: quantise from the registers / LDS
#pragma unroll
    for (int k = 0; k < S; ++k) {
        if (k < nall) {
#pragma unroll
            for (int u = 0; u < NV; ++u) {
                const v4u32 w = k < SR ? hold[k < SR ? k : 0][u] : keep_w[((k - SR) * NV + u) * OSQ_WAVE];
                float4 o, q;
                fq4_plain(as_float4(w), o, q, qs, qz, a.qmin, a.qmax);
                store_row16(as_v4u32(o), yrs, lane_off, row[k] * kRowBytes + OSQ_FUSED_PIECE(u));
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
    // tokens beyond the capacity: stream
    for (unsigned int j = gwi + static_cast<unsigned int>(S) * nwv; j < total; j += nwv) {
        unsigned int b = 0u, r;
        if (j < V) {
            for (unsigned int c = 0; c < Bu; c += OSQ_WAVE) {
                const unsigned int i = c + static_cast<unsigned int>(lane) + 1u;
                b += static_cast<unsigned int>(__builtin_popcountll(__ballot(i <= Bu && pre[i <= Bu ? i : Bu] <= j)));
            }
            r = b * Tu + (j - pre[b]);
        } else {
            for (unsigned int c = 0; c < Bu; c += OSQ_WAVE) {
                const unsigned int i = c + static_cast<unsigned int>(lane) + 1u;
                b += static_cast<unsigned int>(__builtin_popcountll(__ballot(i <= Bu && i * Tu - pre[i <= Bu ? i : Bu] <= j - V)));
            }
            r = b * Tu + (pre[b + 1u] - pre[b]) + ((j - V) - (b * Tu - pre[b]));
        }
        const unsigned int soff = uniform(r) * kRowBytes;
#pragma unroll
        for (int u0 = 0; u0 < NV; u0 += CH) {
            v4u32 v[CH];
#pragma unroll
            for (int u = 0; u < CH; ++u) v[u] = __builtin_amdgcn_raw_buffer_load_b128(xrs, lane_off, soff + (u0 + u) * 1024u, kNt);
#pragma unroll
            for (int u = 0; u < CH; ++u) {
                float4 o, q;
                fq4_plain(as_float4(v[u]), o, q, qs, qz, a.qmin, a.qmax);
                store_row16(as_v4u32(o), yrs, lane_off, soff + (u0 + u) * 1024u);
            }
        }
    }
    OSQ_FSTAMP(6);
#undef OSQ_FUSED_TOKEN
#undef OSQ_FUSED_PIECE
}

}  // namespace osq

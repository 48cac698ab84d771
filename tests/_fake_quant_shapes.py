"""Launch shapes, inputs, expected words and guard-banded outputs for the NINE forward fake-quant kernels of
csrc/fake_quant.hip: dense vector, scalar fallback, strided scalar, strided vector, head split, head split for several
sites, per-channel rows, per-channel generic and the GELU form.  No GPU is needed to import this module or to run its
predictor; tests/test_oracle_fake_quant_shapes.py checks it on the CPU, tests/test_gpu_fake_quant_shapes.py uses it.

Expected words: oracle/fake_quant_oracle.py (the separately rounded fp32 chain).  anchor() ties those words to plain
float64 arithmetic, so that the oracle and the kernels cannot share an error unnoticed.
"""
from typing import NamedTuple

import numpy as np

from oracle import fake_quant_oracle as FQ

F32 = np.float32

# ------------------------------------------------------------------ the launchers' constants, each with the line it restates
BLOCK = 256             # fake_quant.hip: constexpr int kThreads = 256;
WAVE = 64               # osq_device.h:   #define OSQ_WAVE 64
FQ_CAP = 8192           # fake_quant.hip: OSQ_AB_KNOB(int, g_fq_max_blocks, 8192);  (dense vector, strided vector, head split, GELU)
FQ_UNROLL = 2           # fake_quant.hip: OSQ_AB_KNOB(int, g_fq_unroll, 2);         (sizes the dense grid; unroll of the y-only kernel)
Q_UNROLL = 4            # fake_quant.hip: if (x_quant) { OSQ_FQ_NT(true, 4) }       (unroll of the return_quantized kernel)
VEC_UNROLL = 2          # fake_quant.hip: fq_headsplit_kernel<2, NT>, fq_tensor_vec_kernel<false, 2, NT, true>, `i += 2 * stride`
MAX_BLOCKS = 2048       # osq_host.h:     constexpr int kMaxBlocks = 2048;          (scalar, strided scalar, per-channel generic)
ROWS_CAP = 4096         # fake_quant.hip: grid_for(rows, kThreads / OSQ_WAVE, kMaxBlocks * 2)   (per-channel rows: 4 rows a workgroup)
HEADSPLIT_CAP = 8192    # fake_quant.hip: std::min(g_fq_max_blocks, 8192)
HEADSPLIT_MAX_DV = 64   # fake_quant.hip: dvv >= 1 && dvv <= 64
HEADSPLIT_SITES = 4     # fake_quant.hip: constexpr int kHeadSplitSites = 4;
ROW_LOADS = {4: 4, 2: 2}    # osq_device.h: Granule<float>::kRowLoads = 4, Granule<T>::kRowLoads = 2 (bf16 / fp16), by itemsize
GRANULE = {4: 4, 2: 8}      # osq_device.h: Granule<float>::kPer = 4, Granule<T>::kPer = 8: elements of one 16-byte load
ROWS_MIN_INNER = 64     # fake_quant.hip: inner % G::kPer == 0 && inner >= 64
LSQ_EPS = F32(1.1920928955078125e-07)   # osq_device.h: kLsqEps
# The tables stop far below two more bounds of the launchers: the write-through descriptor (kWtMaxFloat4 = 2^28 - 1 float4,
# 4 GiB) and the 2^30 float4 of the 32-bit index maps.  A test of either needs tensors of 4 to 16 GiB: out of scope.

ZP_INT32, ZP_FLOAT32 = 0, 1
MODE_CODE = {"fixed": 0, "lsq": 1, "lsqplus": 2}
SANITIZE = 16


def grid_for(items, per_block, cap=MAX_BLOCKS):
    """osq_host.h: grid_for."""
    return max(1, min(cap, (items + per_block - 1) // per_block))


# ------------------------------------------------------------------ which loops a launch reaches

def stream_loops(n, stride, unroll):
    """Loops of `for (; i + (U-1)*S < n; i += U*S) body; for (; i < n; i += S) rem;` over the threads i0 = 0..S-1:
    body (some thread runs the unrolled body), body2 (twice), rem (some thread runs the remainder loop), rem2 (twice),
    rem_after_body (one thread runs both: only possible once the grid is capped)."""
    S, U, loops = stride, unroll, set()
    trips = 0 if n <= (U - 1) * S else (n - (U - 1) * S - 1) // (U * S) + 1        # of thread 0, which runs the most
    if trips >= 1:
        loops.add("body")
    if trips >= 2:
        loops.add("body2")
    r = n % (U * S)
    if r:
        loops.add("rem")
        if n > U * S:
            loops.add("rem_after_body")
        if U >= 3 and r > S:
            loops.add("rem2")
    return loops


def stream_loops_brute(n, stride, unroll):
    """The same by walking every thread (the CPU test compares the two)."""
    loops = set()
    for i0 in range(stride):
        i, b, m = i0, 0, 0
        while i + (unroll - 1) * stride < n:
            b += 1
            i += unroll * stride
        while i < n:
            m += 1
            i += stride
        loops |= {k for k, on in (("body", b >= 1), ("body2", b >= 2), ("rem", m >= 1), ("rem2", m >= 2),
                                  ("rem_after_body", b >= 1 and m >= 1)) if on}
    return loops


def _flat_loops(n, grid):
    return {"trip1"} | ({"trip2"} if n > grid * BLOCK else set())


def predict_per_tensor(n, aligned=True, want_q=False, unroll=FQ_UNROLL, cap=FQ_CAP):
    """osq_fake_quant_per_tensor -> (kernel, loops)."""
    if not aligned:
        return ("scalar_q" if want_q else "scalar"), _flat_loops(n, grid_for(n, BLOCK, MAX_BLOCKS))
    n4, tail = divmod(n, 4)
    grid = grid_for(n4, BLOCK * unroll, cap)                       # sized by g_fq_unroll whichever kernel runs
    loops = stream_loops(n4, grid * BLOCK, Q_UNROLL if want_q else unroll)
    if tail:
        loops.add("tail")
    if grid == cap:
        loops.add("capped")
    return ("dense_q" if want_q else "dense"), loops


def predict_gelu(n, cap=FQ_CAP):
    """osq_gelu_fake_quant_per_tensor -> (kernel, loops)."""
    n4, tail = divmod(n, 4)
    grid = grid_for(max(n4, 1), BLOCK * VEC_UNROLL, cap)
    loops = stream_loops(n4, grid * BLOCK, VEC_UNROLL)
    if tail:
        loops.add("tail")
    return "gelu", loops


def is_headsplit(sizes, xs, ys):
    """The launcher's pattern: x = [B,T,h,d] memory seen as [B,h,T,d], y dense, d / 4 a power of two <= 64."""
    s, dv = sizes, sizes[3] // 4
    return (dv >= 1 and dv & (dv - 1) == 0 and dv <= HEADSPLIT_MAX_DV
            and xs[0] == s[2] * s[1] * s[3] and xs[1] == s[3] and xs[2] == s[1] * s[3]
            and ys[0] == s[1] * s[2] * s[3] and ys[1] == s[2] * s[3] and ys[2] == s[3])


def predict_strided(sizes, xs, ys, aligned=True, want_q=False, headsplit=1, cap=FQ_CAP):
    """osq_fake_quant_per_tensor_strided -> (kernel, loops); strides in elements."""
    n = int(np.prod(sizes, dtype=np.int64))
    vec = (not want_q and xs[3] == 1 and ys[3] == 1 and sizes[3] % 4 == 0 and aligned
           and all(a % 4 == 0 and b % 4 == 0 and a >= 0 and b >= 0 for a, b in zip(xs[:3], ys[:3])))
    if vec and headsplit and is_headsplit(sizes, xs, ys):
        grid = grid_for(n // 4, BLOCK * VEC_UNROLL, min(cap, HEADSPLIT_CAP))
        loops = stream_loops(n // 4, grid * BLOCK, VEC_UNROLL)
        return "headsplit", loops | ({"capped"} if grid == min(cap, HEADSPLIT_CAP) else set())
    if vec:
        grid = grid_for(n // 4, BLOCK * VEC_UNROLL, cap)
        loops = stream_loops(n // 4, grid * BLOCK, VEC_UNROLL)
        return "strided_vec", loops | ({"capped"} if grid == cap else set())
    return ("strided_scalar_q" if want_q else "strided_scalar"), _flat_loops(n, grid_for(n, BLOCK, MAX_BLOCKS))


def predict_headsplit_multi(n_sites, B, T, h, d, cap=FQ_CAP):
    """osq_fake_quant_headsplit_multi -> (kernel, loops): every site walks a grid of cap / n_sites + 1 workgroups at most."""
    n4 = B * T * h * d // 4
    site_cap = min(cap, HEADSPLIT_CAP) // n_sites + 1
    grid = grid_for(n4, BLOCK * VEC_UNROLL, site_cap)
    loops = stream_loops(n4, grid * BLOCK, VEC_UNROLL)
    return "headsplit_multi", loops | ({"capped"} if grid == site_cap else set())


def predict_channel(outer, channels, inner, itemsize=4, aligned=True):
    """osq_fake_quant_per_channel -> (kernel, loops).  Rows kernel: a wave walks a row (the row's loops are those of 64 lanes
    over inner / granule loads), row_trip2 = some wave walks a second row."""
    g = GRANULE[itemsize]
    if aligned and inner % g == 0 and inner >= ROWS_MIN_INNER:
        rows = outer * channels
        grid = grid_for(rows, BLOCK // WAVE, ROWS_CAP)
        loops = {"row_" + k for k in stream_loops(inner // g, WAVE, ROW_LOADS[itemsize])}
        if rows > grid * (BLOCK // WAVE):
            loops.add("row_trip2")
        return "channel_rows", loops
    n = outer * channels * inner
    return "channel_generic", _flat_loops(n, grid_for(n, BLOCK, MAX_BLOCKS))


# every loop of every kernel: the tables below must reach each (tests/test_oracle_fake_quant_shapes.py)
ALL_LOOPS = {
    "dense": {"body", "body2", "rem", "rem_after_body", "tail", "capped"},
    "dense_q": {"body", "rem", "rem2", "tail", "capped"},    # U = 4 on a grid sized for 2: the body needs the cap
    "scalar": {"trip1", "trip2"}, "scalar_q": {"trip1", "trip2"},
    "strided_scalar": {"trip1", "trip2"}, "strided_scalar_q": {"trip1"},
    "strided_vec": {"body", "rem", "rem_after_body", "capped"},
    "headsplit": {"body", "body2", "rem", "rem_after_body", "capped"},
    "headsplit_multi": {"body", "rem"},
    "channel_rows": {"row_body", "row_body2", "row_rem", "row_rem2", "row_rem_after_body", "row_trip2"},
    "channel_generic": {"trip1", "trip2"},
    "gelu": {"body", "rem", "tail"},
}

# ------------------------------------------------------------------ shape tables: (shape, the loop it is there for)
_WG = 2 * BLOCK * 4                                   # elements one workgroup of the y-only dense kernel covers per trip
DENSE_SMALL = [(1, "tail"), (2, "tail"), (3, "tail"), (4, "rem"), (5, "tail"), (1023, "rem"), (1024, "rem"), (1027, "tail"),
               (1028, "body"), (_WG - 1, "body"), (_WG, "body"), (_WG + 1, "tail"), (_WG + 4, "rem"), (_WG + 6, "tail"),
               (3 * _WG - 5, "body"), (5 * _WG + 1027, "rem")]
DENSE_LARGE_N4 = 3 * FQ_CAP * BLOCK + 300             # 300 float4 above 3 * 8192 * 256: the x_quant body and a second U=2 body trip
DENSE_LARGE = 4 * DENSE_LARGE_N4 + 3
SCALAR = [(1, "trip1"), (3, "trip1"), (255, "trip1"), (257, "trip1"), (2049, "trip1"), (MAX_BLOCKS * BLOCK + 37, "trip2")]
SCALAR_OFFSETS = (4, 8, 12)
GELU = [(1, "tail"), (3, "tail"), (4, "rem"), (6, "tail"), (1025, "tail"), (2047, "tail"), (2048, "body"), (6 * 1024 + 2, "tail")]
# strided scalar: (base shape, slices as (start, stop, step) per axis, element offset of the base, want x_quant, reason)
STRIDED_SCALAR = [
    ((1000,), ((3, 997, 3),), 0, False, "trip1"),
    ((37, 21), ((1, 36, 1), (2, 19, 1)), 0, False, "trip1"),                  # innermost 17: no multiple of 4
    ((5, 9, 14), ((0, 5, 2), (1, 9, 1), (0, 13, 1)), 1, False, "trip1"),       # misaligned base
    ((3, 4, 6, 10), ((0, 3, 1), (0, 4, 2), (1, 6, 1), (0, 10, 3)), 0, False, "trip1"),
    ((3, 5, 7, 12), ((0, 3, 1), (1, 5, 1), (0, 7, 2), (0, 12, 1)), 0, True, "trip1"),   # a view the vector kernel would take, with x_quant
    ((MAX_BLOCKS * BLOCK // 64 + 2, 130), ((0, None, 1), (0, 65, 1)), 0, False, "trip2"),
]
# strided vector: (base shape, view builder name, reason); built by strided_vec_view()
STRIDED_VEC = [
    ((3, 5, 7, 24), "slice_last_4:20", "body"),          # sizes[3] / 4 = 4 at an aligned offset
    ((2, 10, 3, 4), "step_middle", "rem"),               # sizes[3] / 4 = 1, stepped axis 1
    ((5, 6, 7, 12), "step_middle", "body"),              # sizes[3] / 4 = 3, sizes[1] = 3, sizes[2] = 7
    ((1, 5, 2, 64), "expand_0_to_3", "body"),            # stride 0, sizes[3] / 4 = 16
    ((3, 1, 11, 64), "expand_1_to_5", "body"),           # stride 0 in the middle
    ((2, 5, 3, 512), "headsplit_view", "body"),          # d / 4 = 128: the head-split pattern, beyond its kernel
    ((33, 512, 4, 256), "headsplit_view_d512", "capped"),   # [33,512,2,512] seen as [33,2,512,512]: 2 * 8192 * 256 + 131072 float4
]
HEAD_D = (4, 8, 16, 32, 64, 128, 256)
HEAD_H = (1, 3, 12, 16)
HEAD_T = (1, 5, 37, 128)
HEAD_B = (1, 3)
HEADSPLIT_LARGE = (65, 512, 12, 64)                    # B, T, h, d: 6 389 760 float4 > 3 * 8192 * 256
HEADSPLIT_MULTI = [(1, 5, 3, 8), (3, 37, 12, 64), (1, 1, 1, 4), (3, 128, 16, 32), (1, 37, 3, 256), (3, 1, 12, 128)]
# per-channel rows: inner in granules by itemsize, then (outer, channels) layouts
ROWS_INNER_G = {4: (16, 17, 63, 64, 65, 191, 192, 193, 255, 256, 257, 449, 513), 2: (8, 9, 63, 64, 65, 127, 128, 129, 193, 257)}
ROWS_LAYOUTS = [(1, 5), (3, 7)]
ROWS_TRIP2 = (1, ROWS_CAP * 4 + 5, 64)                 # outer, channels, inner: 16 389 rows
GENERIC = [  # (shape, ch_axis, element offset of the base, reason)
    ((7, 1), 0, 0, "trip1"), ((5, 3), 0, 0, "trip1"), ((4, 63), 0, 0, "trip1"), ((9, 66), 0, 0, "trip1"),
    ((3, 4, 66), 1, 0, "trip1"), ((6, 5, 7), 2, 0, "trip1"), ((12, 64), 0, 1, "trip1"),
    ((MAX_BLOCKS * BLOCK // 63 + 2, 63), 0, 0, "trip2"),
]


def knob_sizes(blocks, unroll):
    """n4 around the trips of a grid capped at `blocks` workgroups (tests on the tunable build)."""
    S = blocks * BLOCK
    return [0, 1, unroll * S - 1, unroll * S, unroll * S + 1, 2 * unroll * S + S + 5]


# ------------------------------------------------------------------ parameter sets and expected words

class Params(NamedTuple):
    name: str
    mode: str          # "fixed" / "lsq" / "lsqplus"
    zp_float: bool     # fp32 zero point (else int32)
    scale: float
    zp: float
    qmin: int
    qmax: int
    g: float
    sanitize: bool
    sigma: float


P_FIXED = Params("fixed_i32", "fixed", False, 0.11, 29, 0, 63, 1.0, False, 3.0)
P_LSQ = Params("lsq_i32", "lsq", False, 0.037, 17, 0, 63, 0.0123, False, 3.0)
P_LSQPLUS = Params("lsqplus_f32", "lsqplus", True, 0.0123, -3.25, -128, 127, 0.002, False, 1.0)
P_POW2 = Params("fixed_pow2", "fixed", False, 0.5, 0, -8, 7, 1.0, False, 2.0)            # exact ties
P_FINE = Params("lsqplus_fine", "lsqplus", True, 3e-4, 100.0, 0, 255, 0.01, False, 0.05)
P_SANITIZE = Params("lsqplus_sanitize", "lsqplus", True, -0.037, 80.5, 0, 63, 0.004, True, 3.0)   # negative scale, zero point out of range
P_SANITIZE_LSQ = Params("lsq_sanitize", "lsq", False, -0.11, 29, 0, 63, 0.05, True, 3.0)
PARAM_SETS = (P_FIXED, P_LSQ, P_LSQPLUS, P_POW2, P_FINE, P_SANITIZE, P_SANITIZE_LSQ)
MAIN_SETS = (P_FIXED, P_LSQ, P_LSQPLUS, P_SANITIZE)


def repaired(P):
    """(scale, zero_point) as fp32 after the SANITIZE repair of osq_device.h tensor_params -- scale.abs_().clamp_(min=eps),
    and for LSQ+ with its fp32 zero point zero_point.clamp_(qmin, qmax) -- which the launch must also write back."""
    s, z = F32(P.scale), F32(P.zp)
    if P.sanitize:
        s = np.maximum(np.abs(s), LSQ_EPS)
        if P.mode == "lsqplus" and P.zp_float:
            z = np.clip(z, F32(P.qmin), F32(P.qmax))
    return F32(s), F32(z)


def effective(P):
    """The fp32 (scale, zero_point) that reach the quantizer."""
    s, z = repaired(P)
    se, ze = FQ.lsq_effective(s, z, F32(P.g), P.mode)
    return F32(se), F32(ze)


def expected(x, P):
    """(x_quant, y) of the oracle for a per-tensor parameter set."""
    se, ze = effective(P)
    q = FQ.quantize_affine(x, se, ze, P.qmin, P.qmax)
    return q, FQ.dequantize_affine(q, se, ze)


def channel_params(channels, P, seed):
    """Per-channel (scale, zero_point) around a parameter set: fp32 arrays (zero point integer-valued for int32 storage)."""
    rng = np.random.default_rng(seed)
    s = (F32(abs(P.scale)) * rng.uniform(0.5, 2.0, channels)).astype(F32)
    z = rng.integers(P.qmin, P.qmax + 1, channels).astype(F32)
    if P.zp_float:
        z = (z + rng.uniform(-0.4, 0.4, channels)).astype(F32)
    return s, z


def expected_channel(x, s, z, ch_axis, P):
    """(x_quant, y) of the oracle, per channel; no SANITIZE form exists per channel (include/osq_hip.h)."""
    se, ze = FQ.lsq_effective(s, z, F32(P.g), P.mode)
    shp = [1] * x.ndim
    shp[ch_axis] = -1
    se, ze = np.asarray(se, F32).reshape(shp), np.asarray(ze, F32).reshape(shp)
    q = FQ.quantize_affine(x, se, ze, P.qmin, P.qmax)
    return q, FQ.dequantize_affine(q, se, ze)


# ------------------------------------------------------------------ the float64 anchor of those words

EXEMPT_SHARE = 1e-3


def anchor(x, q, y, s_eff, z_eff, qmin, qmax):
    """Check the fp32 words (q, y) for FINITE x against float64 arithmetic with no fp32 intermediate:
        u = x64 / s64,  q64 = clip(rint(u) + z, qmin, qmax),  y64 = (q - z) * s64.
    An element is exempt from the integer comparison only if | |u - floor(u)| - 0.5 | <= |u| * 2^-23 (the fp32 quotient is
    within 2^-24 relative of u: only such an element can round to the other side; factor 2 of margin).  Asserts that the
    exempt share is at most 1e-3 (so no caller passes by exempting its failures), q == q64 outside it (for a zero point
    that is no integer: to the one rounding of the sum, 2^-24), and |y - y64| <= 2^-23 |y64| everywhere.
    s_eff / z_eff broadcast against x.  Returns (exempt share, q disagreements inside the exempt set, max y error / |y64|)."""
    x64 = np.asarray(x, np.float64)
    s64, z64 = np.asarray(s_eff, np.float64), np.asarray(z_eff, np.float64)
    assert np.isfinite(x64).all() and (s64 > 0).all()
    u = x64 / s64
    assert (np.abs(u) < 2.0 ** 127).all(), "the anchor is for quotients that fp32 holds"
    exempt = np.abs(np.abs(u - np.floor(u)) - 0.5) <= np.abs(u) * 2.0 ** -23
    share = float(exempt.mean()) if exempt.size else 0.0
    assert share <= EXEMPT_SHARE, share
    q64 = np.clip(np.rint(u) + z64, qmin, qmax)
    q_ = np.asarray(q, np.float64)
    if (z64 == np.rint(z64)).all():
        bad = q_ != q64
    else:
        bad = np.abs(q_ - q64) > 2.0 ** -24 * np.abs(q64)
    assert not (bad & ~exempt).any(), int((bad & ~exempt).sum())
    y64 = (q_ - z64) * s64
    err = np.abs(np.asarray(y, np.float64) - y64)
    assert (err <= 2.0 ** -23 * np.abs(y64)).all()
    nz = y64 != 0
    rel = float((err[nz] / np.abs(y64[nz])).max()) if nz.any() else 0.0
    return share, int((bad & exempt).sum()), rel


# ------------------------------------------------------------------ inputs

def specials(scale):
    """The fixed list of special inputs for a quantizer of scale `scale` (> 0): NaN, +-inf, +-0, +-subnormal, a value whose
    quotient overflows (-> inf -> NaN through round_ste), and ties (k + 0.5) * scale -- exact, and decided identically in
    fp32 and float64, when the scale is a power of two."""
    s = F32(abs(scale))
    big = F32(3.0e38) if s < 1 else F32(np.finfo(F32).max)
    ties = [F32((k + 0.5)) * s for k in (0, 1, 2, -1, -2, -3, 6, 7)]
    return np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-40, -1e-40, big, -big] + ties, dtype=F32)


def normal_data(n, P, seed):
    """Seeded normal data of the parameter set's sigma; a few columns (of rows of 64) are outliers, 8 sigma wide."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n) * P.sigma).astype(F32)
    for col in (5, 41, 62):
        x[col::64] *= F32(8.0)
    return x


def plant(x, positions, scale):
    """Write the specials, in turn, at the given flat positions of x (in place); positions out of range are dropped."""
    sp = specials(scale)
    flat = x.reshape(-1)
    pos = sorted({int(p) for p in positions if 0 <= int(p) < flat.size})
    for k, p in enumerate(pos):
        flat[p] = sp[k % sp.size]
    return x


def stream_positions(n, grid, unroll):
    """Structural element positions of a 16-byte streaming launch over n elements: the first and last element, the last
    float4 of every unrolled trip and the float4 after it (the first of the next trip or of the remainder loop), the first
    float4 of every later stride of the grid, and every tail element."""
    n4, S = n // 4, grid * BLOCK
    pos = {0, 1, 2, 3, n - 1}
    f4 = set()
    for k in range(1, 4):
        f4 |= {k * unroll * S - 1, k * unroll * S, k * unroll * S + 1}
    for k in range(1, 3 * unroll + 1):
        f4 |= {k * S - 1, k * S}
    r = n4 - n4 % (unroll * S)
    f4 |= {r - 1, r, n4 - 1}
    for f in f4:
        if 0 <= f < n4:
            pos |= {4 * f, 4 * f + 3}
    pos |= set(range(4 * n4, n))
    return pos


def row_positions(rows, inner):
    """First and last element of every row (at most 64 rows spread over the tensor, the first and last among them)."""
    pick = sorted(set(np.linspace(0, rows - 1, min(rows, 64)).astype(np.int64).tolist()))
    return {r * inner for r in pick} | {r * inner + inner - 1 for r in pick}


def per_tensor_input(n, P, seed, grid=1, unroll=FQ_UNROLL):
    x = normal_data(n, P, seed)
    return plant(x, stream_positions(n, grid, unroll), repaired(P)[0])


def strided_vec_view(t, how):
    """The view of table STRIDED_VEC named `how`, of a torch tensor t of the table's base shape."""
    if how == "slice_last_4:20":
        return t[..., 4:20]
    if how == "step_middle":
        return t[:, ::2]
    if how == "expand_0_to_3":
        return t.expand(3, -1, -1, -1)
    if how == "expand_1_to_5":
        return t.expand(-1, 5, -1, -1)
    if how == "headsplit_view":                       # t = [B, T, h, d] memory
        return t.permute(0, 2, 1, 3)
    if how == "headsplit_view_d512":                  # t = [B, T, 4, 256] memory = [B, T, 2, 512]
        return t.reshape(t.shape[0], t.shape[1], 2, 512).permute(0, 2, 1, 3)
    raise ValueError(how)


def slice_view(t, slices):
    return t[tuple(slice(a, b, c) for a, b, c in slices)]


# ------------------------------------------------------------------ guard-banded device outputs

SENTINEL = 0x7FC5A5A5          # a quiet NaN whose payload no arithmetic here produces
GUARD = 4096                   # floats on each side of the payload (a multiple of 4: the payload keeps the buffer's alignment)
CANON_NAN = np.uint32(0x7FC00000)


class Guarded:
    """n floats at byte offset `offset` (mod 16) inside a larger device buffer; payload and guards pre-filled with SENTINEL."""

    def __init__(self, n, device, offset=0, guard=GUARD):
        import torch
        assert offset % 4 == 0 and 0 <= offset < 16 and guard % 4 == 0 and guard >= 4096
        self.n, self.start = n, guard + offset // 4
        self.buf = torch.full((guard + n + guard + 4,), SENTINEL, dtype=torch.int32, device=device)
        assert self.buf.data_ptr() % 16 == 0
        self.t = self.buf.view(torch.float32)[self.start:self.start + n]
        assert self.t.data_ptr() % 16 == offset

    def ptr(self):
        return self.t.data_ptr()

    def report(self):
        """(payload words as uint32 with NaNs other than the sentinel canonicalised, any guard word changed, number of payload
        words that still hold the sentinel)."""
        w = self.buf.cpu().numpy().view(np.uint32)
        guards_hit = bool((w[:self.start] != SENTINEL).any() or (w[self.start + self.n:] != SENTINEL).any())
        pay = w[self.start:self.start + self.n].copy()
        unwritten = pay == SENTINEL
        nan = (np.isnan(pay.view(F32))) & ~unwritten
        pay[nan] = CANON_NAN
        return pay, guards_hit, int(unwritten.sum())


def words(a):
    """uint32 words of an fp32 array, every NaN canonical."""
    a = np.ascontiguousarray(np.asarray(a, F32)).reshape(-1)
    w = a.view(np.uint32).copy()
    w[np.isnan(a)] = CANON_NAN
    return w


def check_guarded(g, want, tag):
    """The three checks of every case: words equal to the oracle's, no guard word changed, no payload word left unwritten."""
    pay, guards_hit, unwritten = g.report()
    assert not guards_hit, (tag, "a word outside the output changed")
    assert unwritten == 0, (tag, "payload words never written", unwritten, np.flatnonzero(pay == SENTINEL)[:8].tolist())
    w = words(want)
    if not np.array_equal(pay, w):
        bad = np.flatnonzero(pay != w)
        raise AssertionError((tag, "words differ", bad.size, bad[:8].tolist(), pay[bad[:4]].view(F32).tolist(),
                              w[bad[:4]].view(F32).tolist()))

"""The three 16-bit-only kernels of csrc/lowp.hip -- the in-dtype chain, its backward, the per-tensor widening form -- on the
whole input domain and at every loop edge: tables of expected words, predictors of the launchers, size and alignment tables.
No GPU is needed to import this module; tests/test_oracle_lowp_shapes.py checks it on the CPU, tests/test_gpu_lowp_shapes.py
uses it.

A bf16 / fp16 input is one of 65536 words, so what a kernel must give for ANY tensor is a table lookup:
    y[i]  = y_table[x[i]]                                             (chain forward)
    dx[i] = in_range[x[i]] ? g_table[g[i]] : zero_word                (chain backward: the mask depends on x alone, the kept
                                                                       value rd(rd(g * s) / s) on g alone)
    y[i]  = widen_table[x[i]]                                         (widening form, fp32 words)
The 16-bit tables come from tests/_lowp_chain.py (pinned to plain torch arithmetic on the whole domain by the CPU file), the
fp32 ones from oracle/fake_quant_oracle.py on the exactly widened values.
"""
import functools
from types import SimpleNamespace as NS
from typing import NamedTuple

import numpy as np

import _lowp_chain as L
from oracle import fake_quant_oracle as FQ

F32 = np.float32
DTYPES = sorted(L.DTYPES)
ALL_WORDS = np.arange(65536, dtype=np.uint16)

# (bit, symmetric, scale, zero_point): the nine sets of tests/golden/lowp.npz, then a fine scale, a scale above every fp16
# quotient's ulp, a scale whose products underflow in fp16, and a zero point at quant_max.  A float zero point is a float here.
PARAMS = (
    (8, False, 0.0371, 128), (8, True, 0.05, 0), (4, False, 0.25, 7), (4, True, 0.25, 0), (2, False, 0.5, 1),
    (6, False, 0.01, 30), (5, True, 0.125, 0), (8, False, 0.0371, 127.5), (3, False, 0.3, 2.25),
    (8, False, 3e-5, 100), (8, True, 1024.0, 0), (8, False, 1e-30, 3), (6, False, 0.07, 63),
)
# beyond the thirteen: a negative scale (a Python number passes through the reference unrepaired): exact zeros of either sign
EVERY_WORD_PARAMS = PARAMS + ((8, True, -0.05, 0),)
EDGE_PARAMS = (PARAMS[0], PARAMS[7])       # 190 to 258 distinct outputs: a shifted or repeated granule shows


def qrange(bit, symmetric):
    return (-(1 << (bit - 1)), (1 << (bit - 1)) - 1) if symmetric else (0, (1 << bit) - 1)


def param_id(p):
    return f"{p[0]}{'s' if p[1] else 'a'}-{p[2]:g}-{p[3]:g}"


# ------------------------------------------------------------------ tables of the chain

@functools.lru_cache(maxsize=None)
def chain_tables(dn, params):
    """y_table, in_range_table, g_table (uint16 / bool arrays of 65536 entries, NaNs canonical), zero_word, the kept x word
    the g table was taken against, and the sentinel for outputs of this (dtype, parameter set)."""
    dt = L.DTYPES[dn]
    bit, sym, s, zp = params
    qmin, qmax = qrange(bit, sym)
    y = L.canon(L.chain_forward(ALL_WORDS, dt, s, zp, qmin, qmax), dt)
    xi = L.x_int(ALL_WORDS, dt, s, zp)
    in_range = (xi >= F32(qmin)) & (xi <= F32(qmax))          # from x_int itself: a probe with g = 1 cannot tell when g * s rounds to 0
    kept = int(np.flatnonzero(in_range)[0])
    g = L.canon(L.chain_backward(np.full(65536, kept, np.uint16), ALL_WORDS, dt, s, zp, qmin, qmax), dt)
    with np.errstate(all="ignore"):
        zero_word = int(L.to_words(F32(0.0) / F32(s), dt).reshape(-1)[0])
    for a in (y, in_range, g):
        a.setflags(write=False)
    return NS(y=y, in_range=in_range, g=g, zero_word=zero_word, kept=kept, qmin=qmin, qmax=qmax,
              sentinel=_free_word(y, g, zero_word))


def expected_dx(t, x_words, g_words):
    """dx words of the factorised backward for tables t."""
    return np.where(t.in_range[x_words], t.g[g_words], np.uint16(t.zero_word)).astype(np.uint16)


SENTINEL_START = 0x5A5A


def _free_word(y, g, zero_word):
    """The first word from SENTINEL_START upwards that is finite in both dtypes and that neither table holds.  No ONE word is free of
    all of PARAMS (the g tables of the power-of-two scales are near permutations of the domain, and between them they hold
    every finite word), so the sentinel is chosen per (dtype, parameter set)."""
    used = np.zeros(65536, bool)
    used[y] = used[g] = True
    used[zero_word] = True
    for w in range(SENTINEL_START, 0x10000):
        if not used[w] and all((w & m) != m for m in L._EXP_MASK.values()):        # finite read as either dtype
            return w
    raise AssertionError("no finite word outside the tables")


# ------------------------------------------------------------------ tables of the widening form

MODE_CODE = {"fixed": 0, "lsq": 1, "lsqplus": 2}
SANITIZE = 16                                                  # include/osq_hip.h: OSQ_PARAM_SANITIZE
LSQ_EPS = F32(np.finfo(np.float32).eps)                        # osq_device.h: kLsqEps


class Widen(NamedTuple):
    name: str
    mode: str          # "fixed" / "lsq" / "lsqplus"
    sanitize: bool
    zp_float: bool     # fp32 zero point (else int32)
    scale: float
    zp: float
    qmin: int
    qmax: int
    g: float


W_FIXED_I32 = Widen("fixed_i32", "fixed", False, False, 0.0371, 128, 0, 255, 1.0)
W_FIXED_F32 = Widen("fixed_f32", "fixed", False, True, 0.0371, 127.5, 0, 255, 1.0)
WIDEN_MODES = (
    W_FIXED_I32, W_FIXED_F32,
    Widen("lsq", "lsq", False, False, 0.0371, 128, 0, 255, 0.37),
    Widen("lsqplus", "lsqplus", False, True, 0.05, 3.25, -128, 127, 2.0 ** -6),
    Widen("sanitize_lsq_negative", "lsq", True, False, -0.0371, 128, 0, 255, 0.37),
    Widen("sanitize_lsq_below_eps", "lsq", True, False, 3e-9, 17, 0, 63, 0.37),
    Widen("sanitize_lsqplus_zp_high", "lsqplus", True, True, -0.11, 80.5, 0, 63, 2.0 ** -6),
)
WIDEN_EDGE_MODES = (W_FIXED_I32, W_FIXED_F32)                  # EDGE_PARAMS as the widening form takes them


def repaired(W):
    """(scale, zero_point) as fp32 after the repair osq_device.h tensor_params states for OSQ_PARAM_SANITIZE: scale.abs_(),
    scale.clamp_(min=eps), and for LSQ+ with an fp32 zero point zero_point.clamp_(qmin, qmax).  The launch writes them back."""
    s, z = F32(W.scale), F32(W.zp)
    if W.sanitize:
        s = np.maximum(np.abs(s), LSQ_EPS)
        if W.mode == "lsqplus" and W.zp_float:
            z = np.clip(z, F32(W.qmin), F32(W.qmax))
    return F32(s), F32(z)


def f32_words(a):
    """uint32 words of an fp32 array, every NaN canonical."""
    a = np.ascontiguousarray(np.asarray(a, F32)).reshape(-1)
    w = a.view(np.uint32).copy()
    w[np.isnan(a)] = CANON_NAN32
    return w


@functools.lru_cache(maxsize=None)
def widen_table(dn, W):
    """fp32 words (NaNs canonical) of the oracle's fake-quant of every word of the dtype, widened exactly."""
    x = L.to_f32(ALL_WORDS, L.DTYPES[dn])
    s, z = repaired(W)
    if W.mode == "fixed":
        _, y = FQ.fake_quantize_per_tensor_affine(x, s, z, W.qmin, W.qmax)
    elif W.mode == "lsq":
        _, y = FQ.fake_quantize_learnable_per_tensor(x, s, z, W.qmin, W.qmax, F32(W.g))
    else:
        _, y = FQ.fake_quantize_learnableplus_per_tensor(x, s, z, W.qmin, W.qmax, F32(W.g))
    w = f32_words(y)
    w.setflags(write=False)
    return w


# ------------------------------------------------------------------ sentinels and guard bands

SENTINEL32 = 0x7FC5A5A5        # fp32 outputs: a quiet NaN whose payload no arithmetic here produces (a widened 16-bit NaN has a
CANON_NAN32 = np.uint32(0x7FC00000)   # zero low half); compared as a word, every OTHER NaN is canonicalised
GUARD = 256                    # elements on each side of an output (a multiple of 8: the payload keeps the buffer's alignment)

# ------------------------------------------------------------------ the launchers' constants, each with the line it restates
BLOCK = 256                    # lowp.hip: constexpr int kThreads = 256;
CHAIN_UNROLL = 2               # lowp.hip: constexpr int kUnroll = 2;
WIDEN_UNROLL = 4               # lowp.hip: constexpr int kWidenUnroll = 4;
CAP = 8192                     # lowp.hip: constexpr int kMaxGrid = 8192;
CHAIN_VEC = 8                  # elements of one 16-byte granule of T
WIDEN_VEC = 4                  # elements a lane reads at once in the widening kernel (8 bytes in, 16 bytes out)
G = CAP * BLOCK * CHAIN_UNROLL * CHAIN_VEC          # 33,554,432 elements: the chain's grid reaches the cap
assert G == CAP * BLOCK * WIDEN_UNROLL * WIDEN_VEC  # ... and the widening kernel's at the same size


def grid_for(items, per_block, cap):
    """osq_host.h: grid_for."""
    return max(1, min(cap, (items + per_block - 1) // per_block))


def thread_loops(n_vec, stride, unroll):
    """The distinct (unrolled trips, remainder iterations) over the threads i0 = 0 .. stride-1 of
        for (; i + (U-1)*S < n; i += U*S) body;   for (; i < n; i += S) rem;
    by walking the loops for every thread (vectorised), with the pair of thread 0 and of the last thread."""
    i0 = np.arange(stride, dtype=np.int64)
    reach = n_vec - i0 - (unroll - 1) * stride
    trips = np.where(reach > 0, (reach - 1) // (unroll * stride) + 1, 0)
    left = n_vec - (i0 + trips * unroll * stride)
    rem = np.where(left > 0, (left - 1) // stride + 1, 0)
    pairs = {(int(k) >> 8, int(k) & 255) for k in np.unique(trips * 256 + rem)}      # rem < unroll <= 4
    return pairs, (int(trips[0]), int(rem[0])), (int(trips[-1]), int(rem[-1]))


def _predict(n, vec, unroll, loop_unroll, vector_ok):
    n_vec = n // vec if vector_ok else 0
    grid = grid_for(n_vec if n_vec else (n + vec - 1) // vec, BLOCK * unroll, CAP)
    stride = BLOCK * grid
    forms = set()
    pairs, first, last = thread_loops(n_vec, stride, loop_unroll)
    for trips, rem in pairs:
        if trips:
            forms.add(f"unrolled×{trips}")
        if rem:
            forms.add(f"remainder×{rem}")
        if trips and rem:
            forms.add("unrolled then remainder")
    tail = n - n_vec * vec
    if not vector_ok:
        forms.add("elements only")
    elif tail:
        forms.add("tail")
    if grid == CAP:
        forms.add("capped")
    return NS(n_vec=n_vec, grid=grid, stride=stride, forms=forms, tail=tail if vector_ok else 0, pairs=pairs, first=first, last=last,
              element_passes=(tail + stride - 1) // stride)


def predict_chain(n, x_off=0, y_off=0):
    """lowp.hip launch_chain + lowp_chain_kernel; offsets in bytes past a 16-byte boundary."""
    return _predict(n, CHAIN_VEC, CHAIN_UNROLL, CHAIN_UNROLL, x_off % 16 == 0 and y_off % 16 == 0)


def predict_backward(n, x_off=0, g_off=0, dx_off=0):
    """lowp.hip launch_chain_backward + lowp_chain_backward_kernel: the grid is sized as the forward's (two granules a lane),
    the kernel has ONE plain strided loop -- the unrolled loop with an unroll of 1, so its forms are unrolled×k: k passes."""
    return _predict(n, CHAIN_VEC, CHAIN_UNROLL, 1, x_off % 16 == 0 and g_off % 16 == 0 and dx_off % 16 == 0)


def predict_widen(n, x_off_bytes=0, y_off_bytes=0):
    """lowp.hip launch_widen_tensor + lowp_widen_tensor_kernel: the vector path needs x 8-byte and y 16-byte aligned."""
    return _predict(n, WIDEN_VEC, WIDEN_UNROLL, WIDEN_UNROLL, x_off_bytes % 8 == 0 and y_off_bytes % 16 == 0)


# ------------------------------------------------------------------ size and alignment tables

def _sizes(n_vecs, vec, tails):
    return sorted({v * vec + t for v in n_vecs for t in tails} - {0})


# granule counts on both sides of 1 and of 256, 512, 1024: where a lane's first unrolled trip, the last remainder-only launch
# and the second workgroup begin (predict_chain says which); tails 0, 1 and the longest
CHAIN_SIZES = _sizes((0, 1, 2, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025), CHAIN_VEC, (0, 1, 7))
# ... and of 256, 512, 768, 1024 (remainder ×1, ×2, ×3, the first unrolled trip), 1025 and 2049 (a grid of 2 and of 3)
WIDEN_SIZES = _sizes((0, 1, 2, 255, 256, 257, 258, 511, 512, 513, 767, 768, 769, 770, 1023, 1024, 1025, 1026, 2047, 2048, 2049,
                      2050), WIDEN_VEC, (0, 1, 3))
# the smallest sizes at which the grid cap binds (G is fixed by the launcher's constants; not a workload)
CHAIN_CAPPED = (G, G + 13, 5 * G // 2 + 25)
BACKWARD_CAPPED = (G + 13,)
WIDEN_CAPPED = (G, G + 7, 9 * G // 4 + 13)

# byte offsets of each pointer past a 16-byte boundary
CHAIN_ALIGN = ((0, 0), (2, 0), (0, 2), (2, 2))                                  # (x, y)
BACKWARD_ALIGN = ((0, 0, 0), (2, 0, 0), (0, 2, 0), (0, 0, 2), (2, 2, 2))        # (x, g, dx)
WIDEN_ALIGN = ((0, 0), (2, 0), (8, 0), (0, 4), (0, 16), (8, 16), (2, 4))        # (x, y): x + 8 and y + 16 stay on the vector path

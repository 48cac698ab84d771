"""Numpy restatement of the integer linear rule (include/osq_hip.h, "integer linear"; csrc/linear_int.hip) -- int64 sums,
float32 steps -- the raw-to-effective parameter helpers, and the seeded cases tests/test_linear_int_cpu.py,
tests/test_gpu_linear_int.py and tests/test_gpu_linear_int_edges.py share."""
from collections import namedtuple

import numpy as np

from oracle import fake_quant_oracle as FQ

F32 = np.float32
EPS32 = F32(np.finfo(np.float32).eps)                          # the learnable quantizers' `eps` buffer (kLsqEps of csrc/osq_device.h)
MODES = FQ.MODES                                               # "fixed", "lsq", "lsqplus": the library's PARAM_FIXED / _LSQ / _LSQPLUS
RANGES = {"asym8": (0, 255), "sym8": (-128, 127), "asym6": (0, 63), "sym6": (-32, 31)}
# (input range, where its zero point lies, weight range, where its zero points lie, per-channel weights)
QUANTS = (("asym8", "inside", "sym8", "inside", True), ("asym6", "inside", "sym6", "inside", True),
          ("asym8", "qmin", "asym8", "qmax", False), ("asym8", "qmax", "asym8", "qmin", True),
          ("sym8", "inside", "asym6", "inside", False))
Quant = namedtuple("Quant", "scale zero_point qmin qmax")      # effective parameters: float32 arrays of 1 or N entries


def _mode(mode):
    return mode if isinstance(mode, str) else MODES[int(mode) & 3]     # a launch mode may carry PARAM_SANITIZE


def effective(raw_scale, raw_zp, mode, g):
    """(scale, zero point) that reach the quantizer from the raw words under ``mode`` and grad factor ``g`` (effective_params of
    csrc/osq_device.h), float32 arrays of the raw ones' size: what ``Quant`` holds."""
    s, z = FQ.lsq_effective(np.atleast_1d(raw_scale), np.atleast_1d(raw_zp), g, _mode(mode))
    return s.astype(F32), z.astype(F32)


def repaired(raw_scale, raw_zp, mode, zp_is_float, qmin, qmax):
    """(scale, zero point) the in-launch repair leaves in memory (tensor_params of csrc/osq_device.h under PARAM_SANITIZE): |s|,
    at least eps, a NaN kept; the zero point clipped into [qmin, qmax] only for LSQ+ with a float32 zero point."""
    s, z = np.abs(np.atleast_1d(raw_scale).astype(F32)), np.atleast_1d(raw_zp).astype(F32)
    s = np.where(s < EPS32, EPS32, s)
    if _mode(mode) == "lsqplus" and zp_is_float:
        z = np.where(z < F32(qmin), F32(qmin), z)
        z = np.where(z > F32(qmax), F32(qmax), z)
    return s.astype(F32), z.astype(F32)


def effective_case(case, x_mode="fixed", x_g=1.0, w_mode="fixed", w_g=1.0):
    """``case`` with RAW parameters -> the case ``rule`` takes: both quantizers' effective parameters."""
    x, xq, w, wq, bias = case
    return (x, xq._replace(**dict(zip(("scale", "zero_point"), effective(xq.scale, xq.zero_point, x_mode, x_g)))), w,
            wq._replace(**dict(zip(("scale", "zero_point"), effective(wq.scale, wq.zero_point, w_mode, w_g)))), bias)


def units(x, q):
    """u of the rule in float32 steps (NaN where x has no code): x [R, K]; q's parameters have 1 or R entries."""
    s, z = q.scale.reshape(-1, 1), q.zero_point.reshape(-1, 1)
    with np.errstate(all="ignore"):
        u = (x.astype(F32) / s).astype(F32)
        r = np.rint(u)
        xq = np.clip((((r - u).astype(F32) + u).astype(F32) + z).astype(F32), F32(q.qmin), F32(q.qmax))
    return np.where(xq == np.rint(xq), xq - F32(q.qmin), np.nan)


def rule(x, xq, w, wq, bias=None):
    """(out [M, N] float32, a [M, K] as bytes, rowsum [M] int32) of the rule; a row of x without codes has row sum -2**31 and
    a NaN row of out (its bytes are not specified); a zero point that is no integer inside its range makes all of out NaN."""
    k = x.shape[1]
    ux, uw = units(x, xq), units(w, wq)
    no_row = np.isnan(ux).any(1)
    a, b = np.nan_to_num(ux).astype(np.int64) - 128, np.nan_to_num(uw).astype(np.int64) - 128
    bad = np.isnan(uw).any() or not all(np.all((q.zero_point == np.rint(q.zero_point)) & (q.zero_point >= q.qmin)
                                               & (q.zero_point <= q.qmax)) for q in (xq, wq))
    zx, zw = (0, np.zeros(1, np.int64)) if bad else (int(xq.zero_point[0]) - xq.qmin - 128, wq.zero_point.astype(np.int64) - wq.qmin - 128)
    ab = np.matmul(a.astype(np.float64), b.astype(np.float64).T).astype(np.int64)       # integers below 2**53: exact
    n = ab - zw[None, :] * a.sum(1)[:, None] - zx * b.sum(1)[None, :] + k * zx * zw[None, :]
    assert bad or np.abs(n[~no_row]).max(initial=0) <= 255 * 255 * k
    out = (n.astype(F32) * (xq.scale * wq.scale).astype(F32)[None, :]).astype(F32)
    if bias is not None:
        out = (out + bias[None, :]).astype(F32)
    out[no_row | bad] = np.nan
    return out, (a & 0xFF).astype(np.uint8), np.where(no_row, -2 ** 31, a.sum(1)).astype(np.int32)


def make_quant(rng, name, where, spread, n=1):
    """n quantizers whose codes span about ``spread`` (a little less: some values clamp), the zero points where ``where`` says."""
    qmin, qmax = RANGES[name]
    zp = {"qmin": qmin, "qmax": qmax, "inside": 0 if qmin < 0 else (qmin + qmax + 1) // 2}[where] + np.zeros(n)
    if where == "inside" and qmin == 0:
        zp += rng.integers(-5, 6, n)
    return Quant((spread / (qmax - qmin) * rng.uniform(0.8, 1.0, n)).astype(F32), zp.astype(F32), qmin, qmax)


def make_case(seed, m, n, k, quant, with_bias):
    """Seeded operands of one case: x [M, K], xq, w [N, K], wq, bias or None; one-sided ranges get one-sided values."""
    rng = np.random.default_rng(seed)
    x_name, x_where, w_name, w_where, per_channel = quant
    shift = {"qmin": 2.5, "qmax": -2.5, "inside": 0.0}
    x = (rng.standard_normal((m, k)) + shift[x_where]).astype(F32)
    w = ((rng.standard_normal((n, k)) + shift[w_where]) * 0.1).astype(F32)
    xq, wq = make_quant(rng, x_name, x_where, 6.0), make_quant(rng, w_name, w_where, 0.6, n if per_channel else 1)
    return x, xq, w, wq, (rng.standard_normal(n).astype(F32) if with_bias else None)


# ---- the cases tests/test_gpu_linear_int_edges.py and tests/test_linear_int_cpu.py share -------------------------------------
EDGE_KS = (128, 144, 176, 192, 240, 256, 272, 512, 528, 768, 784, 1008, 1040, 2064, 3072, 4096)
EDGE_MS, EDGE_N = (1, 32, 33), 36
MODE_QUANT = ("asym8", "inside", "asym8", "inside", True)      # zero points near 128 on both sides: every correction term is live
X_MODES = (("fixed", True), ("fixed", False), ("lsq", True), ("lsq", False), ("lsqplus", False))     # (mode, int32 zero point)
W_MODES = MODES
GRAD_FACTORS = ("site", 0.3)                                   # "site": 1 / sqrt(M K qmax), what a model's LSQ / LSQ+ site hands over
REPAIRS = ("negative scale", "tiny scale", "zero point above", "zero point below")


def grad_factor(kind, m, k, qmax):
    return FQ.lsqplus_grad_factor(m * k, qmax) if kind == "site" else float(kind)


def scales_that_move(rng, base, mode, g, n=1):
    """The first n of 2**17 seeded scales in [0.8, 1] * base whose effective word under (mode, g) is not the raw word: about 0.1 %
    of them at a site's grad factor, 3 % at 0.3."""
    cand = (base * rng.uniform(0.8, 1.0, 1 << 17)).astype(F32)
    moved = cand[effective(cand, np.zeros_like(cand), mode, g)[0] != cand]
    assert moved.size >= n, (mode, g, moved.size)
    return moved[:n].copy()


def edge_case(m, k):
    """Section A: seeded normal data (every position differs), the quantizer sets rotating, bias on every other case."""
    i = EDGE_KS.index(k) * len(EDGE_MS) + EDGE_MS.index(m)
    return make_case(2000 + i, m, EDGE_N, k, QUANTS[i % len(QUANTS)], i % 2 == 0)


def mode_case(m, x_mode, g_kind, w_mode, n=EDGE_N, k=144):
    """Section B: (raw case, grad factor).  Under a learnable mode the input scale, and the scales of channels 1 and 33, are
    ones that grad_scale moves; LSQ+ zero points are raw fractions (+0.25) that round_ste makes integers."""
    x, xq, w, wq, bias = make_case(3000 + m, m, n, k, MODE_QUANT, True)
    g, rng = grad_factor(g_kind, m, k, xq.qmax), np.random.default_rng(77)
    if x_mode != "fixed":
        xq = xq._replace(scale=scales_that_move(rng, xq.scale[0], x_mode, g))
    if w_mode != "fixed":
        ws = wq.scale.copy()
        ws[[1, 33]] = scales_that_move(rng, ws[1], w_mode, g, 2)
        wq = wq._replace(scale=ws)
    if x_mode == "lsqplus":
        xq = xq._replace(zero_point=xq.zero_point + F32(0.25))
    if w_mode == "lsqplus":
        wq = wq._replace(zero_point=wq.zero_point + F32(0.25))
    return (x, xq, w, wq, bias), g


def words(a):
    return a.shape, a.dtype, a.tobytes()


def mode_reference(m, x_mode, g_kind, w_mode):
    """(raw case, grad factor, rule's words) of a section B case, after the conditions that give it teeth: the launch is good,
    and a kernel that took either quantizer's raw words for the effective ones would write other words of out (all NaN for
    the weight's fractional zero points)."""
    raw, g = mode_case(m, x_mode, g_kind, w_mode)
    want = rule(*effective_case(raw, x_mode, g, w_mode, g))
    assert np.isfinite(want[0]).all()
    if x_mode != "fixed":
        assert effective(raw[1].scale, raw[1].zero_point, x_mode, g)[0] != raw[1].scale
        assert words(rule(*effective_case(raw, "fixed", 1.0, w_mode, g))[0]) != words(want[0])
    if w_mode != "fixed":
        ignored = rule(*effective_case(raw, x_mode, g, "fixed", 1.0))[0]
        assert words(ignored) != words(want[0]) and (w_mode != "lsqplus" or np.isnan(ignored).all())
    return raw, g, want


def repair_case(m, mode, what, n=EDGE_N, k=144):
    """Section C: (raw case, grad factor, zero point is int32): fixed / lsq with an int32 zero point or lsqplus with its float32 one, one
    raw word of the input quantizer in need of the repair (an int32 word holds the truncated value and is never repaired)."""
    x, xq, w, wq, bias = make_case(3100 + m, m, n, k, MODE_QUANT, True)
    zp_int = mode != "lsqplus"
    s, z = xq.scale.copy(), xq.zero_point.copy()
    if what == "negative scale":
        s = -s
    elif what == "tiny scale":
        s[:] = 1e-9
    else:
        z[:] = xq.qmax + 3.5 if what == "zero point above" else xq.qmin - 2
        z = np.trunc(z) if zp_int else z
    return (x, xq._replace(scale=s, zero_point=z), w, wq, bias), grad_factor("site", m, k, xq.qmax), zp_int


def repair_reference(m, mode, what, sanitize=True):
    """(raw case, grad factor, zp_int, (scale, zero point) left in memory, rule's words) of a section C case."""
    raw, g, zp_int = repair_case(m, mode, what)
    xq = raw[1]
    left = repaired(xq.scale, xq.zero_point, mode, not zp_int, xq.qmin, xq.qmax) if sanitize else (xq.scale, xq.zero_point)
    fixed = (raw[0], xq._replace(scale=left[0], zero_point=left[1])) + raw[2:]
    return raw, g, zp_int, left, rule(*effective_case(fixed, mode, g))

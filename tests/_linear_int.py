"""Numpy restatement of the integer linear rule (include/osq_hip.h, "integer linear"; csrc/linear_int.hip) -- int64 sums,
float32 steps -- and the seeded cases tests/test_linear_int_cpu.py and tests/test_gpu_linear_int.py share."""
from collections import namedtuple

import numpy as np

F32 = np.float32
RANGES = {"asym8": (0, 255), "sym8": (-128, 127), "asym6": (0, 63), "sym6": (-32, 31)}
# (input range, where its zero point lies, weight range, where its zero points lie, per-channel weights)
QUANTS = (("asym8", "inside", "sym8", "inside", True), ("asym6", "inside", "sym6", "inside", True),
          ("asym8", "qmin", "asym8", "qmax", False), ("asym8", "qmax", "asym8", "qmin", True),
          ("sym8", "inside", "asym6", "inside", False))
Quant = namedtuple("Quant", "scale zero_point qmin qmax")      # effective parameters: float32 arrays of 1 or N entries


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

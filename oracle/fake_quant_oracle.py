"""Oracle (test infrastructure): fake-quant forward / LSQ+ backward in NumPy fp32.

Follows ``quant_transformer/quantization/util_quant.py`` of the reference.  Every
operation is a separately rounded fp32 operation, in the reference's order: true
division, round-half-even, add zero-point, clamp, subtract zero-point, multiply.
"""
import numpy as np

F32 = np.float32


def _f32(a):
    return np.asarray(a, dtype=F32)


def round_ste_value(u):
    """Forward value of ``round_ste`` (util_quant.py:4-8): ``(u.round() - u) + u``.

    For finite ``u`` this equals ``rint(u)`` exactly; for +-inf it is NaN
    (inf - inf), which the reference inherits and so do we.
    """
    u = _f32(u)
    with np.errstate(invalid="ignore"):
        return (np.round(u) - u) + u


def grad_scale_value(t, g):
    """Forward value of ``grad_scale`` (util_quant.py:70-71): ``(t - t*g) + t*g``."""
    t = _f32(t)
    tg = t * F32(g)
    return (t - tg) + tg


def quantize_affine(x, scale, zero_point, quant_min, quant_max):
    """Integer-valued tensor ``x_quant`` of util_quant.py:12-13 (fp32 storage)."""
    x = _f32(x)
    scale = _f32(scale)
    zero_point = _f32(zero_point)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        x_int = round_ste_value(x / scale) + zero_point
        # np.clip propagates NaN exactly as torch.clamp does
        return np.clip(x_int, F32(quant_min), F32(quant_max))


def dequantize_affine(x_quant, scale, zero_point):
    """util_quant.py:14: ``(x_quant - zero_point) * scale``."""
    with np.errstate(invalid="ignore", over="ignore"):
        return (_f32(x_quant) - _f32(zero_point)) * _f32(scale)


def fake_quantize_per_tensor_affine(x, scale, zero_point, quant_min, quant_max):
    """util_quant.py:11-15.  ``scale``/``zero_point`` are scalars.  Returns (x_quant, x_dequant)."""
    xq = quantize_affine(x, F32(scale), F32(zero_point), quant_min, quant_max)
    return xq, dequantize_affine(xq, F32(scale), F32(zero_point))


def _broadcast_shape(x, ch_axis):
    shape = [1] * x.ndim
    shape[ch_axis] = x.shape[ch_axis]
    return shape


def fake_quantize_per_channel_affine(x, scale, zero_point, ch_axis, quant_min, quant_max):
    """util_quant.py:18-26.  ``scale``/``zero_point`` have one entry per index of ``ch_axis``."""
    x = _f32(x)
    shp = _broadcast_shape(x, ch_axis)
    s = _f32(scale).reshape(shp)
    z = _f32(zero_point).reshape(shp)
    xq = quantize_affine(x, s, z, quant_min, quant_max)
    return xq, dequantize_affine(xq, s, z)


def lsq_effective_scale(scale, grad_factor):
    """util_quant.py:30,40: forward value of ``grad_scale(scale, g)``."""
    return grad_scale_value(scale, grad_factor)


def lsqplus_effective_params(scale, zero_point, grad_factor):
    """util_quant.py:49-51 / 59-63: values of scale and zero-point that reach the quantizer.

    zero_point <- (zp.round() - zp) + zp ; scale <- grad_scale(scale) ; zp <- grad_scale(zp).
    """
    zp = _f32(zero_point)
    zp = (np.round(zp) - zp) + zp
    return grad_scale_value(scale, grad_factor), grad_scale_value(zp, grad_factor)


def fake_quantize_learnableplus_per_tensor(x, scale, zero_point, quant_min, quant_max, grad_factor):
    """util_quant.py:48-55 forward.  Returns (x_quant, x_dequant)."""
    s, z = lsqplus_effective_params(scale, zero_point, grad_factor)
    s = s.reshape(()) if s.size == 1 else s
    z = z.reshape(()) if z.size == 1 else z
    xq = quantize_affine(x, s, z, quant_min, quant_max)
    return xq, dequantize_affine(xq, s, z)


def fake_quantize_learnableplus_per_channel(x, scale, zero_point, ch_axis, quant_min, quant_max, grad_factor):
    """util_quant.py:58-67 forward."""
    x = _f32(x)
    s, z = lsqplus_effective_params(scale, zero_point, grad_factor)
    shp = _broadcast_shape(x, ch_axis)
    s, z = s.reshape(shp), z.reshape(shp)
    xq = quantize_affine(x, s, z, quant_min, quant_max)
    return xq, dequantize_affine(xq, s, z)


def fake_quantize_learnable_per_tensor(x, scale, zero_point, quant_min, quant_max, grad_factor):
    """util_quant.py:29-34 forward (LSQ: integer zero-point, learnable scale)."""
    s = lsq_effective_scale(scale, grad_factor)
    s = s.reshape(()) if s.size == 1 else s
    xq = quantize_affine(x, s, F32(zero_point), quant_min, quant_max)
    return xq, dequantize_affine(xq, s, F32(zero_point))


MODES = ("fixed", "lsq", "lsqplus")            # the library's OSQ_PARAM_FIXED / _LSQ / _LSQPLUS = 0 / 1 / 2


def _mode_name(mode):
    if isinstance(mode, str):
        if mode not in MODES:
            raise ValueError(f"mode must be one of {MODES}, got {mode!r}")
        return mode
    return MODES[int(mode)]


def lsq_effective(scale, zero_point, grad_factor, mode):
    """(scale, zero_point) that reach the quantizer, fp32: util_quant.py:49-51 (LSQ+), :30 (LSQ: the scale only), or the
    parameters themselves (Fixed)."""
    mode = _mode_name(mode)
    if mode == "lsqplus":
        return lsqplus_effective_params(scale, zero_point, grad_factor)
    if mode == "lsq":
        return lsq_effective_scale(scale, grad_factor), _f32(zero_point)
    return _f32(scale), _f32(zero_point)


def lsq_grad_factors(grad_factor, mode):
    """(factor of scale.grad, factor of zero_point.grad): grad_scale's backward (util_quant.py:70-71) where the mode sends
    the parameter through grad_scale -- both for LSQ+, the scale for LSQ, neither for Fixed."""
    mode = _mode_name(mode)
    g = float(grad_factor)
    return (1.0 if mode == "fixed" else g), (g if mode == "lsqplus" else 1.0)


def lsq_backward_terms(x, grad_out, scale, zero_point, quant_min, quant_max, grad_factor, mode, ch_axis=-1):
    """The fp32 per-element arrays autograd forms in the backward of util_quant.py:29-67, each the shape of ``x``:

        ds_mul = gy * (xq - z)              mul backward wrt the scale
        ds_div = -g_in * ((x / s) / s)      div backward wrt the denominator
        g_in   = inside ? gy * s : 0        add backward wrt the zero point (through x_int; the clamp's mask)
        ng_mul = -(gy * s)                  sub backward wrt the zero point (through xq - z)
        dx     = g_in / s                   div backward wrt the numerator

    scale.grad = (sum ds_mul + sum ds_div) * factor, zero_point.grad = (sum g_in + sum ng_mul) * factor (lsq_grad_factors).
    ``mode``: "lsqplus" / "lsq" / "fixed" (or 2 / 1 / 0).  ``ch_axis`` = -1: per-tensor, scale / zero_point of one element;
    otherwise an axis of x (negative axes count from the end, as util_quant's reshape does) with one parameter per index.
    Returns a dict of the five arrays."""
    x = _f32(x)
    gy = _f32(grad_out)
    s, z = lsq_effective(scale, zero_point, grad_factor, mode)
    s, z = np.asarray(s, F32), np.asarray(z, F32)
    if ch_axis == -1 and s.size == 1:
        s, z = F32(s.reshape(-1)[0]), F32(z.reshape(-1)[0])
    else:
        shp = _broadcast_shape(x, ch_axis)
        s, z = s.reshape(shp), z.reshape(shp)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        u = x / s
        x_int = round_ste_value(u) + z
        inside = (x_int >= F32(quant_min)) & (x_int <= F32(quant_max))
        xq = np.clip(x_int, F32(quant_min), F32(quant_max))
        g_mul = gy * s                       # d/d(xq - z) of (xq - z) * s
        g_in = np.where(inside, g_mul, F32(0))
        dx = g_in / s                        # div backward wrt numerator
        ds_mul = gy * (xq - z)               # mul backward wrt s
        ds_div = -g_in * ((x / s) / s)       # div backward wrt denominator
    return {"ds_mul": ds_mul.astype(F32), "ds_div": ds_div.astype(F32), "g_in": g_in.astype(F32),
            "ng_mul": (-g_mul).astype(F32), "dx": dx.astype(F32)}


def _per_channel_rows(a, ch_axis):
    """[channels, outer * inner]: every channel's elements gathered in memory order."""
    if ch_axis == -1:
        return a.reshape(1, -1)
    return np.moveaxis(a, ch_axis, 0).reshape(a.shape[ch_axis], -1)


def _exact_sum(rows, how):
    """Correctly rounded float64 sum of every row of fp32 terms.  "fsum": math.fsum (exact whatever the data);
    "float64": NumPy's float64 sum, for callers that have PROVED every partial sum exact (then the order is immaterial).
    A row that holds a NaN or an infinity takes IEEE's answer for it (fsum refuses inf - inf)."""
    import math
    out = np.empty(rows.shape[0], np.float64)
    for c, r in enumerate(rows):
        r64 = r.astype(np.float64)
        if how == "float64" or not np.isfinite(r64).all():
            with np.errstate(invalid="ignore", over="ignore"):
                out[c] = r64.sum()
        else:
            out[c] = math.fsum(r64.tolist())
    return out


class LsqExact(dict):
    """Result of lsq_backward_exact: a dict with attribute access."""
    __getattr__ = dict.__getitem__


def lsq_backward_exact(x, grad_out, scale, zero_point, quant_min, quant_max, grad_factor, mode, ch_axis=-1, how="fsum"):
    """The gradients with their two sums CORRECTLY ROUNDED: per channel, S_s = sum(ds_mul) + sum(ds_div) and
    S_z = sum(g_in) + sum(ng_mul) over the fp32 terms of lsq_backward_terms as one exact sum rounded once to float64
    (math.fsum; ``how="float64"`` where the caller proves float64 exact), then the mode's factor as a float64 product
    with the fp32 value of ``grad_factor`` (what the kernels are handed).

    Returns dx [fp32, x's shape] and, each a float64 array with one entry per channel (one entry for per-tensor):
    dscale, dzp, S_s, S_z, and the condition scales A_s = sum|ds_mul| + sum|ds_div|, A_z = sum|g_in| + sum|ng_mul|
    (an fp32 summation of n terms in any order errs by at most about n * 2^-24 * A, a float64 one rounded once by
    2^-24 * |S|; kappa = A / |S|)."""
    t = lsq_backward_terms(x, grad_out, scale, zero_point, quant_min, quant_max, grad_factor, mode, ch_axis)
    rows = {k: _per_channel_rows(t[k], ch_axis) for k in ("ds_mul", "ds_div", "g_in", "ng_mul")}
    S_s = _exact_sum(np.concatenate([rows["ds_mul"], rows["ds_div"]], axis=1), how)
    S_z = _exact_sum(np.concatenate([rows["g_in"], rows["ng_mul"]], axis=1), how)
    with np.errstate(invalid="ignore", over="ignore"):
        A_s = np.abs(rows["ds_mul"]).astype(np.float64).sum(axis=1) + np.abs(rows["ds_div"]).astype(np.float64).sum(axis=1)
        A_z = np.abs(rows["g_in"]).astype(np.float64).sum(axis=1) + np.abs(rows["ng_mul"]).astype(np.float64).sum(axis=1)
        fs, fz = lsq_grad_factors(F32(grad_factor), mode)
        dscale, dzp = S_s * np.float64(fs), S_z * np.float64(fz)
    return LsqExact(dx=t["dx"], dscale=dscale, dzp=dzp, S_s=S_s, S_z=S_z, A_s=A_s, A_z=A_z)


def lsq_backward_reference_order(x, grad_out, scale, zero_point, quant_min, quant_max, grad_factor, mode, ch_axis=-1, vec=8):
    """The gradients with the reductions done the way autograd does them on the reference's CPU (one thread):
    scale.grad and zero_point.grad are each the fp32 sum of TWO ``sum_to_size`` reductions -- mul backward and div
    backward for the scale, add backward and sub backward for the zero point (util_quant.py:48-55) --, every reduction
    torch's fp32 ``sum`` in ATen's order (oracle/aten_sum.py), then grad_scale's factor (util_quant.py:70-71) as an fp32
    multiplication where the mode has one.  Per-tensor (ch_axis = -1): one flat vector of any length.  Per-channel:
    ch_axis = 0 only (x seen as [channels, inner]: every row the same cascade over the contiguous inner axis).
    Returns (dx [fp32], dscale [fp32, scalar or [channels]], dzero_point [likewise])."""
    from .aten_sum import aten_sum, aten_sum_flat
    x = _f32(x)
    t = lsq_backward_terms(x, grad_out, scale, zero_point, quant_min, quant_max, grad_factor, mode, ch_axis)
    mode = _mode_name(mode)
    g = F32(grad_factor)
    if ch_axis == -1:
        total = lambda a: aten_sum_flat(a.reshape(-1), vec, np.float32)   # noqa: E731  (any length: the one-thread order)
        ds = F32(total(t["ds_mul"]) + total(t["ds_div"]))
        dz = F32(total(t["g_in"]) + total(t["ng_mul"]))
        return t["dx"], (ds if mode == "fixed" else F32(ds * g)), (F32(dz * g) if mode == "lsqplus" else dz)
    if ch_axis % x.ndim != 0:
        raise ValueError("reference-order per-channel sums: ch_axis = 0 (rows over the contiguous inner axis) only")
    rows = lambda a: aten_sum(np.ascontiguousarray(a.reshape(x.shape[0], -1), dtype=F32), vec, np.float32)   # noqa: E731
    ds = (rows(t["ds_mul"]) + rows(t["ds_div"])).astype(F32)
    dz = (rows(t["g_in"]) + rows(t["ng_mul"])).astype(F32)
    return t["dx"], (ds if mode == "fixed" else (ds * g).astype(F32)), ((dz * g).astype(F32) if mode == "lsqplus" else dz)


def lsqplus_backward_per_tensor(x, grad_out, scale, zero_point, quant_min, quant_max, grad_factor):
    """Gradients autograd produces for util_quant.py:48-55 (per-tensor LSQ+).

    Elementwise parts are written with the fp32 operations autograd executes
    (lsq_backward_terms: mul backward ``gy*s``, clamp mask, div backward ``g/s`` and
    ``-g*((x/s)/s)``); the two reductions are accumulated in float64 because the
    reference's own fp32 summation order is an implementation detail of torch.
    Returns (dx [fp32], dscale [float64 scalar], dzero_point [float64 scalar]).
    """
    t = lsq_backward_terms(x, grad_out, scale, zero_point, quant_min, quant_max, grad_factor, "lsqplus")
    with np.errstate(invalid="ignore", over="ignore"):
        dz_elem = t["g_in"] + t["ng_mul"]    # +1 through x_int, -1 through (xq - z)
        g = float(grad_factor)
        dscale = (t["ds_mul"].astype(np.float64).sum() + t["ds_div"].astype(np.float64).sum()) * g
        dzp = dz_elem.astype(np.float64).sum() * g
    return t["dx"], dscale, dzp


def lsqplus_backward_per_tensor_reference_order(x, grad_out, scale, zero_point, quant_min, quant_max, grad_factor, vec=8):
    """lsq_backward_reference_order for per-tensor LSQ+.  Equal to the reference's own run (tests/golden/lsqplus.npz) bit
    for bit.  Returns (dx [fp32], dscale [fp32 scalar], dzero_point [fp32 scalar])."""
    return lsq_backward_reference_order(x, grad_out, scale, zero_point, quant_min, quant_max, grad_factor, "lsqplus", -1, vec)


def lsqplus_backward_per_channel_reference_order(x, grad_out, scale, zero_point, quant_min, quant_max, grad_factor, vec=8):
    """Per-channel (ch_axis = 0, x = [channels, inner]) counterpart: sum_to_size reduces every row with torch's fp32 ``sum``
    over the contiguous inner axis (the same cascade per row).  Returns (dx, dscale [channels], dzero_point [channels]),
    equal to tests/golden/lsqplus.npz's ``pc_*`` bit for bit."""
    return lsq_backward_reference_order(x, grad_out, scale, zero_point, quant_min, quant_max, grad_factor, "lsqplus", 0, vec)


def lsqplus_grad_factor(numel, quant_max, channels=None):
    """fake_quant.py:195-204: ``1/sqrt(numel*qmax)`` or ``1/sqrt(numel/C*qmax)`` (Python float)."""
    if channels is None:
        return 1.0 / (numel * quant_max) ** 0.5
    return 1.0 / (numel / channels * quant_max) ** 0.5

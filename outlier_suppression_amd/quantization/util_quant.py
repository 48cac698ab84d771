"""Functional fake-quant API with the reference's names (quant_transformer/quantization/util_quant.py).

Each function is ONE fused HIP launch (forward) and, under autograd, one launch for
the backward.  ``scale`` / ``zero_point`` may be Python numbers or device tensors;
numbers are uploaded (the reference passes ``.item()`` values at fake_quant.py:124).

bf16 / fp16 ``x`` (README, "Defaults"): ``fake_quantize_per_tensor_affine`` with Python numbers or 0-dim tensors stays in
x's dtype, every op rounded to it as in torch's eager chain; with >= 1-dim tensor parameters, and for every other function,
torch's type promotion makes the result fp32, equal to the same call on ``x.float()``.
"""
import torch

from .. import ops
from ..ops import PARAM_FIXED, PARAM_LSQ, PARAM_LSQPLUS


def _as_scale(v, like):
    if torch.is_tensor(v):
        return v if v.dim() else v.reshape(1)
    return torch.tensor([float(v)], dtype=torch.float32, device=like.device)


def _as_zero_point(v, like, learnable=False):
    if torch.is_tensor(v):
        v = v if v.dim() else v.reshape(1)
        if v.dtype in (torch.int32, torch.float32):
            return v
        return v.to(torch.float32 if v.is_floating_point() else torch.int32)
    if learnable or isinstance(v, float) and not float(v).is_integer():
        return torch.tensor([float(v)], dtype=torch.float32, device=like.device)
    return torch.tensor([int(v)], dtype=torch.int32, device=like.device)


def round_ste(x):
    """util_quant.py:4-8.  Kept for API completeness: value round-half-even(x), gradient 1."""
    return (x.round() - x).detach() + x


def grad_scale(t, scale):
    """util_quant.py:70-71."""
    return (t - (t * scale)).detach() + (t * scale)


def _scalar(v):
    """A Python number or a 0-dim tensor: what keeps a bf16 / fp16 x in its dtype (decided before _as_scale reshapes it)."""
    return not torch.is_tensor(v) or v.dim() == 0


def _learnable_params(x, scale, zero_point):
    if ops.is_lowp(x) and _scalar(scale) and _scalar(zero_point):
        raise NotImplementedError("bf16 / fp16 learnable fake-quant takes [1] / [C] tensor parameters (the quantizers' own)")


def _channel_axis(x, ch_axis):
    """The reference indexes ``x.shape[ch_axis]`` (util_quant.py:20,39,61): a negative axis counts from the end.  ops.fake_quant
    keeps -1 for "per-tensor", so the per-channel functions hand it the axis counted from the front."""
    ch_axis = int(ch_axis)
    if not -x.dim() <= ch_axis < x.dim():
        raise IndexError(f"ch_axis {ch_axis} is out of range for a tensor of {x.dim()} dimensions")
    return ch_axis % x.dim()


def fake_quantize_per_tensor_affine(x, scale, zero_point, quant_min, quant_max):
    """util_quant.py:11-15."""
    scalar = _scalar(scale) and _scalar(zero_point)
    return ops.fake_quant(x, _as_scale(scale, x), _as_zero_point(zero_point, x), -1, quant_min, quant_max, PARAM_FIXED,
                          scalar_params=scalar)


def fake_quantize_per_channel_affine(x, scale, zero_point, ch_axis, quant_min, quant_max):
    """util_quant.py:18-26."""
    return ops.fake_quant(x, _as_scale(scale, x), _as_zero_point(zero_point, x), _channel_axis(x, ch_axis), quant_min, quant_max, PARAM_FIXED)


def fake_quantize_learnable_per_tensor_affine_training(x, scale, zero_point, quant_min, quant_max, grad_factor):
    """util_quant.py:29-34 (LSQ)."""
    _learnable_params(x, scale, zero_point)
    return ops.fake_quant(x, _as_scale(scale, x), _as_zero_point(zero_point, x), -1, quant_min, quant_max,
                          PARAM_LSQ, grad_factor)


def fake_quantize_learnable_per_channel_affine_training(x, scale, zero_point, ch_axis, quant_min, quant_max, grad_factor):
    """util_quant.py:37-45 (LSQ)."""
    _learnable_params(x, scale, zero_point)
    return ops.fake_quant(x, _as_scale(scale, x), _as_zero_point(zero_point, x), _channel_axis(x, ch_axis), quant_min, quant_max,
                          PARAM_LSQ, grad_factor)


def fake_quantize_learnableplus_per_tensor_affine_training(x, scale, zero_point, quant_min, quant_max, grad_factor):
    """util_quant.py:48-55 (LSQ+)."""
    _learnable_params(x, scale, zero_point)
    return ops.fake_quant(x, _as_scale(scale, x), _as_zero_point(zero_point, x, True), -1, quant_min, quant_max,
                          PARAM_LSQPLUS, grad_factor)


def fake_quantize_learnableplus_per_channel_affine_training(x, scale, zero_point, ch_axis, quant_min, quant_max,
                                                            grad_factor):
    """util_quant.py:58-67 (LSQ+)."""
    _learnable_params(x, scale, zero_point)
    return ops.fake_quant(x, _as_scale(scale, x), _as_zero_point(zero_point, x, True), _channel_axis(x, ch_axis), quant_min, quant_max,
                          PARAM_LSQPLUS, grad_factor)

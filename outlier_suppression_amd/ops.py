"""Tensor-level entry points: torch tensors in, C-ABI kernel launches out.

Everything here runs on the current HIP stream and never synchronises with the
host.  No arithmetic on tensor data happens in Python; torch only allocates.
"""
import ctypes
import math
import os
from typing import NamedTuple

import torch

from . import _hip
from ._hip import (PARAM_FIXED, PARAM_LSQ, PARAM_LSQPLUS, PARAM_MODE_MASK, PARAM_SANITIZE, PARAM_NO_PERSISTENT, UPDATE_AVERAGE,  # noqa: F401
                   UPDATE_NONE, UPDATE_RUNNING, ZP_FLOAT32, ZP_INT32)


def _zp_type(zero_point):
    if zero_point.dtype == torch.int32:
        return ZP_INT32
    if zero_point.dtype == torch.float32:
        return ZP_FLOAT32
    raise TypeError(f"zero_point must be int32 or float32, got {zero_point.dtype}")


def _check_f32(*tensors):
    for t in tensors:
        if t is not None and t.dtype != torch.float32:
            raise TypeError(f"outlier_suppression_amd kernels compute in float32, got {t.dtype}")


# bf16 / fp16 inputs: the min / max observers and per-channel fake-quant read all three element types (_elem_code); the in-dtype
# chain and the per-tensor widening forward are 16-bit only (_lowp_code); every other function is fp32 only (_check_f32)
LOWP_DTYPES = {torch.bfloat16: _hip.DTYPE_BF16, torch.float16: _hip.DTYPE_F16}
_ELEM_CODES = {torch.float32: _hip.DTYPE_F32, **LOWP_DTYPES}


def is_lowp(x):
    return x.dtype in LOWP_DTYPES


def _lowp_code(x):
    code = LOWP_DTYPES.get(x.dtype)
    if code is None:
        raise TypeError(f"outlier_suppression_amd: expected a bfloat16 or float16 tensor, got {x.dtype}")
    return code


def _elem_code(x):
    """osq_dtype of x's elements: read once, where the pointer is taken."""
    code = _ELEM_CODES.get(x.dtype)
    if code is None:
        raise TypeError(f"outlier_suppression_amd kernels compute in float32, got {x.dtype}")
    return code


def is_dense(x):
    """True if x's elements occupy one gap-free block of memory (any dim order)."""
    if x.is_contiguous():
        return True
    expected = 1
    for size, stride in sorted(zip(x.shape, x.stride()), key=lambda p: (p[1], p[0])):
        if size == 1:
            continue
        if stride != expected:
            return False
        expected *= size
    return True


def _i64x4(vals):
    vals = list(vals)
    vals = [1] * (4 - len(vals)) + vals if len(vals) <= 4 else None
    if vals is None:
        raise NotImplementedError("strided fake-quant supports at most 4 dims")
    return (ctypes.c_int64 * 4)(*vals)


def _pad4_strides(x):
    st = list(x.stride())
    return (ctypes.c_int64 * 4)(*([0] * (4 - len(st)) + st))


# ---------------------------------------------------------------------------------------
# fake-quant forward
# ---------------------------------------------------------------------------------------

def fake_quant_per_tensor(x, scale, zero_point, quant_min, quant_max, mode=PARAM_FIXED, grad_factor=1.0,
                          return_quantized=False):
    """(x_dequant[, x_quant]) of util_quant.py:11-15 / 29-34 / 48-55 (forward).  scale/zero_point: 1-element device tensors."""
    lib = _hip.load()
    _hip.require_device(x, scale, zero_point)
    _check_f32(x, scale)
    st = _hip.stream_ptr(x.device)
    if (x.dim() == 4 and not return_quantized and not x.is_contiguous() and x.numel()
            and (x.stride(-1) == 1 or x.stride(-2) == 1)):
        # Head-split views of attention ([B,h,T,d] / [B,h,d,T] seen through [B,T,h,d] memory): quantise into the
        # layout the batched matmul that follows wants -- contiguous, or the transpose of a contiguous tensor for the
        # key -- instead of x's own strides, which torch.matmul would first copy out (reshape of a permuted view).
        xt = x if x.stride(-1) == 1 else x.transpose(-1, -2)
        if xt.shape[-1] % 4 == 0 and all(sv % 4 == 0 for sv in xt.stride()[:3]) and xt.data_ptr() % 16 == 0:
            yt = torch.empty(xt.shape, dtype=x.dtype, device=x.device)
            _hip.check(lib.osq_fake_quant_per_tensor_strided(
                xt.data_ptr(), yt.data_ptr(), None, _i64x4(xt.shape), _pad4_strides(xt), _pad4_strides(yt),
                _hip.ptr(scale), _hip.ptr(zero_point), _zp_type(zero_point), mode, float(grad_factor),
                int(quant_min), int(quant_max), st), "fake_quant_per_tensor_strided")
            return yt if xt is x else yt.transpose(-1, -2)
    if is_dense(x):
        y = torch.empty_like(x)
        xq = torch.empty_like(x) if return_quantized else None
        _hip.check(lib.osq_fake_quant_per_tensor(_hip.ptr(x), _hip.ptr(y), _hip.ptr(xq), x.numel(), _hip.ptr(scale),
                                                 _hip.ptr(zero_point), _zp_type(zero_point), mode, float(grad_factor),
                                                 int(quant_min), int(quant_max), st), "fake_quant_per_tensor")
    else:
        if x.dim() > 4:
            x = x.contiguous()
            return fake_quant_per_tensor(x, scale, zero_point, quant_min, quant_max, mode, grad_factor, return_quantized)
        y = torch.empty(x.shape, dtype=x.dtype, device=x.device)
        xq = torch.empty_like(y) if return_quantized else None
        _hip.check(lib.osq_fake_quant_per_tensor_strided(
            _hip.ptr(x), _hip.ptr(y), _hip.ptr(xq), _i64x4(x.shape), _pad4_strides(x), _pad4_strides(y),
            _hip.ptr(scale), _hip.ptr(zero_point), _zp_type(zero_point), mode, float(grad_factor),
            int(quant_min), int(quant_max), st), "fake_quant_per_tensor_strided")
    return (y, xq) if return_quantized else y


def _channel_split(x, ch_axis):
    ch_axis = ch_axis % x.dim()
    outer = 1
    for s in x.shape[:ch_axis]:
        outer *= s
    inner = 1
    for s in x.shape[ch_axis + 1:]:
        inner *= s
    return outer, x.shape[ch_axis], inner


def _check_per_channel(what, channels, a, b):
    if a.numel() != channels or b.numel() != channels:
        raise ValueError(f"{what}: {channels} channels but the per-channel tensors have {a.numel()}/{b.numel()} entries")


def fake_quant_per_channel(x, scale, zero_point, ch_axis, quant_min, quant_max, mode=PARAM_FIXED, grad_factor=1.0,
                           return_quantized=False):
    """util_quant.py:18-26 / 37-45 / 58-67 (forward).  x fp32, bf16 or fp16; the result is fp32 (torch promotes a 16-bit x
    that meets fp32 [C] parameters) and word-equal to the call on x.float().  return_quantized: fp32 x only."""
    lib = _hip.load()
    _hip.require_device(x, scale, zero_point)
    _check_f32(scale)
    code = _elem_code(x)
    if code != _hip.DTYPE_F32:
        if return_quantized:
            raise NotImplementedError("per-channel fake-quant of a bf16 / fp16 tensor has no return_quantized form")
        mode &= PARAM_MODE_MASK
    x = x.contiguous()
    outer, channels, inner = _channel_split(x, ch_axis)
    _check_per_channel("per-channel fake-quant", channels, scale, zero_point)
    y = torch.empty_like(x, dtype=torch.float32)
    xq = torch.empty_like(x) if return_quantized else None
    _hip.check(lib.osq_fake_quant_per_channel(code, _hip.ptr(x), _hip.ptr(y), _hip.ptr(xq), outer, channels, inner,
                                              _hip.ptr(scale), _hip.ptr(zero_point), _zp_type(zero_point), mode,
                                              float(grad_factor), int(quant_min), int(quant_max),
                                              _hip.stream_ptr(x.device)), "fake_quant_per_channel")
    return (y, xq) if return_quantized else y


# ---------------------------------------------------------------------------------------
# integer codes: the quantised tensor as packed unsigned integers, and back
# ---------------------------------------------------------------------------------------

class Codes(NamedTuple):
    """A quantised tensor as integers (format: include/osq_hip.h, "integer codes").  codes: uint8, u = x_quant - quant_min,
    one per byte (code_bits 8) or two per byte over the flattened tensor (code_bits 4); scale / zero_point: the fp32
    EFFECTIVE parameters that reached the quantiser, [channels]; shape / ch_axis: of the tensor the codes came from."""
    codes: torch.Tensor
    scale: torch.Tensor
    zero_point: torch.Tensor
    quant_min: int
    quant_max: int
    code_bits: int
    shape: tuple
    ch_axis: int


def _code_bits(quant_min, quant_max, code_bits):
    if code_bits is None:
        return 4 if quant_max - quant_min <= 15 else 8
    return int(code_bits)


def _codes_split(shape, ch_axis):
    """[outer, channels, inner] of a coded tensor; per-tensor (ch_axis -1): the rows of the tensor as `outer`, one channel."""
    shape = tuple(shape)
    if ch_axis == -1:
        rows = shape[0] if len(shape) >= 2 else 1
        numel = 1
        for s in shape:
            numel *= s
        return rows, 1, (numel // rows if rows else 0)
    ch_axis = ch_axis % len(shape)
    outer = inner = 1
    for s in shape[:ch_axis]:
        outer *= s
    for s in shape[ch_axis + 1:]:
        inner *= s
    return outer, shape[ch_axis], inner


def quantize_codes(x, scale, zero_point, ch_axis, quant_min, quant_max, mode=PARAM_FIXED, grad_factor=1.0, code_bits=None):
    """The integer tensor of util_quant.py:12-13 as a ``Codes`` record.  x fp32, bf16 or fp16; ch_axis -1: per-tensor.
    code_bits None: 4 when quant_max - quant_min <= 15, else 8.  Raises ValueError when some element has no integer code
    (a NaN or infinite value, a fractional zero point): one host read of the launch's counter -- export is not a hot path."""
    lib = _hip.load()
    _hip.require_device(x, scale, zero_point)
    _check_f32(scale)
    code = _elem_code(x)
    x = x.contiguous()
    outer, channels, inner = _codes_split(x.shape, ch_axis)
    _check_per_channel("quantize_codes", channels, scale, zero_point)
    bits = _code_bits(quant_min, quant_max, code_bits)
    n = x.numel()
    codes = torch.empty((n * bits + 7) // 8, dtype=torch.uint8, device=x.device)
    s_eff = torch.empty(channels, dtype=torch.float32, device=x.device)
    z_eff = torch.empty(channels, dtype=torch.float32, device=x.device)
    rejected = torch.zeros(1, dtype=torch.int32, device=x.device)
    _hip.check(lib.osq_quantize_codes(code, _hip.ptr(x), _hip.ptr(codes), outer, channels, inner, _hip.ptr(scale),
                                      _hip.ptr(zero_point), _zp_type(zero_point), mode & PARAM_MODE_MASK, float(grad_factor),
                                      int(quant_min), int(quant_max), bits, _hip.ptr(s_eff), _hip.ptr(z_eff), _hip.ptr(rejected),
                                      _hip.stream_ptr(x.device)), "quantize_codes")
    bad = int(rejected.item())
    if bad:
        raise ValueError(f"quantize_codes: {bad} of {n} elements have no integer code (x_quant is NaN or not an integer: "
                         "a NaN / infinite value or a non-integer zero point)")
    return Codes(codes, s_eff, z_eff, int(quant_min), int(quant_max), bits, tuple(x.shape), int(ch_axis))


def dequantize_codes(record, out=None):
    """fp32 tensor of ``record.shape``: (float(u + quant_min) - zero_point) * scale, word-equal to the fake-quant of the
    tensor the codes came from.  out: a contiguous fp32 tensor of that shape to write into."""
    lib = _hip.load()
    _hip.require_device(record.codes, record.scale, record.zero_point, out)
    _check_f32(record.scale, record.zero_point, out)
    shape = tuple(record.shape)
    outer, channels, inner = _codes_split(shape, record.ch_axis)
    n = outer * channels * inner
    if record.codes.dtype != torch.uint8 or record.codes.numel() != (n * record.code_bits + 7) // 8 or not record.codes.is_contiguous():
        raise ValueError(f"dequantize_codes: {record.codes.numel()} {record.codes.dtype} codes for shape {shape} at {record.code_bits} bits")
    _check_per_channel("dequantize_codes", channels, record.scale, record.zero_point)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=record.codes.device)
    elif tuple(out.shape) != shape or not out.is_contiguous():
        raise ValueError(f"dequantize_codes: out must be a contiguous tensor of shape {shape}")
    _hip.check(lib.osq_dequantize_codes(_hip.ptr(record.codes), _hip.ptr(out), outer, channels, inner, _hip.ptr(record.scale),
                                        _hip.ptr(record.zero_point), int(record.quant_min), int(record.code_bits),
                                        _hip.stream_ptr(out.device)), "dequantize_codes")
    return out


# ---------------------------------------------------------------------------------------
# backward (STE for x; LSQ/LSQ+ for scale / zero_point)
# ---------------------------------------------------------------------------------------

def _like_layout(g, x):
    """grad_out arranged in memory exactly like x (x is dense)."""
    if g.stride() == x.stride() and g.is_cuda:
        return g
    out = torch.empty_like(x)
    out.copy_(g)
    return out


def lsq_backward_per_tensor(x, grad_out, scale, zero_point, quant_min, quant_max, mode, grad_factor,
                            need_scale=True, need_zp=True):
    lib = _hip.load()
    _hip.require_device(x, grad_out, scale, zero_point)
    _check_f32(x, grad_out, scale)
    if not is_dense(x):
        x = x.contiguous()
    elif x.data_ptr() % 16:
        x = x.clone()              # the kernel reads 16 bytes per lane: a misaligned saved input (a slice of a larger buffer) is copied once
    g = _like_layout(grad_out, x)
    dx = torch.empty_like(x)
    ds = torch.empty(1, dtype=torch.float32, device=x.device) if need_scale else None
    dz = torch.empty(1, dtype=torch.float32, device=x.device) if need_zp else None
    ws = _hip.workspace(x.device)
    order = reference_sum_order("bwd")
    if order and x.numel() > 0 and ordered_sum_fits(x.numel(), order):     # set_strict(backward=True): autograd's four fp32 reductions in torch's one-thread order
        scratch, nbytes = _ordered_scratch(x.device, x.numel(), 4)
        _hip.check(lib.osq_lsq_backward_per_tensor_ordered(_hip.ptr(x), _hip.ptr(g), _hip.ptr(dx), x.numel(), _hip.ptr(scale),
                                                           _hip.ptr(zero_point), _zp_type(zero_point), mode, float(grad_factor),
                                                           int(quant_min), int(quant_max), _hip.ptr(ds), _hip.ptr(dz), order,
                                                           _hip.ptr(scratch), nbytes, _hip.ptr(ws), _hip.stream_ptr(x.device)),
                   "lsq_backward_per_tensor_ordered")
        return dx, ds, dz
    # order-free sums (the default): float64 accumulation rounded once; also what a tensor beyond the ordered kernels' capacity takes
    _hip.check(lib.osq_lsq_backward_per_tensor(_hip.ptr(x), _hip.ptr(g), _hip.ptr(dx), x.numel(), _hip.ptr(scale),
                                               _hip.ptr(zero_point), _zp_type(zero_point), mode, float(grad_factor),
                                               int(quant_min), int(quant_max), _hip.ptr(ds), _hip.ptr(dz), _hip.ptr(ws),
                                               _hip.stream_ptr(x.device)), "lsq_backward_per_tensor")
    return dx, ds, dz


def lsq_backward_per_channel(x, grad_out, scale, zero_point, ch_axis, quant_min, quant_max, mode, grad_factor,
                             need_scale=True, need_zp=True):
    lib = _hip.load()
    _hip.require_device(x, grad_out, scale, zero_point)
    _check_f32(x, grad_out, scale)
    x = x.contiguous()
    g = grad_out.contiguous()
    outer, channels, inner = _channel_split(x, ch_axis)
    dx = torch.empty_like(x)
    if x.numel() == 0:
        # nothing to launch (and no channel may mean no parameter storage): the sums over no elements are zeros, as
        # autograd's sum_to_size gives them -- not whatever an uninitialised allocation holds
        zeros = lambda: torch.zeros(channels, dtype=torch.float32, device=x.device)   # noqa: E731
        return dx, (zeros() if need_scale else None), (zeros() if need_zp else None)
    ds = torch.empty(channels, dtype=torch.float32, device=x.device) if need_scale else None
    dz = torch.empty(channels, dtype=torch.float32, device=x.device) if need_zp else None
    _hip.check(lib.osq_lsq_backward_per_channel(_hip.ptr(x), _hip.ptr(g), _hip.ptr(dx), outer, channels, inner,
                                                _hip.ptr(scale), _hip.ptr(zero_point), _zp_type(zero_point), mode,
                                                float(grad_factor), int(quant_min), int(quant_max), _hip.ptr(ds),
                                                _hip.ptr(dz), reference_sum_order("bwd"), _hip.stream_ptr(x.device)),
               "lsq_backward_per_channel")
    return dx, ds, dz


def lsq_sanitize_(scale, zero_point, eps, quant_min, quant_max):
    """In place: scale <- max(|scale|, eps); fp32 zero_point <- clamp(zero_point, qmin, qmax).  One launch."""
    lib = _hip.load()
    _hip.require_device(scale, zero_point)
    _check_f32(scale, zero_point)
    _hip.check(lib.osq_lsq_sanitize(_hip.ptr(scale), _hip.ptr(zero_point), scale.numel(), float(eps), int(quant_min),
                                    int(quant_max), _hip.stream_ptr(scale.device)), "lsq_sanitize")


# ---------------------------------------------------------------------------------------
# bf16 / fp16 fake-quant (README "Defaults": which call keeps x.dtype and which promotes to fp32)
# ---------------------------------------------------------------------------------------

def _lowp_flat(x):
    """x itself when its elements form one gap-free block (any dim order), else a contiguous copy: one extra pass."""
    return x if is_dense(x) else x.contiguous()


def fake_quant_chain_lowp(x, scale, zero_point, quant_min, quant_max):
    """FixedFakeQuantize per-tensor in x's dtype (bf16 / fp16): every op of util_quant.py:12-14 rounded to x.dtype, as the
    reference computes it with Python-number parameters.  scale / zero_point: 1-element device tensors.  ONE launch."""
    lib = _hip.load()
    _hip.require_device(x, scale, zero_point)
    _check_f32(scale)
    x = _lowp_flat(x)
    y = torch.empty_like(x)
    _hip.check(lib.osq_fake_quant_chain_lowp(_lowp_code(x), _hip.ptr(x), _hip.ptr(y), x.numel(), _hip.ptr(scale),
                                             _hip.ptr(zero_point), _zp_type(zero_point), int(quant_min), int(quant_max),
                                             _hip.stream_ptr(x.device)), "fake_quant_chain_lowp")
    return y


def fake_quant_chain_backward_lowp(x, grad_out, scale, zero_point, quant_min, quant_max):
    """d/dx of fake_quant_chain_lowp for an upstream gradient in x.dtype.  ONE launch."""
    lib = _hip.load()
    _hip.require_device(x, grad_out, scale, zero_point)
    _check_f32(scale)
    x = _lowp_flat(x)
    g = _like_layout(grad_out, x) if grad_out.dtype == x.dtype else _like_layout(grad_out.to(x.dtype), x)
    dx = torch.empty_like(x)
    _hip.check(lib.osq_fake_quant_chain_backward_lowp(_lowp_code(x), _hip.ptr(x), _hip.ptr(g), _hip.ptr(dx), x.numel(),
                                                      _hip.ptr(scale), _hip.ptr(zero_point), _zp_type(zero_point),
                                                      int(quant_min), int(quant_max), _hip.stream_ptr(x.device)),
               "fake_quant_chain_backward_lowp")
    return dx


def fake_quant_per_tensor_widen(x, scale, zero_point, quant_min, quant_max, mode=PARAM_FIXED, grad_factor=1.0):
    """Per-tensor fake-quant of a bf16 / fp16 x with fp32 [1] parameters: fp32 result, word-equal to
    fake_quant_per_tensor(x.float(), ...) (PARAM_SANITIZE included).  ONE launch, 2 B in + 4 B out per element."""
    lib = _hip.load()
    _hip.require_device(x, scale, zero_point)
    _check_f32(scale)
    x = _lowp_flat(x)
    y = torch.empty_like(x, dtype=torch.float32)
    _hip.check(lib.osq_fake_quant_per_tensor_widen(_lowp_code(x), _hip.ptr(x), _hip.ptr(y), x.numel(), _hip.ptr(scale),
                                                   _hip.ptr(zero_point), _zp_type(zero_point), mode, float(grad_factor),
                                                   int(quant_min), int(quant_max), _hip.stream_ptr(x.device)),
               "fake_quant_per_tensor_widen")
    return y


def _lowp_chain(x, ch_axis, mode, scalar_params):
    """True when a bf16 / fp16 call keeps x.dtype: Fixed per-tensor with Python-number / 0-dim parameters."""
    return scalar_params and ch_axis == -1 and (mode & PARAM_MODE_MASK) == PARAM_FIXED


def _forward(x, scale, zero_point, ch_axis, quant_min, quant_max, mode, grad_factor, scalar_params):
    if ch_axis != -1:
        return fake_quant_per_channel(x, scale, zero_point, ch_axis, quant_min, quant_max, mode, grad_factor)
    if not is_lowp(x):
        return fake_quant_per_tensor(x, scale, zero_point, quant_min, quant_max, mode, grad_factor)
    if _lowp_chain(x, ch_axis, mode, scalar_params):
        return fake_quant_chain_lowp(x, scale, zero_point, quant_min, quant_max)
    return fake_quant_per_tensor_widen(x, scale, zero_point, quant_min, quant_max, mode, grad_factor)


class _FakeQuantFn(torch.autograd.Function):
    """Differentiable fake-quant: forward = one HIP launch, backward = one HIP launch (bf16 / fp16 rows that promote to
    fp32: one more, the widening of x)."""

    @staticmethod
    def forward(ctx, x, scale, zero_point, ch_axis, quant_min, quant_max, mode, grad_factor, scalar_params=False):
        ctx.cfg = (ch_axis, quant_min, quant_max, mode & PARAM_MODE_MASK, grad_factor)    # PARAM_SANITIZE is forward-only
        ctx.chain = is_lowp(x) and _lowp_chain(x, ch_axis, mode, scalar_params)
        ctx.save_for_backward(x, scale, zero_point)
        return _forward(x, scale, zero_point, ch_axis, quant_min, quant_max, mode, grad_factor, scalar_params)

    @staticmethod
    def backward(ctx, grad_out):
        x, scale, zero_point = ctx.saved_tensors
        ch_axis, quant_min, quant_max, mode, grad_factor = ctx.cfg
        if ctx.chain:          # the parameters were numbers: x only (fake_quant refuses parameters that want a gradient)
            dx = fake_quant_chain_backward_lowp(x, grad_out, scale, zero_point, quant_min, quant_max)
            return (dx if ctx.needs_input_grad[0] else None), None, None, None, None, None, None, None, None
        x_dtype = x.dtype
        if is_lowp(x):
            # the promoted rows: autograd's sums see the same fp32 numbers as for x.float(), so the fp32 kernels (every
            # summation tier) apply to x widened once; dx is rounded to x.dtype once, as torch's to() backward does
            x = x.float()
        need_s = ctx.needs_input_grad[1]
        need_z = ctx.needs_input_grad[2] and zero_point.dtype == torch.float32
        if ch_axis == -1:
            dx, ds, dz = lsq_backward_per_tensor(x, grad_out, scale, zero_point, quant_min, quant_max, mode, grad_factor,
                                                 need_s, need_z)
        else:
            dx, ds, dz = lsq_backward_per_channel(x, grad_out, scale, zero_point, ch_axis, quant_min, quant_max, mode,
                                                  grad_factor, need_s, need_z)
        if ds is not None:
            ds = ds.reshape(scale.shape)
        if dz is not None:
            dz = dz.reshape(zero_point.shape)
        if dx.dtype != x_dtype:
            dx = dx.to(x_dtype)
        return (dx if ctx.needs_input_grad[0] else None), ds, dz, None, None, None, None, None, None


def fake_quant(x, scale, zero_point, ch_axis, quant_min, quant_max, mode=PARAM_FIXED, grad_factor=1.0, scalar_params=False):
    """Fake-quant with autograd when any input needs a gradient, a bare launch otherwise.

    scalar_params: the caller's parameters were Python numbers or 0-dim tensors (FixedFakeQuantize per-tensor passes
    ``.item()`` values).  It matters for bf16 / fp16 x only: a Fixed per-tensor call then stays in x.dtype (the in-dtype
    chain); every other bf16 / fp16 call meets fp32 [1] / [C] parameters and returns fp32, as torch's type promotion does."""
    needs = torch.is_grad_enabled() and (x.requires_grad or scale.requires_grad or
                                         (zero_point.is_floating_point() and zero_point.requires_grad))
    if needs:
        if (is_lowp(x) and _lowp_chain(x, ch_axis, mode, scalar_params)
                and (scale.requires_grad or (zero_point.is_floating_point() and zero_point.requires_grad))):
            raise NotImplementedError("bf16 / fp16 fake-quant with number parameters: gradients flow to x only")
        return _FakeQuantFn.apply(x, scale, zero_point, ch_axis, quant_min, quant_max, mode, grad_factor, scalar_params)
    return _forward(x, scale.detach(), zero_point.detach(), ch_axis, quant_min, quant_max, mode, grad_factor, scalar_params)


# ---------------------------------------------------------------------------------------
# observers
# ---------------------------------------------------------------------------------------

def calculate_qparams(min_val, max_val, quant_min, quant_max, symmetric, scale_out=None, zero_point_out=None,
                      zp_dtype=None):
    """observer.py:101-119 on device.  Returns (scale fp32, zero_point) with zero_point int32 when
    symmetric and fp32 otherwise unless ``zp_dtype`` / ``zero_point_out`` says differently."""
    lib = _hip.load()
    _hip.require_device(min_val, max_val)
    f64 = torch.float64 in (min_val.dtype, max_val.dtype)          # torch's promotion: float64 as soon as either statistic is
    mn = min_val.detach().to(torch.float64 if f64 else torch.float32).contiguous()
    mx = max_val.detach().to(torch.float64 if f64 else torch.float32).contiguous()
    if scale_out is None:
        scale_out = torch.empty(mn.shape, dtype=torch.float32, device=mn.device)
    if zero_point_out is None:
        dt = zp_dtype if zp_dtype is not None else (torch.int32 if symmetric else torch.float32)
        zero_point_out = torch.empty(mn.shape, dtype=dt, device=mn.device)
    fn = lib.osq_calculate_qparams_f64 if f64 else lib.osq_calculate_qparams
    _hip.check(fn(_hip.ptr(mn), _hip.ptr(mx), mn.numel(), int(quant_min), int(quant_max),
                                         int(bool(symmetric)), _hip.ptr(scale_out), _hip.ptr(zero_point_out),
                                         _zp_type(zero_point_out), _hip.stream_ptr(mn.device)), "calculate_qparams")
    return scale_out, zero_point_out


class QParamSink:
    """Where a fused observer launch should write scale / zero_point (None = do not compute)."""
    __slots__ = ("scale", "zero_point")

    def __init__(self, scale=None, zero_point=None):
        self.scale, self.zero_point = scale, zero_point

    def args(self):
        if self.scale is None:
            return None, None, ZP_INT32
        return _hip.ptr(self.scale), _hip.ptr(self.zero_point), _zp_type(self.zero_point)


_NO_SINK = QParamSink()


def observe_flat(x, rule, cnt, min_val, max_val, quant_min, quant_max, symmetric, sink=None, cur=None):
    """Global min/max of a dense fp32 / bf16 / fp16 tensor + running statistic (+ qparams): ONE launch.  The statistics of a
    16-bit x are those of x.float()."""
    lib = _hip.load()
    _hip.require_device(x, min_val, max_val)
    _check_f32(min_val, max_val)
    code = _elem_code(x)
    if not is_dense(x):
        x = x.contiguous()
    s_ptr, z_ptr, z_type = (sink or _NO_SINK).args()
    ws = _hip.workspace(x.device)
    _hip.check(lib.osq_observe_flat(code, _hip.ptr(x), x.numel(), rule, int(cnt), _hip.ptr(min_val), _hip.ptr(max_val),
                                    _hip.ptr(cur), int(quant_min), int(quant_max), int(bool(symmetric)), s_ptr, z_ptr,
                                    z_type, _hip.ptr(ws), _hip.stream_ptr(x.device)), "observe_flat")


def observe_channels(x, ch_axis, rule, cnt, min_val, max_val, quant_min, quant_max, symmetric, sink=None):
    """Per-channel min/max of an fp32 / bf16 / fp16 tensor + running statistic (+ qparams): ONE launch."""
    lib = _hip.load()
    _hip.require_device(x, min_val, max_val)
    _check_f32(min_val, max_val)
    code = _elem_code(x)
    x = x.contiguous()
    outer, channels, inner = _channel_split(x, ch_axis)
    _check_per_channel("observe_channels", channels, min_val, max_val)
    s_ptr, z_ptr, z_type = (sink or _NO_SINK).args()
    _hip.check(lib.osq_observe_channels(code, _hip.ptr(x), outer, channels, inner, rule, int(cnt), _hip.ptr(min_val),
                                        _hip.ptr(max_val), int(quant_min), int(quant_max), int(bool(symmetric)), s_ptr,
                                        z_ptr, z_type, _hip.stream_ptr(x.device)), "observe_channels")


_view_cache = {}


def token_view(x, seq_pos, n_lengths=None):
    """Describe x as [batch, tokens, feat_outer, feat_inner] the way observer.py:72-80 permutes it.

    With a length-B mask on a tensor whose dim 0 is larger (BART's [B*h, T, S] attention
    probabilities) ``zip`` in observer.py:82 only visits the first B rows: ``n_lengths`` trims batch.
    """
    key = (x.shape, x.stride(), seq_pos, n_lengths)
    view = _view_cache.get(key)          # a model calls each site with the same geometry over and over
    if view is not None:
        return view
    if x.dim() not in (3, 4):
        raise NotImplementedError("masked observers support 3-D and 4-D activations (observer.py:76-79)")
    seq_pos = seq_pos % x.dim()
    if seq_pos == 0:
        raise ValueError("seq_pos must not be the batch axis")
    others = [d for d in range(x.dim()) if d != seq_pos]
    sz, st = x.shape, x.stride()
    batch = sz[0] if n_lengths is None else min(sz[0], n_lengths)
    if len(others) == 3:
        fo, fi = others[1], others[2]
        outer, inner, s_outer, s_inner = sz[fo], sz[fi], st[fo], st[fi]
    else:
        fi = others[1]
        outer, inner, s_outer, s_inner = 1, sz[fi], 0, st[fi]
    view = _hip.TokenView(batch, sz[seq_pos], outer, inner, st[0], st[seq_pos], s_outer, s_inner)
    if len(_view_cache) < 4096:
        _view_cache[key] = view
    return view


_token_scratch = {}
_wide_min_slots = 32769


_tuning = {}          # what set_tuning has been given (the summation-order switches decide which entry point a call takes)


def tunable_build():
    """True when the loaded library is the -DOSQ_TUNABLE development build (`make dbg`), whose osq_set_tuning also accepts
    the performance A/B knobs; the release library holds their measured winners as compile-time constants."""
    return bool((_hip._lib or _hip.load()).osq_build_flags() & 1)


def set_tuning(key, value, lib=None):
    """Performance / path-selection knobs of the library (osq_set_tuning).  Results never change -- except for the two
    summation-order switches ("mse_sum_order", "bwd_sum_order": 8 / 16 = the reference's one-thread CPU order, see
    outlier_suppression_amd.set_strict), which pick WHICH of two roundings of the same sum is returned.
    "bwd_sum_order" is host state only: the backward's entry points take the order as an argument per call."""
    if key == "bwd_sum_order":
        if int(value) not in (0, 8, 16):
            raise ValueError("bwd_sum_order must be 0, 8 or 16")
    else:
        _hip.check((lib or _hip.load()).osq_set_tuning(key.encode(), int(value)), f"set_tuning({key})")
    _tuning[key] = int(value)


def reference_sum_order(kind):
    """SIMD width (8 / 16) of the reference host whose summation order the "mse" / "bwd" sums follow, or 0."""
    v = _tuning.get("mse_sum_order" if kind == "mse" else "bwd_sum_order", 0)
    return v if v in (8, 16) else 0


def ordered_sum_fits(n, lanes):
    """Whether the reference-order kernels take a vector of n elements summed on `lanes` SIMD lanes (csrc/aten_order.h:
    cascade step 2^P with P <= 5, i.e. up to 2^23 rows of 4 * lanes columns: 268 M fp32 / 134 M float64 elements at 8 lanes).
    Larger tensors keep the order-free sums."""
    size = (int(n) // lanes) // 4
    p = max(4, ((size - 1).bit_length() if size > 1 else 0) // 4)
    return p <= 5


def _ordered_scratch(device, n, n_sums):
    nbytes = int(_hip.load().osq_ordered_sum_scratch_bytes(int(n), int(n_sums)))
    return torch.empty(nbytes, dtype=torch.uint8, device=device), nbytes


def set_wide_min_slots(slots):
    """Token-slot count from which the finaliser uses its three multi-workgroup launches (default 32769:
    above the register capacity of the two-workgroup kernel)."""
    global _wide_min_slots
    _hip.check(_hip.load().osq_set_wide_min_slots(int(slots)), "set_wide_min_slots")
    _wide_min_slots = int(slots)



# ---------------------------------------------------------------------------------------
# persistent launches: time-outs must not stay silent
# ---------------------------------------------------------------------------------------
# The one-launch observe + fake-quant step and the resident MSEFast searches are grids whose workgroups wait for each
# other; when they are not resident together (another process on the GPU, another stream's long kernel on the CUs) a
# bounded wait expires, the launch writes NaN and raises a sticky flag in its workspace.  Every such launch marks its
# (device, stream) workspace here; check_persistent() -- called at the host's synchronisation points: the state
# togglers, state_dict(), the end of calibrate / find_ratio / learn_scale / calibrate_sharded / ptq.run, the flush of a
# deferred observer pass that ran searches -- reads the flags of the marked workspaces (one stream synchronisation
# each, nothing when nothing persistent ran), resets the state blocks and raises.
_persistent_dirty = set()


class PersistentLaunchTimeout(RuntimeError):
    pass


def _mark_persistent(device):
    _persistent_dirty.add((_hip._device_index(device), _hip.raw_stream(device)))


def check_persistent(where=""):
    """Raise PersistentLaunchTimeout if a persistent launch since the last check timed out.  Synchronises the streams
    that ran persistent launches since then; free when there were none."""
    if not _persistent_dirty:
        return
    lib = _hip.load()
    failed = []
    for key in sorted(_persistent_dirty):
        ws = _hip._workspaces.get(key)
        if ws is None:
            continue
        f, r = ctypes.c_int(0), ctypes.c_int(0)
        with torch.cuda.device(key[0]):
            _hip.check(lib.osq_persistent_status(ws.data_ptr(), ctypes.byref(f), ctypes.byref(r), 1, key[1]), "persistent_status")
        if f.value or r.value:
            failed.append((key[0], f.value, r.value))
    _persistent_dirty.clear()
    if failed:
        what = "; ".join(f"device {d}: fused observe+fake-quant step status {f}, resident MSEFast search status {r}" for d, f, r in failed)
        raise PersistentLaunchTimeout(
            f"outlier_suppression_amd{' (' + where + ')' if where else ''}: a persistent launch timed out waiting for its own "
            f"workgroups ({what}).  Its outputs and the statistics / scale / zero_point it wrote are NaN-poisoned: everything "
            "computed since the previous check is invalid.  Cause: the grid was not resident together -- another process is "
            "using this GPU, or another stream of this process kept CUs busy.  Set OSQ_FUSED_STEP=0 (launch-per-stage "
            "kernels, no cross-workgroup waits) when the GPU is shared.  The launch state has been reset.")


def _scratch(device, n):
    """(token_min, token_max, list_scratch): per (device, stream) scratch, grown on demand.  The three
    views are cached per slot count: building tensor views costs microseconds on a path that runs per site."""
    key = (device.index, _hip.raw_stream(device))
    entry = _token_scratch.get(key)
    if entry is not None:
        views = entry[1].get(n)
        if views is not None:
            return views
    if entry is None or entry[0].numel() < 4 * n:
        entry = (torch.empty(4 * max(n, 4096), dtype=torch.float32, device=device), {})
        _token_scratch[key] = entry
    buf = entry[0]
    views = (buf[:n], buf[n:2 * n], buf[2 * n:4 * n])
    if len(entry[1]) < 64:
        entry[1][n] = views
    return views


def _lengths_i64(lengths):
    return lengths if lengths is None or lengths.dtype == torch.int64 else lengths.to(torch.int64)


def token_minmax(x, seq_pos, lengths=None, out=None):
    """Per-token fp32 (min, max) over the features of an fp32 / bf16 / fp16 tensor (any strides) for tokens t < lengths[b];
    padded slots untouched."""
    lib = _hip.load()
    _hip.require_device(x, lengths)
    code = _elem_code(x)
    lengths = _lengths_i64(lengths)
    view = token_view(x, seq_pos, None if lengths is None else lengths.numel())
    n = view.batch * view.tokens
    tmin, tmax = out if out is not None else _scratch(x.device, n)[:2]
    if tmin.numel() < n or tmax.numel() < n:
        raise ValueError(f"token_minmax: the output rows hold {tmin.numel()} slots, this tensor has {n} (batch x tokens)")
    _hip.check(lib.osq_token_minmax(code, _hip.ptr(x), ctypes.byref(view), _hip.ptr(lengths), _hip.ptr(tmin), _hip.ptr(tmax),
                                    _hip.stream_ptr(x.device)), "token_minmax")
    return tmin, tmax, view.batch, view.tokens, lengths


def token_range_finalize(tmin, tmax, batch, tokens, lengths, prune, percentile, rule, cnt, min_val, max_val,
                         quant_min, quant_max, symmetric, sink=None, cur=None):
    """Percentile pruning / plain extrema over valid tokens + running statistic (+ qparams): ONE launch."""
    lib = _hip.load()
    s_ptr, z_ptr, z_type = (sink or _NO_SINK).args()
    dev = tmin.device
    lst = _scratch(dev, batch * tokens)[2] if batch * tokens >= _wide_min_slots else None
    _hip.check(lib.osq_token_range_finalize(_hip.ptr(tmin), _hip.ptr(tmax), batch, tokens, _hip.ptr(lengths),
                                            int(bool(prune)), float(percentile if prune else 1.0), rule, int(cnt),
                                            _hip.ptr(min_val), _hip.ptr(max_val), _hip.ptr(cur), int(quant_min),
                                            int(quant_max), int(bool(symmetric)), s_ptr, z_ptr, z_type,
                                            _hip.ptr(_hip.workspace(dev)), _hip.ptr(lst), _hip.stream_ptr(dev)),
               "token_range_finalize")


def observe_tokens(x, seq_pos, lengths, prune, percentile, rule, cnt, min_val, max_val, quant_min, quant_max,
                   symmetric, sink=None, cur=None):
    """token_minmax + token_range_finalize behind ONE call of the binding (the per-site hot path of a
    calibration forward: host time per quantizer call is of the order of the kernels' own run time).
    x fp32, bf16 or fp16 (the extrema are read from the data as it lies; the finaliser is fp32 either way).
    Returns (batch, tokens, lengths_int64)."""
    lib = _hip.load()
    _hip.require_device(x, lengths)
    code = _elem_code(x)
    lengths = _lengths_i64(lengths)
    view = token_view(x, seq_pos, None if lengths is None else lengths.numel())
    dev = x.device
    n = view.batch * view.tokens
    tmin, tmax, lst = _scratch(dev, n)
    s_ptr, z_ptr, z_type = (sink or _NO_SINK).args()
    rc = lib.osq_observe_tokens(code, x.data_ptr(), ctypes.byref(view), _hip.ptr(lengths), tmin.data_ptr(), tmax.data_ptr(),
                                1 if prune else 0, float(percentile) if prune else 1.0, rule, int(cnt),
                                _hip.ptr(min_val), _hip.ptr(max_val), _hip.ptr(cur), int(quant_min), int(quant_max),
                                1 if symmetric else 0, s_ptr, z_ptr, z_type, _hip.workspace(dev).data_ptr(),
                                lst.data_ptr() if n >= _wide_min_slots else None, _hip.raw_stream(dev))
    if rc != 0:
        _hip.check(rc, "observe_tokens")
    return view.batch, view.tokens, lengths


def observe_tokens_fake_quant(x, seq_pos, lengths, prune, percentile, rule, cnt, min_val, max_val, quant_min, quant_max,
                              symmetric, scale, zero_point, mode, grad_factor, cur=None, persistent=True):
    """A whole quantizer call (observe the masked activation, refresh scale / zero_point, fake-quantise) behind ONE
    call of the binding.  x: dense fp32 on the device.  cur: 2-float device slot that also receives this batch's own
    (min, max) while the running statistic moves as usual.  persistent=False: THIS call runs as three ordinary launches
    instead of the one-launch persistent form (a grid that needs every CU of the device for itself -- a caller that shares the
    GPU across streams or tenants opts out per call; same results).  Returns (y, batch, tokens, lengths_int64)."""
    if not persistent:
        mode = mode | PARAM_NO_PERSISTENT
    lib = _hip._lib or _hip.load()
    if not (lengths.is_cuda and scale.is_cuda and zero_point.is_cuda and min_val.is_cuda):
        _hip.require_device(x, lengths, scale, zero_point, min_val, max_val)
    if lengths.dtype != torch.int64:
        if lengths.is_floating_point():
            raise TypeError("observation_mask must hold integer lengths")
        lengths = lengths.to(torch.int64)
    view = token_view(x, seq_pos, lengths.numel())
    dev = x.device
    n = view.batch * view.tokens
    tmin, tmax, lst = _scratch(dev, n)
    y = torch.empty_like(x)
    rc = lib.osq_observe_tokens_fake_quant(x.data_ptr(), ctypes.byref(view), lengths.data_ptr(), tmin.data_ptr(), tmax.data_ptr(),
                                           1 if prune else 0, float(percentile) if prune else 1.0, rule, cnt,
                                           min_val.data_ptr(), max_val.data_ptr(), None if cur is None else cur.data_ptr(),
                                           quant_min, quant_max, 1 if symmetric else 0,
                                           scale.data_ptr(), zero_point.data_ptr(), _zp_type(zero_point), y.data_ptr(), x.numel(),
                                           mode, grad_factor, _hip.workspace(dev).data_ptr(),
                                           lst.data_ptr() if n >= _wide_min_slots else None, _hip.raw_stream(dev))
    if rc != 0:
        _hip.check(rc, "observe_tokens_fake_quant")
    _persistent_dirty.add((dev.index, _hip.raw_stream(dev)))
    return y, view.batch, view.tokens, lengths


def token_range_finalize_batched(token_min, token_max, n_quantizers, n_batches, batch, tokens, lengths, prune_flags,
                                 percentile, cur_table):
    """Re-threshold the cached per-token extrema of every (quantizer, batch) pair in ONE launch.
    token_min/token_max: [n_quantizers, n_batches, batch*tokens] fp32; lengths: [n_batches, batch] int64 (one mask for
    every quantizer), [n_quantizers, n_batches, batch] (every quantizer its own) or None; prune_flags: [n_quantizers]
    int32; cur_table: [n_batches, n_quantizers, 2] fp32 (written)."""
    lib = _hip.load()
    _hip.require_device(token_min, token_max, lengths, prune_flags, cur_table)
    per_q = 0
    if lengths is not None:
        if lengths.dtype != torch.int64 or not lengths.is_contiguous():
            raise ValueError("token_range_finalize_batched: lengths must be a contiguous int64 tensor")
        if tuple(lengths.shape) == (n_quantizers, n_batches, batch):
            per_q = 1
        elif tuple(lengths.shape) != (n_batches, batch):
            raise ValueError(f"token_range_finalize_batched: lengths has shape {tuple(lengths.shape)}, expected "
                             f"({n_batches}, {batch}) or ({n_quantizers}, {n_batches}, {batch})")
    if token_min.shape[-1] < batch * tokens or tuple(token_min.shape[:2]) != (n_quantizers, n_batches):
        raise ValueError("token_range_finalize_batched: token arrays do not cover [n_quantizers, n_batches, batch*tokens]")
    _hip.check(lib.osq_token_range_finalize_batched(_hip.ptr(token_min), _hip.ptr(token_max), token_min.stride(1),
                                                    int(n_quantizers), int(n_batches), int(batch), int(tokens),
                                                    _hip.ptr(lengths), per_q, _hip.ptr(prune_flags), float(percentile),
                                                    _hip.ptr(cur_table), _hip.ptr(_hip.workspace(token_min.device)),
                                                    _hip.stream_ptr(token_min.device)),
               "token_range_finalize_batched")


def observer_update(cur_min, cur_max, rule, cnt, min_val, max_val):
    lib = _hip.load()
    _hip.require_device(cur_min, cur_max, min_val, max_val)
    _check_f32(cur_min, cur_max, min_val, max_val)
    _hip.check(lib.osq_observer_update(_hip.ptr(cur_min), _hip.ptr(cur_max), cur_min.numel(), rule, int(cnt),
                                       _hip.ptr(min_val), _hip.ptr(max_val), _hip.stream_ptr(min_val.device)),
               "observer_update")


# ---------------------------------------------------------------------------------------
# MSEFast
# ---------------------------------------------------------------------------------------

SIDE = {"no": 0, "pos": 1, "neg": 2}


def batch_minmax(x, observation_mask=None, seq_pos=-1):
    """(min, max) of this tensor alone (padding excluded) as a 2-float device tensor; no state touched."""
    cur = torch.empty(2, dtype=torch.float32, device=x.device)
    if observation_mask is not None:
        tmin, tmax, batch, tokens, lengths = token_minmax(x, seq_pos, observation_mask)
        token_range_finalize(tmin, tmax, batch, tokens, lengths, False, 1.0, UPDATE_NONE, 0, None, None, 0, 1, False,
                             None, cur)
    else:
        observe_flat(x, UPDATE_NONE, 0, None, None, 0, 1, False, None, cur)
    return cur


def msefast_rows(w, ch_axis, quant_min, quant_max, symmetric, one_side, two_d):
    """One bounded-Brent search per channel (observer.py:496-517), all rows in one launch."""
    lib = _hip.load()
    _hip.require_device(w)
    _check_f32(w)
    ch_axis = ch_axis % w.dim()
    if ch_axis != 0:                                  # observer.py:11-21: channel axis first, rest flattened
        order = list(range(w.dim()))
        order[ch_axis], order[0] = 0, ch_axis
        w = w.permute(order)
    rows2d = w.reshape(w.shape[0], -1).contiguous()
    rows, cols = rows2d.shape
    bmin = torch.empty(rows, dtype=torch.float32, device=w.device)
    bmax = torch.empty(rows, dtype=torch.float32, device=w.device)
    nfev = torch.empty(rows, dtype=torch.int32, device=w.device)
    _hip.check(lib.osq_msefast_rows(_hip.ptr(rows2d), rows, cols, int(quant_min), int(quant_max), int(bool(symmetric)),
                                    SIDE[one_side], int(bool(two_d)), _hip.ptr(bmin), _hip.ptr(bmax), _hip.ptr(nfev),
                                    _hip.stream_ptr(w.device)), "msefast_rows")
    return bmin, bmax, nfev


class MseSearch:
    """One per-tensor MSEFast search between its begin and its commit (state on the device, what the launches need)."""
    __slots__ = ("state", "x", "view", "lengths", "args", "elems")


def msefast_tensor_begin(x, cur, observation_mask, seq_pos, quant_min, quant_max, symmetric, one_side, two_d,
                         float64_input=False):
    lib = _hip.load()
    dev = x.device
    r = MseSearch()
    r.state = torch.zeros(int(lib.osq_msefast_state_bytes()), dtype=torch.uint8, device=dev)
    _hip.check(lib.osq_msefast_tensor_begin(_hip.ptr(r.state), _hip.ptr(cur), int(quant_min), int(quant_max),
                                            int(bool(symmetric)), SIDE[one_side], int(bool(two_d)), int(bool(float64_input)),
                                            _hip.stream_ptr(dev)), "msefast_begin")
    if observation_mask is not None or not is_dense(x):
        lengths = observation_mask
        if lengths is not None and lengths.dtype != torch.int64:
            lengths = lengths.to(torch.int64)
        if observation_mask is None:
            x = x.contiguous()
            view = None
        else:
            view = token_view(x, seq_pos, lengths.numel())
    else:
        view, lengths = None, None
    if view is None and x.data_ptr() % 16:
        x = x.clone()          # the flat kernels read 16 bytes per lane: a misaligned buffer (a slice of a larger one) is copied once
    r.x, r.view, r.lengths, r.elems = x, view, lengths, x.numel()
    r.args = (int(quant_min), int(quant_max), int(bool(symmetric)))
    return r


def msefast_ordered_fits(r):
    """The float64 form of a search's sum is the finer one (half the lanes): it decides."""
    order = reference_sum_order("mse")
    return bool(order) and ordered_sum_fits(r.elems, order // 2)


def msefast_tensor_run(r, chunk=None, two_d=True):
    """The loss evaluations of one search: one persistent launch when the tensor fits the grid's registers, otherwise one
    launch per evaluation, enqueued in chunks (the converged flag is read back once per chunk; the reference syncs on
    every evaluation)."""
    lib = _hip.load()
    dev = r.x.device
    st = _hip.stream_ptr(dev)
    ws = _hip.workspace(dev)
    order = reference_sum_order("mse")
    if order and msefast_ordered_fits(r):
        return _msefast_tensor_run_ordered(r, chunk, two_d)
    # order-free sums.  (With the reference order set and a tensor beyond the ordered kernels' capacity the resident form
    # answers OSQ_ERR_UNSUPPORTED and the streaming evaluations below run: no library state is toggled for one call.)
    rc = lib.osq_msefast_tensor_search(_hip.ptr(r.state), _hip.ptr(r.x), r.x.numel(), None if r.view is None else ctypes.byref(r.view),
                                       _hip.ptr(r.lengths), _hip.ptr(ws), st)
    if rc not in (0, _hip.ERR_UNSUPPORTED):
        _hip.check(rc, "msefast_tensor_search")
    if rc == 0:
        _mark_persistent(dev)
    done = torch.zeros(1, dtype=torch.int32, device=dev)
    chunk = chunk or (64 if two_d else 32)
    launched = 0
    while rc != 0:
        if r.view is None:
            _hip.check(lib.osq_msefast_tensor_evals_flat(_hip.ptr(r.state), _hip.ptr(r.x), r.x.numel(), chunk, _hip.ptr(ws), st),
                       "msefast_evals_flat")
        else:
            _hip.check(lib.osq_msefast_tensor_evals_tokens(_hip.ptr(r.state), _hip.ptr(r.x), ctypes.byref(r.view),
                                                           _hip.ptr(r.lengths), chunk, _hip.ptr(ws), st), "msefast_evals_tokens")
        launched += chunk
        _hip.check(lib.osq_msefast_tensor_done(_hip.ptr(r.state), _hip.ptr(done), st), "msefast_done")
        if int(done.item()) or launched > 500 * 500:
            break


def _msefast_tensor_run_ordered(r, chunk, two_d):
    """The strict form of a per-tensor search ("mse_sum_order" 8 / 16): the site is laid out once the way the reference's
    remove_padding / flatten does (observer.py:72-84) and every loss evaluation is one launch that adds the squared errors
    in the order of torch.sum on a one-thread host (csrc/aten_order.h)."""
    lib = _hip.load()
    dev = r.x.device
    st = _hip.stream_ptr(dev)
    ws = _hip.workspace(dev)
    if r.view is None:
        flat, n, n_dev = r.x, r.x.numel(), None
    else:
        n = r.view.batch * r.view.tokens * r.view.feat_outer * r.view.feat_inner
        flat = torch.empty(n, dtype=torch.float32, device=dev)
        n_dev = torch.zeros(1, dtype=torch.int64, device=dev)
        _hip.check(lib.osq_gather_valid_tokens(_hip.ptr(r.x), ctypes.byref(r.view), _hip.ptr(r.lengths), _hip.ptr(flat),
                                               _hip.ptr(n_dev), st), "gather_valid_tokens")
    scratch, nbytes = _ordered_scratch(dev, n, 1)
    done = torch.zeros(1, dtype=torch.int32, device=dev)
    chunk = chunk or (64 if two_d else 32)
    launched = 0
    while True:
        _hip.check(lib.osq_msefast_tensor_evals_ordered(_hip.ptr(r.state), _hip.ptr(flat), n, _hip.ptr(n_dev), chunk,
                                                        _hip.ptr(scratch), nbytes, _hip.ptr(ws), st), "msefast_evals_ordered")
        launched += chunk
        _hip.check(lib.osq_msefast_tensor_done(_hip.ptr(r.state), _hip.ptr(done), st), "msefast_done")
        if int(done.item()) or launched > 500 * 500:
            break


ORDERED_GROUP_SITES = 128     # searches one table of osq_msefast_ordered_multi_* holds
# Bytes of site data (and of gathered copies of masked sites, alive together) one group of rounds may hold: a MEMORY bound,
# not a speed knob -- a group runs its own ~600 rounds, so splitting a forward's searches multiplies the launches, and a
# round's cost is dominated by its ~14 000 workgroups' start-up, not by where the bytes come from (measured: groups that fit
# the 256 MiB Infinity Cache are 1.4-2.6x SLOWER than one group, profiles/r05_mse_group_ab.txt).  Masked sites count with all
# their slots (the valid share is only known on the device).  BERT-base [32,128]: 0.57 GB, one group.  0 = no bound.
ORDERED_GROUP_BYTES = int(os.environ.get("OSQ_MSE_GROUP_MIB", "2048")) << 20


ORDERED_CHUNK = max(1, int(os.environ.get("OSQ_MSE_CHUNK", "64")))          # rounds enqueued between two looks at a group's all-done flag
ORDERED_STREAMS = max(1, int(os.environ.get("OSQ_MSE_STREAMS", "2")))     # concurrent groups of nested searches (see msefast_ordered_groups)


def msefast_ordered_groups(searches, two_d):
    """Partition the searches of a flush into the groups whose rounds run together.

    A round is one launch = one loss evaluation of every unfinished search of its group.  Rounds of DIFFERENT groups are
    independent, so the groups run on separate streams (msefast_tensor_run_ordered_groups): the short 1-D searches (~20
    rounds: attention probabilities, one-sided) no longer sit in the tables of the nested ones (hundreds of rounds), and
    one group's ramp and tail are filled by the other's workgroups.  Measured on BASELINE configs[3]: 1.06 s with one
    table per forward -> 0.98-1.03 s with the 1-D searches on their own stream and the nested ones dealt into 1-6 groups
    (the number of groups does not matter beyond that: a round is bound by its float64 arithmetic and its loads, not by
    launch overhead -- profiles/r05_mse_streams_ab.txt).  Hence: the nested (2-D) searches are dealt into ORDERED_STREAMS
    groups of about equal bytes (largest first onto the lightest group), the 1-D searches form one more group; every group
    is bounded by ORDERED_GROUP_SITES and ORDERED_GROUP_BYTES.  Grouping never changes a result: every search's
    evaluations are its own (tests/test_gpu_strict_order.py)."""
    groups = []
    nested = [r for r, nd in zip(searches, two_d) if nd]
    flat = [r for r, nd in zip(searches, two_d) if not nd]
    if nested:
        k = min(ORDERED_STREAMS, len(nested))
        lanes, load = [[] for _ in range(k)], [0] * k
        for r in sorted(nested, key=lambda r: -int(r.elems)):            # stable: equal sizes keep their forward order
            i = load.index(min(load))
            lanes[i].append(r)
            load[i] += int(r.elems)
        groups += [g for g in lanes if g]
    if flat:
        groups.append(flat)
    out = []
    for g in groups:                                                      # the table's and the memory bound's limits
        cur, used = [], 0
        for r in g:
            nbytes = 4 * int(r.elems)
            if cur and (len(cur) == ORDERED_GROUP_SITES or (ORDERED_GROUP_BYTES and used + nbytes > ORDERED_GROUP_BYTES)):
                out.append(cur)
                cur, used = [], 0
            cur.append(r)
            used += nbytes
        if cur:
            out.append(cur)
    return out


def _ordered_group_prepare(group, launch_stream=None):
    """Lay out the masked sites of a group (remove_padding order) and build the group's table.  Every ALLOCATION (gathered
    copies, scratch, table) and its zero fill happens on the CURRENT stream -- the caller's: the blocks come from, and go back
    to, the pool the rest of the calibration allocates from, not a side stream's private pool --; the gathers and the table's
    preparation are launched on `launch_stream` (default: the current one), which first waits for those fills."""
    lib = _hip.load()
    n_sites = len(group)
    assert 0 < n_sites <= ORDERED_GROUP_SITES
    dev = group[0].x.device
    flats, ns, n_devs = [], [], []
    for r in group:
        if r.view is None:
            flats.append(r.x)
            ns.append(r.x.numel())
            n_devs.append(None)
        else:
            n = r.view.batch * r.view.tokens * r.view.feat_outer * r.view.feat_inner
            flats.append(torch.empty(n, dtype=torch.float32, device=dev))
            ns.append(n)
            n_devs.append(torch.zeros(1, dtype=torch.int64, device=dev))
    sizes = [int(lib.osq_ordered_sum_scratch_bytes(int(n), 1)) for n in ns]
    offs, total = [], 0
    for b in sizes:
        offs.append(total)
        total += (b + 255) // 256 * 256
    scratch = torch.empty(total, dtype=torch.uint8, device=dev)
    table_bytes = int(lib.osq_msefast_ordered_multi_bytes(n_sites))
    table = torch.zeros(table_bytes, dtype=torch.uint8, device=dev)
    done = torch.zeros(1, dtype=torch.int32, device=dev)
    ctx = {"table": table, "n_sites": n_sites, "blocks": 0, "done": done, "keep": (flats, n_devs, scratch, group), "launched": 0}

    def launches():
        st = _hip.stream_ptr(dev)
        for r, flat, n_dev in zip(group, flats, n_devs):
            if r.view is not None:
                _hip.check(lib.osq_gather_valid_tokens(_hip.ptr(r.x), ctypes.byref(r.view), _hip.ptr(r.lengths), _hip.ptr(flat),
                                                       _hip.ptr(n_dev), st), "gather_valid_tokens")
        vp = ctypes.c_void_p
        states = (vp * n_sites)(*[_hip.ptr(r.state) for r in group])
        xs = (vp * n_sites)(*[_hip.ptr(f) for f in flats])
        n_arr = (ctypes.c_int64 * n_sites)(*ns)
        nd_arr = (vp * n_sites)(*[_hip.ptr(t) for t in n_devs])
        sc_arr = (vp * n_sites)(*[scratch.data_ptr() + o for o in offs])
        sb_arr = (ctypes.c_size_t * n_sites)(*sizes)
        blocks = ctypes.c_int(0)
        _hip.check(lib.osq_msefast_ordered_multi_prepare(_hip.ptr(table), table_bytes, states, xs, n_arr, nd_arr, sc_arr, sb_arr, n_sites,
                                                         ctypes.byref(blocks), st), "msefast_ordered_multi_prepare")
        ctx["blocks"] = blocks.value

    if launch_stream is None:
        launches()
    else:
        filled = torch.cuda.Event()
        filled.record(torch.cuda.current_stream(dev))
        launch_stream.wait_event(filled)
        with torch.cuda.stream(launch_stream):
            launches()
    return ctx


def _ordered_group_rounds(ctx, chunk):
    """Enqueue `chunk` rounds of a prepared group and its all-done check on the CURRENT stream (nothing waits)."""
    lib = _hip.load()
    dev = ctx["table"].device
    _hip.check(lib.osq_msefast_ordered_multi_evals(_hip.ptr(ctx["table"]), ctx["n_sites"], ctx["blocks"], chunk, _hip.ptr(ctx["done"]),
                                                   _hip.stream_ptr(dev)), "msefast_ordered_multi_evals")
    ctx["launched"] += chunk


def msefast_tensor_run_ordered_group(group, chunk=None):
    """The strict form of several searches (MseSearch records of one device, e.g. the MSEFast observers of one forward):
    rounds of ONE launch = one loss evaluation of every unfinished search, each sum in the order of torch.sum on a
    one-thread host (csrc/aten_order.h, osq_msefast_ordered_multi_*).  Same numbers as _msefast_tensor_run_ordered
    search by search (tests/test_gpu_strict_order.py)."""
    chunk = chunk or ORDERED_CHUNK
    ctx = _ordered_group_prepare(group)
    while True:
        _ordered_group_rounds(ctx, chunk)
        if int(ctx["done"].item()) or ctx["launched"] > 500 * 500:
            break
    return ctx["launched"]


_side_streams = {}


def msefast_tensor_run_ordered_groups(groups, chunk=None):
    """Several groups of strict searches CONCURRENTLY (see msefast_ordered_groups for why), at most ORDERED_STREAMS + 1 at a
    time: a group is prepared -- its gathered copies of masked sites, scratch and table allocated -- only when a stream is
    free, and dropped as soon as its searches have converged, so ORDERED_GROUP_BYTES bounds the memory of
    ORDERED_STREAMS + 1 groups, not of a whole flush (a flush that the byte cap splits into many groups used to hold all of
    them at once).  The side streams start behind everything the caller's stream has been given; the caller's stream
    continues behind all of them -- ALSO when a launch, a prepare or a read-back raises: the records' tensors must not be
    freed under rounds that are still queued.  The records of `groups` must stay referenced by the caller until then (they
    are: the flush commits them afterwards)."""
    chunk = chunk or ORDERED_CHUNK
    groups = [g for g in groups if g]
    if not groups:
        return 0
    if len(groups) == 1:
        return msefast_tensor_run_ordered_group(groups[0], chunk)
    dev = groups[0][0].x.device
    main = torch.cuda.current_stream(dev)
    start = torch.cuda.Event()
    start.record(main)
    lanes = min(len(groups), ORDERED_STREAMS + 1)
    streams = []
    for i in range(lanes):
        key = (_hip._device_index(dev), i)
        s = _side_streams.get(key)
        if s is None:
            s = _side_streams[key] = torch.cuda.Stream(device=dev)
        s.wait_event(start)
        streams.append(s)
    queue = list(groups)
    free = list(streams)
    pending, launched = [], 0
    try:
        while queue or pending:
            while queue and free:                    # a free stream takes the next group: allocations on the caller's stream
                s = free.pop(0)
                pending.append((s, _ordered_group_prepare(queue.pop(0), launch_stream=s)))
            for s, ctx in pending:                   # every unfinished group gets its next rounds before anybody waits
                with torch.cuda.stream(s):
                    _ordered_group_rounds(ctx, chunk)
            still = []
            for s, ctx in pending:
                with torch.cuda.stream(s):
                    finished = int(ctx["done"].item())      # synchronises with s: the group's rounds so far are complete
                if not finished and ctx["launched"] <= 500 * 500:
                    still.append((s, ctx))
                else:
                    launched += ctx["launched"]
                    ctx.clear()                      # the group's copies, scratch and table go back to the pool now
                    free.append(s)
            pending = still
    finally:
        for s in streams:                            # normal end or exception: nothing the caller frees is still in use
            main.wait_stream(s)
    return launched


def msefast_tensor_run_group(group):
    """Several searches (MseSearch records of one device) in ONE persistent launch; False = the group does not fit (nothing
    launched).  The caller sizes groups with msefast_resident_slots."""
    lib = _hip.load()
    n = len(group)
    dev = group[0].x.device
    states = (ctypes.c_void_p * n)(*[_hip.ptr(r.state) for r in group])
    xs = (ctypes.c_void_p * n)(*[_hip.ptr(r.x) for r in group])
    ns = (ctypes.c_int64 * n)(*[r.x.numel() for r in group])
    views = (_hip.TokenView * n)()
    for i, r in enumerate(group):
        if r.view is not None:
            views[i] = r.view
    lens = (ctypes.c_void_p * n)(*[_hip.ptr(r.lengths) for r in group])
    rc = lib.osq_msefast_tensor_search_multi(states, xs, ns, views, lens, n, _hip.ptr(_hip.workspace(dev)), _hip.stream_ptr(dev))
    if rc == _hip.ERR_UNSUPPORTED:
        return False
    _hip.check(rc, "msefast_tensor_search_multi")
    _mark_persistent(dev)
    return True


def msefast_resident_slots(elems):
    return int(_hip.load().osq_msefast_resident_slots(int(elems)))


_resident_limits = None


def msefast_resident_limits():
    """(float4 slots per lane, searches) one osq_msefast_tensor_search_multi launch can hold."""
    global _resident_limits
    if _resident_limits is None:
        a, b = ctypes.c_int(0), ctypes.c_int(0)
        _hip.check(_hip.load().osq_msefast_resident_limits(ctypes.byref(a), ctypes.byref(b)), "msefast_resident_limits")
        _resident_limits = (a.value, b.value)
    return _resident_limits


def msefast_tensor_commit(r, rule, cnt, min_val, max_val, sink=None, ref_float64=None):
    """ref_float64: int32[2] on the device (the reference's dtype of min_val / max_val so far, see osq_hip.h) or None."""
    lib = _hip.load()
    dev = r.x.device
    quant_min, quant_max, symmetric = r.args
    s_ptr, z_ptr, z_type = (sink or _NO_SINK).args()
    nfev = torch.empty(1, dtype=torch.int32, device=dev)
    _hip.check(lib.osq_msefast_tensor_commit(_hip.ptr(r.state), rule, int(cnt), _hip.ptr(min_val), _hip.ptr(max_val),
                                             quant_min, quant_max, symmetric, s_ptr, z_ptr, z_type,
                                             _hip.ptr(nfev), _hip.ptr(ref_float64), _hip.stream_ptr(dev)), "msefast_commit")
    return nfev


def msefast_tensor_stats(r):
    """int32[4] on the device: evaluations so far (nfev), pairs the search's loss memo holds, evaluations it answered, converged
    flag (osq_msefast_tensor_stats; the memo: include/osq_hip.h)."""
    out = torch.empty(4, dtype=torch.int32, device=r.x.device)
    _hip.check(_hip.load().osq_msefast_tensor_stats(_hip.ptr(r.state), _hip.ptr(out), _hip.stream_ptr(r.x.device)), "msefast_tensor_stats")
    return out


def msefast_tensor(x, cur, observation_mask, seq_pos, quant_min, quant_max, symmetric, one_side, two_d,
                   rule, cnt, min_val, max_val, sink=None, chunk=None, float64_input=False):
    """Per-tensor search (observer.py:497-499), begin -> loss evaluations -> commit.  min_val/max_val: float64."""
    r = msefast_tensor_begin(x, cur, observation_mask, seq_pos, quant_min, quant_max, symmetric, one_side, two_d, float64_input)
    msefast_tensor_run(r, chunk, two_d)
    return msefast_tensor_commit(r, rule, cnt, min_val, max_val, sink)


# ---------------------------------------------------------------------------------------
# remaining observers: LSQPlus (moments), AvgQuantile (histogram), MSE (grid)
# ---------------------------------------------------------------------------------------

def _source(x, observation_mask, seq_pos):
    """(x, n, view_or_None, lengths) for kernels that stream either a flat tensor or valid tokens."""
    if observation_mask is None:
        if not is_dense(x):
            x = x.contiguous()
        return x, x.numel(), None, None
    lengths = observation_mask if observation_mask.dtype == torch.int64 else observation_mask.to(torch.int64)
    return x, x.numel(), token_view(x, seq_pos, lengths.numel()), lengths


def observe_moments(x, ch_axis, min_val, max_val, quant_min, quant_max, symmetric, sink=None):
    lib = _hip.load()
    _hip.require_device(x, min_val, max_val)
    _check_f32(x, min_val, max_val)
    x = x.contiguous()
    outer, channels, inner = (1, 1, x.numel()) if ch_axis == -1 else _channel_split(x, ch_axis)
    s_ptr, z_ptr, z_type = (sink or _NO_SINK).args()
    _hip.check(lib.osq_observe_moments(_hip.ptr(x), outer, channels, inner, _hip.ptr(min_val), _hip.ptr(max_val),
                                       int(quant_min), int(quant_max), int(bool(symmetric)), s_ptr, z_ptr, z_type,
                                       _hip.ptr(_hip.workspace(x.device)), _hip.stream_ptr(x.device)), "observe_moments")


def observe_quantile(x, observation_mask, seq_pos, cur, threshold, hist_scratch, rule, cnt, min_val, max_val,
                     quant_min, quant_max, symmetric, sink=None):
    lib = _hip.load()
    _hip.require_device(x, cur, hist_scratch, min_val, max_val)
    _check_f32(x, min_val, max_val)
    x, n, view, lengths = _source(x, observation_mask, seq_pos)
    s_ptr, z_ptr, z_type = (sink or _NO_SINK).args()
    _hip.check(lib.osq_observe_quantile(_hip.ptr(x), n, ctypes.byref(view) if view is not None else None, _hip.ptr(lengths),
                                        _hip.ptr(cur), float(threshold), _hip.ptr(hist_scratch), rule, int(cnt),
                                        _hip.ptr(min_val), _hip.ptr(max_val), int(quant_min), int(quant_max),
                                        int(bool(symmetric)), s_ptr, z_ptr, z_type, _hip.stream_ptr(x.device)),
               "observe_quantile")


def mse_grid_tensor(x, observation_mask, seq_pos, cur, quant_min, quant_max, symmetric, one_side, two_d, rule, cnt,
                    min_val, max_val, sink=None):
    lib = _hip.load()
    _hip.require_device(x, cur, min_val, max_val)
    _check_f32(x, min_val, max_val)
    x, n, view, lengths = _source(x, observation_mask, seq_pos)
    n_cand = int(lib.osq_mse_grid_candidates(int(quant_min), int(quant_max), int(bool(two_d))))
    nbytes = int(lib.osq_mse_grid_scratch_bytes(int(quant_min), int(quant_max), int(bool(two_d))))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=x.device)      # losses + every workgroup's partial sums: the grid is one launch
    losses = scratch[:4 * n_cand].view(torch.float32)
    s_ptr, z_ptr, z_type = (sink or _NO_SINK).args()
    _hip.check(lib.osq_mse_grid_tensor(_hip.ptr(x), n, ctypes.byref(view) if view is not None else None, _hip.ptr(lengths),
                                       _hip.ptr(cur), int(quant_min), int(quant_max), int(bool(symmetric)), SIDE[one_side],
                                       int(bool(two_d)), _hip.ptr(scratch), nbytes, rule, int(cnt), _hip.ptr(min_val),
                                       _hip.ptr(max_val), s_ptr, z_ptr, z_type, _hip.ptr(_hip.workspace(x.device)),
                                       _hip.stream_ptr(x.device)), "mse_grid_tensor")
    return losses


def mse_grid_rows(w, ch_axis, quant_min, quant_max, symmetric, one_side, two_d):
    lib = _hip.load()
    _hip.require_device(w)
    _check_f32(w)
    ch_axis = ch_axis % w.dim()
    if ch_axis != 0:
        order = list(range(w.dim()))
        order[ch_axis], order[0] = 0, ch_axis
        w = w.permute(order)
    rows2d = w.reshape(w.shape[0], -1).contiguous()
    rows, cols = rows2d.shape
    bmin = torch.empty(rows, dtype=torch.float32, device=w.device)
    bmax = torch.empty(rows, dtype=torch.float32, device=w.device)
    _hip.check(lib.osq_mse_grid_rows(_hip.ptr(rows2d), rows, cols, int(quant_min), int(quant_max), int(bool(symmetric)),
                                     SIDE[one_side], int(bool(two_d)), _hip.ptr(bmin), _hip.ptr(bmax),
                                     _hip.stream_ptr(w.device)), "mse_grid_rows")
    return bmin, bmax


# ---------------------------------------------------------------------------------------
# gamma migration
# ---------------------------------------------------------------------------------------

# moved by every kernel of this package that writes a WEIGHT through its raw pointer (torch's ``_version`` does not see
# those writes): cached fake-quantised weights (quantization/weight_cache.py) are keyed on it
weight_epoch = 0


def gamma_fold_(weight, gamma):
    """In place W[:, j] *= gamma[j] (gamma_migration.py:70-71)."""
    global weight_epoch
    weight_epoch += 1
    lib = _hip.load()
    _hip.require_device(weight, gamma)
    _check_f32(weight, gamma)
    if not weight.is_contiguous():
        raise ValueError("gamma_fold_: weight must be contiguous")
    cols = weight.shape[-1]
    if gamma.numel() != cols:
        raise ValueError("gamma_fold_: gamma must have one entry per input feature")
    _hip.check(lib.osq_gamma_fold(_hip.ptr(weight), _hip.ptr(gamma.contiguous()), weight.numel() // cols, cols,
                                  _hip.stream_ptr(weight.device)), "gamma_fold")
    return weight


def gamma_split_bias(beta, gamma):
    lib = _hip.load()
    _hip.require_device(beta, gamma)
    _check_f32(beta, gamma)
    out = torch.empty_like(beta, memory_format=torch.contiguous_format)
    _hip.check(lib.osq_gamma_split_bias(_hip.ptr(beta.contiguous()), _hip.ptr(gamma.contiguous()), _hip.ptr(out),
                                        beta.numel(), _hip.stream_ptr(beta.device)), "gamma_split_bias")
    return out


def gamma_residual(inp, hidden, gamma=None):
    """input * gamma + hidden (util_layernorm.py:49-52), inference path (no autograd)."""
    lib = _hip.load()
    _hip.require_device(inp, hidden, gamma)
    _check_f32(inp, hidden, gamma)
    a, h = inp.contiguous(), hidden.contiguous()
    cols = a.shape[-1]
    out = torch.empty_like(a)
    _hip.check(lib.osq_gamma_residual(_hip.ptr(a), _hip.ptr(h), _hip.ptr(gamma), _hip.ptr(out), a.numel() // cols, cols,
                                      _hip.stream_ptr(a.device)), "gamma_residual")
    return out


# ---------------------------------------------------------------------------------------
# residual + LayerNorm + fake-quant in one pass
# ---------------------------------------------------------------------------------------

def layernorm_fusable(x, *operands):
    """Layout rules of osq_residual_layernorm_fake_quant."""
    cols = x.shape[-1] if x.dim() else 0
    if not (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.numel() and cols % 4 == 0 and cols <= 4096
            and x.data_ptr() % 16 == 0):
        return False
    for t in operands:
        if t is not None and not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.data_ptr() % 16 == 0):
            return False
    return True


def residual_layernorm_fake_quant(x, hidden, gamma, weight, bias, eps, quant=None):
    """y = fake_quant(layer_norm(x*gamma + hidden) * weight + bias) in ONE launch; every operand but x may be None.
    quant: None (no fake-quant) or (scale, zero_point, quant_min, quant_max, mode, grad_factor)."""
    lib = _hip.load()
    _hip.require_device(x, hidden, gamma, weight, bias)
    cols = x.shape[-1]
    rows = x.numel() // cols
    if hidden is not None and hidden.shape != x.shape:
        raise ValueError("residual_layernorm_fake_quant: hidden must have x's shape")
    for name, t in (("gamma", gamma), ("weight", weight), ("bias", bias)):
        if t is not None and t.numel() != cols:
            raise ValueError(f"residual_layernorm_fake_quant: {name} must have {cols} entries")
    y = torch.empty_like(x)
    if quant is None:
        s_ptr, z_ptr, z_type, mode, gf, qmin, qmax = None, None, ZP_INT32, PARAM_FIXED, 1.0, 0, 1
    else:
        scale, zero_point, qmin, qmax, mode, gf = quant
        _hip.require_device(scale, zero_point)
        s_ptr, z_ptr, z_type = scale.data_ptr(), zero_point.data_ptr(), _zp_type(zero_point)
    _hip.check(lib.osq_residual_layernorm_fake_quant(x.data_ptr(), _hip.ptr(hidden), _hip.ptr(gamma), _hip.ptr(weight),
                                                     _hip.ptr(bias), float(eps), y.data_ptr(), rows, cols, s_ptr, z_ptr,
                                                     z_type, int(mode), float(gf), int(qmin), int(qmax),
                                                     _hip.raw_stream(x.device)), "residual_layernorm_fake_quant")
    return y


# ---------------------------------------------------------------------------------------
# GELU + fake-quant in one pass (the intermediate-activation site)
# ---------------------------------------------------------------------------------------

def is_exact_gelu(fn):
    """True for the callables HF models use for hidden_act='gelu' (erf form)."""
    import torch.nn.functional as F
    if fn is F.gelu:
        return True
    if isinstance(fn, torch.nn.GELU):
        return getattr(fn, "approximate", "none") == "none"
    inner = getattr(fn, "act", None)            # transformers.activations.GELUActivation(use_gelu_python=False)
    return type(fn).__name__ == "GELUActivation" and inner is F.gelu


def fake_quant_headsplit_multi(xs, params, heads):
    """The query / key / value sites of one attention block as ONE launch (osq_fake_quant_headsplit_multi).
    xs: 1..4 contiguous [B, T, heads * d] fp32 tensors of one shape; params[i] = (scale, zero_point, quant_min, quant_max,
    mode, grad_factor) of site i.  Returns the dense [B, heads, T, d] fake-quantised head-split tensors -- the bits of
    fake_quant_per_tensor on each ``x.view(B, T, heads, d).permute(0, 2, 1, 3)`` -- or None when the kernel does not take the
    geometry (nothing was launched)."""
    lib = _hip.load()
    n = len(xs)
    b, t, width = xs[0].shape
    d = width // heads
    table = (_hip.HeadSplitSite * n)()
    ys = []
    for i, (x, (scale, zero_point, quant_min, quant_max, mode, grad_factor)) in enumerate(zip(xs, params)):
        y = torch.empty((b, heads, t, d), dtype=x.dtype, device=x.device)
        ys.append(y)
        e = table[i]
        e.x, e.y, e.scale, e.zero_point = x.data_ptr(), y.data_ptr(), scale.data_ptr(), zero_point.data_ptr()
        e.zp_type, e.mode, e.grad_factor, e.quant_min, e.quant_max = _zp_type(zero_point), int(mode), float(grad_factor), int(quant_min), int(quant_max)
    rc = lib.osq_fake_quant_headsplit_multi(table, n, b, t, heads, d, _hip.stream_ptr(xs[0].device))
    if rc == _hip.ERR_UNSUPPORTED:
        return None
    _hip.check(rc, "fake_quant_headsplit_multi")
    return ys


def fake_quant_kv_append(sites, heads):
    """One decoder step's attention sites as ONE launch (osq_fake_quant_kv_append).  ``sites``: 1..4 tuples
    ``(x, y, offset, params, src, src_rows)`` of one batch size B:

    * x -- the step's contiguous [B, t, heads * d] fp32 projection (t may differ between sites);
    * y -- a dense [B, heads, cap, d] buffer; ``y[:, :, offset:offset + t]`` receives the head-split fake-quant of x, the
      bits of ``fake_quant_per_tensor`` on ``x.view(B, t, heads, d).transpose(1, 2)``;
    * params -- (scale, zero_point, quant_min, quant_max, mode, grad_factor) of the site;
    * src / src_rows -- None, or a [B', heads, S', d] tensor whose last two dimensions are dense (a ``[:, :, :S']`` view of
      a cache buffer is) with S' >= offset, and None or an int64 device index of length B: ``y[:, :, :offset] =
      src.index_select(0, src_rows)[:, :, :offset]`` in the same launch.  ``src`` being ``y`` without an index copies
      nothing (in-place append).

    Returns the list of y, or None when the kernel does not take the geometry (nothing was launched)."""
    lib = _hip.load()
    n = len(sites)
    if not 1 <= n <= 4:
        raise ValueError("fake_quant_kv_append: 1..4 sites")
    b = sites[0][0].shape[0]
    d = sites[0][1].shape[-1]
    table = (_hip.KvAppendSite * n)()
    for i, (x, y, offset, params, src, rows) in enumerate(sites):
        if not _kv_site(table[i], "fake_quant_kv_append", x, y, offset, params, src, rows, b, heads, d, torch.float32):
            return None
    rc = lib.osq_fake_quant_kv_append(table, n, b, heads, d, _hip.stream_ptr(sites[0][0].device))
    if rc == _hip.ERR_UNSUPPORTED:
        return None
    _hip.check(rc, "fake_quant_kv_append")
    return [site[1] for site in sites]


def _kv_site(e, what, x, y, offset, params, src, rows, b, heads, d, dtype):
    """Fill one entry of a KV-append table (osq_kv_append_site / osq_kv_codes_site) after checking its tensors; y and src
    hold ``dtype`` elements.  ``offset`` None (the _at forms): the launch reads the position, and a src is the buffer the
    prefix comes from, whatever its length.  False: a source layout the kernel does not take."""
    scale, zero_point, quant_min, quant_max, mode, grad_factor = params
    from_pos = offset is None
    if from_pos:
        offset = 0
    _hip.require_device(x, y, scale, zero_point)
    _check_f32(x, scale)
    if y.dtype != dtype:
        raise TypeError(f"{what}: y must be {dtype}, got {y.dtype}")
    t = x.shape[1]
    if (x.dim() != 3 or x.shape[0] != b or x.shape[2] != heads * d or not x.is_contiguous() or y.dim() != 4
            or tuple(y.shape[:2]) != (b, heads) or y.shape[3] != d or not y.is_contiguous()):
        raise ValueError(f"{what}: x must be [B, t, heads*d] and y [B, heads, cap, d], both contiguous")
    if not 0 <= offset or offset + t > y.shape[2]:
        raise ValueError(f"{what}: offset {offset} + {t} tokens exceeds the capacity {y.shape[2]}")
    e.x, e.y, e.scale, e.zero_point = x.data_ptr(), y.data_ptr(), scale.data_ptr(), zero_point.data_ptr()
    e.tokens, e.cap, e.offset = t, y.shape[2], int(offset)
    if src is not None and (from_pos or offset > 0):
        _hip.require_device(src)
        if src.dtype != dtype:
            raise TypeError(f"{what}: src must be {dtype}, got {src.dtype}")
        if src.dim() != 4 or src.shape[1] != heads or src.shape[3] != d or src.shape[2] < offset:
            raise ValueError(f"{what}: src must be [B', heads, S' >= offset, d]")
        st = src.stride()
        if st[3] != 1 or st[2] != d or st[1] % d or st[1] // d < src.shape[2] or st[0] != heads * st[1]:
            return False
        e.src, e.src_batch, e.src_cap = src.data_ptr(), src.shape[0], st[1] // d
        if rows is not None:
            _hip.require_device(rows)
            if rows.dtype != torch.int64 or rows.dim() != 1 or rows.shape[0] != b or not rows.is_contiguous():
                raise ValueError(f"{what}: src_rows must be a contiguous int64 [B] device tensor")
            e.src_rows = rows.data_ptr()
        elif src.shape[0] != b:
            raise ValueError(f"{what}: src batch differs from B and no src_rows given")
    e.zp_type, e.mode, e.grad_factor = _zp_type(zero_point), int(mode), float(grad_factor)
    e.quant_min, e.quant_max = int(quant_min), int(quant_max)
    return True


def _kv_position(what, sites, pos):
    """The position word and the per-site flags of an _at append: a site whose offset is None appends at ``*pos``."""
    _hip.require_device(pos)
    if pos.dtype != torch.int32 or pos.numel() != 1:
        raise TypeError(f"{what}: pos must be one int32")
    return (ctypes.c_int32 * len(sites))(*[int(site[2] is None) for site in sites])


def fake_quant_kv_append_at(sites, heads, pos):
    """fake_quant_kv_append with the position read by the launch (osq_fake_quant_kv_append_at): ``pos`` is one int32 on
    the device, and a site whose ``offset`` is None appends at ``[*pos, *pos + t)`` and copies ``[0, *pos)`` of its src (a
    [B', heads, S', d] buffer, S' its capacity) through src_rows.  A captured graph of the call serves every position; the
    buffers hold what fake_quant_kv_append writes for that offset.  A position that does not fit writes nothing."""
    lib = _hip.load()
    n = len(sites)
    if not 1 <= n <= 4:
        raise ValueError("fake_quant_kv_append_at: 1..4 sites")
    at = _kv_position("fake_quant_kv_append_at", sites, pos)
    b = sites[0][0].shape[0]
    d = sites[0][1].shape[-1]
    table = (_hip.KvAppendSite * n)()
    for i, (x, y, offset, params, src, rows) in enumerate(sites):
        if not _kv_site(table[i], "fake_quant_kv_append_at", x, y, offset, params, src, rows, b, heads, d, torch.float32):
            return None
    rc = lib.osq_fake_quant_kv_append_at(table, n, b, heads, d, pos.data_ptr(), at, _hip.stream_ptr(sites[0][0].device))
    if rc == _hip.ERR_UNSUPPORTED:
        return None
    _hip.check(rc, "fake_quant_kv_append_at")
    return [site[1] for site in sites]


def fake_quant_kv_append_codes_at(sites, heads, rejected, pos):
    """fake_quant_kv_append_codes with the position read by the launch (osq_fake_quant_kv_append_codes_at); sites, pos and
    the None offset as in fake_quant_kv_append_at.  A position that does not fit writes nothing and adds 1 to ``rejected``
    when a site is coded."""
    return _kv_append_codes(sites, heads, rejected, pos)


def fake_quant_kv_append_codes(sites, heads, rejected):
    """fake_quant_kv_append with a destination kind per site (osq_fake_quant_kv_append_codes, csrc/kv_codes.hip).
    ``sites``: 1..4 tuples ``(x, y, offset, params, src, src_rows, record, write_record)``:

    * record None -- an fp32 site, exactly fake_quant_kv_append's (the query site);
    * record ``(scale_eff, zp_eff)``, two one-element fp32 device tensors -- y and src are uint8 buffers of the same
      [B, heads, cap, d] geometry and receive the codes ``x_quant - quant_min`` (quant_max - quant_min <= 255), the bytes of
      ``quantize_codes`` on the head-split view; the kept prefix is copied as bytes.  ``write_record``: this launch writes
      the record (the tensor's first append); otherwise it compares its effective parameters with the record bit for bit.
    * rejected -- the cache's int32 device counter: elements without a code (code 0 written), a record mismatch and the
      elements behind a src_rows entry out of range are added to it.

    Returns the list of y, or None when the kernel does not take the geometry (nothing was launched)."""
    return _kv_append_codes(sites, heads, rejected, None)


def _kv_append_codes(sites, heads, rejected, _pos):
    """fake_quant_kv_append_codes (``_pos`` None) and fake_quant_kv_append_codes_at: one table, two entry points."""
    lib = _hip.load()
    n = len(sites)
    if not 1 <= n <= 4:
        raise ValueError("fake_quant_kv_append_codes: 1..4 sites")
    _hip.require_device(rejected)
    if rejected.dtype != torch.int32 or rejected.numel() != 1:
        raise TypeError("fake_quant_kv_append_codes: rejected must be one int32")
    what = "fake_quant_kv_append_codes" if _pos is None else "fake_quant_kv_append_codes_at"
    at = None if _pos is None else _kv_position(what, sites, _pos)
    b = sites[0][0].shape[0]
    d = sites[0][1].shape[-1]
    table = (_hip.KvCodesSite * n)()
    for i, (x, y, offset, params, src, rows, record, write_record) in enumerate(sites):
        e = table[i]
        if not _kv_site(e, "fake_quant_kv_append_codes", x, y, offset, params, src, rows, b, heads, d,
                        torch.float32 if record is None else torch.uint8):
            return None
        if record is not None:
            if params[3] - params[2] > 255:
                raise ValueError("fake_quant_kv_append_codes: quant_max - quant_min does not fit a byte")
            _hip.require_device(*record)
            _check_f32(*record)
            e.scale_eff, e.zp_eff, e.coded, e.write_record = record[0].data_ptr(), record[1].data_ptr(), 1, int(bool(write_record))
    if _pos is None:
        rc = lib.osq_fake_quant_kv_append_codes(table, n, b, heads, d, rejected.data_ptr(), _hip.stream_ptr(sites[0][0].device))
    else:
        rc = lib.osq_fake_quant_kv_append_codes_at(table, n, b, heads, d, rejected.data_ptr(), _pos.data_ptr(), at,
                                                   _hip.stream_ptr(sites[0][0].device))
    if rc == _hip.ERR_UNSUPPORTED:
        return None
    _hip.check(rc, what)
    return [site[1] for site in sites]


def gelu_fake_quant_per_tensor(x, scale, zero_point, quant_min, quant_max, mode=PARAM_FIXED, grad_factor=1.0):
    """fake_quant(F.gelu(x)) in ONE launch; x dense fp32 on the device."""
    lib = _hip.load()
    _hip.require_device(x, scale, zero_point)
    _check_f32(x, scale)
    if not x.is_contiguous():
        x = x.contiguous()
    if x.data_ptr() % 16:          # a slice of a larger buffer: the two launches this one replaces (same numbers)
        return fake_quant_per_tensor(torch.nn.functional.gelu(x), scale, zero_point, quant_min, quant_max, mode, grad_factor)
    y = torch.empty_like(x)
    _hip.check(lib.osq_gelu_fake_quant_per_tensor(x.data_ptr(), y.data_ptr(), x.numel(), scale.data_ptr(),
                                                  zero_point.data_ptr(), _zp_type(zero_point), int(mode),
                                                  float(grad_factor), int(quant_min), int(quant_max),
                                                  _hip.raw_stream(x.device)), "gelu_fake_quant_per_tensor")
    return y


# ---------------------------------------------------------------------------------------
# pre-softmax scaling + mask -> softmax -> fake-quant in one pass (the attention-probabilities site)
# ---------------------------------------------------------------------------------------

def _as_4d(x):
    return (1,) * (4 - x.dim()) + tuple(x.shape)


def _mask_fusable(mask, shape, device):
    """The mask rule of the attention sites over whole sequences: None, or fp32 on ``device``, of at most four dims,
    broadcastable to ``shape`` with a contiguous last axis (any strides, 0 included, on the others)."""
    if mask is None:
        return True
    if not (mask.device == device and mask.dtype == torch.float32 and mask.dim() <= 4):
        return False
    try:
        m = mask.expand(shape)
    except RuntimeError:
        return False
    return shape[-1] == 1 or m.stride(-1) == 1


def attention_softmax_fusable(scores, mask=None):
    """Layout rules of osq_attention_softmax_fake_quant: scores a contiguous fp32 [.., T, S] tensor of at most four dims
    on the device; mask None, or fp32 on the same device, broadcastable to scores with a contiguous last axis (any
    strides, 0 included, on the others).  Every row width is taken (cols % 4 == 0 and cols <= 2048 the fast kernel)."""
    if not (scores.is_cuda and scores.dtype == torch.float32 and 1 <= scores.dim() <= 4 and scores.is_contiguous()
            and scores.numel()):
        return False
    return _mask_fusable(mask, scores.shape, scores.device)


def attention_softmax_fake_quant(scores, mask=None, *, alpha=None, divisor=None, quant=None):
    """probs = fake_quant(softmax(pre(scores) + mask, dim=-1)) in ONE launch on the current stream.
    pre: ``scores * alpha`` (with a mask: the bits of ``torch.add(mask, scores, alpha=alpha)`` -- exact for the power-of-two
    alpha callers pass), ``scores / divisor`` (IEEE division), or ``scores`` (neither given).  mask: None or broadcastable
    to scores (see attention_softmax_fusable).  quant: None (softmax only) or (scale, zero_point, quant_min, quant_max,
    mode, grad_factor) as for residual_layernorm_fake_quant."""
    lib = _hip.load()
    _hip.require_device(scores, mask)
    if alpha is not None and divisor is not None:
        raise ValueError("attention_softmax_fake_quant: give alpha or divisor, not both")
    if not attention_softmax_fusable(scores, mask):
        raise ValueError("attention_softmax_fake_quant: scores must be a contiguous fp32 tensor of <= 4 dims and mask "
                         "an fp32 tensor broadcastable to it with a contiguous last axis")
    b, h, t, s = _as_4d(scores)
    sb = sh = st = 0
    if mask is not None:
        strides = (0,) * (4 - scores.dim()) + tuple(mask.expand(scores.shape).stride())
        sb, sh, st = strides[0], strides[1], strides[2]
    y = torch.empty_like(scores)
    _hip.check(lib.osq_attention_softmax_fake_quant(scores.data_ptr(), _hip.ptr(mask), b, h, t, s, sb, sh, st,
                                                    1.0 if alpha is None else float(alpha),
                                                    1.0 if divisor is None else float(divisor), y.data_ptr(),
                                                    *_quant_group(quant), _hip.raw_stream(scores.device)),
               "attention_softmax_fake_quant")
    return y


# ---------------------------------------------------------------------------------------
# attention over a whole sequence: both products, mask, softmax, two quantizers in one launch
# ---------------------------------------------------------------------------------------

ATTENTION_TQ = 32          # kBlkTQ of csrc/attention_block.hip: the query rows of a workgroup
ATTENTION_TK = 32          # kBlkTK: the key columns of a score tile
ATTENTION_MAX_KV = 1024    # kBlkMaxS
ATTENTION_HEAD_DIMS = (16, 32, 64, 128)


def attention_fusable(q, k, v, mask=None, group=1):
    """Layout rules of osq_attention_fake_quant: q [B, h, T, d], k / v [B, h, S, d], fp32 on one device, with a contiguous
    last axis and any strides on the others (dense tensors, BERT's permuted views of [B, T, H], ``[:, :, :S]`` views of cache
    buffers); mask None, or fp32 on that device, broadcastable to [B, h, T, S] with a contiguous last axis (any strides, 0
    included, on the others).  With ``group`` = G (osq_attention_fake_quant_shared) q is [B * G, h, T, d] and its rows
    b * G .. b * G + G - 1 share row b of k, v and mask.  What the library refuses on top (head_dim, S, alignment) it says
    itself."""
    if not (q.dim() == 4 and k.dim() == 4 and v.dim() == 4 and q.is_cuda and q.numel() and k.numel()):
        return False
    if group < 1 or q.shape[0] % group:
        return False
    b, (h, t, d) = q.shape[0] // group, q.shape[1:]
    s = k.shape[2]
    if tuple(k.shape) != (b, h, s, d) or tuple(v.shape) != (b, h, s, d):
        return False
    for x in (q, k, v):
        if x.dtype != torch.float32 or x.device != q.device or (d > 1 and x.stride(3) != 1):
            return False
    return _mask_fusable(mask, (b, h, t, s), q.device)


def _attention(what, entry, q, k, v, mask, quants, n_required, max_kv, alpha, divisor, want_probs, out, probs_out, group=1):
    """The body of attention_fake_quant and attention_int_fake_quant below; ``what`` is the caller's name in messages, ``entry``
    the library's function.  ``quants``: the quantizer records in the order of the entry's groups, the context's last.  The
    first ``n_required`` of them are the operands of exact products: each must be there, per-tensor, on the device of q and
    of at most 256 codes, and the context's, where given, per-tensor on that device.  ``max_kv``: the keys the kernel takes.
    ``group``: the rows of q that share a row of k / v / mask (attention_fusable); the library's ``entry + "_shared"`` whatever
    its value, so that there is one call below.
    Returns out -- with ``want_probs`` or ``probs_out`` the pair (out, probabilities) -- or None when the call is not taken;
    what the library would refuse by head size, length or code range is asked before anything is allocated."""
    lib = _hip.load()
    _hip.require_device(q, k, v, mask)
    if alpha is not None and divisor is not None:
        raise ValueError(f"{what}: give alpha or divisor, not both")
    group = int(group)
    if group < 1:
        raise ValueError(f"{what}: group must be at least 1")
    if not attention_fusable(q, k, v, mask, group):
        return None
    if n_required:
        checked = list(quants[:n_required]) + [x for x in quants[n_required:] if x is not None]
        if not all(_per_tensor_quant(x, q.device) for x in checked):
            return None
    bq, h, t, d = q.shape              # bq = b * group rows of q, out and the probabilities over b rows of k, v and mask
    b, s = k.shape[0], k.shape[2]
    msb = msh = mst = 0
    if mask is not None:
        msb, msh, mst = mask.expand(b, h, t, s).stride()[:3]
    for given, shape, name in ((out, (bq, t, h * d), "out"), (probs_out, (bq, h, t, s), "probs_out")):
        if given is not None and (given.dtype != torch.float32 or tuple(given.shape) != shape or not given.is_contiguous()
                                  or given.device != q.device):
            raise ValueError(f"{what}: {name} must be a contiguous fp32 tensor of shape {shape}")
    groups = [_quant_group(x) for x in quants]
    if d not in ATTENTION_HEAD_DIMS or s > max_kv or any(g[6] - g[5] > ATTENTION_INT_MAX_RANGE for g in groups[:n_required]):
        return None
    if out is None:
        out = torch.empty((bq, t, h * d), dtype=torch.float32, device=q.device)
    want_probs = want_probs or probs_out is not None
    probs = probs_out if probs_out is not None or not want_probs else torch.empty((bq, h, t, s), dtype=torch.float32, device=q.device)
    # the stride of an axis of one element is never multiplied by anything but 0
    strides = [0 if x.shape[i] == 1 else x.stride(i) for x in (q, k, v) for i in range(3)]
    rc = getattr(lib, entry + "_shared")(q.data_ptr(), k.data_ptr(), v.data_ptr(), _hip.ptr(mask), out.data_ptr(),
                                         _hip.ptr(probs), b, group, h, t, s, d, *strides, msb, msh, mst,
                                         1.0 if alpha is None else float(alpha), 1.0 if divisor is None else float(divisor),
                                         *[x for g in groups for x in g], _hip.raw_stream(q.device))
    if rc == _hip.ERR_UNSUPPORTED:
        return None
    _hip.check(rc, what)
    return (out, probs) if want_probs else out


def attention_fake_quant(q, k, v, mask, probs_quant, ctx_quant, alpha=None, divisor=None, want_probs=False, *, out=None,
                         probs_out=None, group=1):
    """``fq_ctx(merge_heads(fq_probs(softmax(pre(q @ k^T) + mask)) @ v))`` for whole sequences in ONE launch
    (osq_attention_fake_quant, csrc/attention_block.hip): the [B, h, T, S] scores are never written.

    q [B, h, T, d], k / v [B, h, S, d] and mask as attention_fusable states; nothing is copied.  pre: ``alpha`` / ``divisor``
    as in attention_softmax_fake_quant (give one or neither).  probs_quant / ctx_quant: None (no quantizer) or
    (scale, zero_point, quant_min, quant_max, mode, grad_factor).  ``out`` / ``probs_out``: contiguous fp32 [B, T, h * d] /
    [B, h, T, S] tensors to write into (``probs_out`` implies ``want_probs``).  Returns the [B, T, h * d] output -- with
    ``want_probs`` the pair (output, fake-quantised probabilities [B, h, T, S]) -- or None when the layout is not fusable or the library refuses
    it (head_dim outside 16 / 32 / 64 / 128, S above 1024, a misaligned pointer or stride): nothing was launched, the
    caller runs the eager sequence.

    ``group`` = G > 1 (osq_attention_fake_quant_shared): q is [B * G, h, T, d], k / v [B, h, S, d] and mask broadcastable to
    [B, h, T, S]; rows b * G .. b * G + G - 1 of q attend over row b.  out [B * G, T, h * d] and the probabilities
    [B * G, h, T, S] are word for word those of the call without a group on k, v and mask ``repeat_interleave``d G times."""
    return _attention("attention_fake_quant", "osq_attention_fake_quant", q, k, v, mask, (probs_quant, ctx_quant), 0,
                      ATTENTION_MAX_KV, alpha, divisor, want_probs, out, probs_out, group)


ATTENTION_INT_TQ = 128         # kIntTQ of csrc/attention_int.hip: the query rows of a workgroup
ATTENTION_INT_TK = 32          # kIntTK: the keys of a tile
ATTENTION_INT_CHUNK = 128      # kIntChunk: the keys whose context terms are summed in fp32 before they join the int32 sum
ATTENTION_INT_MAX_KV = 16384   # kIntMaxS
ATTENTION_INT_MAX_RANGE = 255  # quant_max - quant_min of the q / k / v / probabilities quantizers


def _per_tensor_quant(quant, device):
    """``quant`` is a (scale, zero_point, ...) record of ONE scale and ONE zero point on ``device``."""
    return (quant is not None and quant[0].numel() == 1 and quant[1].numel() == 1 and quant[0].device == device
            and quant[1].device == device)


def attention_int_fake_quant(q, k, v, mask, q_quant, k_quant, v_quant, probs_quant, ctx_quant, alpha=None, divisor=None,
                             want_probs=False, *, out=None, probs_out=None, group=1):
    """attention_fake_quant on the INTEGER CODES of the quantizers that produced q, k and v and of the probabilities
    quantizer (osq_attention_fake_quant_int, csrc/attention_int.hip): both products on the bf16 matrix instruction, exact --
    the context is word for word ``fq_ctx(float(sum_j n_p[j] * n_v[j]) * (s_p * s_v))``; no limit at 1024 keys.

    q, k, v, mask, ``alpha`` / ``divisor``, ``out`` / ``probs_out``, ``group`` (osq_attention_fake_quant_int_shared) and the
    return convention are attention_fake_quant's.
    q_quant / k_quant / v_quant / probs_quant: (scale, zero_point, quant_min, quant_max, mode, grad_factor), per-tensor, on
    the device of q, ``quant_max - quant_min <= 255`` -- all four required; ctx_quant: such a record or None.  Returns None
    when one of them is missing, per-channel, elsewhere or too wide, when the layout is not fusable or the library refuses
    it (head_dim outside 16 / 32 / 64 / 128, S above 16384, a misaligned pointer or stride): nothing was launched."""
    return _attention("attention_int_fake_quant", "osq_attention_fake_quant_int", q, k, v, mask,
                      (q_quant, k_quant, v_quant, probs_quant, ctx_quant), 4, ATTENTION_INT_MAX_KV, alpha, divisor, want_probs,
                      out, probs_out, group)


# ---------------------------------------------------------------------------------------
# one decoding step's attention over the KV cache: scores, mask, softmax, two quantizers in one launch
# ---------------------------------------------------------------------------------------

def _kv_cap(x, b, h, s, d, dtype=torch.float32):
    """cap of a [B, h, S, d] fp32 (``dtype``) tensor laid out as the first S positions of a [B, h, cap, d] buffer (a ``[:, :, :S]`` view of
    a cache buffer, or a dense tensor: cap == S), or None when it is laid out otherwise."""
    if x.dim() != 4 or tuple(x.shape) != (b, h, s, d) or x.dtype != dtype:
        return None
    st = x.stride()
    if st[3] != 1 or (s > 1 and st[2] != d):
        return None
    if h > 1:
        row = st[1]
    elif b > 1:
        row = st[0]
    else:
        row = s * d
    if row % d or row // d < s or (b > 1 and st[0] != h * row):
        return None
    return row // d


def _quant_group(quant):
    if quant is None:
        return [None, None, ZP_INT32, PARAM_FIXED, 1.0, 0, 1]
    scale, zero_point, qmin, qmax, mode, gf = quant
    _hip.require_device(scale, zero_point)
    _check_f32(scale)
    return [scale.data_ptr(), zero_point.data_ptr(), _zp_type(zero_point), int(mode), float(gf), int(qmin), int(qmax)]


def _codes_args(what, codes):
    """The launch arguments of a coded cache, ``codes = (k_record, v_record, rejected)``: each record
    ``(scale_eff, zp_eff, quant_min)`` with one-element fp32 device tensors, rejected the cache's int32 device counter."""
    k_record, v_record, rejected = codes
    _hip.require_device(rejected, k_record[0], k_record[1], v_record[0], v_record[1])
    _check_f32(k_record[0], k_record[1], v_record[0], v_record[1])
    if rejected.dtype != torch.int32 or rejected.numel() != 1:
        raise TypeError(f"{what}: rejected must be one int32")
    return (k_record[0].data_ptr(), k_record[1].data_ptr(), int(k_record[2]),
            v_record[0].data_ptr(), v_record[1].data_ptr(), int(v_record[2]), rejected.data_ptr())


def _strided_rows(t, b, heads_axis, width):
    """Row stride of an fp32 [b, heads_axis, 1, W >= width] tensor with a dense last axis whose rows lie evenly apart, or
    None when it is laid out otherwise."""
    if (t.dtype != torch.float32 or t.dim() != 4 or tuple(t.shape[:3]) != (b, heads_axis, 1) or t.shape[3] < width
            or (t.shape[3] > 1 and t.stride(3) != 1)):
        return None
    row = t.stride(1) if heads_axis > 1 else (t.stride(0) if b > 1 else t.shape[3])
    if row < t.shape[3] or (heads_axis > 1 and b > 1 and t.stride(0) != heads_axis * row):
        return None
    return row


def _decode_attention(what, q, k, v, mask, probs_quant, ctx_quant, *, group=None, codes=None, at=None, out=None, probs_out=None,
                      want_probs=False):
    """The body of the four decode_attention_* functions below (csrc/decode_attention.hip); ``what`` is the caller's name in
    messages.  ``group``: None for the one-query entry points, else the shared ones with that many query rows per row of
    k / v.  ``at``: None for the static forms, which take k / v as views and the length from their
    shape, or ``(kv_len, kv_len_add, kv_max, grad_table)`` for the length read by the launch over whole buffers.  Returns
    out -- with ``want_probs`` the pair (out, probabilities) -- or None when the library does not take the layout."""
    lib = _hip.load()
    kv_len, kv_len_add, kv_max, grad_table = at if at is not None else (None, 0, 0, None)
    _hip.require_device(q, k, v, mask, kv_len, grad_table, out, probs_out)
    _check_f32(q)
    if at is not None and (kv_len.dtype != torch.int32 or kv_len.numel() != 1):
        raise TypeError(f"{what}: kv_len must be one int32")
    shared, group = group is not None, 1 if group is None else int(group)
    if group < 1:
        raise ValueError(f"{what}: group must be at least 1")
    dtype = torch.float32 if codes is None else torch.uint8
    if q.dim() != 4 or q.shape[2] != 1 or not q.is_contiguous() or k.dim() != 4 or v.dim() != 4 or q.shape[0] % group:
        return None
    rows, h, _, d = q.shape
    b = rows // group
    if at is None:
        s = k.shape[2]
        k_cap, v_cap = _kv_cap(k, b, h, s, d, dtype), _kv_cap(v, b, h, s, d, dtype)
        if k_cap is None or v_cap is None:
            return None
        if mask is not None and not (mask.dtype == torch.float32 and tuple(mask.shape) == (b, 1, 1, s) and mask.is_contiguous()):
            return None
    else:
        if (k.dtype != dtype or v.dtype != dtype or not k.is_contiguous() or not v.is_contiguous()
                or tuple(k.shape[:2]) != (b, h) or tuple(v.shape[:2]) != (b, h) or k.shape[3] != d or v.shape[3] != d):
            return None
        s, k_cap, v_cap = int(kv_max), k.shape[2], v.shape[2]
        if k_cap < s or v_cap < s:
            raise ValueError(f"{what}: kv_max exceeds the capacity of k / v")
        strides = [0 if t is None else _strided_rows(t, b, heads_axis, s) for t, heads_axis in ((mask, 1), (probs_out, h))]
        if None in strides:
            return None
        if grad_table is not None and (grad_table.dtype != torch.float32 or grad_table.numel() < s + 1
                                       or not grad_table.is_contiguous()):
            raise ValueError(f"{what}: grad_table must hold kv_max + 1 contiguous floats")
    if out is None:
        out = torch.empty((rows, 1, h * d), dtype=torch.float32, device=q.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (rows, 1, h * d) or not out.is_contiguous():
        raise ValueError(f"{what}: out must be a contiguous fp32 [B, 1, h * d] tensor")
    if want_probs:
        probs_out = torch.empty((rows, h, 1, s), dtype=torch.float32, device=q.device)
    if at is None:
        head = (q.data_ptr(), k.data_ptr(), v.data_ptr(), _hip.ptr(mask), out.data_ptr(), _hip.ptr(probs_out), b,
                *((group,) if shared else ()), h, d, s, k_cap, v_cap)
    else:
        head = (q.data_ptr(), k.data_ptr(), v.data_ptr(), _hip.ptr(mask), strides[0], out.data_ptr(), _hip.ptr(probs_out),
                strides[1], b, h, d, kv_len.data_ptr(), int(kv_len_add), s, k_cap, v_cap, _hip.ptr(grad_table))
    name = ("shared_codes" if codes is not None else "shared") if shared else ("codes" if codes is not None else "fake_quant")
    entry = getattr(lib, "osq_decode_attention_" + name + ("_at" if at is not None else ""))
    record = () if codes is None else _codes_args(what, codes)
    rc = entry(*head, *record, *_quant_group(probs_quant), *_quant_group(ctx_quant), _hip.raw_stream(q.device))
    if rc == _hip.ERR_UNSUPPORTED:
        return None
    _hip.check(rc, what)
    return (out, probs_out) if want_probs else out


def decode_attention_fake_quant(q, k, v, mask, probs_quant, ctx_quant, want_probs=False):
    """``fq_ctx(merge_heads(fq_probs(softmax(q @ k^T + mask)) @ v))`` for ONE query token in ONE launch
    (osq_decode_attention_fake_quant, csrc/decode_attention.hip).

    q: dense [B, h, 1, d] fp32, the fake-quantised, scaled query.  k / v: [B, h, S, d] fp32, dense or ``[:, :, :S]`` views of
    [B, h, cap, d] cache buffers (each with its own cap); nothing is copied.  mask: None or a dense additive [B, 1, 1, S].
    probs_quant / ctx_quant: None (no quantizer) or (scale, zero_point, quant_min, quant_max, mode, grad_factor).
    Returns the [B, 1, h * d] output -- with ``want_probs`` the pair (output, fake-quantised probabilities [B, h, 1, S]) --
    or None when the library does not take the layout (nothing was launched): the caller runs the eager sequence."""
    return _decode_attention("decode_attention_fake_quant", q, k, v, mask, probs_quant, ctx_quant, want_probs=want_probs)


def decode_attention_codes(q, k, v, mask, probs_quant, ctx_quant, k_record, v_record, rejected, want_probs=False):
    """decode_attention_fake_quant over a coded cache (osq_decode_attention_codes): k / v are uint8 [B, h, S, d] code
    tensors, dense or ``[:, :, :S]`` views of [B, h, cap, d] buffers; k_record / v_record ``(scale_eff, zp_eff, quant_min)``
    with one-element fp32 device tensors; rejected the cache's int32 device counter -- non-zero: every output word is NaN.
    The outputs are word-equal to decode_attention_fake_quant on the dequantised k / v.  Returns as that function does."""
    codes = (k_record, v_record, rejected)
    _codes_args("decode_attention_codes", codes)        # this form has always checked the record before the layout
    return _decode_attention("decode_attention_codes", q, k, v, mask, probs_quant, ctx_quant, codes=codes, want_probs=want_probs)


def decode_attention_at(q, k, v, kv_len, kv_len_add, kv_max, mask, probs_quant, ctx_quant, grad_table=None, codes=None,
                        out=None, probs_out=None):
    """decode_attention_fake_quant / decode_attention_codes with the length read by the launch
    (osq_decode_attention_fake_quant_at / osq_decode_attention_codes_at): ``kv_len`` is one int32 on the device and the
    launch attends over ``*kv_len + kv_len_add`` positions, so a captured graph of the call serves every step.

    k / v: whole contiguous [B, h, cap, d] cache buffers (fp32, or uint8 with ``codes = (k_record, v_record, rejected)``),
    cap >= kv_max.  mask: None or fp32 [B, 1, 1, W >= kv_max] with a dense last axis; probs_out: None or fp32
    [B, h, 1, W >= kv_max] likewise: columns [0, length) are read / written.  grad_table: None or ``kv_max + 1`` device
    floats, entry n the probabilities quantizer's grad factor at length n (util_layernorm.decode_grad_table).  out: the
    [B, 1, h * d] tensor to write, or None for a new one.  A length outside [1, kv_max] gives NaN in every word of out.
    Returns out, or None when the library does not take the layout (nothing was launched)."""
    return _decode_attention("decode_attention_at", q, k, v, mask, probs_quant, ctx_quant, codes=codes,
                             at=(kv_len, kv_len_add, kv_max, grad_table), out=out, probs_out=probs_out)


def decode_attention_shared(q, k, v, mask, probs_quant, ctx_quant, group, codes=None, want_probs=False):
    """decode_attention_fake_quant / decode_attention_codes for query rows that share their keys and values
    (osq_decode_attention_shared / osq_decode_attention_shared_codes, csrc/decode_attention.hip): beam search's
    cross-attention, one copy of K / V per batch row.

    q: dense [B * group, h, 1, d] fp32; query row ``b * group + g`` attends to row b of k / v ([B, h, S, d], fp32, or uint8
    with ``codes = (k_record, v_record, rejected)``; dense or ``[:, :, :S]`` views of [B, h, cap, d] buffers) and of mask
    (None or a dense additive [B, 1, 1, S]).  One workgroup serves up to 8 query rows from one pass over K and V.  The
    outputs are word-equal to decode_attention_fake_quant (decode_attention_codes) on k / v / mask repeated ``group`` times
    along the batch.  Returns the [B * group, 1, h * d] output -- with ``want_probs`` the pair (output, probabilities
    [B * group, h, 1, S]) -- or None where the launch refuses (group above 64, S above 1024, a head_dim or layout the
    library does not take; nothing was launched)."""
    return _decode_attention("decode_attention_shared", q, k, v, mask, probs_quant, ctx_quant, group=group, codes=codes,
                             want_probs=want_probs)


def dequantize_kv_codes(codes, record, out=None):
    """The fp32 buffer of a coded cache buffer: ``codes`` a contiguous uint8 [B, h, cap, d] tensor, ``record`` its
    (scale_eff, zp_eff, quant_min); the result has the same geometry and, position by position, the words the fp32 cache
    holds (osq_dequantize_codes with one channel, reading the record)."""
    scale_eff, zp_eff, quant_min = record
    return dequantize_codes(Codes(codes, scale_eff, zp_eff, int(quant_min), int(quant_min) + 255, 8, tuple(codes.shape), -1), out)


def beam_select(logits, running_scores, keep, seq=None, cur=0, ngram=0, ban_ids=None):
    """The continuations of one beam-search step (osq_beam_select, csrc/beam_select.hip): per batch row the first ``keep`` of
    ``log_softmax(logits)`` with the banned tokens at -inf plus the running beam scores, over all beams -- what
    ``torch.topk((procs(seq, log_softmax(logits)).view(bsz, nb, vocab) + running_scores[:, :, None]).view(bsz, -1), keep)``
    returns for the no-repeat-ngram and min-length processors, under a strict order: larger value first, equal values by
    smaller index, NaN first.

    logits: fp32 [bsz * nb, vocab] with a dense last axis and any row stride (a ``[:, -1, :]`` view is taken as it lies).
    running_scores: fp32 [bsz, nb].  seq: int64 [bsz * nb, >= cur] token history with a dense last axis, needed when
    ``ngram > 0``; ``cur`` its current length.  ban_ids: None or up to 16 int64 ids on the device, banned in every row.
    Returns (top_lp [bsz, keep] fp32, top_idx [bsz, keep] int64, the flat index beam * vocab + token).  Three launches on the
    current stream, no synchronisation; a shape the library does not take raises."""
    return _beam_select("beam_select", logits, running_scores, keep, seq, cur, ngram, ban_ids)


def _beam_select(what, logits, running_scores, keep, seq, cur, ngram, ban_ids, at=None, outs=(None, None, None)):
    """The one body of beam_select and beam_select_at (``what``, in front of every message).  ``at``: None -- ``cur`` is the
    host's position and running_scores is made contiguous -- or (cur_add, cur_max, ban_below) with ``cur`` the device word
    and a running_scores that must be contiguous already.  ``outs``: (top_lp, top_idx, workspace), None for a new one."""
    lib = _hip.load()
    _hip.require_device(logits, running_scores, seq, ban_ids, None if at is None else cur, *outs)
    _check_f32(logits, running_scores)
    if running_scores.dim() != 2 or logits.dim() != 2 or (at is not None and not running_scores.is_contiguous()):
        raise ValueError(f"{what}: logits must be [bsz * nb, vocab] and running_scores "
                         + ("[bsz, nb]" if at is None else "a contiguous [bsz, nb]"))
    if at is not None and (cur.dtype != torch.int32 or cur.numel() != 1 or cur.device != logits.device):
        raise TypeError(f"{what}: cur must be one int32 on the device of logits")
    bsz, nb = running_scores.shape
    rows, vocab = logits.shape
    if rows != bsz * nb or (vocab > 1 and logits.stride(1) != 1) or (rows > 1 and logits.stride(0) < vocab):
        raise ValueError(f"{what}: logits must hold bsz * nb rows with a dense last axis")
    running_scores = running_scores.contiguous()                 # with ``at`` it is: nothing is copied
    cur_add, cur_max, ban_below = (0, cur, 0) if at is None else (int(at[0]), int(at[1]), int(at[2]))
    seq_stride = 0
    if seq is not None:
        if (seq.dtype != torch.int64 or seq.dim() != 2 or seq.shape[0] != rows or seq.shape[1] < cur_max
                or (seq.shape[1] > 1 and seq.stride(1) != 1)):
            raise ValueError(f"{what}: seq must be int64 [bsz * nb, >= {'cur' if at is None else 'cur_max'}] with a dense last axis")
        seq_stride = seq.stride(0) if rows > 1 else seq.shape[1]
    elif ngram > 0:
        raise ValueError(f"{what}: ngram > 0 needs seq")
    n_ban = 0
    if ban_ids is not None:
        if ban_ids.dtype != torch.int64 or ban_ids.dim() != 1 or not ban_ids.is_contiguous():
            raise ValueError(f"{what}: ban_ids must be a contiguous 1-d int64 tensor")
        n_ban = ban_ids.numel()
    keep = int(keep)
    device = logits.device
    top_lp, top_idx, workspace = outs
    for t, dtype, name in ((top_lp, torch.float32, "top_lp"), (top_idx, torch.int64, "top_idx")):
        if t is not None and (t.dtype != dtype or tuple(t.shape) != (bsz, keep) or not t.is_contiguous() or t.device != device):
            raise ValueError(f"{what}: {name} must be a contiguous {dtype} [bsz, keep] tensor on the device of logits")
    if top_lp is None:
        top_lp = torch.empty((bsz, keep), dtype=torch.float32, device=device)
    if top_idx is None:
        top_idx = torch.empty((bsz, keep), dtype=torch.int64, device=device)
    nbytes = int(lib.osq_beam_select_workspace_bytes(bsz, nb, vocab, keep))
    if workspace is None:
        workspace = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=device)
    elif (workspace.dtype != torch.uint8 or not workspace.is_contiguous() or workspace.numel() < nbytes
            or workspace.device != device):
        raise ValueError(f"{what}: workspace must be a contiguous uint8 tensor of at least {nbytes} bytes")
    operands = (logits.data_ptr(), logits.stride(0) if rows > 1 else vocab, running_scores.data_ptr(), _hip.ptr(seq), seq_stride)
    results = (bsz, nb, vocab, keep, top_lp.data_ptr(), top_idx.data_ptr(), workspace.data_ptr())
    if at is None:
        rc = lib.osq_beam_select(*operands, int(cur), int(ngram), _hip.ptr(ban_ids), n_ban, *results, nbytes,
                                 _hip.raw_stream(device))
    else:
        rc = lib.osq_beam_select_at(*operands, cur.data_ptr(), cur_add, cur_max, int(ngram), _hip.ptr(ban_ids), n_ban, ban_below,
                                    *results, workspace.numel(), _hip.raw_stream(device))
    _hip.check(rc, what)
    return top_lp, top_idx


def beam_select_workspace_bytes(bsz, nb, vocab, keep):
    """Bytes of workspace a beam_select / beam_select_at call of this geometry needs (at least 8, for a tensor to exist)."""
    return max(int(_hip.load().osq_beam_select_workspace_bytes(int(bsz), int(nb), int(vocab), int(keep))), 8)


def beam_select_at(logits, running_scores, keep, cur, cur_add, cur_max, seq=None, ngram=0, ban_ids=None, ban_below=0,
                   top_lp=None, top_idx=None, workspace=None):
    """beam_select with the position read by the launch (osq_beam_select_at): ``cur`` is one int32 on the device and the call
    selects at position ``*cur + cur_add``, so a captured graph of the call serves every step.  ``cur_max`` is the largest
    position the call may meet: with ``ngram > 0``, seq rows hold at least that many tokens.  ``ban_ids`` apply while the
    position is below ``ban_below`` (the min-length rule).  For a position in [0, cur_max] the result is word-equal to
    ``beam_select`` at that position; outside it every word of top_lp is NaN and every top_idx 0.

    running_scores must be contiguous (nothing is copied here).  top_lp / top_idx: the contiguous fp32 / int64 [bsz, keep]
    tensors to write, workspace: a contiguous uint8 tensor of at least ``beam_select_workspace_bytes`` bytes -- a captured
    step names static buffers; None: new ones.  Returns (top_lp, top_idx)."""
    return _beam_select("beam_select_at", logits, running_scores, keep, seq, cur, ngram, ban_ids,
                        at=(cur_add, cur_max, ban_below), outs=(top_lp, top_idx, workspace))


class BeamBuffers:
    """One set of beam-search state on a device, as osq_beam_advance reads and writes it: ``running`` /  ``finished``
    [bsz, nb, max_length] int64, ``running_scores`` / ``scores`` [bsz, nb] fp32, ``finished_len`` [bsz, nb] int64, ``done``
    [bsz, nb] bool, ``improvable`` [bsz, 1] bool; and what a step writes beside the state: ``beam_idx`` / ``next_tokens``
    [bsz * nb] int64, the ``go_on`` int32 word and the call's ``workspace``."""
    STATE = ("running", "running_scores", "finished", "scores", "finished_len", "done", "improvable")
    _DTYPES = (torch.int64, torch.float32, torch.int64, torch.float32, torch.int64, torch.bool, torch.bool)

    def __init__(self, bsz, nb, max_length, device):
        shapes = ((bsz, nb, max_length), (bsz, nb), (bsz, nb, max_length), (bsz, nb), (bsz, nb), (bsz, nb), (bsz, 1))
        for name, shape, dtype in zip(self.STATE, shapes, self._DTYPES):
            setattr(self, name, torch.zeros(shape, dtype=dtype, device=device))
        self.beam_idx = torch.zeros(bsz * nb, dtype=torch.int64, device=device)
        self.next_tokens = torch.zeros(bsz * nb, dtype=torch.int64, device=device)
        self.go_on = torch.zeros(1, dtype=torch.int32, device=device)
        self.workspace = torch.zeros(4 * bsz, dtype=torch.uint8, device=device)


def _beam_advance_operands(what, top_lp, top_idx, state, out, eos_ids, early_stopping):
    """The checks beam_advance and beam_advance_at share; (tensors, outs, bsz, nb, keep, max_length, n_eos, mode, device)."""
    names = BeamBuffers.STATE
    tensors = [getattr(state, n) for n in names]
    outs = [getattr(out, n) for n in names]
    extra = [out.beam_idx, out.next_tokens, out.go_on, out.workspace]
    _hip.require_device(top_lp, top_idx, eos_ids, *tensors, *outs, *extra)
    if top_lp.dim() != 2 or top_lp.shape != top_idx.shape or top_lp.dtype != torch.float32 or top_idx.dtype != torch.int64:
        raise ValueError(f"{what}: top_lp must be fp32 [bsz, keep] and top_idx int64 [bsz, keep]")
    bsz, keep = top_lp.shape
    if state.running.dim() != 3 or state.running.shape[0] != bsz:
        raise ValueError(f"{what}: running must be [bsz, nb, max_length]")
    _, nb, max_length = state.running.shape
    shapes = ((bsz, nb, max_length), (bsz, nb), (bsz, nb, max_length), (bsz, nb), (bsz, nb), (bsz, nb), (bsz,))
    for group, which in ((tensors, "state"), (outs, "out")):
        for name, t, shape, dtype in zip(names, group, shapes, BeamBuffers._DTYPES):
            ok_dtype = t.dtype == dtype or (dtype == torch.bool and t.dtype == torch.uint8)
            if not ok_dtype or t.numel() != math.prod(shape) or tuple(t.shape[:len(shape)]) != shape or not t.is_contiguous():
                raise ValueError(f"{what}: {which}.{name} must be a contiguous {dtype} tensor of shape {shape}")
    for name, t, n, dtype in (("beam_idx", out.beam_idx, bsz * nb, torch.int64), ("next_tokens", out.next_tokens, bsz * nb, torch.int64),
                              ("go_on", out.go_on, 1, torch.int32)):
        if t.dtype != dtype or t.numel() != n or not t.is_contiguous():
            raise ValueError(f"{what}: out.{name} must be a contiguous {dtype} tensor of {n} elements")
    if out.workspace.dtype != torch.uint8 or not out.workspace.is_contiguous():
        raise ValueError(f"{what}: out.workspace must be a contiguous uint8 tensor")
    device = top_lp.device
    every = [top_lp, top_idx, *tensors, *outs, *extra] + ([] if eos_ids is None else [eos_ids])
    if any(t.device != device for t in every):
        raise ValueError(f"{what}: all tensors must be on one device")
    reads = [top_lp, top_idx, *tensors] + ([] if eos_ids is None else [eos_ids])
    writes = [*outs, *extra]
    spans = lambda ts: [(t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()) for t in ts if t.numel()]  # noqa: E731
    w = spans(writes)
    for i, (lo, hi) in enumerate(w):
        if any(lo < h and l < hi for l, h in spans(reads) + w[:i]):
            raise ValueError(f"{what}: an output shares memory with an input or another output (the gathers read the "
                             "old state: state and out are two sets)")
    n_eos = 0
    if eos_ids is not None:
        if eos_ids.dtype != torch.int64 or eos_ids.dim() != 1 or not eos_ids.is_contiguous():
            raise ValueError(f"{what}: eos_ids must be a contiguous 1-d int64 tensor")
        n_eos = eos_ids.numel()
    if early_stopping not in (False, True, "never"):
        raise ValueError(f'{what}: early_stopping is False, True or "never"')
    mode = 2 if early_stopping == "never" else int(bool(early_stopping))
    return tensors, outs, bsz, nb, keep, max_length, n_eos, mode, device


def beam_advance(top_lp, top_idx, state, out, cur, vocab, eos_ids=None, early_stopping=False, len_div=1.0, best_div=1.0,
                 reciprocal=True):
    """The bookkeeping of one beam-search step after the selection (osq_beam_advance, csrc/beam_advance.hip): from ``top_lp``
    / ``top_idx`` [bsz, keep] and the ``state`` at length ``cur`` (prompt of one token) into ``out`` -- the new state,
    ``out.beam_idx`` (the cache rows of the kept beams), ``out.next_tokens`` (= out.running[:, :, cur]) and the ``out.go_on``
    word -- what generation._advance_beams_torch computes, word for word, under a strict order of ties.

    ``state`` / ``out``: two BeamBuffers (or objects with their attributes) of one geometry that share no memory: the gathers
    read the old state.  eos_ids: None or up to 16 int64 ids on the device.  early_stopping: False, True or "never".
    len_div / best_div: ``(cur + 1 - 1) ** length_penalty`` and ``best_len ** length_penalty`` as Python computes them.
    reciprocal: divide as torch's GPU kernel does by a host scalar, v * float32(1 / div) with the reciprocal taken in
    double; False: the correctly rounded v / float32(div), as torch's CPU kernel does.
    Two launches on the current stream, no synchronisation, nothing allocated; returns ``out``."""
    lib = _hip.load()
    tensors, outs, bsz, nb, keep, max_length, n_eos, mode, device = _beam_advance_operands(
        "beam_advance", top_lp, top_idx, state, out, eos_ids, early_stopping)
    top_lp, top_idx = top_lp.contiguous(), top_idx.contiguous()
    rc = lib.osq_beam_advance(top_lp.data_ptr(), top_idx.data_ptr(), *(t.data_ptr() for t in tensors),
                              _hip.ptr(eos_ids) if n_eos else None, n_eos, bsz, nb, keep, int(vocab), max_length, int(cur), mode,
                              float(len_div), float(best_div), int(bool(reciprocal)), *(t.data_ptr() for t in outs),
                              out.beam_idx.data_ptr(), out.next_tokens.data_ptr(), out.go_on.data_ptr(),
                              out.workspace.data_ptr(), out.workspace.numel(), _hip.raw_stream(device))
    _hip.check(rc, "beam_advance")
    return out


def beam_div_tables(max_length, length_penalty, early_stopping, reciprocal, device, prompt=1):
    """The two factor tables of beam_advance_at for a search up to ``max_length``: (len_table, best_table), fp32
    [max_length] on ``device``.  Entry ``cur`` is the word beam_advance derives at that length from the Python expressions of
    the search (generation._beam_search_advanced),

        len_div  = (cur + 1 - prompt) ** length_penalty
        best_div = best_len ** length_penalty,   best_len = max_length - prompt with early_stopping == "never" and a positive
                                                 penalty, else cur + 1 - prompt

    as ``float32(1.0 / div)`` with ``reciprocal`` (the reciprocal in double, rounded once) and ``float32(div)`` without.
    Entries below ``prompt`` belong to no step (a length of zero tokens has no divisor): they hold NaN."""
    max_length, prompt = int(max_length), int(prompt)
    nan = float("nan")
    tables = ([], [])
    for cur in range(max_length):
        if cur < prompt:
            divs = (nan, nan)
        else:
            best_len = (max_length - prompt) if (early_stopping == "never" and length_penalty > 0.0) else (cur + 1 - prompt)
            divs = ((cur + 1 - prompt) ** length_penalty, best_len ** length_penalty)
        for table, div in zip(tables, divs):
            table.append(1.0 / div if reciprocal and div == div else div)
    # float64 -> float32 rounds to nearest even, as the C cast of the static entry point does
    return tuple(torch.tensor(t, dtype=torch.float64).to(torch.float32).to(device) for t in tables)


def beam_advance_at(top_lp, top_idx, state, out, cur, cur_add, vocab, len_table, best_table, eos_ids=None,
                    early_stopping=False, reciprocal=True):
    """beam_advance with the position read by the launch (osq_beam_advance_at): ``cur`` is one int32 on the device and the
    step is taken at length ``*cur + cur_add``, so a captured graph of the call serves every step.  len_table / best_table:
    ``beam_div_tables`` of the search, built with the same ``reciprocal``.  For a length in [1, max_length) everything written
    is word-equal to ``beam_advance`` at that length; outside it ``out.go_on`` receives -1 and nothing else is written.
    top_lp / top_idx must be contiguous (nothing is copied here).  Returns ``out``."""
    lib = _hip.load()
    tensors, outs, bsz, nb, keep, max_length, n_eos, mode, device = _beam_advance_operands(
        "beam_advance_at", top_lp, top_idx, state, out, eos_ids, early_stopping)
    _hip.require_device(cur, len_table, best_table)
    if not (top_lp.is_contiguous() and top_idx.is_contiguous()):
        raise ValueError("beam_advance_at: top_lp and top_idx must be contiguous")
    if cur.dtype != torch.int32 or cur.numel() != 1 or cur.device != device:
        raise TypeError("beam_advance_at: cur must be one int32 on the device of top_lp")
    for name, t in (("len_table", len_table), ("best_table", best_table)):
        if t.dtype != torch.float32 or t.dim() != 1 or t.numel() < max_length or not t.is_contiguous() or t.device != device:
            raise ValueError(f"beam_advance_at: {name} must hold max_length contiguous floats on the device of top_lp")
    rc = lib.osq_beam_advance_at(top_lp.data_ptr(), top_idx.data_ptr(), *(t.data_ptr() for t in tensors),
                                 _hip.ptr(eos_ids) if n_eos else None, n_eos, bsz, nb, keep, int(vocab), max_length,
                                 cur.data_ptr(), int(cur_add), mode, len_table.data_ptr(), best_table.data_ptr(),
                                 int(bool(reciprocal)), *(t.data_ptr() for t in outs), out.beam_idx.data_ptr(),
                                 out.next_tokens.data_ptr(), out.go_on.data_ptr(), out.workspace.data_ptr(),
                                 out.workspace.numel(), _hip.raw_stream(device))
    _hip.check(rc, "beam_advance_at")
    return out


class GreedyBuffers:
    """The state of a greedy search on a device, as osq_greedy_advance reads and writes it: ``seq`` [bsz, max_length] int64
    (the token history, filled up to the current length), ``unfinished`` [bsz] uint8, and what a step writes beside them:
    ``next_tokens`` [bsz] int64 (= seq[:, cur]), the ``go_on`` int32 word and the call's ``workspace`` (sized on first use:
    it depends on the vocabulary -- or here, given ``vocab``)."""

    def __init__(self, bsz, max_length, device, vocab=None):
        self.seq = torch.zeros((bsz, max_length), dtype=torch.int64, device=device)
        self.unfinished = torch.ones(bsz, dtype=torch.uint8, device=device)
        self.next_tokens = torch.zeros(bsz, dtype=torch.int64, device=device)
        self.go_on = torch.zeros(1, dtype=torch.int32, device=device)
        self.workspace = None
        if vocab is not None:
            self.room(vocab)

    def room(self, vocab):
        """The workspace for rows of ``vocab`` logits (allocated once: a captured step names it)."""
        nbytes = max(int(_hip.load().osq_greedy_advance_workspace_bytes(self.seq.shape[0], int(vocab))), 8)
        if self.workspace is None or self.workspace.numel() < nbytes:
            self.workspace = torch.empty(nbytes, dtype=torch.uint8, device=self.seq.device)
        return self.workspace


def _advance_operands(what, logits, buffers, ban_ids, eos_ids):
    """The checks every advance call shares, and its arguments but the position, the settings and the draw: (head, (n_ban,
    n_eos), state, outputs, stream) -- logits and seq with their strides; unfinished and the shape; next_tokens, go_on and
    the workspace."""
    seq, unfinished, next_tokens, go_on = buffers.seq, buffers.unfinished, buffers.next_tokens, buffers.go_on
    _hip.require_device(logits, seq, unfinished, next_tokens, go_on, ban_ids, eos_ids)
    _check_f32(logits)
    if logits.dim() != 2 or seq.dim() != 2 or seq.dtype != torch.int64:
        raise ValueError(f"{what}: logits must be fp32 [bsz, vocab] and buffers.seq int64 [bsz, max_length]")
    bsz, vocab = logits.shape
    max_length = seq.shape[1]
    if (vocab > 1 and logits.stride(1) != 1) or (bsz > 1 and logits.stride(0) < vocab):
        raise ValueError(f"{what}: logits must have a dense last axis")
    if seq.shape[0] != bsz or (max_length > 1 and seq.stride(1) != 1) or (bsz > 1 and seq.stride(0) < max_length):
        raise ValueError(f"{what}: buffers.seq must hold bsz rows with a dense last axis")
    for name, t, dtype in (("unfinished", unfinished, torch.uint8), ("next_tokens", next_tokens, torch.int64)):
        if t.dtype != dtype or tuple(t.shape) != (bsz,) or not t.is_contiguous():
            raise ValueError(f"{what}: buffers.{name} must be a contiguous {dtype} [bsz] tensor")
    if go_on.dtype != torch.int32 or go_on.numel() != 1:
        raise ValueError(f"{what}: buffers.go_on must be one int32")
    counts = []
    for name, ids in (("ban_ids", ban_ids), ("eos_ids", eos_ids)):
        if ids is not None and (ids.dtype != torch.int64 or ids.dim() != 1 or not ids.is_contiguous()):
            raise ValueError(f"{what}: {name} must be a contiguous 1-d int64 tensor")
        counts.append(0 if ids is None else ids.numel())
    device = logits.device
    every = [seq, unfinished, next_tokens, go_on] + [t for t in (ban_ids, eos_ids) if t is not None]
    if any(t.device != device for t in every):
        raise ValueError(f"{what}: all tensors must be on one device")
    ws = buffers.room(vocab)
    head = (logits.data_ptr(), logits.stride(0) if bsz > 1 else vocab, seq.data_ptr(), seq.stride(0) if bsz > 1 else max_length)
    state = (unfinished.data_ptr(), bsz, vocab, max_length)
    return head, counts, state, (next_tokens.data_ptr(), go_on.data_ptr(), ws.data_ptr(), ws.numel()), _hip.raw_stream(device)


def _advance(family, at, logits, buffers, cur, cur_add, ngram, ban_ids, ban_below, forced, eos_ids, pad, draw=None, group=1,
             logprobs=None):
    """The call path of greedy_advance, sample_advance, sample_nucleus and (``at``) their _at forms: the checks, the arguments
    in the C ABI's order, the call, and None for a call the library does not take.  ``cur`` is the position or, ``at``, the
    device word, to which ``cur_add`` and ``ban_below`` belong; ``forced`` is the static form's token or the _at form's
    (forced_bos, forced_eos); ``draw`` is a sampling family's (seed, temperature, top_k, top_p, uniforms), of which
    sample_nucleus passes no top_k on.  ``group`` / ``logprobs`` (the sampling families): anything but (1, None) goes to the
    family's _group entry point, which takes them after the draw."""
    what = family + ("_at" if at else "")
    grouped = ()
    if int(group) != 1 or logprobs is not None:
        if draw is None:
            raise ValueError(f"{what}: group and logprobs belong to the sampling families")
        bsz, max_length = logits.shape[0], buffers.seq.shape[1]
        if int(group) < 1 or bsz % int(group):
            raise ValueError(f"{what}: group must be at least 1 and divide bsz")
        if logprobs is not None:
            _hip.require_device(logprobs)
            if (logprobs.dtype != torch.float32 or tuple(logprobs.shape) != (bsz, max_length) or logprobs.device != logits.device
                    or (max_length > 1 and logprobs.stride(1) != 1) or (bsz > 1 and logprobs.stride(0) < max_length)):
                raise ValueError(f"{what}: logprobs must be a float32 [bsz, max_length] tensor with a dense last axis on the "
                                 "device of logits")
        grouped = (int(group), _hip.ptr(logprobs), 0 if logprobs is None else (logprobs.stride(0) if bsz > 1 else max_length))
    lib = _hip.load()
    if draw is not None:
        seed, temperature, top_k, top_p, uniforms = draw
        top_k = int(top_k)
        if not 0 <= top_k <= 64:                     # the workspace's size follows it: refused before one is sized
            raise ValueError(f"{what}: top_k must lie in [0, 64]")
        if not isinstance(buffers, SampleBuffers):
            raise TypeError(f"{what}: buffers must be an ops.SampleBuffers")
        buffers.top_k = max(buffers.top_k, top_k)
        buffers.nucleus = buffers.nucleus or family == "sample_nucleus"
    head, (n_ban, n_eos), state, outputs, stream = _advance_operands(what, logits, buffers, ban_ids, eos_ids)
    if draw is not None:
        if uniforms is not None:
            _hip.require_device(uniforms)
            if (uniforms.dtype != torch.float32 or tuple(uniforms.shape) != (logits.shape[0],) or not uniforms.is_contiguous()
                    or uniforms.device != logits.device):
                raise ValueError(f"{what}: uniforms must be a contiguous float32 [bsz] tensor on the device of logits")
        draw = (int(seed) & 0xFFFFFFFFFFFFFFFF, float(temperature), *((top_k,) if family == "sample_advance" else ()),
                float(top_p), _hip.ptr(uniforms))
    ban, eos = (_hip.ptr(ban_ids) if n_ban else None, n_ban), (_hip.ptr(eos_ids) if n_eos else None, n_eos)
    token = lambda t: -1 if t is None else int(t)    # noqa: E731
    if at:
        _hip.require_device(cur)
        if cur.dtype != torch.int32 or cur.numel() != 1 or cur.device != logits.device:
            raise TypeError(f"{what}: cur must be one int32 on the device of logits")
        position = (cur.data_ptr(), int(cur_add))
        settings = (int(ngram), *ban, int(ban_below), token(forced[0]), token(forced[1]), *eos, int(pad))
    else:
        position = (int(cur),)
        settings = (int(ngram), *ban, token(forced), *eos, int(pad))
    entry = "osq_" + (family + "_group" + ("_at" if at else "") if grouped else what)
    rc = getattr(lib, entry)(*head, *position, *settings, *state, *outputs, *(draw or ()), *grouped, stream)
    if rc == _hip.ERR_UNSUPPORTED:
        return None
    _hip.check(rc, what)
    return buffers


def greedy_advance(logits, buffers, cur, ngram=0, ban_ids=None, forced=None, eos_ids=None, pad=0):
    """One greedy decoding step after the model (osq_greedy_advance, csrc/greedy_advance.hip): from the fp32 ``logits``
    [bsz, vocab] (a dense last axis, any row stride) and ``buffers`` (a GreedyBuffers) at history length ``cur`` -- the banned
    tokens (``ban_ids``: None or up to 16 int64 ids on the device; ``ngram``: the no-repeat-ngram size), the arg-max of every
    row in torch.argmax's order (or ``forced``, a token id, whatever the logits hold), with ``eos_ids`` (None or up to 16 int64
    ids on the device) the ``pad`` of finished rows and the update of ``buffers.unfinished`` -- into ``buffers.seq[:, cur]``,
    ``buffers.next_tokens`` and the ``buffers.go_on`` word: what generation._greedy computes, token for token.
    Three launches on the current stream, no synchronisation; returns ``buffers``, or None when the library does not take
    the call (the caller takes its other path)."""
    return _advance("greedy_advance", False, logits, buffers, cur, 0, ngram, ban_ids, 0, forced, eos_ids, pad)


def greedy_advance_at(logits, buffers, cur, cur_add=0, ngram=0, ban_ids=None, ban_below=0, forced_bos=None, forced_eos=None,
                      eos_ids=None, pad=0):
    """greedy_advance with the position read by the launches (osq_greedy_advance_at): ``cur`` is one int32 on the device and
    the step is taken at length ``*cur + cur_add``, so a captured graph of the call serves every step.  ``ban_ids`` apply while
    the length is below ``ban_below`` (the min-length rule), ``forced_bos`` is the token at length 1 and ``forced_eos`` the
    token at length max_length - 1 (it wins where both fire).  For a length in [1, max_length) everything written is word-equal
    to ``greedy_advance`` at that length; outside it ``buffers.go_on`` receives -1 and nothing else is written."""
    return _advance("greedy_advance", True, logits, buffers, cur, cur_add, ngram, ban_ids, ban_below, (forced_bos, forced_eos),
                    eos_ids, pad)


class SampleBuffers(GreedyBuffers):
    """GreedyBuffers for osq_sample_advance: the same state, a workspace sized for (vocab, top_k) -- and, with ``nucleus``,
    for osq_sample_nucleus (osq_sample_nucleus_workspace_bytes) as well, so that one set of buffers serves both calls.
    ``logprobs=True``: a zero-filled fp32 ``logprobs`` [bsz, max_length] for the steps' ``logprobs=`` (else None)."""

    def __init__(self, bsz, max_length, device, vocab=None, top_k=0, nucleus=False, logprobs=False):
        self.top_k = int(top_k)
        self.nucleus = bool(nucleus)
        super().__init__(bsz, max_length, device, vocab)
        self.logprobs = torch.zeros((bsz, max_length), dtype=torch.float32, device=device) if logprobs else None

    def room(self, vocab):
        lib = _hip.load()
        nbytes = max(int(lib.osq_sample_advance_workspace_bytes(self.seq.shape[0], int(vocab), self.top_k)), 8)
        if self.nucleus:
            nbytes = max(nbytes, int(lib.osq_sample_nucleus_workspace_bytes(self.seq.shape[0], int(vocab))))
        if self.workspace is None or self.workspace.numel() < nbytes:
            self.workspace = torch.empty(nbytes, dtype=torch.uint8, device=self.seq.device)
        return self.workspace


def sample_advance(logits, buffers, cur, seed, temperature=1.0, top_k=0, top_p=1.0, ngram=0, ban_ids=None, forced=None,
                   eos_ids=None, pad=0, uniforms=None, *, group=1, logprobs=None):
    """One sampling step after the model (osq_sample_advance, csrc/sample_advance.hip): ``greedy_advance`` with a seeded
    draw in the place of the arg-max.  From the fp32 ``logits`` [bsz, vocab] and ``buffers`` (a SampleBuffers) at history
    length ``cur``: the banned tokens, z = logits / ``temperature``, the ``top_k`` largest (0: all; up to 64; equal values by
    smaller token, exactly top_k of them), the ``top_p`` cut over their renormalised weights (with top_k >= 1), and the token
    the row's uniform u selects -- Philox4x32-10 keyed by ``seed`` at counter (row, cur), or ``uniforms`` [bsz] fp32 in [0, 1)
    on the device -- then greedy_advance's pad / eos arithmetic, ``buffers.seq[:, cur]``, ``buffers.next_tokens`` and
    ``buffers.go_on``.  Three launches on the current stream, no synchronisation; returns ``buffers``, or None when the
    library does not take the call (top_k == 0 with top_p < 1: the caller takes its other path -- ``sample_nucleus`` below,
    where it asked for that kernel, else its torch lines).

    ``group=G`` (osq_sample_advance_group; here and in the three calls below): row r is sequence r % G of input r // G and
    draws at counter (r // G, cur, r % G), so that a sequence's draws do not depend on the launch shape.  ``logprobs``: a
    float32 [bsz, max_length] tensor whose word [r, cur] receives the log of the probability with which the rule drew the
    token (0 on a forced step and for a finished row, -inf for a row without a survivor); no other word of it is written."""
    return _advance("sample_advance", False, logits, buffers, cur, 0, ngram, ban_ids, 0, forced, eos_ids, pad,
                    (seed, temperature, top_k, top_p, uniforms), group, logprobs)


def sample_advance_at(logits, buffers, cur, seed, cur_add=0, temperature=1.0, top_k=0, top_p=1.0, ngram=0, ban_ids=None,
                      ban_below=0, forced_bos=None, forced_eos=None, eos_ids=None, pad=0, uniforms=None, *, group=1,
                      logprobs=None):
    """sample_advance with the position read by the launches (osq_sample_advance_at): ``cur`` is one int32 on the device and
    the step is taken at length ``*cur + cur_add``; ``ban_below``, ``forced_bos`` and ``forced_eos`` as in greedy_advance_at.
    The seed is an argument and the generator has no state, so a captured graph of the call serves every step.  For a length
    in [1, max_length) everything written is word-equal to ``sample_advance`` at that length; outside it ``buffers.go_on``
    receives -1 and nothing else is written."""
    return _advance("sample_advance", True, logits, buffers, cur, cur_add, ngram, ban_ids, ban_below, (forced_bos, forced_eos),
                    eos_ids, pad, (seed, temperature, top_k, top_p, uniforms), group, logprobs)


def sample_nucleus(logits, buffers, cur, seed, temperature=1.0, top_p=1.0, ngram=0, ban_ids=None, forced=None, eos_ids=None,
                   pad=0, uniforms=None, *, group=1, logprobs=None):
    """One sampling step after the model from a nucleus over the whole vocabulary (osq_sample_nucleus,
    csrc/sample_nucleus.hip): ``sample_advance`` for top_k == 0 and any ``top_p`` in (0, 1].  Every token left is ranked
    (larger z first, equal z by smaller token), rank i stays iff the weights ranked above it sum below top_p of the total,
    and the row's uniform selects among the kept ranks -- found by two bisections over a fixed-order fp32 sum held in
    registers, without a sort (the rule: include/osq_hip.h).  Bans, ``forced``, pad / eos, ``buffers.seq[:, cur]``,
    ``buffers.next_tokens``, ``buffers.go_on`` and the uniforms are sample_advance's.  Two launches on the current stream, no
    synchronisation; returns ``buffers``, or None when the library does not take the call (a vocabulary above 51200)."""
    return _advance("sample_nucleus", False, logits, buffers, cur, 0, ngram, ban_ids, 0, forced, eos_ids, pad,
                    (seed, temperature, 0, top_p, uniforms), group, logprobs)


def sample_nucleus_at(logits, buffers, cur, seed, cur_add=0, temperature=1.0, top_p=1.0, ngram=0, ban_ids=None, ban_below=0,
                      forced_bos=None, forced_eos=None, eos_ids=None, pad=0, uniforms=None, *, group=1, logprobs=None):
    """sample_nucleus with the position read by the launches (osq_sample_nucleus_at): ``cur`` is one int32 on the device and
    the step is taken at length ``*cur + cur_add``; everything else as sample_advance_at.  For a length in [1, max_length)
    everything written is word-equal to ``sample_nucleus`` at that length; outside it ``buffers.go_on`` receives -1 and
    nothing else is written."""
    return _advance("sample_nucleus", True, logits, buffers, cur, cur_add, ngram, ban_ids, ban_below, (forced_bos, forced_eos),
                    eos_ids, pad, (seed, temperature, 0, top_p, uniforms), group, logprobs)


def sample_uniforms(seed, bsz, cur, device, group=1):
    """The uniforms sample_advance draws at history length ``cur`` with ``seed`` for ``bsz`` inputs of ``group`` sequences each
    (osq_sample_uniforms_group): fp32 [bsz * group] on ``device``, word-equal to model.sampling.uniforms on the host."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"outlier_suppression_amd: tensors must live on a HIP device (got device={device}); there is no CPU path.")
    if int(group) < 1:
        raise ValueError("sample_uniforms: group must be at least 1")
    out = torch.empty(int(bsz) * int(group), dtype=torch.float32, device=device)
    _hip.check(_hip.load().osq_sample_uniforms_group(int(seed) & 0xFFFFFFFFFFFFFFFF, out.numel(), int(group), int(cur),
                                                     out.data_ptr(), _hip.raw_stream(device)), "sample_uniforms")
    return out


# ---------------------------------------------------------------------------------------
# teacher-forced scoring (csrc/token_logprob.hip)
# ---------------------------------------------------------------------------------------
_token_logprob_ws = {}          # (device, stream) -> [workspace, a capture has named it]
_token_logprob_named = []       # outgrown workspaces that a captured graph names: kept alive for its replays


def token_logprob_fits(rows, vocab):
    """True where one launch indexes ``rows`` rows of ``vocab`` logits (at most 2^31 - 1 (row, 4096-token chunk) pairs)."""
    rows, vocab = int(rows), int(vocab)
    return rows >= 0 and 1 <= vocab <= 2 ** 31 - 4097 and rows * ((vocab + 4095) // 4096) <= 2 ** 31 - 1


def _token_logprob_workspace(device, rows, vocab):
    """The (device, stream) scratch of the scoring launches, grown on demand.  Call once with the shape before capturing:
    a capture allocates nothing then, and the workspace it names outlives a later, larger call."""
    nbytes = max(int(_hip.load().osq_token_logprob_workspace_bytes(rows, vocab)), 8)
    key = (_hip._device_index(device), _hip.raw_stream(device))
    entry = _token_logprob_ws.get(key)
    if entry is None or entry[0].numel() < nbytes:
        if entry is not None and entry[1]:
            _token_logprob_named.append(entry[0])
        entry = [torch.empty(nbytes, dtype=torch.uint8, device=device), False]
        _token_logprob_ws[key] = entry
    if not entry[1] and torch.cuda.is_current_stream_capturing():
        entry[1] = True
    return entry[0]


def _token_logprob_operands(what, logits, labels):
    _hip.require_device(logits, labels)
    _check_f32(logits)
    if logits.dim() != 2 or labels.dim() != 1 or labels.dtype != torch.int64 or labels.shape[0] != logits.shape[0]:
        raise ValueError(f"{what}: logits must be fp32 [rows, vocab] and labels int64 [rows]")
    rows, vocab = logits.shape
    if vocab < 1 or (vocab > 1 and logits.stride(1) != 1) or (rows > 1 and logits.stride(0) < vocab):
        raise ValueError(f"{what}: logits must have a dense last axis of at least one token")
    if labels.device != logits.device or (rows > 1 and labels.stride(0) != 1):
        raise ValueError(f"{what}: labels must be contiguous on the device of logits")
    if not token_logprob_fits(rows, vocab):
        raise ValueError(f"{what}: more (row, 4096-token chunk) pairs than one launch indexes")
    return rows, vocab, logits.stride(0) if rows > 1 else vocab


def _token_logprob_out(what, out, name, shape, dtype, device):
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if out.dtype != dtype or tuple(out.shape) != tuple(shape) or out.device != device or not out.is_contiguous():
        raise ValueError(f"{what}: {name} must be a contiguous {dtype} tensor of shape {tuple(shape)} on the device of logits")
    return out


def _token_logprob(what, logits, labels, ignore_index, out, reduce):
    lib = _hip.load()
    rows, vocab, stride = _token_logprob_operands(what, logits, labels)
    dev, out = logits.device, tuple(out) if out is not None else ()
    out = out + (None,) * ((4 if reduce else 2) - len(out))
    logprob = _token_logprob_out(what, out[1 if reduce else 0], "logprob", (rows,), torch.float32, dev)
    lse = _token_logprob_out(what, out[2 if reduce else 1], "lse", (rows,), torch.float32, dev)
    loss = counts = None
    if reduce:
        loss = _token_logprob_out(what, out[0], "loss", (), torch.float32, dev)
        counts = _token_logprob_out(what, out[3], "counts", (2,), torch.int64, dev)
    ws = _token_logprob_workspace(dev, rows, vocab)
    rc = lib.osq_token_logprob(logits.data_ptr(), stride, labels.data_ptr(), rows, vocab, int(ignore_index), logprob.data_ptr(),
                               lse.data_ptr(), _hip.ptr(loss), _hip.ptr(counts), ws.data_ptr(), _hip.raw_stream(dev))
    _hip.check(rc, what)
    return (loss, logprob, lse, counts) if reduce else (logprob, lse)


def token_logprob(logits, labels, ignore_index=-100, out=None):
    """The log-probability the rows of ``logits`` give their ``labels`` (osq_token_logprob, csrc/token_logprob.hip; the rule:
    include/osq_hip.h, "teacher-forced scoring"): (logprob, lse), fp32 [rows] each -- ``-F.cross_entropy(logits, labels,
    reduction='none', ignore_index=...)`` and ``logsumexp(logits, -1)``, without a tensor of the logits' size.  logits: fp32
    [rows, vocab] with a dense last axis and any row stride; labels: int64 [rows].  A row whose label is ``ignore_index``
    gives 0 (its lse is written all the same); a label outside the vocabulary gives NaN -- nothing asserts on the device.
    ``out=(logprob, lse)``: the tensors to write, so that a captured call allocates nothing (the workspace is kept per device
    and stream).  Two launches on the current stream, no synchronisation."""
    return _token_logprob("token_logprob", logits, labels, ignore_index, out, False)


def lm_loss(logits, labels, ignore_index=-100, out=None):
    """token_logprob and the loss over the rows in one call: (loss, logprob, lse, counts) -- ``loss`` one fp32,
    ``F.cross_entropy(logits, labels, ignore_index=...)`` (NaN where every row is ignored, as torch gives, and NaN where a
    label lies outside the vocabulary), ``counts`` int64 [2]: the rows scored and the rows with such a label.  Reading counts
    is the caller's synchronisation; this call has none.  ``out=(loss, logprob, lse, counts)``.  Three launches."""
    return _token_logprob("lm_loss", logits, labels, ignore_index, out, True)


def token_logprob_backward(logits, labels, lse, row_grad=None, scalar_grad=None, counts=None, ignore_index=-100, out=None):
    """The gradient of token_logprob / lm_loss for the logits from ``lse`` alone (osq_token_logprob_backward):
    ``coef * (exp(logits - lse[:, None]) - onehot(labels))`` per row (a row of at most 4096 tokens renormalised by the
    kernel's own sum of its exponentials, which takes the rounding of lse out), 0 for an ignored row and for a label outside
    the vocabulary.  coef is ``row_grad`` [rows] fp32 -- the upstream gradient of the rows' NEGATIVE log-probabilities -- or,
    without it, ``scalar_grad / counts[0]``: the upstream gradient of the mean loss (one fp32 on the device) over the rows
    lm_loss counted (its ``counts``), divided on the device.  ``out``: the fp32 [rows, vocab] tensor to write (dense last
    axis, any row stride), else a new contiguous one.  One launch, no synchronisation."""
    lib = _hip.load()
    what = "token_logprob_backward"
    rows, vocab, stride = _token_logprob_operands(what, logits, labels)
    dev = logits.device
    _hip.require_device(lse, row_grad, scalar_grad, counts, out)
    _check_f32(lse, row_grad, scalar_grad, out)
    for name, t, n in (("lse", lse, rows), ("row_grad", row_grad, rows), ("scalar_grad", scalar_grad, 1)):
        if t is not None and (t.numel() != n or t.device != dev or not t.is_contiguous()):
            raise ValueError(f"{what}: {name} must be a contiguous fp32 tensor of {n} elements on the device of logits")
    if row_grad is None and (scalar_grad is None or counts is None):
        raise ValueError(f"{what}: give row_grad, or scalar_grad with the counts of lm_loss")
    if counts is not None and (counts.dtype != torch.int64 or counts.numel() != 2 or counts.device != dev
                               or not counts.is_contiguous()):
        raise ValueError(f"{what}: counts must be the int64 [2] tensor of lm_loss")
    if out is None:
        out = torch.empty((rows, vocab), dtype=torch.float32, device=dev)
    elif (tuple(out.shape) != (rows, vocab) or out.device != dev or (vocab > 1 and out.stride(1) != 1)
          or (rows > 1 and out.stride(0) < vocab)):
        raise ValueError(f"{what}: out must be fp32 [rows, vocab] with a dense last axis on the device of logits")
    rc = lib.osq_token_logprob_backward(logits.data_ptr(), stride, labels.data_ptr(), lse.data_ptr(), _hip.ptr(row_grad),
                                        _hip.ptr(scalar_grad), _hip.ptr(counts), rows, vocab, int(ignore_index), out.data_ptr(),
                                        out.stride(0) if rows > 1 else vocab, _hip.raw_stream(dev))
    _hip.check(rc, what)
    return out

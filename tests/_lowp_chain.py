"""Host emulation of the bf16 / fp16 fake-quant chain and its backward (README "Defaults", include/osq_hip.h).

The reference's FixedFakeQuantize per-tensor call runs util_quant.py:12-14 in x's dtype: every op computes in fp32 and
rounds to the dtype (RNE).  Here each op is a NumPy float32 operation (IEEE, true division) followed by an explicit
rounding through torch's CPU conversion, which keeps NaN a NaN.  tests/test_oracle_lowp.py pins this emulation against
the reference's own outputs (tests/golden/lowp.npz), so tests may use it for shapes and seeds beyond the fixture.
16-bit tensors travel as uint16 words (numpy has no bfloat16).
"""
import numpy as np
import torch

DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
_CANON_NAN = {torch.bfloat16: 0x7FC0, torch.float16: 0x7E00}
_EXP_MASK = {torch.bfloat16: 0x7F80, torch.float16: 0x7C00}


def to_f32(words, dtype):
    """uint16 words -> exact float32 values."""
    w = np.ascontiguousarray(words, dtype=np.uint16)
    return torch.from_numpy(w.view(np.int16)).view(dtype).float().numpy()


def to_words(v, dtype):
    """float32 values -> uint16 words of their RNE rounding to dtype."""
    return torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(dtype).view(torch.int16).numpy().view(np.uint16)


def tensor_words(t):
    """uint16 words of a bf16 / fp16 tensor (any device)."""
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def from_words(words, dtype, device=None):
    t = torch.from_numpy(np.ascontiguousarray(words, dtype=np.uint16).view(np.int16).copy()).view(dtype)
    return t if device is None else t.to(device)


def canon(words, dtype):
    """Every NaN word replaced by one canonical word: NaN equals NaN whatever its payload."""
    w = np.array(words, dtype=np.uint16, copy=True)
    m = _EXP_MASK[dtype]
    w[((w & m) == m) & ((w & 0x7FFF) != m)] = _CANON_NAN[dtype]
    return w


def _rd(v, dtype):
    return to_f32(to_words(v, dtype), dtype)


def _x_int(x, dtype, s, zp):
    a = _rd(x / s, dtype)
    r = np.rint(a)
    b = _rd(_rd(r - a, dtype) + a, dtype)
    return _rd(b + zp, dtype)


def x_int(words, dtype, scale, zero_point):
    """fp32 values of the chain's x_int (the number its clamp and the backward's mask see) for uint16 words of x."""
    with np.errstate(all="ignore"):
        return _x_int(to_f32(words, dtype), dtype, np.float32(scale), np.float32(zero_point))


def chain_forward(x_words, dtype, scale, zero_point, quant_min, quant_max):
    """y words of util_quant.fake_quantize_per_tensor_affine(x, scale, zero_point, ...) with Python-number parameters."""
    x = to_f32(x_words, dtype)
    s, z = np.float32(scale), np.float32(zero_point)
    qmin, qmax = np.float32(quant_min), np.float32(quant_max)
    with np.errstate(all="ignore"):
        xi = _x_int(x, dtype, s, z)
        c = np.where(xi < qmin, qmin, xi)
        c = np.where(xi > qmax, qmax, c)
        c = _rd(c, dtype)
        return to_words(_rd(c - z, dtype) * s, dtype)


def chain_backward(x_words, g_words, dtype, scale, zero_point, quant_min, quant_max):
    """dx words of the same call under autograd for an upstream gradient in dtype."""
    x, g = to_f32(x_words, dtype), to_f32(g_words, dtype)
    s, z = np.float32(scale), np.float32(zero_point)
    with np.errstate(all="ignore"):
        xi = _x_int(x, dtype, s, z)
        gs = _rd(g * s, dtype)
        m = np.where((xi >= np.float32(quant_min)) & (xi <= np.float32(quant_max)), gs, np.float32(0.0))
        return to_words(m / s, dtype)

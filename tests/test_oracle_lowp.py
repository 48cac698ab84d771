"""bf16 / fp16 inputs on the CPU: the host emulation of the in-dtype chain (tests/_lowp_chain.py) against the reference's
outputs (tests/golden/lowp.npz, word for word), and the C ABI of the entry points that take an element type (exported, declared,
rejecting bad arguments before any launch)."""
import ctypes
import os

import numpy as np
import pytest

import _lowp_chain as L

HERE = os.path.dirname(os.path.abspath(__file__))
LOWP_SYMBOLS = ("osq_fake_quant_chain_lowp", "osq_fake_quant_chain_backward_lowp", "osq_fake_quant_per_tensor_widen")   # 16-bit only
DTYPE_SYMBOLS = ("osq_observe_flat", "osq_observe_channels", "osq_token_minmax", "osq_observe_tokens",          # fp32 / bf16 / fp16
                 "osq_fake_quant_per_channel")
REMOVED_SYMBOLS = ("osq_fake_quant_per_channel_widen", "osq_observe_flat_lowp", "osq_observe_channels_lowp",
                   "osq_token_minmax_lowp")


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(HERE, "golden", "lowp.npz"))


def _qrange(bit, symmetric):
    return (-(1 << (bit - 1)), (1 << (bit - 1)) - 1) if symmetric else (0, (1 << bit) - 1)


@pytest.mark.parametrize("dn", sorted(L.DTYPES))
def test_emulation_equals_reference_words(fx, dn):
    dt = L.DTYPES[dn]
    x, gy = fx[f"x_{dn}"], fx[f"gy_{dn}"]
    assert len(fx["chain_cases"]) >= 8
    for ci, (bit, sym, s, zp, _) in enumerate(fx["chain_cases"]):
        qmin, qmax = _qrange(int(bit), int(sym))
        y = L.chain_forward(x, dt, s, zp, qmin, qmax)
        np.testing.assert_array_equal(L.canon(y, dt), L.canon(fx[f"chain_{dn}_{ci}_y"], dt), err_msg=f"case {ci} y")
        dx = L.chain_backward(x, gy, dt, s, zp, qmin, qmax)
        np.testing.assert_array_equal(L.canon(dx, dt), L.canon(fx[f"chain_{dn}_{ci}_dx"], dt), err_msg=f"case {ci} dx")


@pytest.mark.parametrize("dn", sorted(L.DTYPES))
def test_fixture_covers_the_edges(fx, dn):
    dt = L.DTYPES[dn]
    x = L.to_f32(fx[f"x_{dn}"], dt)
    assert np.isnan(x).any() and np.isposinf(x).any() and np.isneginf(x).any()
    assert (np.signbit(x) & (x == 0)).any() and (~np.signbit(x) & (x == 0)).any()
    tiny = float(np.finfo(np.float16).tiny) if dn == "f16" else 2.0 ** -126
    assert ((x != 0) & (np.abs(x) < tiny)).any()                    # subnormals of the dtype
    if dn == "f16":   # x / 0.01 overflows fp16: NaN through inf - inf, as in the reference
        ci = [i for i, c in enumerate(fx["chain_cases"]) if c[2] == 0.01][0]
        y = L.to_f32(fx[f"chain_f16_{ci}_y"], dt)
        assert np.isnan(y[np.isfinite(x) & (np.abs(x) > 700)]).all()


def test_lowp_abi_exported_and_validated():
    from outlier_suppression_amd import _hip
    lib = _hip.load()
    assert _hip.ABI_VERSION == 10 and lib.osq_abi_version() == 10
    for name in LOWP_SYMBOLS + DTYPE_SYMBOLS:
        assert hasattr(lib, name) and name in _hip.SIGNATURES, name
    for name in REMOVED_SYMBOLS:
        assert not hasattr(lib, name) and name not in _hip.SIGNATURES, name
    f32, bf16, f16, bad = _hip.DTYPE_F32, _hip.DTYPE_BF16, _hip.DTYPE_F16, 7
    assert (f32, bf16, f16) == (0, 1, 2)
    p = ctypes.c_void_p(16)
    view = _hip.TokenView(2, 4, 1, 8, 32, 8, 0, 1)
    tail = (1, 1.0, 0, 0, None, None, None, 0, 255, 0, None, None, 0, None, None, None)      # osq_observe_tokens after token_max
    for dt in (bf16, f16):
        assert lib.osq_fake_quant_chain_lowp(dt, None, None, 16, p, p, 0, 0, 255, None) == -1
        assert b"null" in lib.osq_last_error()
        assert lib.osq_fake_quant_chain_backward_lowp(dt, p, None, p, 16, p, p, 0, 0, 255, None) == -1
        assert lib.osq_fake_quant_per_tensor_widen(dt, p, p, 16, None, p, 0, 0, 1.0, 0, 255, None) == -1
        assert lib.osq_fake_quant_per_tensor_widen(dt, p, p, 16, p, p, 0, 64, 1.0, 0, 255, None) == -1   # bad mode
        # the integers before dequantisation exist for fp32 x only; zp_type and mode are checked for 16-bit x
        assert lib.osq_fake_quant_per_channel(dt, p, p, p, 1, 4, 4, p, p, 0, 0, 1.0, 0, 255, None) == -1
        assert b"x_quant" in lib.osq_last_error()
        assert lib.osq_fake_quant_per_channel(dt, p, p, None, 1, 4, 4, p, p, 0, 64, 1.0, 0, 255, None) == -1
        assert lib.osq_fake_quant_per_channel(dt, p, p, None, 1, 4, 4, p, p, 5, 0, 1.0, 0, 255, None) == -1
    for dt in (f32, bf16, f16):
        assert lib.osq_fake_quant_per_channel(dt, None, p, None, 1, 4, 4, p, p, 0, 0, 1.0, 0, 255, None) == -1
        assert b"null" in lib.osq_last_error()
        assert lib.osq_observe_flat(dt, None, 16, 0, 0, None, None, None, 0, 255, 0, None, None, 0, p, None) == -1
        assert lib.osq_observe_flat(dt, p, 16, 1, 0, None, None, None, 0, 255, 0, None, None, 0, p, None) == -1
        assert lib.osq_observe_channels(dt, None, 1, 4, 4, 0, 0, None, None, 0, 255, 0, None, None, 0, None) == -1
        assert lib.osq_token_minmax(dt, p, ctypes.byref(view), None, None, p, None) == -1
        assert lib.osq_observe_tokens(dt, p, ctypes.byref(view), None, None, p, *tail) == -1
    # an unknown element type is refused whatever else the call holds
    assert lib.osq_fake_quant_chain_lowp(bad, p, p, 16, p, p, 0, 0, 255, None) == -1
    assert b"dtype" in lib.osq_last_error()
    assert lib.osq_fake_quant_chain_lowp(f32, p, p, 16, p, p, 0, 0, 255, None) == -1      # 16-bit only: no fp32 chain
    assert lib.osq_fake_quant_chain_backward_lowp(0, p, p, p, 16, p, p, 0, 0, 255, None) == -1
    assert lib.osq_fake_quant_per_tensor_widen(bad, p, p, 16, p, p, 0, 0, 1.0, 0, 255, None) == -1
    assert lib.osq_fake_quant_per_tensor_widen(f32, p, p, 16, p, p, 0, 0, 1.0, 0, 255, None) == -1
    for call in (lambda: lib.osq_fake_quant_per_channel(bad, p, p, None, 1, 4, 4, p, p, 0, 0, 1.0, 0, 255, None),
                 lambda: lib.osq_observe_flat(bad, p, 16, 0, 0, None, None, None, 0, 255, 0, None, None, 0, p, None),
                 lambda: lib.osq_observe_channels(bad, p, 1, 4, 4, 0, 0, None, None, 0, 255, 0, None, None, 0, None),
                 lambda: lib.osq_token_minmax(bad, p, ctypes.byref(view), None, p, p, None),
                 lambda: lib.osq_observe_tokens(bad, p, ctypes.byref(view), None, p, p, *tail)):
        assert lib.osq_fake_quant_chain_lowp(bf16, None, None, 16, p, p, 0, 0, 255, None) == -1     # another error text in between
        assert call() == -1
        assert b"dtype" in lib.osq_last_error()


def test_fp32_entry_points_still_refuse_half():
    """The 16-bit dispatch lives one level up (ops.fake_quant, util_quant, the observers)."""
    import torch
    from outlier_suppression_amd import ops
    x = torch.zeros(8, dtype=torch.bfloat16)
    with pytest.raises(TypeError):
        ops._check_f32(x)
    assert ops.is_lowp(x) and ops.is_lowp(x.half()) and not ops.is_lowp(x.float())

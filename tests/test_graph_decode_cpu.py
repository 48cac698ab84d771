"""CPU: what the captured decoding step (model/graph_decode.py, generate(graph=True)) needs where no GPU is involved: the
four position-from-device entry points in the header's "Added within 10" list and in ``_hip.SIGNATURES``; the grad-factor
table the attention launch reads on the device, against the quantizer's own ``_grad_factor`` as a launch argument carries
it, bit for bit; the switch, its setter and its environment variable; and the reason generate() gives on CPU tensors.
The launches and the graphs run on the GPU (tests/test_gpu_decode_at.py, tests/test_gpu_graph_decode_model.py)."""
import ctypes
import os
import re
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("osq_fake_quant_kv_append_at", "osq_fake_quant_kv_append_codes_at", "osq_decode_attention_fake_quant_at",
           "osq_decode_attention_codes_at")


def test_entry_points_are_listed_and_bound():
    from outlier_suppression_amd import _hip
    header = open(os.path.join(ROOT, "include", "osq_hip.h")).read()
    added = re.search(r"Added within 10 \(no existing signature changed\):(.*?)\*/", header, re.S).group(1)
    listed = set(re.findall(r"osq_\w+", added))
    for name in SYMBOLS:
        assert name in listed, f"{name} is not in the header's 'Added within 10' list"
        assert re.search(r"^int " + name + r"\(", header, re.M), f"{name} is not declared"
        assert name in _hip.SIGNATURES
    assert re.search(r"#define OSQ_ABI_VERSION 10\b", header) and _hip.ABI_VERSION == 10
    # the _at forms take the static form's arguments and the position: the site tables are the static forms' own
    assert _hip.SIGNATURES["osq_fake_quant_kv_append_at"][1][0] == _hip.SIGNATURES["osq_fake_quant_kv_append"][1][0]
    assert _hip.SIGNATURES["osq_fake_quant_kv_append_codes_at"][1][0] == _hip.SIGNATURES["osq_fake_quant_kv_append_codes"][1][0]
    for at, static, extra in (("osq_decode_attention_fake_quant_at", "osq_decode_attention_fake_quant", 5),
                              ("osq_decode_attention_codes_at", "osq_decode_attention_codes", 5)):
        assert len(_hip.SIGNATURES[at][1]) == len(_hip.SIGNATURES[static][1]) + extra


def _as_launch_argument(x):
    """The fp32 word a Python float becomes as a c_float argument of a launch."""
    return np.float32(ctypes.c_float(x).value)


@pytest.mark.parametrize("quant_max", [63, 255])
@pytest.mark.parametrize("rows", [4, 3072])
def test_grad_table_has_the_bits_of_the_static_call(rows, quant_max):
    """Entry n of the table is what decode_attention_fake_quant hands the static launch at kv_len == n: the quantizer's
    ``_grad_factor`` of a [rows, 1, n] tensor, rounded to fp32 -- for EVERY length the kernel takes."""
    from outlier_suppression_amd import util_layernorm as UL
    from outlier_suppression_amd.quantization import Quantizer
    bit = {63: 6, 255: 8}[quant_max]
    q = Quantizer(None, NS(quantizer="LSQPlusFakeQuantize", observer="AvgMinMaxObserver", bit=bit, symmetric=False, ch_axis=-1))
    assert q.quant_max == quant_max and q.param_mode != 0
    table = UL.decode_grad_table(q, rows, 4096)
    assert table.dtype == torch.float32 and table.shape == (4097,) and table.device.type == "cpu"
    want = np.array([_as_launch_argument(q._grad_factor(UL._Numel(rows * n))) for n in range(1, 4097)], dtype=np.float32)
    got = table.numpy()[1:]
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert len(np.unique(got)) == 4096 and got[0] == _as_launch_argument(1.0 / (rows * quant_max) ** 0.5)


def test_grad_table_of_a_fixed_quantizer_is_one():
    from outlier_suppression_amd import util_layernorm as UL
    from outlier_suppression_amd.quantization import Quantizer
    q = Quantizer(None, NS(quantizer="FixedFakeQuantize", observer="AvgMinMaxObserver", bit=8, symmetric=False, ch_axis=-1))
    assert bool((UL.decode_grad_table(q, 12, 40)[1:] == 1.0).all())


@pytest.fixture()
def switch():
    from outlier_suppression_amd import util_layernorm as UL
    old = UL.GRAPH_DECODE
    yield UL
    UL.GRAPH_DECODE = old


def test_switch_is_off_by_default_and_settable(switch):
    import outlier_suppression_amd as osq
    assert switch.GRAPH_DECODE is False or os.environ.get("OSQ_GRAPH_DECODE", "") not in ("", "0")
    osq.set_graph_decode(True)
    assert switch.GRAPH_DECODE is True
    osq.set_graph_decode(False)
    assert switch.GRAPH_DECODE is False
    osq.set_graph_decode()
    assert switch.GRAPH_DECODE is True


@pytest.mark.parametrize("value, want", [(None, False), ("", False), ("0", False), ("1", True), ("yes", True)])
def test_environment_variable(value, want):
    import outlier_suppression_amd as osq
    env = {} if value is None else {"OSQ_GRAPH_DECODE": value}
    assert osq.graph_decode_from_environment(env) is want


def test_environment_reaches_reset_tier(switch, monkeypatch):
    import outlier_suppression_amd as osq
    from outlier_suppression_amd import ops
    monkeypatch.setattr(ops, "set_tuning", lambda key, value, lib=None: None)
    monkeypatch.setenv("OSQ_GRAPH_DECODE", "1")
    osq.reset_tier()
    assert switch.GRAPH_DECODE is True
    monkeypatch.delenv("OSQ_GRAPH_DECODE")
    osq.reset_tier()
    assert switch.GRAPH_DECODE is False


def test_cpu_tensors_are_a_reason_not_an_error():
    from outlier_suppression_amd.model import graph_decode
    reason = graph_decode.why_not(None, torch.device("cpu"), True, 20)
    assert reason and "CPU" in reason
    info = graph_decode.DecodeGraphInfo(reason)
    assert (info.captured, info.replays, info.reason) == (0, 0, reason)

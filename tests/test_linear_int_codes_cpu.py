"""What a machine without a GPU can say about ops.linear_int_codes and quantization/linear_int.py ``ffn``: the entry point is
declared and bound, the refusals come before any launch, and a CPU model keeps the chain."""
import os
import re
from types import SimpleNamespace as NS

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_entry_point_is_declared_within_abi_10_and_bound():
    from outlier_suppression_amd import _hip
    header = open(os.path.join(ROOT, "include", "osq_hip.h")).read()
    added = re.search(r"Added within 10.*?\*/", header, re.S).group(0)
    assert "osq_linear_int_codes" in added and "#define OSQ_ABI_VERSION 10" in header
    assert len(_hip.SIGNATURES["osq_linear_int_codes"][1]) == 31


def operands(n, k=32):
    from outlier_suppression_amd import ops
    record = (torch.ones(1), torch.zeros(1, dtype=torch.int32), 0, 255, ops.PARAM_FIXED, 1.0)
    entry = ops.WeightCodes(torch.zeros(n, k, dtype=torch.uint8), torch.zeros(n, dtype=torch.int32), torch.ones(n),
                            torch.zeros(n, dtype=torch.int32), torch.zeros(1, dtype=torch.int32))
    return torch.zeros(2, k, dtype=torch.uint8), torch.zeros(2, dtype=torch.int32), record, entry, None, record


@pytest.mark.parametrize("n, activation, why", ((40, "gelu", "N is not a multiple of 16"), (16400, None, "N exceeds 16384"),
                                                (48, "tanh", "activation"), (48, "gelu", "not on a GPU")))
def test_refusals_launch_nothing(monkeypatch, n, activation, why):
    from outlier_suppression_amd import _hip, ops
    monkeypatch.setattr(_hip, "load", lambda: pytest.fail("the library was asked for"))
    with pytest.raises(ValueError, match=why):
        ops.linear_int_codes(*operands(n), activation)


def test_ffn_keeps_the_chain_on_a_cpu_model():
    from transformers import BertConfig, BertForSequenceClassification
    from outlier_suppression_amd.quant_model import quantize_model
    from outlier_suppression_amd.quantization import linear_int
    qc = NS(quantizer="FixedFakeQuantize", observer="MinMaxObserver", bit=8, symmetric=False, ch_axis=-1)
    cfg = BertConfig(vocab_size=60, hidden_size=32, num_hidden_layers=1, num_attention_heads=2, intermediate_size=64,
                     max_position_embeddings=20, num_labels=2)
    q = quantize_model(BertForSequenceClassification(cfg).eval(), qc, qc)
    layer = q.bert.encoder.layer[0]
    assert linear_int.FUSE_FFN and linear_int.weight_why_not(layer.output.dense) is not None
    with torch.no_grad():
        assert linear_int.ffn(layer.intermediate.dense, layer.intermediate.intermediate_act_fn,
                              layer.intermediate.intermediate_act_fn_post_act_fake_quantize, layer.output.dense, torch.randn(2, 5, 32)) is None

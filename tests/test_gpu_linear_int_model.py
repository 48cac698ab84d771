"""Integer linear layers (util_layernorm.FUSE_LINEAR_INT, csrc/linear_int.hip) inside the quantized models: the tiny pipelines
of tests/test_gpu_model.py with the switch on, at the bars tests/test_gpu_attention_int_model.py holds them to; a frozen BERT
after gamma migration, alone and with FUSE_ATTENTION_INT and FUSE_SOFTMAX; generate(num_beams=3) against the switch-off call."""
from types import SimpleNamespace as NS

import pytest
import torch

import test_gpu_model
from test_gpu_bart_decode import A_Q, FUSED_VS_EAGER_LOGITS, W_Q, setup  # noqa: F401  (setup: that file's module fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]


@pytest.fixture()
def switch():
    import outlier_suppression_amd as osq
    from outlier_suppression_amd import _hip, util_layernorm as UL
    _hip.load()
    old = UL.FUSE_LINEAR_INT, UL.FUSE_ATTENTION_INT, UL.FUSE_SOFTMAX
    UL.linear_int.reset()
    yield osq.set_fast_linear_int
    for setter, on in zip((osq.set_fast_linear_int, osq.set_fast_attention_int, osq.set_fast_softmax), old):
        setter(on)


@pytest.fixture(scope="module")
def migrated():
    """(model, batch): a tiny W6A6 BERT whose LayerNorm sites gamma migration has replaced, then calibrated and frozen."""
    from transformers import BertConfig, BertForSequenceClassification
    from outlier_suppression_amd.gamma_migration import delay_ln
    from outlier_suppression_amd.quant_model import quantize_model
    from outlier_suppression_amd.quantization import disable_all, enable_calibration_woquantization, enable_quantization
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    cfg = BertConfig(vocab_size=120, hidden_size=32, num_hidden_layers=2, num_attention_heads=2, intermediate_size=64,
                     max_position_embeddings=40, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    fp = BertForSequenceClassification(cfg).eval()
    for m in fp.modules():
        if isinstance(m, torch.nn.LayerNorm):
            m.weight.data.uniform_(0.5, 2.0)              # a gamma worth migrating
    q = delay_ln(quantize_model(fp.to(dev), W_Q, A_Q).to(dev), NS(a_qconfig=A_Q, w_qconfig=W_Q), NS(model_type="bert", task_type="glue"))
    ids = torch.randint(3, 120, (4, 17), generator=torch.Generator().manual_seed(1)).to(dev)
    batch = dict(input_ids=ids, attention_mask=torch.ones_like(ids), token_type_ids=torch.zeros_like(ids))
    enable_calibration_woquantization(q)
    with torch.no_grad():
        q(**batch)
    disable_all(q)
    enable_quantization(q)
    return q, batch


@pytest.mark.parametrize("kind", list(test_gpu_model.PIPELINES) + ["bart"])
def test_pipelines_with_the_switch_on(golden, switch, kind):
    """tests/test_gpu_model.py's pipelines as they stand (gamma migration included), switch on: frozen passes take the integer
    launches, calibration passes run F.linear; BART's quantizes activations only, so every linear runs F.linear and says so."""
    from outlier_suppression_amd import util_layernorm as UL
    switch(True)
    if kind == "bart":
        test_gpu_model.test_bart_pipeline_matches_reference(golden)
    else:
        test_gpu_model.test_pipeline_matches_reference(golden, kind, False)
    assert UL.linear_int.eager > 0 and (UL.linear_int.fused > 0 or (kind == "bart" and "weight quantizer" in UL.linear_int.reason))


@pytest.mark.parametrize("others", (False, True), ids=("alone", "with_attention_int_and_softmax"))
def test_migrated_forward_counts_and_distance(switch, migrated, others):
    """One frozen forward after gamma migration: every linear is bound and takes the integer launches once (fused = bound,
    eager = the rest = 0); the logits against the switch-off forward at the bar that file holds the one-launch attention to."""
    import outlier_suppression_amd as osq
    from outlier_suppression_amd import util_layernorm as UL
    from outlier_suppression_amd.quantization import linear_int
    from outlier_suppression_amd.quantization.quantized_module import QLinear
    (q, batch), logits = migrated, {}
    assert sum(isinstance(m, UL.QuantizedSplitLayerNorm) for m in q.modules()) == 4
    linears = [m for m in q.modules() if isinstance(m, QLinear)]
    bound = sum(linear_int.producer_of(m) is not None for m in linears)
    assert bound == len(linears) == 2 * 6 + 2                # query / key / value, two dense per block and its FFN; pooler, classifier
    osq.set_fast_attention_int(others)
    osq.set_fast_softmax(others)
    for on in (True, False):
        switch(on)
        UL.linear_int.reset()
        with torch.no_grad():
            logits[on] = q(**batch)[0]
        assert (UL.linear_int.fused, UL.linear_int.eager) == ((bound, len(linears) - bound) if on else (0, 0)), UL.linear_int
    d = (logits[True] - logits[False]).abs().max().item()
    print(f"\ninteger linear vs F.linear after gamma migration ({'all three switches' if others else 'alone'}): max |logit diff| {d:.3g}")
    assert d < FUSED_VS_EAGER_LOGITS, d


def test_generate_returns_the_switch_off_tokens(switch, setup):
    s, tokens = setup, {}
    for on in (True, False):
        switch(on)
        with torch.no_grad():
            tokens[on] = s.q.generate(s.ids, attention_mask=s.mask, max_length=20, num_beams=3)
    assert tokens[True].shape == tokens[False].shape and torch.equal(tokens[True], tokens[False]), tokens

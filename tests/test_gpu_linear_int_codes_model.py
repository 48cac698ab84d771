"""quantization/linear_int.py ``ffn`` inside a tiny frozen BERT and BART, W8A8 and W4A8: with FUSE_FFN on (FFN_MAX_ROWS lifted:
these calls have more than 32 rows) the logits are WORD-EQUAL to the chain's and every feed-forward block takes the path; a
greedy generate() under the captured-graph decode, whose 4-row steps take the path by default, returns the same tokens."""
import functools
from types import SimpleNamespace as NS

import pytest
import torch

import _linear_int as LI

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]

A_Q = NS(quantizer="FixedFakeQuantize", observer="MinMaxObserver", bit=8, symmetric=False, ch_axis=-1)


@pytest.fixture()
def switches():
    import outlier_suppression_amd as osq
    from outlier_suppression_amd import _hip, util_layernorm as UL
    from outlier_suppression_amd.quantization import linear_int
    _hip.load()
    old = UL.FUSE_LINEAR_INT, UL.GRAPH_DECODE, linear_int.FUSE_FFN, linear_int.FFN_MAX_ROWS
    osq.set_fast_linear_int(True)
    yield linear_int
    osq.set_fast_linear_int(old[0])
    osq.set_graph_decode(old[1])
    linear_int.FUSE_FFN, linear_int.FFN_MAX_ROWS = old[2:]


BERT = dict(vocab_size=60, hidden_size=32, num_hidden_layers=2, num_attention_heads=2, intermediate_size=64, max_position_embeddings=20)
BART = dict(vocab_size=120, d_model=64, encoder_layers=2, decoder_layers=2, encoder_attention_heads=4, decoder_attention_heads=4,
            encoder_ffn_dim=128, decoder_ffn_dim=128, max_position_embeddings=80, dropout=0.0, attention_dropout=0.0,
            activation_dropout=0.0, pad_token_id=1, bos_token_id=0, eos_token_id=2, decoder_start_token_id=2)


@functools.lru_cache(maxsize=None)
def frozen(kind, w_bits):
    """(model, batch, feed-forward blocks): calibrated on the batch, then frozen."""
    from transformers import BartConfig, BartForConditionalGeneration, BertConfig, BertForSequenceClassification
    from outlier_suppression_amd.quant_model import quantize_model
    from outlier_suppression_amd.quantization import disable_all, enable_calibration_woquantization, enable_quantization
    dev, gen = torch.device("cuda:0"), torch.Generator().manual_seed(1)
    w_q = NS(quantizer="FixedFakeQuantize", observer="MinMaxObserver", bit=w_bits, symmetric=True, ch_axis=0)
    torch.manual_seed(0)
    ids = torch.randint(3, 60, (4, 17), generator=gen).to(dev)
    if kind == "bert":
        fp, blocks, batch = BertForSequenceClassification(BertConfig(**BERT)), 2, dict(input_ids=ids, attention_mask=torch.ones_like(ids))
    else:
        fp, blocks = BartForConditionalGeneration(BartConfig(**BART)), 4
        batch = dict(input_ids=ids, attention_mask=torch.ones_like(ids), decoder_input_ids=ids[:, :12].contiguous())
    q = quantize_model(fp.eval().to(dev), w_q, A_Q).to(dev).eval()
    enable_calibration_woquantization(q)
    with torch.no_grad():
        q(**batch)
    disable_all(q)
    enable_quantization(q)
    return q, batch, blocks


@pytest.mark.parametrize("kind, w_bits", (("bert", 8), ("bert", 4), ("bart", 8), ("bart", 4)))
def test_logits_are_the_chain_s_words(switches, kind, w_bits):
    from outlier_suppression_amd import util_layernorm as UL
    (q, batch, blocks), logits, fused = frozen(kind, w_bits), {}, {}
    assert switches.FFN_MAX_ROWS == 32                   # these calls have 48 to 68 rows: under the default they keep the chain
    for on, limit in ((True, None), (False, None), ("routed", 32)):
        switches.FUSE_FFN, switches.FFN_MAX_ROWS = bool(on), limit
        UL.linear_int.reset()
        with torch.no_grad():
            logits[on] = q(**batch)[0].cpu().numpy()
        assert (UL.linear_int.ffn, UL.linear_int.eager) == (blocks if on is True else 0, 0), UL.linear_int
        fused[on] = UL.linear_int.fused
    assert fused[True] == fused[False] > 2 * blocks
    assert LI.words(logits[True]) == LI.words(logits[False])


def test_a_captured_greedy_decode_returns_the_chain_s_tokens(switches):
    import outlier_suppression_amd as osq
    from outlier_suppression_amd import util_layernorm as UL
    (q, batch, _), tokens = frozen("bart", 8), {}
    osq.set_graph_decode(True)
    for on in (True, False):
        switches.FUSE_FFN = on
        UL.linear_int.reset()
        with torch.no_grad():
            tokens[on] = q.generate(batch["input_ids"], attention_mask=batch["attention_mask"], max_length=6, graph=True)
        assert (UL.linear_int.ffn > 0) == on, UL.linear_int
    assert torch.equal(tokens[True], tokens[False]), tokens

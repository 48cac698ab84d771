"""CPU: how ``cross_group`` and score(share_cross_kv=...) are routed through the quantized BART wrapper, with every quantizer
off (a plain FP model, as in tests/test_bart_decode_cpu.py).  On the CPU no launch takes the key / value sites, so a layer given
a group expands the encoder's rows itself and runs the path it always ran: the values are those of the expanded call, and
score() says why it shared nothing.  The shared computation itself runs on the GPU (tests/test_gpu_score_share_model.py)."""
import pytest
import torch

from test_bart_decode_cpu import batch, tiny_bart, wrapped

N = 3


@pytest.fixture(scope="module")
def model():
    return wrapped(tiny_bart())


def _labels():
    g = torch.Generator().manual_seed(5)
    labels = torch.randint(3, 120, (3 * N, 6), generator=g)
    labels[4, 4:] = -100
    return labels


def test_forward_with_cross_group_is_the_forward_on_expanded_encoder_rows(model):
    ids, mask = batch()
    dec = _labels().clamp_min(3)
    with torch.no_grad():
        enc = model.get_encoder()(ids, attention_mask=mask)
        want = model(attention_mask=mask.repeat_interleave(N, 0), decoder_input_ids=dec,
                     encoder_outputs=(enc.repeat_interleave(N, 0),))[0]
        got = model(attention_mask=mask, decoder_input_ids=dec, encoder_outputs=(enc,), cross_group=N)[0]
        assert [layer.encoder_attn.last_cross_shared for layer in model.model.decoder.layers] == [False, False]
        assert got.shape == (3 * N, 6, 120) and torch.equal(got, want)
        with pytest.raises(ValueError, match="cross_group=2 takes encoder states of 4 rows"):
            model(attention_mask=mask, decoder_input_ids=dec[:8], encoder_outputs=(enc,), cross_group=2)
        with pytest.raises(ValueError, match="without a cache"):
            model(attention_mask=mask, decoder_input_ids=dec, encoder_outputs=(enc,), cross_group=N, use_cache=True)


def test_score_on_the_cpu_says_why_it_shares_nothing(model):
    import outlier_suppression_amd as osq
    ids, mask = batch()
    labels = _labels()
    want = model.score(ids, labels, attention_mask=mask, num_candidates=N)
    assert model.last_share_cross_kv.reason == "not asked for"
    got = model.score(ids, labels, attention_mask=mask, num_candidates=N, share_cross_kv=True)
    info = model.last_share_cross_kv
    assert (info.shared, info.eager, info.reason) == (0, 0, "the tensors are on the CPU"), info
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    model.score(ids, labels[::N], attention_mask=mask, share_cross_kv=True)
    assert "num_candidates == 1" in model.last_share_cross_kv.reason
    osq.set_share_cross_kv(True)
    try:
        model.score(ids, labels, attention_mask=mask, num_candidates=N)
        assert model.last_share_cross_kv.reason == "the tensors are on the CPU"
        model.score(ids, labels, attention_mask=mask, num_candidates=N, share_cross_kv=False)
        assert model.last_share_cross_kv.reason == "not asked for"
    finally:
        osq.set_share_cross_kv(False)


def test_ops_and_wrappers_take_group_with_a_default_of_one():
    import inspect
    from outlier_suppression_amd import ops, util_layernorm as UL
    for fn in (ops.attention_fusable, ops.attention_fake_quant, ops.attention_int_fake_quant, UL.attention_block_fake_quant,
               UL.attention_int_block_fake_quant, UL.attention_int_refusal, UL.attention_sequence_fake_quant):
        assert inspect.signature(fn).parameters["group"].default == 1, fn.__name__

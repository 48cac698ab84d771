"""Whole-sequence attention on integer codes (util_layernorm.FUSE_ATTENTION_INT, csrc/attention_int.hip) inside the quantized
models: (a) the tiny BERT-cls / BERT-QA / RoBERTa pipelines and the tiny BART pipeline of tests/test_gpu_model.py and the
reference's cached decode (tests/golden/bart_decode.npz) with the switch on, at the bars the eager form is held to; (b)
switch on against switch off on the tiny W6A6 LSQ+ BART of tests/test_gpu_bart_decode.py: a plain forward and
score(num_candidates=3) on the logits, generate(num_beams=3) compared and printed; (c) which calls take the integer form; (d) a
model with one per-channel activation quantizer falls back to the eager words."""
import copy
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import test_gpu_model
from test_gpu_bart_decode import (A_Q, FUSED_VS_EAGER_LOGITS, REFERENCE_LOGITS_BAR, W_Q, _reference_pipeline,
                                  setup)  # noqa: F401  (setup: the module fixture of that file, instantiated for this one)
from test_gpu_model import INTEGER_BARS, PIPELINES

pytestmark = pytest.mark.gpu


@pytest.fixture()
def switch():
    """set_fast_attention_int, restored afterwards (the fp32 and decode switches too: tests here turn them on)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import outlier_suppression_amd as osq
    from outlier_suppression_amd import _hip, util_layernorm as UL
    _hip.load()                      # the first load applies the environment's tier, these switches included
    old = UL.FUSE_ATTENTION_INT, UL.FUSE_ATTENTION, UL.FUSE_DECODE_ATTENTION
    yield osq.set_fast_attention_int
    osq.set_fast_attention_int(old[0])
    osq.set_fast_attention(old[1])
    osq.set_fast_decode_attention(old[2])


@pytest.fixture()
def calls(monkeypatch):
    """Every call of ops.attention_int_fake_quant, as (T, S, launched)."""
    from outlier_suppression_amd import ops
    seen = []
    real = ops.attention_int_fake_quant

    def counted(q, k, *a, **kw):
        out = real(q, k, *a, **kw)
        seen.append((q.shape[2], k.shape[2], out is not None))
        return out
    monkeypatch.setattr(ops, "attention_int_fake_quant", counted)
    return seen


# ------------------------------------------------------------------------------------------------ (a) the reference's bars

@pytest.mark.parametrize("kind", list(PIPELINES))
def test_a_bert_pipelines_with_the_switch_on(golden, switch, calls, kind):
    """tests/test_gpu_model.py::test_pipeline_matches_reference, default configuration, run as it stands with the switch on.
    Every attention of a pass whose quantizers only quantize is launched; observer and autograd passes stay eager."""
    switch(True)
    test_gpu_model.test_pipeline_matches_reference(golden, kind, False)
    launched = [c for c in calls if c[2]]
    print(f"\n{kind}: {len(launched)} integer attention blocks, {len(calls) - len(launched)} refused")
    assert launched and len(launched) == len(calls) and all(c[0] > 1 for c in calls)


def test_a_bart_pipeline_with_the_switch_on(golden, switch, calls):
    assert REFERENCE_LOGITS_BAR == 0.1 and INTEGER_BARS["worst"] == 5e-3
    switch(True)
    test_gpu_model.test_bart_pipeline_matches_reference(golden)
    launched = [c for c in calls if c[2]]
    # the activation-quantized pass: per batch 2 encoder blocks + 2 decoder layers x (self + cross)
    print(f"\ntiny BART pipeline: {len(launched)} integer attention blocks")
    assert launched and len(launched) % 6 == 0 and len(launched) == len(calls)


def test_a_reference_cached_decode_with_the_switch_on(golden, switch, calls):
    """The reference's cached greedy decode, teacher-forced with its tokens: the encoder's blocks take the integer form, the
    single-token decoder calls never reach it; per-step logits at REFERENCE_LOGITS_BAR, the greedy token wherever the
    reference's margin exceeds it."""
    dev = torch.device("cuda:0")
    g = golden("bart_decode")
    model = _reference_pipeline(golden, dev)
    ids, mask = torch.from_numpy(g["input_ids"]).to(dev), torch.from_numpy(g["attention_mask"]).to(dev)
    tokens = torch.from_numpy(g["tokens"]).to(dev)
    steps = g["step_logits"].shape[1]
    switch(True)
    del calls[:]
    with torch.no_grad():
        out, cache, enc = model(ids, mask, decoder_input_ids=tokens[:, :1], use_cache=True)
        logits = [out[:, -1]]
        for t in range(1, steps):
            out, cache, _ = model(attention_mask=mask, decoder_input_ids=tokens[:, t:t + 1], encoder_outputs=(enc,),
                                  past_key_values=cache, use_cache=True)
            logits.append(out[:, -1])
    assert len(calls) == len(model.model.encoder.layers) and all(c[2] and c[0] == ids.shape[1] for c in calls)
    got = torch.stack(logits, 1).cpu().numpy()
    err = np.abs(got - g["step_logits"]).max()
    print(f"\ninteger encoder attention vs the reference's cached decode: max |logit diff| {err:.3g} over {steps} steps")
    assert err < REFERENCE_LOGITS_BAR, err
    sure = g["margin"] > REFERENCE_LOGITS_BAR
    assert np.array_equal(got.argmax(-1)[sure], g["tokens"][:, 1:][sure])


# ------------------------------------------------------------------------------------------------ (b) on against off

def _on_off(switch, fn):
    switch(True)
    with torch.no_grad():
        on = fn()
    switch(False)
    with torch.no_grad():
        off = fn()
    return on, off


def test_b_forward_on_against_off(setup, switch, calls):
    s = setup
    on, off = _on_off(switch, lambda: s.q(s.ids, s.mask, decoder_input_ids=s.dec)[0])
    d = (on - off).abs().max().item()
    print(f"\ninteger attention vs eager, plain forward: max |logit diff| {d:.3g}")
    assert len(calls) == 6 and all(c[2] for c in calls)
    assert d < FUSED_VS_EAGER_LOGITS, d


def test_b_score_on_against_off(setup, switch, calls, monkeypatch):
    from outlier_suppression_amd import ops
    s = setup
    labels = torch.randint(3, 120, (9, 10), generator=torch.Generator().manual_seed(2)).to(s.dev)
    logits = []
    real = ops.lm_loss

    def recording(flat, *a, **kw):
        logits.append(flat.clone())
        return real(flat, *a, **kw)
    monkeypatch.setattr(ops, "lm_loss", recording)
    on, off = _on_off(switch, lambda: s.q.score(s.ids, labels, attention_mask=s.mask, num_candidates=3))
    d = (logits[0] - logits[1]).abs().max().item()
    print(f"\ninteger attention vs eager, score(num_candidates=3): max |logit diff| {d:.3g}, "
          f"max |token log-prob diff| {(on[0] - off[0]).abs().max().item():.3g}")
    assert len(calls) == 6 and all(c[2] for c in calls)
    assert d < FUSED_VS_EAGER_LOGITS, d


def test_b_generate_on_against_off(setup, switch, calls):
    """The tokens are compared and the outcome printed (README records it); the assertions are those on the logits above."""
    s = setup
    on, off = _on_off(switch, lambda: s.q.generate(s.ids, attention_mask=s.mask, max_length=20, num_beams=3))
    assert calls and all(c[2] and c[0] > 1 for c in calls)
    same = on.shape == off.shape and torch.equal(on, off)
    print(f"\ninteger attention vs eager, generate(num_beams=3): tokens {'equal' if same else 'DIFFER'}")


# ------------------------------------------------------------------------------------------------ (c) the call pattern

def test_c_call_pattern(setup, switch, calls, monkeypatch):
    import outlier_suppression_amd as osq
    from outlier_suppression_amd import ops
    s = setup
    blocks = len(s.q.model.encoder.layers) + 2 * len(s.q.model.decoder.layers)

    def forward():
        return s.q(s.ids, s.mask, decoder_input_ids=s.dec)
    switch(False)
    with torch.no_grad():
        forward()
    assert calls == []                                   # switch off: the op is never called
    switch(True)
    with torch.no_grad():
        forward()
    assert len(calls) == blocks and all(c[2] for c in calls)          # one launched call per attention block
    t, src = s.dec.shape[1], s.ids.shape[1]
    assert sorted(c[:2] for c in calls) == sorted([(src, src)] * 2 + [(t, t)] * 2 + [(t, src)] * 2)
    # both switches on: the integer form is tried first, the fp32 form sees nothing
    fp32_calls = []
    real_fp32 = ops.attention_fake_quant
    monkeypatch.setattr(ops, "attention_fake_quant", lambda *a, **kw: fp32_calls.append(1) or real_fp32(*a, **kw))
    osq.set_fast_attention(True)
    del calls[:]
    with torch.no_grad():
        forward()
    assert len(calls) == blocks and all(c[2] for c in calls) and fp32_calls == []
    osq.set_fast_attention(False)
    del calls[:]
    with torch.enable_grad():                            # autograd on: eager
        forward()
    assert calls == []
    attn = s.q.model.encoder.layers[0].self_attn
    qz = attn.key_post_act_fake_quantize                 # an observer on: that block is eager, nothing is launched for it
    saved = copy.deepcopy(qz.state_dict())
    qz.enable_observer()
    try:
        with torch.no_grad():
            forward()
    finally:
        qz.disable_observer()
        qz.load_state_dict(saved)
    assert len(calls) == blocks - 1 and all(c[2] for c in calls)
    # a cache: the first, multi-token call takes the block -- cached keys and values included -- the single-token steps the
    # decode op, never the integer block
    del calls[:]
    decode_calls = []
    real = ops.decode_attention_fake_quant

    def counted(*a, **kw):
        out = real(*a, **kw)
        decode_calls.append(out is not None)
        return out
    monkeypatch.setattr(ops, "decode_attention_fake_quant", counted)
    osq.set_fast_decode_attention(True)
    with torch.no_grad():
        _, cache, enc = s.q(s.ids, s.mask, decoder_input_ids=s.dec[:, :3], use_cache=True)
        assert len(calls) == blocks and all(c[2] for c in calls) and decode_calls == []
        s.q(attention_mask=s.mask, decoder_input_ids=s.dec[:, 3:4], encoder_outputs=(enc,), past_key_values=cache, use_cache=True)
        assert len(calls) == blocks and decode_calls == [True] * (2 * len(s.q.model.decoder.layers))
        # two more tokens at once over the cache: T = 2 over cached keys and values takes the integer block again
        del calls[:]
        s.q(attention_mask=s.mask, decoder_input_ids=s.dec[:, 4:6], encoder_outputs=(enc,), past_key_values=cache, use_cache=True)
    assert len(calls) == 2 * len(s.q.model.decoder.layers) and all(c[2] and c[0] == 2 for c in calls)
    osq.set_fast_decode_attention(False)                 # without the decode switch a single-token step is eager
    del calls[:]
    with torch.no_grad():
        s.q(attention_mask=s.mask, decoder_input_ids=s.dec[:, 6:7], encoder_outputs=(enc,), past_key_values=cache, use_cache=True)
    assert calls == []


# ------------------------------------------------------------------------------------------------ (d) a per-channel quantizer

def test_d_per_channel_quantizer_gives_the_eager_words(switch, calls):
    """One activation quantizer of one block per-channel: that block is refused before any launch and runs the eager
    sequence -- the words of the switch off -- while the other blocks take the integer form."""
    from transformers import BartConfig, BartForConditionalGeneration
    from outlier_suppression_amd.quant_model import quantize_model
    from outlier_suppression_amd.quantization import (Quantizer, disable_all, enable_calibration_woquantization,
                                                      enable_quantization)
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    cfg = BartConfig(vocab_size=120, d_model=32, encoder_layers=1, decoder_layers=1, encoder_attention_heads=2,
                     decoder_attention_heads=2, encoder_ffn_dim=64, decoder_ffn_dim=64, max_position_embeddings=40,
                     dropout=0.0, attention_dropout=0.0, activation_dropout=0.0, pad_token_id=1, bos_token_id=0,
                     eos_token_id=2, decoder_start_token_id=2)
    g = torch.Generator().manual_seed(1)
    ids, dec = torch.randint(3, 120, (2, 9), generator=g).to(dev), torch.randint(3, 120, (2, 5), generator=g).to(dev)
    mask = torch.ones_like(ids)
    q = quantize_model(BartForConditionalGeneration(cfg).eval().to(dev), W_Q, A_Q).to(dev).eval()
    enable_calibration_woquantization(q)
    with torch.no_grad():
        q(ids, mask, decoder_input_ids=dec)
    disable_all(q)
    enable_quantization(q)
    # the encoder block's value quantizer per channel of the hidden axis, parameters set by hand around the calibrated ones
    # (the activation observers do not observe per channel under an observation mask)
    attn = q.model.encoder.layers[0].self_attn
    old = attn.value_post_act_fake_quantize
    per_channel = NS(quantizer="FixedFakeQuantize", observer="MinMaxObserver", bit=6, symmetric=False, ch_axis=2)
    fresh = Quantizer(None, per_channel).to(dev)
    fresh.scale = old.scale.detach().abs().repeat(32) * torch.linspace(0.8, 1.2, 32, device=dev)
    zp = min(max(int(round(float(old.zero_point.detach()))), old.quant_min), old.quant_max)
    fresh.zero_point = torch.full((32,), zp, dtype=torch.int32, device=dev)
    fresh.disable_observer()
    fresh.enable_fake_quant()
    attn.value_post_act_fake_quantize = fresh
    assert attn.value_post_act_fake_quantize.scale.numel() == 32
    on, off = _on_off(switch, lambda: q(ids, mask, decoder_input_ids=dec)[0])
    assert len(calls) == 2 and all(c[2] for c in calls)          # the decoder's two blocks; the encoder's never reaches the op
    switch(True)
    with torch.no_grad():
        enc_on = q.get_encoder()(ids, attention_mask=mask)[0]
    switch(False)
    with torch.no_grad():
        enc_off = q.get_encoder()(ids, attention_mask=mask)[0]
    assert torch.equal(enc_on, enc_off)                          # the refused block: the eager words
    assert (on - off).abs().max().item() < FUSED_VS_EAGER_LOGITS

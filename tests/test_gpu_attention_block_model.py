"""The one-launch attention over whole sequences (util_layernorm.FUSE_ATTENTION, csrc/attention_block.hip) inside the
quantized models: (a) the tiny BERT-cls / BERT-QA / RoBERTa pipelines and the tiny BART pipeline of tests/test_gpu_model.py
and the reference's cached decode (tests/golden/bart_decode.npz) with the switch on, at the bars the eager form is held to;
(b) switch on against switch off on the tiny W6A6 LSQ+ BART of tests/test_gpu_bart_decode.py: a plain forward,
score(num_candidates=3) and generate(num_beams=3); (c) which calls take the one-launch form; (d) a head size the kernel
refuses falls back to the eager words."""
import copy

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
    """set_fast_attention, restored afterwards (the decode switch too: one test turns it on)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import outlier_suppression_amd as osq
    from outlier_suppression_amd import _hip, util_layernorm as UL
    _hip.load()                      # the first load applies the environment's tier, these switches included
    old = UL.FUSE_ATTENTION, UL.FUSE_DECODE_ATTENTION
    yield osq.set_fast_attention
    osq.set_fast_attention(old[0])
    osq.set_fast_decode_attention(old[1])


@pytest.fixture()
def calls(monkeypatch):
    """Every call of ops.attention_fake_quant, as (T, S, launched)."""
    from outlier_suppression_amd import ops
    seen = []
    real = ops.attention_fake_quant

    def counted(q, k, *a, **kw):
        out = real(q, k, *a, **kw)
        seen.append((q.shape[2], k.shape[2], out is not None))
        return out
    monkeypatch.setattr(ops, "attention_fake_quant", counted)
    return seen


# ------------------------------------------------------------------------------------------------ (a) the reference's bars

@pytest.mark.parametrize("kind", list(PIPELINES))
def test_a_bert_pipelines_with_the_switch_on(golden, switch, calls, kind):
    """tests/test_gpu_model.py::test_pipeline_matches_reference, default configuration, run as it stands with the switch on:
    PIPELINE_INTEGER_BARS on the integer tensors and its bars on the activation-quantized and fully quantized logits.  The
    block is launched by every pass whose quantizers only quantize; observer and autograd passes keep the eager sequence."""
    switch(True)
    test_gpu_model.test_pipeline_matches_reference(golden, kind, False)
    launched = [c for c in calls if c[2]]
    print(f"\n{kind}: {len(launched)} one-launch attention blocks, {len(calls) - len(launched)} refused")
    assert launched and len(launched) == len(calls)


def test_a_bart_pipeline_with_the_switch_on(golden, switch, calls):
    """tests/test_gpu_model.py::test_bart_pipeline_matches_reference with the switch on: INTEGER_BARS on the integer tensors,
    the activation-quantized logits within 0.1 (REFERENCE_LOGITS_BAR) of the reference's."""
    assert REFERENCE_LOGITS_BAR == 0.1 and INTEGER_BARS["worst"] == 5e-3
    switch(True)
    test_gpu_model.test_bart_pipeline_matches_reference(golden)
    launched = [c for c in calls if c[2]]
    # the activation-quantized pass: per batch 2 encoder blocks + 2 decoder layers x (self + cross)
    print(f"\ntiny BART pipeline: {len(launched)} one-launch attention blocks")
    assert launched and len(launched) % 6 == 0 and len(launched) == len(calls)


def test_a_reference_cached_decode_with_the_switch_on(golden, switch, calls):
    """The reference's cached greedy decode, teacher-forced with its tokens: the encoder's blocks take the one-launch form
    (the single-token decoder calls belong to the decode kernels); per-step logits at REFERENCE_LOGITS_BAR, the greedy token
    wherever the reference's margin exceeds it."""
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
    print(f"\none-launch encoder attention vs the reference's cached decode: max |logit diff| {err:.3g} over {steps} steps")
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
    print(f"\none-launch attention vs eager, plain forward: max |logit diff| {d:.3g}")
    assert len(calls) == 6 and all(c[2] for c in calls)
    assert d < FUSED_VS_EAGER_LOGITS, d
    assert torch.equal(on.argmax(-1), off.argmax(-1))


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
    print(f"\none-launch attention vs eager, score(num_candidates=3): max |logit diff| {d:.3g}, "
          f"max |token log-prob diff| {(on[0] - off[0]).abs().max().item():.3g}")
    assert len(calls) == 6 and all(c[2] for c in calls)
    assert d < FUSED_VS_EAGER_LOGITS, d
    assert torch.equal(logits[0].argmax(-1), logits[1].argmax(-1)) and torch.equal(on[2], off[2])


def test_b_generate_on_against_off(setup, switch, calls):
    s = setup
    on, off = _on_off(switch, lambda: s.q.generate(s.ids, attention_mask=s.mask, max_length=20, num_beams=3))
    assert calls and all(c[2] for c in calls)
    assert on.shape == off.shape and torch.equal(on, off), f"\non  {on.tolist()}\noff {off.tolist()}"


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
    del calls[:]
    with torch.enable_grad():                            # autograd on: eager
        forward()
    assert calls == []
    attn = s.q.model.encoder.layers[0].self_attn
    attn.dropout, attn.training = 0.1, True              # training dropout in one block: that block is eager
    try:
        with torch.no_grad():
            forward()
    finally:
        attn.dropout, attn.training = 0.0, False
    assert len(calls) == blocks - 1 and all(c[2] for c in calls)
    del calls[:]
    qz = attn.context_post_act_fake_quantize             # an observer on: that block is eager, nothing is launched for it
    saved = copy.deepcopy(qz.state_dict())
    qz.enable_observer()
    try:
        with torch.no_grad():
            forward()
    finally:
        qz.disable_observer()
        qz.load_state_dict(saved)
    assert len(calls) == blocks - 1 and all(c[2] for c in calls)
    # a cache: the first, multi-token call takes the block, the single-token steps the decode op
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


# ------------------------------------------------------------------------------------------------ (d) a refused head size

def test_d_refused_head_size_gives_the_eager_words(switch, calls):
    """head_dim 8: the library refuses, nothing is launched, the block runs the eager sequence: the words of the switch off."""
    from transformers import BartConfig, BartForConditionalGeneration
    from outlier_suppression_amd.quant_model import quantize_model
    from outlier_suppression_amd.quantization import disable_all, enable_calibration_woquantization, enable_quantization
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    cfg = BartConfig(vocab_size=120, d_model=32, encoder_layers=1, decoder_layers=1, encoder_attention_heads=4,
                     decoder_attention_heads=4, encoder_ffn_dim=64, decoder_ffn_dim=64, max_position_embeddings=40,
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
    on, off = _on_off(switch, lambda: q(ids, mask, decoder_input_ids=dec)[0])
    assert len(calls) == 3 and not any(c[2] for c in calls)
    assert torch.equal(on, off)

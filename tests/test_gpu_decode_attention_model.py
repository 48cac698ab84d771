"""The one-launch attention of a cached decoding step (util_layernorm.FUSE_DECODE_ATTENTION) inside quantized BART:
(a) the reference's cached greedy decode (tests/golden/bart_decode.npz) with the switch on, at the bars the eager form is
held to; (b) switch on against switch off on the tiny W6A6 LSQ+ BART of test_gpu_bart_decode.py over 12 teacher-forced
steps; (c) generate() with beams, on and off; (d) which calls take the one-launch form."""
import copy

import numpy as np
import pytest
import torch

from test_gpu_bart_decode import (FUSED_VS_EAGER_LOGITS, REFERENCE_LOGITS_BAR, _decode, _reference_pipeline,
                                  setup)  # noqa: F401  (setup: the module fixture of that file, instantiated for this one)
from test_gpu_model import INTEGER_BARS

pytestmark = pytest.mark.gpu


@pytest.fixture()
def fast_decode():
    from outlier_suppression_amd import _hip, set_fast_decode_attention, util_layernorm as UL
    _hip.load()                      # the first load applies the environment's tier, this switch included
    old = UL.FUSE_DECODE_ATTENTION
    set_fast_decode_attention(True)
    yield
    set_fast_decode_attention(old)


@pytest.fixture()
def calls(monkeypatch):
    """Every call of ops.decode_attention_fake_quant, as (kv_len, launched)."""
    from outlier_suppression_amd import ops
    seen = []
    real = ops.decode_attention_fake_quant

    def counted(q, k, *a, **kw):
        out = real(q, k, *a, **kw)
        seen.append((k.shape[2], out is not None))
        return out
    monkeypatch.setattr(ops, "decode_attention_fake_quant", counted)
    return seen


def test_a_reference_golden_with_the_switch_on(golden, fast_decode, calls):
    """test_gpu_bart_decode.py::test_a_cached_decode_against_reference with the one-launch attention: per-step logits at
    REFERENCE_LOGITS_BAR, the greedy token wherever the reference's margin exceeds it, the final layer-0 KV cache as
    integers at INTEGER_BARS."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from outlier_suppression_amd.quantization.fake_quant import QuantizeBase
    dev = torch.device("cuda:0")
    g = golden("bart_decode")
    model = _reference_pipeline(golden, dev)
    names = [n for n, m in model.named_modules() if isinstance(m, QuantizeBase)]
    assert names == [str(s) for s in g["q_names"]]
    ids, mask = torch.from_numpy(g["input_ids"]).to(dev), torch.from_numpy(g["attention_mask"]).to(dev)
    tokens = torch.from_numpy(g["tokens"]).to(dev)
    steps = g["step_logits"].shape[1]
    del calls[:]
    with torch.no_grad():
        out, cache, enc = model(ids, mask, decoder_input_ids=tokens[:, :1], use_cache=True)
        logits = [out[:, -1]]
        for t in range(1, steps):
            out, cache, _ = model(attention_mask=mask, decoder_input_ids=tokens[:, t:t + 1], encoder_outputs=(enc,),
                                  past_key_values=cache, use_cache=True)
            logits.append(out[:, -1])
    assert len(calls) == steps * 2 * len(cache) and all(launched for _, launched in calls)
    got = torch.stack(logits, 1).cpu().numpy()
    err = np.abs(got - g["step_logits"]).max()
    print(f"\none-launch decode attention vs the reference's cached decode: max |logit diff| {err:.3g} over {steps} steps")
    assert err < REFERENCE_LOGITS_BAR, err
    sure = g["margin"] > REFERENCE_LOGITS_BAR
    assert np.array_equal(got.argmax(-1)[sure], g["tokens"][:, 1:][sure])
    quantizers = dict((n, m) for n, m in model.named_modules() if isinstance(m, QuantizeBase))
    attn, cross = "model.decoder.layers.0.self_attn.", "model.decoder.layers.0.encoder_attn."
    fracs = []
    for j, (site, key) in enumerate(((attn + "key_post_act_fake_quantize", "k"), (attn + "value_post_act_fake_quantize", "v"),
                                     (cross + "key_post_act_fake_quantize", "cross_k"),
                                     (cross + "value_post_act_fake_quantize", "cross_v"))):
        i = names.index(site)
        q = quantizers[site]
        ours = cache[0][j].cpu().double().numpy()
        ref = g[f"cache_layer0_{key}"].astype(np.float64)
        assert ours.shape == ref.shape, (key, ours.shape, ref.shape)
        ia = np.rint(ours / q.scale.item() + q.zero_point.item())
        ib = np.rint(ref / g[f"q_scale::{i}"][0] + g[f"q_zp::{i}"][0])
        fracs.append((ia != ib).mean())
        assert np.abs(ia - ib).max() <= 1, key
    assert max(fracs) <= INTEGER_BARS["worst"], fracs


def test_b_switch_on_against_off(setup, fast_decode):
    """12 teacher-forced steps: max |logit difference| below FUSED_VS_EAGER_LOGITS (the project's bar for a one-launch form
    against the eager one), cache contents word-equal (the append launch is the same in both).
    Measured on MI355X: 0 (profiles/decode_attention_ab.txt)."""
    from outlier_suppression_amd import set_fast_decode_attention
    s = setup
    on_logits, on_cache = _decode(s.q, s)
    set_fast_decode_attention(False)
    off_logits, off_cache = _decode(s.q, s)
    d = (on_logits - off_logits).abs().max().item()
    print(f"\none-launch decode attention vs eager, max |logit diff| over 12 steps: {d:.3g}")
    assert d < FUSED_VS_EAGER_LOGITS, d
    for a, b in zip(on_cache, off_cache):
        for x, y in zip(a, b):
            assert torch.equal(x, y)


def test_c_generate_with_beams(setup):
    """generate(num_beams=3) gives the same token ids with the switch on and off; if not, the first differing step and the
    margin between its two best logits are reported (a flip needs a margin below FUSED_VS_EAGER_LOGITS)."""
    from outlier_suppression_amd import set_fast_decode_attention, util_layernorm as UL
    s = setup
    old = UL.FUSE_DECODE_ATTENTION
    try:
        with torch.no_grad():
            set_fast_decode_attention(True)
            on = s.q.generate(s.ids, attention_mask=s.mask, max_length=20, num_beams=3)
            set_fast_decode_attention(False)
            off = s.q.generate(s.ids, attention_mask=s.mask, max_length=20, num_beams=3)
    finally:
        set_fast_decode_attention(old)
    if on.shape != off.shape or not torch.equal(on, off):
        n = min(on.shape[1], off.shape[1])
        step = int((on[:, :n] != off[:, :n]).any(0).nonzero()[0]) if (on[:, :n] != off[:, :n]).any() else n
        row = int((on[:, :n] != off[:, :n])[:, step].nonzero()[0]) if step < n else 0
        with torch.no_grad():
            logits = s.q(s.ids[row:row + 1], s.mask[row:row + 1], decoder_input_ids=off[row:row + 1, :max(step, 1)])[0][0, -1]
        top = logits.topk(2).values
        pytest.fail(f"token ids differ first at step {step} (row {row}); margin of the two best logits there "
                    f"{(top[0] - top[1]).item():.3g}\non  {on.tolist()}\noff {off.tolist()}")


def _first_and_step(model, s):
    """Runs the first, multi-token call of a cache (3 tokens); returns the cache and a function that runs one single-token step."""
    with torch.no_grad():
        _, cache, enc = model(s.ids, s.mask, decoder_input_ids=s.dec[:, :3], use_cache=True)

    def step():
        return model(attention_mask=s.mask, decoder_input_ids=s.dec[:, 3:4], encoder_outputs=(enc,), past_key_values=cache,
                     use_cache=True)
    return cache, step


def test_d_dispatch(setup, calls):
    from outlier_suppression_amd import set_fast_decode_attention, util_layernorm as UL
    s = setup
    layers = len(s.q.model.decoder.layers)
    old = UL.FUSE_DECODE_ATTENTION
    try:
        # switch unset: nothing calls it
        set_fast_decode_attention(False)
        _, step = _first_and_step(s.q, s)
        with torch.no_grad():
            step()
        assert calls == []
        set_fast_decode_attention(True)
        # the first, multi-token call of a cache takes the eager path ...
        _, step = _first_and_step(s.q, s)
        assert calls == []
        # ... a cached step's self- and cross-attention blocks each call it once
        with torch.no_grad():
            step()
        assert len(calls) == 2 * layers and all(launched for _, launched in calls)
        assert sorted(n for n, _ in calls) == sorted([4] * layers + [s.ids.shape[1]] * layers)
        # under autograd: eager
        del calls[:]
        _, step = _first_and_step(s.q, s)
        with torch.enable_grad():
            step()
        assert calls == []
        # a quantizer with its observer on: that block is eager, the others are not
        attn = s.q.model.decoder.layers[0].self_attn
        qz = attn.context_post_act_fake_quantize
        saved = copy.deepcopy(qz.state_dict())
        _, step = _first_and_step(s.q, s)
        qz.enable_observer()
        try:
            with torch.no_grad():
                step()
        finally:
            qz.disable_observer()
            qz.load_state_dict(saved)
        assert len(calls) == 2 * layers - 1 and all(launched for _, launched in calls)
    finally:
        set_fast_decode_attention(old)

"""The KV cache as integer codes (QuantizedBartCache(codes=True), set_cache_codes) inside quantized BART, on the tiny W6A6
LSQ+ BART of test_gpu_bart_decode.py: with codes on and off the logits of 12 teacher-forced steps and the cache read as a
legacy tuple are WORD-equal, with the one-launch decode attention on (a) and off (b); generate() returns the same tokens,
greedy and with beams (c); against the reference's cached decode the coded cache is no further off than the fp32 one (d);
a step of another token count demotes the tensors it appends to (e); a fixed 8-bit configuration (f); the bytes held
(g); a NaN key makes generate() raise (h)."""
import copy
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from test_gpu_bart_decode import W_Q, _decode, _reference_pipeline, setup  # noqa: F401  (setup: that file's module fixture)

pytestmark = pytest.mark.gpu

NAMES = ("k", "v", "cross_k", "cross_v")


@pytest.fixture()
def switches():
    """Both switches as they were, after the test."""
    from outlier_suppression_amd import _hip, util_layernorm as UL
    _hip.load()                      # the first load applies the environment's tier, these switches included
    old = UL.FUSE_DECODE_ATTENTION, UL.CACHE_CODES
    yield UL
    UL.FUSE_DECODE_ATTENTION, UL.CACHE_CODES = old


def _decode_with(model, s, codes, attention, UL, steps=12):
    UL.FUSE_DECODE_ATTENTION, UL.CACHE_CODES = attention, codes
    logits, cache = _decode(model, s, steps)
    assert cache.codes is codes
    return logits, cache


def _same_words(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _assert_codes_equal_fp32(model, s, attention, UL):
    on_logits, on_cache = _decode_with(model, s, True, attention, UL)
    layers = len(on_cache)
    assert on_cache.coded() == [(i, n) for i in range(layers) for n in sorted(NAMES)] and on_cache.demoted() == []
    assert on_cache._k[0].dtype == torch.uint8 and on_cache._cross[0][1].dtype == torch.uint8
    off_logits, off_cache = _decode_with(model, s, False, attention, UL)
    assert off_cache.coded() == [] and off_cache._k[0].dtype == torch.float32
    assert _same_words(on_logits, off_logits)
    on_legacy, off_legacy = on_cache.to_legacy(), off_cache.to_legacy()
    assert len(on_legacy) == len(off_legacy) == layers
    for a, b in zip(on_legacy, off_legacy):
        assert len(a) == len(b) == 4
        for x, y in zip(a, b):
            assert x.dtype == torch.float32 and _same_words(x, y)
    for i in range(layers):
        for x, y in zip(on_cache.past(i), off_cache.past(i)):
            assert _same_words(x, y) and x.stride() == y.stride()
    assert on_cache.rejected() == 0
    return on_cache, off_cache


def test_a_word_equal_with_decode_attention_on(setup, switches, monkeypatch):
    from outlier_suppression_amd import ops
    taken = []
    real = ops.decode_attention_codes
    monkeypatch.setattr(ops, "decode_attention_codes", lambda *a, **kw: taken.append(1) or real(*a, **kw))
    on_cache, _ = _assert_codes_equal_fp32(setup.q, setup, True, switches)
    assert len(taken) == 12 * 2 * len(on_cache)        # every step's self- and cross-attention ran over the codes


def test_b_word_equal_with_decode_attention_off(setup, switches, monkeypatch):
    from outlier_suppression_amd import ops
    taken = []
    real = ops.decode_attention_codes
    monkeypatch.setattr(ops, "decode_attention_codes", lambda *a, **kw: taken.append(1) or real(*a, **kw))
    _assert_codes_equal_fp32(setup.q, setup, False, switches)
    assert taken == []                                  # the eager sequence on the dequantised buffers


@pytest.mark.parametrize("attention", [True, False])
@pytest.mark.parametrize("kw", [dict(num_beams=1, min_length=8), dict(num_beams=3)])
def test_c_generate_same_tokens(setup, switches, kw, attention):
    """The beam reorder runs on bytes (the partner buffer's prefix copy through the row index)."""
    s = setup
    switches.FUSE_DECODE_ATTENTION = attention
    with torch.no_grad():
        off = s.q.generate(s.ids, attention_mask=s.mask, max_length=20, cache_codes=False, **kw)
        on = s.q.generate(s.ids, attention_mask=s.mask, max_length=20, cache_codes=True, **kw)
        switches.CACHE_CODES = True
        by_switch = s.q.generate(s.ids, attention_mask=s.mask, max_length=20, **kw)
    assert torch.equal(on, off), (on, off)
    assert torch.equal(by_switch, off)


def test_d_against_the_reference_decode(golden, switches):
    """tests/golden/bart_decode.npz: the coded cache's logits are no further from the reference's than the fp32 cache's,
    measured here in the same test (they are the same words)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    dev = torch.device("cuda:0")
    g = golden("bart_decode")
    model = _reference_pipeline(golden, dev)
    ids, mask = torch.from_numpy(g["input_ids"]).to(dev), torch.from_numpy(g["attention_mask"]).to(dev)
    tokens = torch.from_numpy(g["tokens"]).to(dev)
    steps = g["step_logits"].shape[1]
    s = NS(ids=ids, mask=mask, dec=tokens)
    errs = {}
    for codes in (False, True):
        logits, cache = _decode_with(model, s, codes, True, switches, steps)
        assert bool(cache.coded()) is codes
        errs[codes] = float(np.abs(logits.cpu().numpy() - g["step_logits"]).max())
    print(f"\nmax |logit - reference| over {steps} steps: fp32 cache {errs[False]:.6g}, coded cache {errs[True]:.6g}")
    assert errs[True] <= errs[False], errs


def test_e_another_token_count_demotes(setup, switches):
    """A first step of 3 tokens, then single-token steps: the LSQ+ grad factor of the self-attention key / value sites
    changes with the token count, so the second step demotes those tensors (one dequantise launch each) and the cache goes
    on in fp32 for them; the cross-attention tensors stay coded.  Logits word-equal to the fp32 cache throughout."""
    s, UL = setup, switches
    UL.FUSE_DECODE_ATTENTION = True
    runs = {}
    for codes in (True, False):
        UL.CACHE_CODES = codes
        with torch.no_grad():
            out, cache, enc = s.q(s.ids, s.mask, decoder_input_ids=s.dec[:, :3], use_cache=True)
            logits = [out]
            if codes:
                assert cache.coded() == [(i, n) for i in range(len(cache)) for n in sorted(NAMES)] and cache.demoted() == []
            for t in range(3, 7):
                out, cache, _ = s.q(attention_mask=s.mask, decoder_input_ids=s.dec[:, t:t + 1], encoder_outputs=(enc,),
                                    past_key_values=cache, use_cache=True)
                logits.append(out)
        runs[codes] = (torch.cat(logits, 1), cache)
    coded, plain = runs[True][1], runs[False][1]
    layers = len(coded)
    assert coded.demoted() == [(i, n) for i in range(layers) for n in ("k", "v")]
    assert coded.coded() == [(i, n) for i in range(layers) for n in ("cross_k", "cross_v")]
    assert coded._k[0].dtype == torch.float32 and coded._cross[0][0].dtype == torch.uint8
    assert _same_words(runs[True][0], runs[False][0])
    for a, b in zip(coded.to_legacy(), plain.to_legacy()):
        for x, y in zip(a, b):
            assert _same_words(x, y)
    assert coded.rejected() == 0


@pytest.fixture(scope="module")
def fixed8(setup):
    """The tiny BART with fixed (not learnable) asymmetric 8-bit activation quantizers: codes 0..255, the full byte."""
    from outlier_suppression_amd.quant_model import quantize_model
    from outlier_suppression_amd.quantization import disable_all, enable_calibration_woquantization, enable_quantization
    s = setup
    a_q = NS(quantizer="FixedFakeQuantize", observer="AvgMinMaxObserver", bit=8, symmetric=False, ch_axis=-1)
    q = quantize_model(copy.deepcopy(s.fp), W_Q, a_q).to(s.dev).eval()
    enable_calibration_woquantization(q)
    with torch.no_grad():
        q(s.ids, s.mask, decoder_input_ids=s.dec)
    disable_all(q)
    enable_quantization(q)
    return q


def test_f_fixed_8bit(setup, fixed8, switches):
    attn = fixed8.model.decoder.layers[0].self_attn.key_post_act_fake_quantize
    assert (attn.quant_min, attn.quant_max) == (0, 255) and attn.zero_point.dtype == torch.int32
    _assert_codes_equal_fp32(fixed8, setup, True, switches)


def test_g_bytes_held(setup, switches):
    """Every tensor of this model qualifies, so the coded cache holds exactly a quarter of the fp32 cache's bytes plus its
    records (two floats per tensor slot) and the counter; after a demotion the demoted tensors count as fp32."""
    on_cache, off_cache = _assert_codes_equal_fp32(setup.q, setup, True, switches)
    layers = len(on_cache)
    extra = layers * 4 * 2 * 4 + 4
    print(f"\ncache.nbytes(): fp32 {off_cache.nbytes()}, codes {on_cache.nbytes()} (records and counter {extra})")
    assert on_cache.coded() == [(i, n) for i in range(layers) for n in sorted(NAMES)]      # none stayed fp32
    assert off_cache.nbytes() % 4 == 0
    assert on_cache.nbytes() <= off_cache.nbytes() // 4 + extra
    assert on_cache.nbytes() == off_cache.nbytes() // 4 + extra
    # demote one tensor by hand: its buffer counts four bytes per element again, its partner buffer is dropped
    before = on_cache.nbytes()
    k = on_cache._k[1]
    spare = on_cache._spare[1][0]
    on_cache.demote(1, "k")
    assert on_cache.demoted() == [(1, "k")] and (1, "k") not in on_cache.coded()
    assert on_cache._k[1].dtype == torch.float32 and on_cache._k[1].shape == k.shape
    assert on_cache.nbytes() == before + 3 * k.numel() - (spare.numel() if spare is not None else 0)
    for x, y in zip(on_cache.to_legacy(), off_cache.to_legacy()):
        for a, b in zip(x, y):
            assert _same_words(a, b)


def test_h_nan_key_makes_generate_raise(setup, switches):
    s = setup
    k_proj = s.q.model.decoder.layers[1].self_attn.k_proj

    def plant(module, args, out):
        out = out.clone()
        out[0, 0, 5] = float("nan")
        return out
    handle = k_proj.register_forward_hook(plant)
    try:
        with torch.no_grad():
            s.q.generate(s.ids, attention_mask=s.mask, max_length=6, num_beams=1, min_length=6, cache_codes=False)
            with pytest.raises(RuntimeError, match=r"holds \d+ elements without an integer code"):
                s.q.generate(s.ids, attention_mask=s.mask, max_length=6, num_beams=1, min_length=6, cache_codes=True)
    finally:
        handle.remove()

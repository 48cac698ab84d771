"""CPU: incremental decoding of the quantized BART wrapper with every quantizer off (a plain FP model, so it runs on the
CPU): the default forward keeps its return value, the cached forward returns the reference's order, the cache reads as
the reference's tuples, ``_reorder_cache`` / ``prepare_inputs_for_generation`` match the reference's classes, and
``generate`` is token-equal to transformers' FP ``generate``.  The quantized decode runs on the GPU
(tests/test_gpu_bart_decode.py)."""
import copy
import os
import sys
import types
from types import SimpleNamespace as NS

import pytest
import torch

REF = "/root/reference"
W_Q = NS(quantizer="FixedFakeQuantize", observer="MinMaxObserver", bit=6, symmetric=True, ch_axis=0)
A_Q = NS(quantizer="LSQPlusFakeQuantize", observer="AvgPruneMinMaxObserver", bit=6, symmetric=False, ch_axis=-1)


def tiny_bart(seed=0, **extra):
    from transformers import BartConfig, BartForConditionalGeneration
    torch.manual_seed(seed)
    cfg = BartConfig(vocab_size=120, d_model=32, encoder_layers=2, decoder_layers=2, encoder_attention_heads=2,
                     decoder_attention_heads=2, encoder_ffn_dim=64, decoder_ffn_dim=64, max_position_embeddings=64,
                     dropout=0.0, attention_dropout=0.0, activation_dropout=0.0, pad_token_id=1, bos_token_id=0,
                     eos_token_id=2, decoder_start_token_id=2, **extra)
    return BartForConditionalGeneration(cfg).eval()


def wrapped(fp, **kw):
    from outlier_suppression_amd.quant_model import quantize_model
    from outlier_suppression_amd.quantization import disable_all
    q = quantize_model(copy.deepcopy(fp), W_Q, A_Q, **kw).eval()
    disable_all(q)
    return q


def batch(seed=1, b=3, s=10):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(3, 120, (b, s), generator=g)
    mask = torch.ones_like(ids)
    mask[1, s - 3:] = 0
    return ids * mask + (1 - mask), mask


@pytest.fixture(scope="module")
def model():
    fp = tiny_bart()
    return fp, wrapped(fp)


def test_default_forward_unchanged(model):
    from outlier_suppression_amd.model.quant_bart import QuantizedBartCache
    _, q = model
    ids, mask = batch()
    with torch.no_grad():
        out = q(ids, mask, decoder_input_ids=ids[:, :5])
        off = q(ids, mask, decoder_input_ids=ids[:, :5], use_cache=False)
    assert len(out) == 2 and len(off) == 2
    assert not any(isinstance(o, QuantizedBartCache) for o in out)
    assert out[0].shape == (3, 5, 120) and out[1].shape == (3, 10, 32)
    assert torch.equal(out[0], off[0]) and torch.equal(out[1], off[1])


def test_return_order_with_cache_and_labels(model):
    from outlier_suppression_amd.model.quant_bart import QuantizedBartCache
    _, q = model
    ids, mask = batch()
    with torch.no_grad():
        logits, cache, enc = q(ids, mask, decoder_input_ids=ids[:, :4], use_cache=True)
        plain = q(ids, mask, decoder_input_ids=ids[:, :4])
        with_labels = q(ids, mask, labels=ids[:, :4].contiguous(), use_cache=True)
    assert isinstance(cache, QuantizedBartCache) and len(cache) == 2
    assert torch.equal(logits, plain[0]) and torch.equal(enc, plain[1])
    k, v, ck, cv = cache[0]
    assert k.shape == (3, 2, 4, 16) and v.shape == k.shape and ck.shape == (3, 2, 10, 16)
    assert cache[0][0].shape[2] == 4                            # quant_bart.py:774 reads the past length there
    assert len(with_labels) == 3 and with_labels[0].dim() == 0  # (loss, logits, enc): labels turn the cache off
    assert not isinstance(with_labels[2], QuantizedBartCache)


def test_cached_steps_equal_uncached_prefix(model):
    """FP: the logits of a step through the cache equal the last position of an uncached forward over the prefix."""
    _, q = model
    ids, mask = batch()
    dec = torch.randint(3, 120, (3, 8), generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        logits, cache, enc = q(ids, mask, decoder_input_ids=dec[:, :1], use_cache=True)
        for t in range(1, 8):
            full = q(ids, mask, decoder_input_ids=dec[:, :t + 1])[0][:, -1]
            logits, cache2, _ = q(attention_mask=mask, decoder_input_ids=dec[:, t:t + 1], encoder_outputs=(enc,),
                                  past_key_values=cache, use_cache=True)
            assert cache2 is cache and cache.get_seq_length() == t + 1
            assert (logits[:, -1] - full).abs().max().item() < 1e-4
        # a plain tuple of tensors (the reference's form) is accepted and gives the same next step
        legacy = tuple(tuple(t.clone() for t in layer) for layer in cache)
        a = q(attention_mask=mask, decoder_input_ids=dec[:, :1], encoder_outputs=(enc,), past_key_values=legacy,
              use_cache=True)[0]
        b = q(attention_mask=mask, decoder_input_ids=dec[:, :1], encoder_outputs=(enc,), past_key_values=cache,
              use_cache=True)[0]
    assert torch.equal(a, b)


def test_reorder_is_lazy_and_matches_index_select(model):
    from outlier_suppression_amd.model.quant_bart import QuantizedBartForConditionalGeneration as QB
    _, q = model
    ids, mask = batch()
    with torch.no_grad():
        _, cache, _ = q(ids, mask, decoder_input_ids=ids[:, :3], use_cache=True)
    before = tuple(tuple(t.clone() for t in layer) for layer in cache)
    idx = torch.tensor([2, 2, 0])
    want = QB._reorder_cache(before, idx)
    assert QB._reorder_cache(cache, idx) is cache
    assert cache._rows[0] is not None                         # recorded, not yet applied
    for got_layer, want_layer in zip(cache, want):
        for g, w in zip(got_layer, want_layer):
            assert torch.equal(g, w)


@pytest.mark.parametrize("kw", [dict(num_beams=1, min_length=6), dict(num_beams=4), dict(num_beams=6),
                                dict(num_beams=1, no_repeat_ngram_size=2, min_length=8, forced_bos_token_id=0),
                                dict(num_beams=4, no_repeat_ngram_size=3, min_length=5, forced_bos_token_id=0),
                                dict(num_beams=6, num_return_sequences=3, length_penalty=2.0, early_stopping=True),
                                dict(num_beams=4, early_stopping="never", length_penalty=0.5)])
def test_generate_matches_transformers_fp(model, kw):
    fp, q = model
    ids, mask = batch()
    with torch.no_grad():
        ref = fp.generate(ids, attention_mask=mask, max_length=16, **kw)
        got = q.generate(ids, attention_mask=mask, max_length=16, **kw)
        uncached = q.generate(ids, attention_mask=mask, max_length=16, use_cache=False, **kw)
    assert torch.equal(got, ref), (got, ref)
    assert torch.equal(uncached, ref)


def test_generate_refuses_sampling(model):
    _, q = model
    ids, mask = batch()
    with pytest.raises(NotImplementedError):
        q.generate(ids, attention_mask=mask, do_sample=True)


def test_generate_takes_trainer_arguments(model):
    """Seq2SeqTrainer's predict_with_generate passes synced_gpus=False; True is refused."""
    fp, q = model
    ids, mask = batch()
    with torch.no_grad():
        got = q.generate(ids, attention_mask=mask, max_length=12, num_beams=4, synced_gpus=False)
        assert torch.equal(got, fp.generate(ids, attention_mask=mask, max_length=12, num_beams=4))
    with pytest.raises(NotImplementedError):
        q.generate(ids, attention_mask=mask, synced_gpus=True)


@pytest.fixture(scope="module")
def ref_bart():
    if not os.path.isdir(REF):
        pytest.skip("reference tree not available")
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_golden_model as M
    M.import_reference()
    gu = types.ModuleType("transformers.generation_utils")
    from transformers.generation import GenerationMixin
    gu.GenerationMixin = GenerationMixin
    sys.modules["transformers.generation_utils"] = gu
    from quant_transformer.model import quant_bart as RB
    return RB


def test_reorder_cache_and_prepare_inputs_match_reference(ref_bart, model):
    from outlier_suppression_amd.model.quant_bart import QuantizedBartForConditionalGeneration as QB
    RB = ref_bart.QuantizedBartForConditionalGeneration
    _, q = model
    ids, mask = batch()
    with torch.no_grad():
        _, cache, enc = q(ids, mask, decoder_input_ids=ids[:, :3], use_cache=True)
    past = tuple(tuple(t.clone() for t in layer) for layer in cache)
    idx = torch.tensor([1, 0, 1])
    for a, b in zip(QB._reorder_cache(past, idx), RB._reorder_cache(past, idx)):
        assert len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))
    for a, b in zip(QB._reorder_cache(cache, idx), RB._reorder_cache(past, idx)):
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    for p in (None, past):
        kw = dict(past=p, attention_mask=mask, use_cache=True, encoder_outputs=(enc,))
        ours = q.prepare_inputs_for_generation(ids[:, :3], **kw)
        theirs = RB.prepare_inputs_for_generation(None, ids[:, :3], **kw)
        assert ours.keys() == theirs.keys()
        assert torch.equal(ours["decoder_input_ids"], theirs["decoder_input_ids"])

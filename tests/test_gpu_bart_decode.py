"""Incremental decoding of the quantized BART wrapper on the GPU, decoded step by step through QuantizedBartCache.

(a) the reference's quantized tiny BART, decoded through its own KV cache (tests/golden/bart_decode.npz), against this
package's run of the same pipeline; then, on a tiny BART calibrated here to W6A6 (LSQ+ activations): (b) cached steps
against the uncached forward over the same prefix (FP and quantized); (c) the one-launch append path
against the eager cat path (util_layernorm.FUSE_KV_APPEND): cache contents word-equal, logits within a measured bar;
(d) generate() with every quantizer off against transformers' FP generate; (e) quantized generate with and without the
cache; and the reference driver's call ``generate(input_ids, attention_mask=..., max_length=62, num_beams=6)``."""
import copy
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from test_gpu_model import INTEGER_BARS, integer_tensor_report

pytestmark = pytest.mark.gpu

W_Q = NS(quantizer="FixedFakeQuantize", observer="MinMaxObserver", bit=6, symmetric=True, ch_axis=0)
A_Q = NS(quantizer="LSQPlusFakeQuantize", observer="AvgMinMaxObserver", bit=6, symmetric=False, ch_axis=-1)
# max |logit(one-launch path) - logit(eager path)| over 12 steps: measured 0 on MI355X (profiles/decode_step_ab.txt).  The
# bar is headroom for a batched matmul over the strided cache view choosing another GEMM kernel than over a dense tensor.
FUSED_VS_EAGER_LOGITS = 1e-4
# the bar test_gpu_model.py::test_bart_pipeline_matches_reference puts on the activation-quantized logits of this model
REFERENCE_LOGITS_BAR = 0.1
# the quantizers of bart_tiny_pipeline.npz / bart_decode.npz (make_golden_model.main_bart)
REF_W_Q = NS(quantizer="FixedFakeQuantize", observer="MinMaxObserver", bit=6, symmetric=True, ch_axis=0)
REF_A_Q = NS(quantizer="LSQPlusFakeQuantize", observer="AvgPruneMinMaxObserver", bit=6, symmetric=False, ch_axis=-1)


def _reference_pipeline(golden, dev):
    """The pipeline of test_bart_pipeline_matches_reference (wrap -> gamma migration -> weight calibration -> one
    observer pass at percentile 0.9 -> activation quantization) on the weights and batches of bart_tiny_pipeline.npz."""
    from transformers import BartConfig, BartForConditionalGeneration
    from outlier_suppression_amd import token_wise_clipping as TWC
    from outlier_suppression_amd.gamma_migration import delay_ln
    from outlier_suppression_amd.quant_model import quantize_model
    from outlier_suppression_amd.quantization import disable_all, enable_calibration_woquantization
    from outlier_suppression_amd.quantization.state import set_observer_name
    g = golden("bart_tiny_pipeline")
    cfg = BartConfig(vocab_size=120, d_model=32, encoder_layers=2, decoder_layers=2, encoder_attention_heads=2,
                     decoder_attention_heads=2, encoder_ffn_dim=64, decoder_ffn_dim=64, max_position_embeddings=40,
                     dropout=0.0, attention_dropout=0.0, activation_dropout=0.0, pad_token_id=1, bos_token_id=0,
                     eos_token_id=2, decoder_start_token_id=2)
    fp = BartForConditionalGeneration(cfg).eval()
    fp.load_state_dict({k[4:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd::")}, strict=False)
    batches = [{k: torch.from_numpy(g[k][b]).to(dev) for k in ("input_ids", "attention_mask", "decoder_input_ids",
                                                               "decoder_attention_mask")} for b in range(3)]
    model = quantize_model(fp.to(dev), REF_W_Q, REF_A_Q).to(dev)
    model = delay_ln(model, NS(a_qconfig=REF_A_Q, w_qconfig=REF_W_Q), NS(model_type="bart", task_type="summ"))
    enable_calibration_woquantization(model, quantizer_type="weight_fake_quant")
    with torch.no_grad():
        model(**batches[0])
    disable_all(model)
    set_observer_name(model)
    TWC.set_ratio(model, 0.9)
    with torch.no_grad():
        for b in batches:
            model(**b)
    TWC.enable_quantization(model)
    return model.eval()


def test_a_cached_decode_against_reference(golden):
    """The reference's cached greedy decode (its own past_key_values) against ours, teacher-forced with its tokens:
    per-step logits at the pipeline bar, the greedy token wherever the reference's margin exceeds the bar, and the final
    layer-0 KV cache as integers (INTEGER_BARS)."""
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
    with torch.no_grad():
        out, cache, enc = model(ids, mask, decoder_input_ids=tokens[:, :1], use_cache=True)
        logits = [out[:, -1]]
        for t in range(1, steps):
            out, cache, _ = model(attention_mask=mask, decoder_input_ids=tokens[:, t:t + 1], encoder_outputs=(enc,),
                                  past_key_values=cache, use_cache=True)
            logits.append(out[:, -1])
    got = torch.stack(logits, 1).cpu().numpy()
    err = np.abs(got - g["step_logits"]).max()
    print(f"\ncached decode vs the reference's cached decode: max |logit diff| {err:.3g} over {steps} steps")
    assert err < REFERENCE_LOGITS_BAR, err
    sure = g["margin"] > REFERENCE_LOGITS_BAR
    assert np.array_equal(got.argmax(-1)[sure], g["tokens"][:, 1:][sure])
    # the final layer-0 cache: integer entries under each run's own parameters
    quantizers = dict((n, m) for n, m in model.named_modules() if isinstance(m, QuantizeBase))
    attn = "model.decoder.layers.0.self_attn."
    cross = "model.decoder.layers.0.encoder_attn."
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
    # the same quantizers through the integer-tensor report of the model tests, on the decoded sequence
    sites = [n for n in names if n.startswith(attn) or n.startswith(cross)]
    idx = [names.index(n) for n in sites]
    rows = integer_tensor_report(model, {"input_ids": ids, "attention_mask": mask, "decoder_input_ids": tokens[:, :steps]},
                                 sites, [g[f"q_scale::{i}"] for i in idx], [g[f"q_zp::{i}"] for i in idx])
    frac = np.array([r[1] for r in rows])
    assert len(rows) == len(sites)
    assert (frac == 0).mean() >= INTEGER_BARS["identical_quantizers"], frac
    assert np.median(frac) <= INTEGER_BARS["median"] and frac.max() <= INTEGER_BARS["worst"], frac


@pytest.fixture(scope="module")
def setup():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from transformers import BartConfig, BartForConditionalGeneration
    from outlier_suppression_amd.quant_model import quantize_model
    from outlier_suppression_amd.quantization import disable_all, enable_calibration_woquantization, enable_quantization
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    cfg = BartConfig(vocab_size=120, d_model=64, encoder_layers=2, decoder_layers=2, encoder_attention_heads=4,
                     decoder_attention_heads=4, encoder_ffn_dim=128, decoder_ffn_dim=128, max_position_embeddings=80,
                     dropout=0.0, attention_dropout=0.0, activation_dropout=0.0, pad_token_id=1, bos_token_id=0,
                     eos_token_id=2, decoder_start_token_id=2)
    fp = BartForConditionalGeneration(cfg).eval().to(dev)
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(3, 120, (3, 14), generator=g)
    mask = torch.ones_like(ids)
    mask[1, 10:] = 0
    ids = (ids * mask + (1 - mask)).to(dev)
    mask = mask.to(dev)
    dec = torch.randint(3, 120, (3, 12), generator=g).to(dev)
    fq = quantize_model(copy.deepcopy(fp), W_Q, A_Q).to(dev).eval()
    disable_all(fq)
    q = quantize_model(copy.deepcopy(fp), W_Q, A_Q).to(dev).eval()
    enable_calibration_woquantization(q)
    with torch.no_grad():
        q(ids, mask, decoder_input_ids=dec)
    disable_all(q)
    enable_quantization(q)
    return NS(fp=fp, fq=fq, q=q, ids=ids, mask=mask, dec=dec, dev=dev)


def _decode(model, s, steps=12):
    """Teacher-forced step-by-step decode through the cache: per-step last-position logits and the cache."""
    with torch.no_grad():
        out, cache, enc = model(s.ids, s.mask, decoder_input_ids=s.dec[:, :1], use_cache=True)
        logits = [out[:, -1]]
        for t in range(1, steps):
            out, cache, _ = model(attention_mask=s.mask, decoder_input_ids=s.dec[:, t:t + 1], encoder_outputs=(enc,),
                                  past_key_values=cache, use_cache=True)
            logits.append(out[:, -1])
    return torch.stack(logits, 1), cache


def _uncached(model, s, steps=12):
    with torch.no_grad():
        return torch.stack([model(s.ids, s.mask, decoder_input_ids=s.dec[:, :t + 1])[0][:, -1] for t in range(steps)], 1)


def test_b_cached_against_uncached(setup):
    s = setup
    got, _ = _decode(s.fq, s)
    assert (got - _uncached(s.fq, s)).abs().max().item() < 1e-4
    got, cache = _decode(s.q, s)
    want = _uncached(s.q, s)
    assert torch.equal(got.argmax(-1), want.argmax(-1))
    # the cache built step by step against the cache of one forward over the whole prefix: at most one quantization step
    with torch.no_grad():
        _, whole, _ = s.q(s.ids, s.mask, decoder_input_ids=s.dec, use_cache=True)
    for i in range(len(cache)):
        attn = s.q.model.decoder.layers[i].self_attn
        for j, qz in enumerate((attn.key_post_act_fake_quantize, attn.value_post_act_fake_quantize)):
            diff = (cache[i][j] - whole[i][j]).abs().max().item()
            assert diff <= qz.scale.abs().item() * (1 + 1e-5), (i, j, diff)


def test_c_one_launch_against_eager(setup):
    from outlier_suppression_amd import util_layernorm as UL
    s = setup
    fused_logits, fused_cache = _decode(s.q, s)
    UL.FUSE_KV_APPEND = False
    try:
        eager_logits, eager_cache = _decode(s.q, s)
    finally:
        UL.FUSE_KV_APPEND = True
    for a, b in zip(fused_cache, eager_cache):
        for x, y in zip(a, b):
            assert torch.equal(x, y)
    d = (fused_logits - eager_logits).abs().max().item()
    print(f"\none-launch vs eager decode, max |logit diff| over 12 steps: {d:.3g}")
    assert d <= FUSED_VS_EAGER_LOGITS, d


@pytest.mark.parametrize("kw", [dict(num_beams=1, min_length=8), dict(num_beams=4), dict(num_beams=6),
                                dict(num_beams=1, no_repeat_ngram_size=2, min_length=10, forced_bos_token_id=0),
                                dict(num_beams=4, no_repeat_ngram_size=3, min_length=6, forced_bos_token_id=0),
                                dict(num_beams=6, no_repeat_ngram_size=3, num_return_sequences=2)])
def test_d_generate_matches_transformers(setup, kw):
    s = setup
    with torch.no_grad():
        ref = s.fp.generate(s.ids, attention_mask=s.mask, max_length=20, **kw)
        got = s.fq.generate(s.ids, attention_mask=s.mask, max_length=20, **kw)
    assert torch.equal(got, ref), (got, ref)


@pytest.mark.parametrize("kw", [dict(num_beams=1, min_length=8), dict(num_beams=4, no_repeat_ngram_size=3)])
def test_e_quantized_generate_cache_on_off(setup, kw):
    s = setup
    with torch.no_grad():
        a = s.q.generate(s.ids, attention_mask=s.mask, max_length=20, **kw)
        b = s.q.generate(s.ids, attention_mask=s.mask, max_length=20, use_cache=False, **kw)
    assert torch.equal(a, b), (a, b)


def test_reference_driver_call(setup):
    """ptq_summ_quant.prepare_input_output's call on the quantized wrapper."""
    s = setup
    with torch.no_grad():
        out = s.q.generate(s.ids, attention_mask=s.mask, max_length=62, num_beams=6)
    assert out.dtype == torch.long and out.shape[0] == 3 and 1 < out.shape[1] <= 62
    assert bool((out[:, 0] == 2).all())

"""One copy of the cross-attention keys / values per batch row inside quantized BART (generate(share_cross_kv=True),
QuantizedBartCache(cross_group=...), util_layernorm.decode_attention_shared_fake_quant) on the tiny W6A6 LSQ+ BART of
test_gpu_bart_decode.py: (a) beam search returns the tokens of the unshared one-launch form under every combination of graph,
beam_graph and cache_codes, also with more beams than one workgroup serves; (b) 12 teacher-forced steps against the unshared
form; (c) the stored cross keys / values are the unshared form's words (codes: bytes and records); (d) the cache's shapes and
bytes; (e) what last_share_cross_kv reports and when it falls back; (f) a multi-token call over a shared cache."""
import itertools

import pytest
import torch

from test_gpu_bart_decode import FUSED_VS_EAGER_LOGITS, setup  # noqa: F401  (setup: that file's module fixture, instantiated here)

pytestmark = pytest.mark.gpu

G = 3


@pytest.fixture()
def fast_decode():
    from outlier_suppression_amd import _hip, set_fast_decode_attention, util_layernorm as UL
    _hip.load()                      # the first load applies the environment's tier, this switch included
    old = UL.FUSE_DECODE_ATTENTION
    set_fast_decode_attention(True)
    yield
    set_fast_decode_attention(old)


def _report_mismatch(s, shared, plain, nb, what):
    """The first differing step and the margin between its two best logits there (a flip needs a margin below
    FUSED_VS_EAGER_LOGITS), as test_gpu_decode_attention_model.py::test_c_generate_with_beams reports it."""
    n = min(shared.shape[1], plain.shape[1])
    differ = shared[:, :n] != plain[:, :n]
    step = int(differ.any(0).nonzero()[0]) if differ.any() else n
    row = int(differ[:, step].nonzero()[0]) if step < n else 0
    src = row // (shared.shape[0] // s.ids.shape[0])
    with torch.no_grad():
        logits = s.q(s.ids[src:src + 1], s.mask[src:src + 1], decoder_input_ids=plain[row:row + 1, :max(step, 1)])[0][0, -1]
    top = logits.topk(2).values
    pytest.fail(f"{what}, num_beams={nb}: token ids differ first at step {step} (row {row}); margin of the two best logits "
                f"there {(top[0] - top[1]).item():.3g}\nshared   {shared.tolist()}\nunshared {plain.tolist()}")


@pytest.mark.parametrize("graph,beam_graph,codes", list(itertools.product([False, True], repeat=3)),
                         ids=lambda v: "on" if v else "off")
def test_a_tokens(setup, fast_decode, graph, beam_graph, codes):
    """generate(num_beams=3, share_cross_kv=True) against the same call without sharing, the one-launch attention on in both."""
    s = setup
    kw = dict(attention_mask=s.mask, max_length=20, num_beams=3, graph=graph, beam_graph=beam_graph, cache_codes=codes)
    plain = s.q.generate(s.ids, **kw)
    assert s.q.last_share_cross_kv.reason == "not asked for" and s.q.last_share_cross_kv.shared == 0
    graphs = repr(s.q.last_decode_graph), repr(s.q.last_beam_graph)
    shared = s.q.generate(s.ids, share_cross_kv=True, **kw)
    info = s.q.last_share_cross_kv
    assert info.reason is None and info.eager == 0 and info.shared >= 1, info
    assert (repr(s.q.last_decode_graph), repr(s.q.last_beam_graph)) == graphs       # sharing changes nothing about the graphs
    if graph:
        assert s.q.last_decode_graph.reason is None, s.q.last_decode_graph
    if shared.shape != plain.shape or not torch.equal(shared, plain):
        _report_mismatch(s, shared, plain, 3, f"graph={graph} beam_graph={beam_graph} cache_codes={codes}")


@pytest.mark.parametrize("kw", [dict(), dict(beam_select=True, beam_advance=True), dict(graph=True, cache_codes=True)],
                         ids=["plain", "select+advance", "graph+codes"])
def test_a_tokens_more_beams_than_a_workgroup_serves(setup, fast_decode, kw):
    """num_beams=9: the group exceeds the 8 query rows of one workgroup, a second chunk of one row."""
    s = setup
    kw = dict(attention_mask=s.mask, max_length=20, num_beams=9, **kw)
    plain = s.q.generate(s.ids, **kw)
    shared = s.q.generate(s.ids, share_cross_kv=True, **kw)
    assert s.q.last_share_cross_kv.reason is None and s.q.last_share_cross_kv.eager == 0
    if shared.shape != plain.shape or not torch.equal(shared, plain):
        _report_mismatch(s, shared, plain, 9, str(kw))


def _beam_tokens(s, steps=12):
    g = torch.Generator().manual_seed(5)
    return torch.randint(3, 120, (s.ids.shape[0] * G, steps), generator=g).to(s.dev)


def _decode(s, dec, share, codes=False, first=1):
    """Teacher-forced decode of G decoder rows per input through the cache: the first call takes ``first`` tokens, then one
    token per step.  ``share``: the encoder states and mask stay at one row per input, over a cache with cross_group=G."""
    from outlier_suppression_amd.model.quant_bart import QuantizedBartCache
    model = s.q
    layers = len(model.model.decoder.layers)
    with torch.no_grad():
        enc = model.get_encoder()(s.ids, attention_mask=s.mask)
        mask = s.mask
        if not share:
            enc, mask = enc.repeat_interleave(G, 0), mask.repeat_interleave(G, 0)
        cache = QuantizedBartCache(layers, capacity=dec.shape[1], codes=codes, cross_group=G if share else 1)
        logits = []
        for a, b in [(0, first)] + [(t, t + 1) for t in range(first, dec.shape[1])]:
            out, cache_out, _ = model(attention_mask=mask, decoder_input_ids=dec[:, a:b], encoder_outputs=(enc,),
                                      past_key_values=cache, use_cache=True)
            assert cache_out is cache
            logits.append(out)
    return torch.cat(logits, 1), cache


@pytest.mark.parametrize("codes", [False, True], ids=["fp32", "codes"])
def test_b_logits_teacher_forced(setup, fast_decode, codes):
    """12 steps with a cross_group=3 cache against the unshared one-launch form.  The attention kernel is word-equal, but
    rocBLAS may order the three times smaller K / V projection differently, so the bar is the project's
    FUSED_VS_EAGER_LOGITS, not zero.  Measured on MI355X: 0 with either cache format (profiles/share_cross_kv_ab.txt)."""
    s = setup
    dec = _beam_tokens(s)
    got, _ = _decode(s, dec, True, codes)
    want, _ = _decode(s, dec, False, codes)
    d = (got - want).abs().max().item()
    print(f"\nshared vs unshared cross K/V ({'codes' if codes else 'fp32'}), max |logit diff| over 12 steps: {d:.3g}")
    assert d < FUSED_VS_EAGER_LOGITS, d


@pytest.mark.parametrize("codes", [False, True], ids=["fp32", "codes"])
def test_c_stored_words(setup, fast_decode, codes, monkeypatch):
    """The same projection output through the shared site (B rows, the grad factor of the B * G-row tensor) and through the
    unshared one (the rows repeated): the cross K / V words are equal -- under codes the bytes and the records too."""
    from outlier_suppression_amd.model.quant_bart import QuantizedBartCache
    s = setup
    attn = s.q.model.decoder.layers[0].encoder_attn
    b = s.ids.shape[0]
    torch.manual_seed(3)
    hidden = torch.randn(b * G, 1, attn.embed_dim, device=s.dev)
    enc = torch.randn(b, s.ids.shape[1], attn.embed_dim, device=s.dev)
    # one projection output for both forms, whatever GEMM kernel the library would pick for B and for B * G rows
    for proj, scale in ((attn.k_proj, 1.0), (attn.v_proj, 0.7)):
        x = torch.randn(b, s.ids.shape[1], attn.embed_dim, device=s.dev) * scale
        monkeypatch.setattr(proj, "forward", lambda inp, x=x: x if inp.shape[0] == b else x.repeat_interleave(G, 0))
    held = []
    with torch.no_grad():
        for group in (G, 1):
            cache = QuantizedBartCache(1, capacity=4, codes=codes, cross_group=group)
            kv = enc if group > 1 else enc.repeat_interleave(G, 0)
            q, _, _ = attn._cached_qkv(cache.slot(0), hidden, kv, None)
            held.append((cache, q))
    (shared, q_shared), (plain, q_plain) = held
    assert torch.equal(q_shared, q_plain)
    assert shared.coded() == plain.coded() == ([(0, "cross_k"), (0, "cross_v")] if codes else [])
    for j, name in enumerate(("cross_k", "cross_v")):
        a, c = shared._cross[0][j], plain._cross[0][j]
        assert a.shape[0] == b and c.shape[0] == b * G and a.dtype == (torch.uint8 if codes else torch.float32)
        assert torch.equal(a.repeat_interleave(G, 0).view(torch.uint8), c.view(torch.uint8)), name
        if codes:
            ra, rc = shared._records[0][name].triple(), plain._records[0][name].triple()
            assert torch.equal(ra[0].view(torch.int32), rc[0].view(torch.int32)), name
            assert torch.equal(ra[1].view(torch.int32), rc[1].view(torch.int32)) and ra[2] == rc[2], name
        assert torch.equal(shared._fp32(0, name, a).repeat_interleave(G, 0), plain._fp32(0, name, c)), name
    assert shared.rejected() == 0 and plain.rejected() == 0


@pytest.mark.parametrize("codes", [False, True], ids=["fp32", "codes"])
def test_d_cache_shape_and_bytes(setup, fast_decode, codes):
    s = setup
    b = s.ids.shape[0]
    dec = _beam_tokens(s, 4)
    _, shared = _decode(s, dec, True, codes)
    _, plain = _decode(s, dec, False, codes)
    cross = 0
    for i in range(len(shared)):
        for a, c in zip(shared._cross[i], plain._cross[i]):
            assert a.shape == (b,) + c.shape[1:] and c.shape[0] == b * G and a.dtype == c.dtype
            cross += c.numel() * c.element_size()
    assert cross % G == 0 and plain.nbytes() - shared.nbytes() == cross // G * (G - 1)
    legacy = shared.to_legacy()
    for layer, ref in zip(legacy, plain.to_legacy()):
        assert len(layer) == 4 and [t.shape for t in layer] == [t.shape for t in ref]
        assert all(t.dtype == torch.float32 for t in layer)
    assert [t.shape for t in shared[0]] == [t.shape for t in plain[0]]
    assert len(shared.past(0)) == 2 and shared.past(0)[0].shape[0] == b * G


def test_e_reporting_and_fallbacks(setup, fast_decode):
    from outlier_suppression_amd.model import generation
    s = setup
    model = s.q
    kw = dict(attention_mask=s.mask, max_length=12, share_cross_kv=True)
    out = model.generate(s.ids, num_beams=3, **kw)
    info = model.last_share_cross_kv
    assert info.reason is None and info.eager == 0 and 1 <= info.shared <= 11 and info.shared >= out.shape[1] - 1, info

    def falls_back(fragment, **over):
        want = model.generate(s.ids, **{**kw, "num_beams": 3, **over, "share_cross_kv": False})
        got = model.generate(s.ids, **{**kw, "num_beams": 3, **over})
        got_info = model.last_share_cross_kv
        assert got_info.shared == 0 and got_info.reason is not None and fragment in got_info.reason, got_info
        assert torch.equal(got, want)

    falls_back("num_beams == 1", num_beams=1)
    falls_back("use_cache=False", use_cache=False)
    model.sample(s.ids, attention_mask=s.mask, max_length=8, seed=1, share_cross_kv=True)
    assert "num_beams == 1" in model.last_share_cross_kv.reason
    with torch.enable_grad():
        assert generation._share_why_not(model, s.dev, True, 3, 14) == "autograd is on"
    torch.set_grad_enabled(False)
    try:
        _fallback_reasons(generation, model, s)
    finally:
        torch.set_grad_enabled(True)


def _fallback_reasons(generation, model, s):
    """The reasons known before the first step, each under its condition (autograd off)."""
    assert generation._share_why_not(model, torch.device("cpu"), True, 3, 14) == "the tensors are on the CPU"
    assert generation._share_why_not(model, s.dev, True, 3, 14) is None
    assert "longer than 1024" in generation._share_why_not(model, s.dev, True, 3, 1025)
    assert generation._share_why_not(model, s.dev, True, 3, 1024) is None
    assert "num_beams above 64" in generation._share_why_not(model, s.dev, True, 65, 14)
    # active dropout
    layer = model.model.decoder.layers[0]
    old = layer.encoder_attn.dropout
    layer.encoder_attn.dropout = 0.1
    model.model.decoder.train()
    try:
        assert generation._share_why_not(model, s.dev, True, 3, 14) == "dropout is active"
    finally:
        layer.encoder_attn.dropout = old
        model.model.decoder.eval()
    # a cross-attention quantizer that also observes
    qz = layer.encoder_attn.key_post_act_fake_quantize
    qz.enable_observer()
    try:
        assert "not in the plain quantising state (decoder layer 0, key)" in generation._share_why_not(model, s.dev, True, 3, 14)
    finally:
        qz.disable_observer()
    # a head size the kernels do not take
    old = layer.encoder_attn.head_dim
    layer.encoder_attn.head_dim = 12
    try:
        assert "head_dim 12" in generation._share_why_not(model, s.dev, True, 3, 14)
    finally:
        layer.encoder_attn.head_dim = old
    assert generation._share_why_not(model, s.dev, True, 3, 14) is None


@pytest.mark.parametrize("codes", [False, True], ids=["fp32", "codes"])
def test_f_multi_token_call_on_a_shared_cache(setup, fast_decode, codes):
    """A first call of 3 tokens, then single tokens, then 2 tokens at once over the shared cache: the several-token calls expand
    K, V and the mask and take the existing path; the logits are the unshared form's within FUSED_VS_EAGER_LOGITS."""
    from outlier_suppression_amd.model.quant_bart import QuantizedBartCache
    s = setup
    dec = _beam_tokens(s, 8)
    got, shared = _decode(s, dec[:, :6], True, codes, first=3)
    want, plain = _decode(s, dec[:, :6], False, codes, first=3)
    assert (got - want).abs().max().item() < FUSED_VS_EAGER_LOGITS
    assert isinstance(shared, QuantizedBartCache) and shared._cross[0][0].shape[0] == s.ids.shape[0]
    with torch.no_grad():
        enc = s.q.get_encoder()(s.ids, attention_mask=s.mask)
        a = s.q(attention_mask=s.mask, decoder_input_ids=dec[:, 6:8], encoder_outputs=(enc,), past_key_values=shared,
                use_cache=True)[0]
        b = s.q(attention_mask=s.mask.repeat_interleave(G, 0), decoder_input_ids=dec[:, 6:8],
                encoder_outputs=(enc.repeat_interleave(G, 0),), past_key_values=plain, use_cache=True)[0]
    d = (a - b).abs().max().item()
    print(f"\nmulti-token call on a shared cache vs unshared, max |logit diff|: {d:.3g}")
    assert d < FUSED_VS_EAGER_LOGITS, d

"""A cached decoding step of quantized BART as a captured graph (model/graph_decode.py, generate(graph=True)), on the tiny
W6A6 LSQ+ BART of test_gpu_bart_decode.py.

(a) 12 teacher-forced steps through a GraphDecoder against the same steps issued one by one with the one-launch attention
on: the logits of every step and the cache read as a legacy tuple are WORD-equal, with the fp32 and the coded cache, greedy
(appending in place: one graph) and with a row permutation pending before every step (A -> B / B -> A: two graphs).
(b) generate(graph=True) returns the tokens of generate(), greedy and with beams, codes on and off, and says that it used
the graphs: a silent fallback fails.  (c) Each condition under which a step cannot be captured returns eager's tokens with
captured == 0 and a reason.  (d) A NaN key under cache_codes=True raises with the graph as without.  (e) Two calls of
different max_length in one process."""
import copy

import pytest
import torch

from test_gpu_bart_decode import setup  # noqa: F401  (that file's module fixture)

pytestmark = pytest.mark.gpu

STEPS = 12


@pytest.fixture()
def switches():
    from outlier_suppression_amd import _hip, util_layernorm as UL
    _hip.load()                      # the first load applies the environment's tier, these switches included
    old = UL.FUSE_DECODE_ATTENTION, UL.CACHE_CODES, UL.GRAPH_DECODE, UL.FUSE_KV_APPEND
    yield UL
    UL.FUSE_DECODE_ATTENTION, UL.CACHE_CODES, UL.GRAPH_DECODE, UL.FUSE_KV_APPEND = old


def _same_words(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _steps(model, s, codes, perm, graph):
    """STEPS teacher-forced steps over one cache of capacity STEPS, ``perm`` (or nothing) reordering the cache before every
    step after the first: issued one by one, or from the second step on through a GraphDecoder."""
    from outlier_suppression_amd.model.graph_decode import GraphDecoder
    from outlier_suppression_amd.model.quant_bart import QuantizedBartCache
    with torch.no_grad():
        cache = QuantizedBartCache(len(model.model.decoder.layers), capacity=STEPS, codes=codes)
        out, got, enc = model(s.ids, s.mask, decoder_input_ids=s.dec[:, :1], past_key_values=cache, use_cache=True)
        assert got is cache
        logits = [out[:, -1].clone()]
        decoder = GraphDecoder(model, enc, s.mask, cache) if graph else None
        for t in range(1, STEPS):
            if perm is not None:
                cache.reorder(perm)
            if graph:
                logits.append(decoder.step(s.dec[:, t:t + 1]).clone())
            else:
                out, _, _ = model(attention_mask=s.mask, decoder_input_ids=s.dec[:, t:t + 1], encoder_outputs=(enc,),
                                  past_key_values=cache, use_cache=True)
                logits.append(out[:, -1].clone())
    return torch.stack(logits, 1), cache, (decoder.info if graph else None)


@pytest.mark.parametrize("moving", [False, True], ids=["greedy", "reordered"])
@pytest.mark.parametrize("codes", [False, True], ids=["fp32", "codes"])
def test_a_steps_word_equal_to_issued_steps(setup, switches, codes, moving):
    s = setup
    switches.FUSE_DECODE_ATTENTION = True
    perm = torch.tensor([1, 2, 0], device=s.dev) if moving else None
    want, want_cache, _ = _steps(s.q, s, codes, perm, graph=False)
    switches.FUSE_DECODE_ATTENTION = False            # a captured step uses the one-launch attention whatever the switch says
    got, got_cache, info = _steps(s.q, s, codes, perm, graph=True)
    assert info.captured == (2 if moving else 1) and info.replays == STEPS - 2 and info.reason is None, info
    assert info.capture_seconds > 0
    assert not torch.isnan(want).any()
    for t in range(STEPS):
        assert _same_words(got[:, t], want[:, t]), f"step {t}"
    assert got_cache.get_seq_length() == want_cache.get_seq_length() == STEPS
    assert got_cache.coded() == want_cache.coded() and bool(got_cache.coded()) is codes
    assert got_cache._k[0].dtype == (torch.uint8 if codes else torch.float32)
    a, b = got_cache.to_legacy(), want_cache.to_legacy()
    assert len(a) == len(b) == len(s.q.model.decoder.layers)
    for la, lb in zip(a, b):
        assert len(la) == len(lb) == 4
        for x, y in zip(la, lb):
            assert _same_words(x, y)
    assert got_cache.rejected() == 0 and int(got_cache._pos.item()) == STEPS


def _counting_steps(monkeypatch):
    """How many decoding steps a generate() call takes: the calls of generation._step_logits."""
    from outlier_suppression_amd.model import generation
    calls = []
    real = generation._step_logits
    monkeypatch.setattr(generation, "_step_logits", lambda *a, **kw: calls.append(1) or real(*a, **kw))
    return calls


@pytest.mark.parametrize("attention", [False, True], ids=["eager-attention", "one-launch-attention"])
@pytest.mark.parametrize("codes", [False, True], ids=["fp32", "codes"])
@pytest.mark.parametrize("kw", [dict(num_beams=1, min_length=8), dict(num_beams=3)], ids=["greedy", "beams"])
def test_b_generate_same_tokens_and_graphs_used(setup, switches, monkeypatch, kw, codes, attention):
    s = setup
    switches.FUSE_DECODE_ATTENTION = attention
    with torch.no_grad():
        want = s.q.generate(s.ids, attention_mask=s.mask, max_length=20, cache_codes=codes, **kw)
        assert s.q.last_decode_graph.captured == 0 and s.q.last_decode_graph.reason
        calls = _counting_steps(monkeypatch)
        got = s.q.generate(s.ids, attention_mask=s.mask, max_length=20, cache_codes=codes, graph=True, **kw)
    info = s.q.last_decode_graph
    assert torch.equal(got, want), (got, want)
    steps = len(calls)
    assert steps >= 7
    assert info.captured == (1 if kw["num_beams"] == 1 else 2) and info.reason is None, info
    assert info.capture_seconds > 0
    assert info.replays >= steps - 3 and info.replays == steps - 2, (info, steps)
    assert switches.FUSE_DECODE_ATTENTION is attention


def test_b_switch_turns_it_on(setup, switches):
    import outlier_suppression_amd as osq
    s = setup
    with torch.no_grad():
        want = s.q.generate(s.ids, attention_mask=s.mask, max_length=12, num_beams=1, min_length=8)
        osq.set_graph_decode(True)
        got = s.q.generate(s.ids, attention_mask=s.mask, max_length=12, num_beams=1, min_length=8)
        assert s.q.last_decode_graph.captured == 1 and s.q.last_decode_graph.capture_seconds > 0
        off = s.q.generate(s.ids, attention_mask=s.mask, max_length=12, num_beams=1, min_length=8, graph=False)
        assert s.q.last_decode_graph.captured == 0
    assert torch.equal(got, want) and torch.equal(off, want)


def _both(model_for, kw, seed=None):
    """generate() and generate(graph=True) on two models made by ``model_for`` (two: a call may move quantizer state)."""
    outs = []
    for graph in (False, True):
        m = model_for()
        if seed is not None:
            torch.manual_seed(seed)
        with torch.no_grad():
            outs.append((m.generate(graph=graph, **kw), m.last_decode_graph))
    return outs


@pytest.mark.parametrize("condition", ["dropout", "observer", "kv_append_off", "no_cache"])
def test_c_fallback_returns_eager_tokens_with_a_reason(setup, switches, condition):
    s = setup
    kw = dict(input_ids=s.ids, attention_mask=s.mask, max_length=10, num_beams=1, min_length=6)
    seed = None

    def model_for():
        m = copy.deepcopy(s.q)
        if condition == "dropout":
            m.model.decoder.train()
            m.model.decoder.dropout = 0.1
        elif condition == "observer":
            m.model.decoder.layers[1].self_attn.key_post_act_fake_quantize.enable_observer()
        return m
    if condition == "dropout":
        seed = 11
    elif condition == "kv_append_off":
        switches.FUSE_KV_APPEND = False
    elif condition == "no_cache":
        kw["use_cache"] = False
    (want, _), (got, info) = _both(model_for, kw, seed)
    assert torch.equal(got, want), (got, want)
    assert info.captured == 0 and info.replays == 0 and info.reason, info
    word = {"dropout": "dropout", "observer": "observer", "kv_append_off": "append", "no_cache": "use_cache"}[condition]
    assert word in info.reason, info


def test_d_nan_key_makes_generate_raise(setup, switches):
    s = setup
    k_proj = s.q.model.decoder.layers[1].self_attn.k_proj

    # the NaN comes from device tensors made here: a hook that writes a Python number into its output copies from the host,
    # which no stream allows while it is capturing
    where = torch.zeros(3, 1, 64, dtype=torch.bool, device=s.dev)
    where[0, 0, 5] = True
    nan = torch.full((), float("nan"), device=s.dev)

    def plant(module, args, out):
        return torch.where(where, nan, out)
    handle = k_proj.register_forward_hook(plant)
    kw = dict(attention_mask=s.mask, max_length=8, num_beams=1, min_length=8)
    try:
        with torch.no_grad():
            s.q.generate(s.ids, cache_codes=False, graph=True, **kw)
            assert s.q.last_decode_graph.captured == 1 and s.q.last_decode_graph.capture_seconds > 0
            with pytest.raises(RuntimeError, match=r"holds \d+ elements without an integer code"):
                s.q.generate(s.ids, cache_codes=True, **kw)
            with pytest.raises(RuntimeError, match=r"holds \d+ elements without an integer code"):
                s.q.generate(s.ids, cache_codes=True, graph=True, **kw)
            assert s.q.last_decode_graph.captured == 1 and s.q.last_decode_graph.replays >= 4
            assert s.q.last_decode_graph.capture_seconds > 0
    finally:
        handle.remove()


def test_e_two_calls_of_different_length(setup, switches):
    s = setup
    with torch.no_grad():
        for max_length in (9, 16):
            kw = dict(attention_mask=s.mask, max_length=max_length, num_beams=3, cache_codes=True)
            want = s.q.generate(s.ids, **kw)
            got = s.q.generate(s.ids, graph=True, **kw)
            assert torch.equal(got, want), max_length
            assert s.q.last_decode_graph.captured == 2 and s.q.last_decode_graph.capture_seconds > 0, s.q.last_decode_graph

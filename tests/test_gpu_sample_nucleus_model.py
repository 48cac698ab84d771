"""sample(sample_nucleus=True) on the tiny W6A6 LSQ+ BART of test_gpu_bart_decode.py with top_k=0, top_p=0.9: under
sample_advance=True and sample_graph=True the steps go to ops.sample_nucleus / ops.sample_nucleus_at
(csrc/sample_nucleus.hip) and return the tokens of the torch lines (model/sampling.py, the same uniforms) -- with graph and
cache_codes each on and off, with use_cache=False and with the whole step as one captured graph -- and the call says how many
steps took it.  With the switch off the same calls fall back with the reason they always gave.

The two paths add the same fp32 weights in different orders, so a draw within 2e-5 W of a boundary may select the neighbouring
token (tests/test_gpu_sample_nucleus.py holds every draw to that band against float64).  SEEDS = (3, 2^63 + 5), the seeds of
tests/test_gpu_sample_advance_model.py: neither met such a draw on this model; a seed that does shows as a token mismatch
here and is then to be checked with _sample_advance.excursion on that step's logits."""
import copy
import itertools

import pytest
import torch

from test_gpu_bart_decode import setup  # noqa: F401  (that file's module fixture)

pytestmark = pytest.mark.gpu

L = 12
SEEDS = (3, 2 ** 63 + 5)
VARIANTS = [dict(graph=g, cache_codes=c) for g, c in itertools.product((False, True), repeat=2)] + [dict(use_cache=False)]
DRAW = dict(top_k=0, top_p=0.9, temperature=1.5)
SETTINGS = dict(max_length=L, min_length=L - 1, no_repeat_ngram_size=2, forced_bos_token_id=0)
WHY = "top_p below 1 without top_k"


@pytest.fixture()
def switches():
    from outlier_suppression_amd import _hip, util_layernorm as UL
    _hip.load()                      # the first load applies the environment's tier, these switches included
    names = ("SAMPLE_NUCLEUS", "SAMPLE_GRAPH", "SAMPLE_ADVANCE", "GREEDY_GRAPH", "GREEDY_ADVANCE", "GRAPH_DECODE", "CACHE_CODES")
    old = [getattr(UL, n) for n in names]
    for n in names:
        setattr(UL, n, False)
    yield UL
    for n, v in zip(names, old):
        setattr(UL, n, v)


@pytest.fixture(scope="module")
def unforced(setup):
    """The model without its configuration's forced_eos_token_id: a call ends where the search ends it."""
    m = copy.deepcopy(setup.q)
    for cfg in (m.config, m.generation_config):
        if cfg is not None:
            cfg.forced_eos_token_id = None
    return m


@pytest.mark.parametrize("variant", VARIANTS, ids=("plain", "codes", "graph", "graph-codes", "no-cache"))
def test_a_the_kernel_returns_the_tokens_of_the_torch_lines(setup, unforced, switches, variant):
    for m, seed in ((unforced, SEEDS[0]), (setup.q, SEEDS[1])):            # setup.q: the configuration's forced eos fires last
        kw = dict(SETTINGS, attention_mask=setup.mask, seed=seed, **DRAW, **variant)
        want = m.sample(setup.ids, **kw)
        info, steps = m.last_sample_advance, want.shape[1] - 1
        assert (info.advanced, info.eager, info.reason) == (0, steps, "not asked for"), info
        off = m.sample(setup.ids, sample_advance=True, **kw)               # the switch off: today's fallback, today's reason
        info = m.last_sample_advance
        assert torch.equal(off, want) and (info.advanced, info.eager, info.reason) == (0, steps, WHY), info
        got = m.sample(setup.ids, sample_advance=True, sample_nucleus=True, **kw)
        info = m.last_sample_advance
        assert got.shape == want.shape and got.dtype == want.dtype and torch.equal(got, want), (got, want)
        assert (info.advanced, info.eager, info.reason) == (steps, 0, None), info
        assert m.last_sample_graph.reason == "not asked for"
        assert (want[:, 1] == 0).all()
        if variant.get("graph"):
            assert m.last_decode_graph.captured == 1 and m.last_decode_graph.reason is None, m.last_decode_graph
    assert steps == L - 1 and (want[:, -1] == 2).all()                     # the forced eos
    other = unforced.sample(setup.ids, sample_advance=True, sample_nucleus=True, **dict(kw, seed=seed + 1))
    assert not torch.equal(other, unforced.sample(setup.ids, sample_advance=True, sample_nucleus=True, **kw))


@pytest.mark.parametrize("codes", (False, True), ids=("fp32-cache", "codes"))
def test_b_whole_step_as_one_graph(setup, unforced, switches, codes):
    for m, seed in ((unforced, SEEDS[0]), (setup.q, SEEDS[1])):
        kw = dict(SETTINGS, attention_mask=setup.mask, seed=seed, cache_codes=codes, **DRAW)
        want = m.sample(setup.ids, graph=True, **kw)                       # the same model step, replayed alone; the torch lines
        steps = want.shape[1] - 1
        assert m.last_sample_graph.reason == m.last_sample_advance.reason == "not asked for"
        off = m.sample(setup.ids, sample_graph=True, **kw)
        assert torch.equal(off, want) and m.last_sample_graph.reason == WHY and m.last_sample_graph.captured == 0
        got = m.sample(setup.ids, sample_graph=True, sample_nucleus=True, **kw)
        info = m.last_sample_graph
        assert got.shape == want.shape and torch.equal(got, want), (got, want)
        assert steps >= 4 and info.reason is None and info.captured == 1 and info.replays == steps - 2, (info, steps)
        assert (m.last_sample_advance.advanced, m.last_sample_advance.eager) == (steps, 0)
        assert (m.last_decode_graph.captured, m.last_decode_graph.replays, m.last_decode_graph.reason) == (1, steps - 2, None)


def test_c_the_switch_leaves_every_other_form_alone(setup, unforced, switches):
    s = setup
    kw = dict(SETTINGS, attention_mask=s.mask, seed=SEEDS[0])
    for draw in (dict(top_k=8, temperature=1.3), dict(top_k=50, top_p=0.9), dict(top_k=0, temperature=1.5)):
        want = unforced.sample(s.ids, sample_advance=True, **kw, **draw)
        assert unforced.last_sample_advance.reason is None
        assert torch.equal(unforced.sample(s.ids, sample_advance=True, sample_nucleus=True, **kw, **draw), want)
        assert unforced.last_sample_advance.reason is None and unforced.last_sample_advance.eager == 0
    want = unforced.sample(s.ids, top_k=100, top_p=0.9, **kw)
    assert torch.equal(unforced.sample(s.ids, sample_advance=True, sample_nucleus=True, top_k=100, top_p=0.9, **kw), want)
    assert unforced.last_sample_advance.reason == "top_k above 64" and unforced.last_sample_advance.advanced == 0
    want = s.q.generate(s.ids, attention_mask=s.mask, max_length=L)        # generate() is untouched
    switches.SAMPLE_NUCLEUS = True
    assert torch.equal(s.q.generate(s.ids, attention_mask=s.mask, max_length=L), want)
    with pytest.raises(NotImplementedError):
        unforced.generate(s.ids, attention_mask=s.mask, max_length=5, do_sample=True)


def test_d_the_switches(setup, unforced, switches, monkeypatch):
    import outlier_suppression_amd as osq
    from outlier_suppression_amd import ops
    s, kw = setup, dict(SETTINGS, attention_mask=setup.mask, seed=SEEDS[0], **DRAW)
    want = unforced.sample(s.ids, **kw)
    steps = want.shape[1] - 1
    osq.set_sample_nucleus(True)
    assert torch.equal(unforced.sample(s.ids, **kw), want) and unforced.last_sample_advance.reason == "not asked for"
    assert torch.equal(unforced.sample(s.ids, sample_advance=True, **kw), want) and unforced.last_sample_advance.advanced == steps
    assert torch.equal(unforced.sample(s.ids, sample_advance=True, sample_nucleus=False, **kw), want)
    assert unforced.last_sample_advance.reason == WHY
    osq.set_sample_graph(True)
    assert torch.equal(unforced.sample(s.ids, **kw), want)
    assert unforced.last_sample_graph.captured == 1 and unforced.last_sample_graph.reason is None
    osq.set_sample_graph(False)
    osq.set_sample_nucleus(False)
    monkeypatch.setattr(ops, "set_tuning", lambda key, value, lib=None: None)
    monkeypatch.setenv("OSQ_SAMPLE_NUCLEUS", "1")
    osq.reset_tier()
    assert switches.SAMPLE_NUCLEUS is True
    monkeypatch.delenv("OSQ_SAMPLE_NUCLEUS")
    osq.reset_tier()
    assert switches.SAMPLE_NUCLEUS is False

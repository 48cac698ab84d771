"""sample(sample_advance=True) and sample(sample_graph=True) (model/generation.py::sample, ops.sample_advance,
graph_decode.SampleStepGraph) on the tiny W6A6 LSQ+ BART of test_gpu_bart_decode.py, with fixed seeds: the kernel path returns
the tokens of the torch lines (model/sampling.py, the same uniforms) -- with graph and cache_codes each on and off, with
use_cache=False and with the whole step as one captured graph -- and says how many steps took it; the forms the kernel does
not have and CPU tensors fall back with a reason; top_k=1 is greedy generate().

The two paths add the same fp32 weights in different orders, so a draw within 2e-5 W of a boundary of the running sums may
select the neighbouring token; the seeds below were not met by such a draw (tests/test_gpu_sample_advance.py holds every draw
to that band against float64)."""
import copy
import itertools

import pytest
import torch

from test_gpu_bart_decode import setup  # noqa: F401  (that file's module fixture)

pytestmark = pytest.mark.gpu

L = 12
SEEDS = (3, 2 ** 63 + 5)
VARIANTS = [dict(graph=g, cache_codes=c) for g, c in itertools.product((False, True), repeat=2)] + [dict(use_cache=False)]
DRAWS = {"top-k": dict(top_k=8, temperature=1.3), "top-k-top-p": dict(top_k=50, top_p=0.9, temperature=0.8),
         "whole-vocabulary": dict(top_k=0, temperature=1.5)}
SETTINGS = dict(max_length=L, min_length=L - 1, no_repeat_ngram_size=2, forced_bos_token_id=0)


@pytest.fixture()
def switches():
    from outlier_suppression_amd import _hip, util_layernorm as UL
    _hip.load()                      # the first load applies the environment's tier, these switches included
    names = ("SAMPLE_GRAPH", "SAMPLE_ADVANCE", "GREEDY_GRAPH", "GREEDY_ADVANCE", "GRAPH_DECODE", "CACHE_CODES")
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


@pytest.mark.parametrize("draw", list(DRAWS))
@pytest.mark.parametrize("variant", VARIANTS, ids=("plain", "codes", "graph", "graph-codes", "no-cache"))
def test_a_the_kernel_returns_the_tokens_of_the_torch_lines(setup, unforced, switches, variant, draw):
    for m, seed in ((unforced, SEEDS[0]), (setup.q, SEEDS[1])):            # setup.q: the configuration's forced eos fires last
        kw = dict(SETTINGS, attention_mask=setup.mask, seed=seed, **DRAWS[draw], **variant)
        want = m.sample(setup.ids, sample_advance=False, **kw)
        info, steps = m.last_sample_advance, want.shape[1] - 1
        assert (info.advanced, info.eager, info.reason) == (0, steps, "not asked for"), info
        got = m.sample(setup.ids, sample_advance=True, **kw)
        info = m.last_sample_advance
        assert got.shape == want.shape and got.dtype == want.dtype and torch.equal(got, want), (got, want)
        assert (info.advanced, info.eager, info.reason) == (steps, 0, None), info
        assert m.last_sample_graph.reason == "not asked for"
        assert (want[:, 1] == 0).all()
        if variant.get("graph"):
            assert m.last_decode_graph.captured == 1 and m.last_decode_graph.reason is None, m.last_decode_graph
    assert steps == L - 1 and (want[:, -1] == 2).all()                     # the forced eos
    other = unforced.sample(setup.ids, sample_advance=True, **dict(kw, seed=seed + 1))
    assert not torch.equal(other, unforced.sample(setup.ids, sample_advance=True, **kw))


@pytest.mark.parametrize("draw", list(DRAWS))
@pytest.mark.parametrize("codes", (False, True), ids=("fp32-cache", "codes"))
def test_b_whole_step_as_one_graph(setup, unforced, switches, codes, draw):
    for m, seed in ((unforced, SEEDS[0]), (setup.q, SEEDS[1])):
        kw = dict(SETTINGS, attention_mask=setup.mask, seed=seed, cache_codes=codes, **DRAWS[draw])
        want = m.sample(setup.ids, graph=True, **kw)                       # the same model step, replayed alone; the torch lines
        steps = want.shape[1] - 1
        assert m.last_sample_graph.reason == m.last_sample_advance.reason == "not asked for"
        got = m.sample(setup.ids, sample_graph=True, **kw)
        info = m.last_sample_graph
        assert got.shape == want.shape and torch.equal(got, want), (got, want)
        assert steps >= 4 and info.reason is None and info.captured == 1 and info.replays == steps - 2, (info, steps)
        assert (m.last_sample_advance.advanced, m.last_sample_advance.eager) == (steps, 0)
        assert (m.last_decode_graph.captured, m.last_decode_graph.replays, m.last_decode_graph.reason) == (1, steps - 2, None)


def test_c_what_the_kernel_does_not_take_falls_back_with_a_reason(setup, unforced, switches):
    s = setup
    kw = dict(SETTINGS, attention_mask=s.mask, seed=SEEDS[0])
    for draw, why in ((dict(top_k=0, top_p=0.9), "top_p below 1 without top_k"), (dict(top_k=100), "top_k above 64")):
        want = unforced.sample(s.ids, **kw, **draw)
        for asked in (dict(sample_advance=True), dict(sample_graph=True)):
            got = unforced.sample(s.ids, **kw, **draw, **asked)
            assert torch.equal(got, want)
            info = unforced.last_sample_advance if "sample_advance" in asked else unforced.last_sample_graph
            assert info.reason == why and unforced.last_sample_advance.advanced == 0, info
    for given in ("graph", "sample_advance"):
        unforced.sample(s.ids, sample_graph=True, top_k=8, **{given: False}, **kw)
        assert unforced.last_sample_graph.reason == f"{given}=False was passed" and unforced.last_sample_graph.captured == 0


def test_d_cpu_tensors_fall_back_with_a_reason(switches):
    from test_bart_decode_cpu import batch, tiny_bart, wrapped
    q = wrapped(tiny_bart())
    ids, mask = batch()
    kw = dict(attention_mask=mask, max_length=10, min_length=10, seed=4, top_k=8)
    want = q.sample(ids, **kw)
    assert torch.equal(q.sample(ids, sample_advance=True, **kw), want) and "CPU" in q.last_sample_advance.reason
    assert torch.equal(q.sample(ids, sample_graph=True, **kw), want) and "CPU" in q.last_sample_graph.reason


def test_e_top_k_one_is_greedy(setup, unforced, switches):
    s = setup
    for m in (unforced, setup.q):
        kw = dict(max_length=L, min_length=6, no_repeat_ngram_size=2, attention_mask=s.mask)
        want = m.generate(s.ids, **kw)
        for asked in (dict(), dict(sample_advance=True), dict(sample_graph=True)):
            assert torch.equal(m.sample(s.ids, seed=9, top_k=1, temperature=0.7, **kw, **asked), want), asked


def test_f_the_switches(setup, unforced, switches):
    import outlier_suppression_amd as osq
    s, kw = setup, dict(SETTINGS, attention_mask=setup.mask, seed=SEEDS[0], top_k=8)
    want = unforced.sample(s.ids, **kw)
    osq.set_sample_advance(True)
    assert torch.equal(unforced.sample(s.ids, **kw), want) and unforced.last_sample_advance.advanced == want.shape[1] - 1
    assert torch.equal(unforced.sample(s.ids, sample_advance=False, **kw), want) and unforced.last_sample_advance.advanced == 0
    osq.set_sample_advance(False)
    osq.set_sample_graph(True)
    assert torch.equal(unforced.sample(s.ids, **kw), want)
    assert unforced.last_sample_graph.captured == 1 and unforced.last_sample_graph.reason is None
    assert torch.equal(unforced.sample(s.ids, sample_graph=False, **kw), want)
    assert unforced.last_sample_graph.reason == "not asked for" and unforced.last_decode_graph.reason == "not asked for"
    with pytest.raises(NotImplementedError):
        unforced.generate(s.ids, attention_mask=s.mask, max_length=5, do_sample=True)

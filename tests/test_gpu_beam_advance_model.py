"""generate(beam_advance=True) (model/generation.py::_beam_search_advanced, ops.beam_advance) on the tiny W6A6 LSQ+ BART of
test_gpu_bart_decode.py: beam search returns the tokens of the switch off -- with graph, beam_select and cache_codes each on
and off, with use_cache=False, with early_stopping=True, with num_return_sequences=2 and in a configuration in which a beam
finishes on an eos before max_length -- and says that every step took the kernel."""
import copy
import itertools

import pytest
import torch

from test_gpu_bart_decode import setup  # noqa: F401  (that file's module fixture)

pytestmark = pytest.mark.gpu

KW = dict(num_beams=3, max_length=12, min_length=5, no_repeat_ngram_size=2)
SWITCHES = [dict(graph=g, beam_select=b, cache_codes=c) for g, b, c in itertools.product((False, True), repeat=3)]
OTHERS = {"no-cache": dict(use_cache=False), "early-stopping": dict(early_stopping=True),
          "two-sequences": dict(num_return_sequences=2), "never": dict(early_stopping="never", length_penalty=0.8),
          "no-cache-select": dict(use_cache=False, beam_select=True)}


@pytest.fixture()
def switches():
    from outlier_suppression_amd import _hip, util_layernorm as UL
    _hip.load()                      # the first load applies the environment's tier, these switches included
    old = UL.BEAM_ADVANCE, UL.BEAM_SELECT, UL.GRAPH_DECODE, UL.CACHE_CODES
    UL.BEAM_ADVANCE = UL.BEAM_SELECT = UL.GRAPH_DECODE = UL.CACHE_CODES = False
    yield UL
    UL.BEAM_ADVANCE, UL.BEAM_SELECT, UL.GRAPH_DECODE, UL.CACHE_CODES = old


@pytest.fixture(scope="module")
def unforced(setup):
    """The model without its configuration's forced_eos_token_id: a call ends where the search ends it."""
    m = copy.deepcopy(setup.q)
    for cfg in (m.config, m.generation_config):
        if cfg is not None:
            cfg.forced_eos_token_id = None
    return m


def _recording(monkeypatch):
    """The steps of a call (one selection each) and the state it ended with."""
    from outlier_suppression_amd.model import generation
    steps, ends = [], []
    select, result = generation._select_continuations, generation._beam_result

    def selected(*a, **kw):
        steps.append(1)
        return select(*a, **kw)

    def ended(state, *a, **kw):
        ends.append((state.done.cpu().clone(), state.finished_len.cpu().clone()))
        return result(state, *a, **kw)
    monkeypatch.setattr(generation, "_select_continuations", selected)
    monkeypatch.setattr(generation, "_beam_result", ended)
    return steps, ends


def _on_and_off(m, s, monkeypatch, kw, min_steps=4):
    steps, ends = _recording(monkeypatch)
    with torch.no_grad():
        want = m.generate(s.ids, attention_mask=s.mask, beam_advance=False, **kw)
        info, n = m.last_beam_advance, len(steps)
        assert n >= min_steps and (info.advanced, info.eager, info.reason) == (0, n, "not asked for"), info
        del steps[:]
        got = m.generate(s.ids, attention_mask=s.mask, beam_advance=True, **kw)
    info = m.last_beam_advance
    assert torch.equal(got, want), (got, want)
    assert len(steps) == n and (info.advanced, info.eager, info.reason) == (n, 0, None), info
    assert torch.equal(ends[0][0], ends[1][0]) and torch.equal(ends[0][1][ends[0][0]], ends[1][1][ends[1][0]])
    return want, ends


@pytest.mark.parametrize("variant", SWITCHES, ids=lambda v: "-".join(k for k, on in v.items() if on) or "plain")
def test_a_same_tokens_with_every_other_switch(setup, unforced, switches, monkeypatch, variant):
    _on_and_off(unforced, setup, monkeypatch, dict(KW, **variant))
    if variant["graph"]:
        assert unforced.last_decode_graph.captured == 2 and unforced.last_decode_graph.reason is None, unforced.last_decode_graph
    if variant["beam_select"]:
        assert unforced.last_beam_select.eager == 0 and unforced.last_beam_select.reason is None, unforced.last_beam_select


@pytest.mark.parametrize("variant", list(OTHERS))
def test_b_same_tokens_in_the_other_modes(setup, unforced, switches, monkeypatch, variant):
    want, _ = _on_and_off(unforced, setup, monkeypatch, dict(KW, **OTHERS[variant]))
    if variant == "two-sequences":
        assert want.shape[0] == 2 * setup.ids.shape[0]


def test_c_a_beam_finishes_on_an_eos_before_max_length(setup, unforced, switches, monkeypatch):
    """min_length=0: the model's first choice after the start token is the eos itself, so every input's first beam finishes
    at length 1 and the search goes on beside it to max_length -- finished slots are kept, merged and compared."""
    for extra in ({}, dict(graph=True, beam_select=True), dict(early_stopping=True), dict(early_stopping="never")):
        kw = dict(num_beams=3, max_length=10, min_length=0, **extra)
        want, ends = _on_and_off(unforced, setup, monkeypatch, kw, min_steps=2)
        done, finished_len = ends[0]
        assert (done & (finished_len < kw["max_length"] - 1)).any(), (done, finished_len)


def test_d_the_switch(setup, unforced, switches):
    import outlier_suppression_amd as osq
    s = setup
    with torch.no_grad():
        want = unforced.generate(s.ids, attention_mask=s.mask, **KW)                 # unset: the torch lines
        assert unforced.last_beam_advance.advanced == 0 and unforced.last_beam_advance.reason == "not asked for"
        osq.set_beam_advance(True)
        got = unforced.generate(s.ids, attention_mask=s.mask, **KW)
        assert unforced.last_beam_advance.advanced >= 4 and unforced.last_beam_advance.eager == 0
        off = unforced.generate(s.ids, attention_mask=s.mask, beam_advance=False, **KW)
        assert unforced.last_beam_advance.advanced == 0
        unforced.generate(s.ids, attention_mask=s.mask, max_length=8, num_beams=1)
        assert unforced.last_beam_advance.advanced == 0 and "greedy" in unforced.last_beam_advance.reason
    assert torch.equal(got, want) and torch.equal(off, want)

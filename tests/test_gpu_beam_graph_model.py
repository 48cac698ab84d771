"""generate(beam_graph=True) (model/graph_decode.py::BeamStepGraphs; ops.beam_select_at, ops.beam_advance_at) on the tiny W6A6
LSQ+ BART of test_gpu_bart_decode.py: a beam search whose steps are replays of a whole captured step -- token copy, model,
selection, bookkeeping, the cache's row index -- returns the tokens of generate(graph=True, beam_select=True,
beam_advance=True), stops on the same step, captures two graphs, and says what it did; where it cannot take the call it
decodes as without the switch and says why."""
import copy

import pytest
import torch

from test_gpu_bart_decode import setup  # noqa: F401  (that file's module fixture)

pytestmark = pytest.mark.gpu

PARENT = dict(graph=True, beam_select=True, beam_advance=True)
KW = dict(num_beams=3, max_length=12, min_length=5, no_repeat_ngram_size=3)
# name -> (the model without its forced eos?, generate()'s arguments)
CONFIGS = {
    "codes": (True, dict(KW, cache_codes=True)),
    "fp32-cache": (True, dict(KW, cache_codes=False)),
    "no-ngram": (True, dict(KW, no_repeat_ngram_size=0)),
    "forced-eos": (False, dict(KW)),
    "forced-eos-codes": (False, dict(KW, cache_codes=True, no_repeat_ngram_size=0)),
    "early-stopping-eos-hit": (True, dict(num_beams=3, max_length=10, min_length=0, early_stopping=True)),
    "two-sequences": (True, dict(KW, num_return_sequences=2)),
    "never": (True, dict(KW, early_stopping="never", length_penalty=0.8)),
}


@pytest.fixture()
def switches():
    from outlier_suppression_amd import _hip, util_layernorm as UL
    _hip.load()                      # the first load applies the environment's tier, these switches included
    names = ("BEAM_GRAPH", "BEAM_ADVANCE", "BEAM_SELECT", "GRAPH_DECODE", "CACHE_CODES")
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


def _counts(m):
    return (m.last_decode_graph.captured, m.last_decode_graph.replays, m.last_beam_select.selected, m.last_beam_select.eager,
            m.last_beam_advance.advanced, m.last_beam_advance.eager)


def _ends(monkeypatch):
    """The state every call ends with: (done, finished_len) on the host."""
    from outlier_suppression_amd.model import generation
    ends, result = [], generation._beam_result

    def ended(state, *a, **kw):
        ends.append((state.done.cpu().clone(), state.finished_len.cpu().clone()))
        return result(state, *a, **kw)
    monkeypatch.setattr(generation, "_beam_result", ended)
    return ends


@pytest.mark.parametrize("name", list(CONFIGS))
def test_a_same_tokens_same_steps(setup, unforced, switches, monkeypatch, name):
    plain, kw = CONFIGS[name]
    m = unforced if plain else setup.q
    ends = _ends(monkeypatch)
    with torch.no_grad():
        want = m.generate(setup.ids, attention_mask=setup.mask, **PARENT, **kw)
        steps = m.last_beam_advance.advanced
        parent = _counts(m)
        assert steps >= 4 and m.last_beam_advance.eager == 0 and m.last_beam_graph.reason == "not asked for"
        got = m.generate(setup.ids, attention_mask=setup.mask, beam_graph=True, **kw)
    info = m.last_beam_graph
    assert got.shape == want.shape and torch.equal(got, want), (got, want)
    assert info.reason is None and info.captured == 2, info
    assert info.capture_seconds > 0 and m.last_decode_graph.capture_seconds > 0      # the one capture path times into both
    assert info.replays + info.issued + 2 == steps, (info, steps)                    # it stopped on the same step
    forced = not plain and steps == kw["max_length"] - 1
    assert info.issued == (1 if forced else 0), info
    # the three switches it implies count the steps they served, replayed ones included, as the parent form does
    mine = list(_counts(m))
    mine[1] += info.issued                                                            # an issued step is no replay
    assert tuple(mine) == parent, (mine, parent)
    assert torch.equal(ends[0][0], ends[1][0]) and torch.equal(ends[0][1][ends[0][0]], ends[1][1][ends[1][0]])
    if name == "early-stopping-eos-hit":                                              # a beam ended on an eos before max_length
        done, finished_len = ends[1]
        assert bool((done & (finished_len < kw["max_length"] - 1)).any()), (done, finished_len)
    if name == "two-sequences":
        assert got.shape[0] == 2 * setup.ids.shape[0]


def test_b_the_parent_form_is_what_it_was(setup, unforced, switches):
    """graph + beam_select + beam_advance without the new switch: model-only graphs, the selection and the bookkeeping
    outside them."""
    with torch.no_grad():
        unforced.generate(setup.ids, attention_mask=setup.mask, **PARENT, **KW)
    info = unforced.last_beam_graph
    assert (info.captured, info.replays, info.issued, info.reason) == (0, 0, 0, "not asked for"), info
    assert unforced.last_decode_graph.captured == 2 and unforced.last_beam_select.eager == 0
    assert unforced.last_decode_graph.capture_seconds > 0 and info.capture_seconds == 0


def test_c_falls_back_and_says_why(setup, unforced, switches):
    import outlier_suppression_amd as osq
    s = setup
    with torch.no_grad():
        want = unforced.generate(s.ids, attention_mask=s.mask, **KW)                  # every switch off
        plain = _counts(unforced)
        for off in ("graph", "beam_select", "beam_advance"):
            given = dict(PARENT, **{off: False})
            ref = unforced.generate(s.ids, attention_mask=s.mask, **given, **KW)
            counts = _counts(unforced)
            got = unforced.generate(s.ids, attention_mask=s.mask, beam_graph=True, **given, **KW)
            info = unforced.last_beam_graph
            assert torch.equal(got, ref)
            assert (info.captured, info.replays, info.issued) == (0, 0, 0) and f"{off}=False" in info.reason, info
            assert _counts(unforced) == counts                                        # exactly the call without the switch
        got = unforced.generate(s.ids, attention_mask=s.mask, beam_graph=True, beam_advance=False, **KW)
        assert torch.equal(got, want) and _counts(unforced) == plain and "beam_advance=False" in unforced.last_beam_graph.reason
        unforced.generate(s.ids, attention_mask=s.mask, beam_graph=True, max_length=8, num_beams=1)
        assert "greedy" in unforced.last_beam_graph.reason and unforced.last_decode_graph.reason == "not asked for"
        osq.set_beam_graph(True)                                                      # the package switch asks as the argument does
        parent = unforced.generate(s.ids, attention_mask=s.mask, beam_graph=False, **PARENT, **KW)
        got = unforced.generate(s.ids, attention_mask=s.mask, **KW)
        assert torch.equal(got, parent) and unforced.last_beam_graph.captured == 2 and unforced.last_beam_graph.reason is None
        assert unforced.last_beam_graph.capture_seconds > 0 and unforced.last_decode_graph.capture_seconds > 0
        off = unforced.generate(s.ids, attention_mask=s.mask, beam_graph=False, **KW)
        assert torch.equal(off, want) and unforced.last_beam_graph.reason == "not asked for" and _counts(unforced) == plain

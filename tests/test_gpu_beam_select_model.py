"""generate(beam_select=True) (model/generation.py::_select_continuations, ops.beam_select) on the tiny W6A6 LSQ+ BART of
test_gpu_bart_decode.py: beam search with no_repeat_ngram_size=2 and min_length=5 returns the tokens of the torch lines --
issued, with graph=True, with cache_codes=True and with use_cache=False -- and says how many steps took the kernel.

What entitles the test to equal tokens: the eager run's inputs of every step are recorded by wrapping the helper, and on
every step the smallest distance between two distinct neighbours among ranks 1 .. keep + 1 (tests/_beam_select.py, float64)
is asserted to be at least 1e-4, five times the kernel's value bound (tests/test_gpu_beam_select.py)."""
import copy

import pytest
import torch

import _beam_select as BS
from test_gpu_bart_decode import setup  # noqa: F401  (that file's module fixture)

pytestmark = pytest.mark.gpu

KW = dict(num_beams=3, max_length=12, min_length=5, no_repeat_ngram_size=2)
EOS = 2
VARIANTS = {"issued": {}, "graph": dict(graph=True), "codes": dict(cache_codes=True), "no-cache": dict(use_cache=False)}


@pytest.fixture()
def switches():
    from outlier_suppression_amd import _hip, util_layernorm as UL
    _hip.load()                      # the first load applies the environment's tier, these switches included
    old = UL.BEAM_SELECT, UL.GRAPH_DECODE, UL.CACHE_CODES
    UL.BEAM_SELECT = False
    yield UL
    UL.BEAM_SELECT, UL.GRAPH_DECODE, UL.CACHE_CODES = old


@pytest.fixture(scope="module")
def unforced(setup):
    """The model without its configuration's forced_eos_token_id: no step of a call is a forced one."""
    m = copy.deepcopy(setup.q)
    for cfg in (m.config, m.generation_config):
        if cfg is not None:
            cfg.forced_eos_token_id = None
    return m


def _recording(monkeypatch):
    """Every call of the helper of steps a-c: (logits, token history, running scores, keep) on the CPU."""
    from outlier_suppression_amd.model import generation
    seen = []
    real = generation._select_continuations

    def recorded(logits, flat, running_scores, *rest, **kw):
        seen.append((logits.float().cpu(), flat.cpu(), running_scores.cpu(), rest[4]))
        return real(logits, flat, running_scores, *rest, **kw)
    monkeypatch.setattr(generation, "_select_continuations", recorded)
    return seen


def _assert_gaps(seen, forced_bos=False):
    for logits, flat, running, keep in seen:
        cur = flat.shape[1]
        if forced_bos and cur == 1:      # a forced step: one candidate per beam at 0, the rest -inf; torch lines on both sides
            continue
        gap = BS.gap(logits.numpy(), running.numpy(), keep, flat.numpy(), cur, KW["no_repeat_ngram_size"],
                     (EOS,) if cur < KW["min_length"] else ())
        assert gap >= 1e-4, f"step at length {cur}: gap {gap:.3g}: the model's logits do not separate the candidates"


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_a_same_tokens_and_every_step_selected(setup, unforced, switches, monkeypatch, variant):
    s, m, kw = setup, unforced, dict(KW, **VARIANTS[variant])
    seen = _recording(monkeypatch)
    with torch.no_grad():
        want = m.generate(s.ids, attention_mask=s.mask, beam_select=False, **kw)
        info, steps = m.last_beam_select, len(seen)
        assert steps >= 4 and (info.selected, info.eager, info.reason) == (0, steps, "not asked for"), info
        _assert_gaps(seen)
        del seen[:]
        got = m.generate(s.ids, attention_mask=s.mask, beam_select=True, **kw)
    info = m.last_beam_select
    assert torch.equal(got, want), (got, want)
    assert len(seen) == steps and (info.selected, info.eager, info.reason) == (steps, 0, None), info
    if variant == "graph":
        assert m.last_decode_graph.captured == 2 and m.last_decode_graph.reason is None, m.last_decode_graph


def test_b_forced_steps_take_the_torch_lines(setup, unforced, switches, monkeypatch):
    s = setup
    seen = _recording(monkeypatch)
    with torch.no_grad():
        # forced_bos_token_id: exactly the first step
        want = unforced.generate(s.ids, attention_mask=s.mask, forced_bos_token_id=5, **KW)
        _assert_gaps(seen, forced_bos=True)
        steps = len(seen)
        got = unforced.generate(s.ids, attention_mask=s.mask, forced_bos_token_id=5, beam_select=True, **KW)
        info = unforced.last_beam_select
        assert torch.equal(got, want) and (got[:, 1] == 5).all()
        assert (info.selected, info.eager, info.reason) == (steps - 1, 1, None), info
        # the configuration's forced_eos_token_id: the step at max_length - 1, where the call gets there
        del seen[:]
        want = s.q.generate(s.ids, attention_mask=s.mask, **KW)
        _assert_gaps(seen[:-1] if seen[-1][1].shape[1] == KW["max_length"] - 1 else seen)
        last = sum(1 for _, flat, _, _ in seen if flat.shape[1] == KW["max_length"] - 1)
        steps = len(seen)
        got = s.q.generate(s.ids, attention_mask=s.mask, beam_select=True, **KW)
        info = s.q.last_beam_select
        assert torch.equal(got, want)
        assert (info.selected, info.eager, info.reason) == (steps - last, last, None), info


def test_c_the_switch(setup, unforced, switches):
    import outlier_suppression_amd as osq
    s = setup
    with torch.no_grad():
        want = unforced.generate(s.ids, attention_mask=s.mask, **KW)                 # unset: the torch lines
        assert unforced.last_beam_select.selected == 0 and unforced.last_beam_select.reason == "not asked for"
        osq.set_beam_select(True)
        got = unforced.generate(s.ids, attention_mask=s.mask, **KW)
        assert unforced.last_beam_select.selected >= 4 and unforced.last_beam_select.eager == 0
        off = unforced.generate(s.ids, attention_mask=s.mask, beam_select=False, **KW)
        assert unforced.last_beam_select.selected == 0
        greedy = unforced.generate(s.ids, attention_mask=s.mask, max_length=8, num_beams=1)
        assert unforced.last_beam_select.selected == 0 and "greedy" in unforced.last_beam_select.reason
    assert torch.equal(got, want) and torch.equal(off, want) and greedy.shape[0] == 3


def test_d_a_processor_the_kernel_does_not_restate_is_a_reason(setup, unforced, switches, monkeypatch):
    """Anything else in the processor list: every step takes the torch lines and the call says why."""
    from transformers.generation.logits_process import LogitsProcessor
    from outlier_suppression_amd.model import generation

    class Identity(LogitsProcessor):
        def __call__(self, input_ids, scores):
            return scores
    real = generation._processors

    def with_identity(*a, **kw):
        procs = real(*a, **kw)
        procs.append(Identity())
        return procs
    s = setup
    with torch.no_grad():
        want = unforced.generate(s.ids, attention_mask=s.mask, **KW)
        monkeypatch.setattr(generation, "_processors", with_identity)
        got = unforced.generate(s.ids, attention_mask=s.mask, beam_select=True, **KW)
    info = unforced.last_beam_select
    assert torch.equal(got, want) and info.selected == 0 and info.eager >= 4 and "Identity" in info.reason, info

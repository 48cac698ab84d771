"""generate(greedy_advance=True) and generate(greedy_graph=True) (model/generation.py::_greedy_advanced, ops.greedy_advance,
graph_decode.GreedyStepGraph) on the tiny W6A6 LSQ+ BART of test_gpu_bart_decode.py: greedy decoding returns the tokens of the
switches off, torch.equal -- with graph and cache_codes each on and off and with use_cache=False, under min_length, the
n-gram rule with a forced bos, the configuration's forced eos, and a set of eos ids on which rows finish at different steps (so
that pad is written) -- stops on the same step, and says that every step took the kernel; the whole step as one captured graph
gives the same tokens from one graph, the forced eos of the last step a replay like any other."""
import copy
import itertools
from types import SimpleNamespace as NS

import pytest
import torch

from test_gpu_bart_decode import setup  # noqa: F401  (that file's module fixture)

pytestmark = pytest.mark.gpu

L = 12
VARIANTS = [dict(graph=g, cache_codes=c) for g, c in itertools.product((False, True), repeat=2)] + [dict(use_cache=False)]
# name -> (the model without its forced eos?, generate()'s arguments)
CONFIGS = {
    "min-length": (True, dict(max_length=L, min_length=8)),
    "ngram-min-length-forced-bos": (True, dict(max_length=L, no_repeat_ngram_size=2, min_length=10, forced_bos_token_id=0)),
    "forced-eos": (False, dict(max_length=L, min_length=5)),
    "rows-finish-apart": (True, None),
}


@pytest.fixture()
def switches():
    from outlier_suppression_amd import _hip, util_layernorm as UL
    _hip.load()                      # the first load applies the environment's tier, these switches included
    names = ("GREEDY_GRAPH", "GREEDY_ADVANCE", "BEAM_GRAPH", "GRAPH_DECODE", "CACHE_CODES")
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


def _finish_steps(tokens, eos):
    """Per row of a sequence decoded WITHOUT an eos: the first generated position holding one of ``eos`` (None: none)."""
    steps = []
    for row in tokens[:, 1:].tolist():
        hits = [i + 1 for i, t in enumerate(row) if t in eos]
        steps.append(hits[0] if hits else None)
    return steps


def _encoder_sensitive(setup, q_scale, v_scale):
    """The tiny BART with its cross-attention queries and values scaled up, quantized and calibrated as test_gpu_bart_decode's
    is: the plain model decodes the same tokens for every input (the decoder outweighs what it reads from the encoder), and
    rows that decode alike finish alike."""
    from test_gpu_bart_decode import A_Q, W_Q
    from outlier_suppression_amd.quant_model import quantize_model
    from outlier_suppression_amd.quantization import disable_all, enable_calibration_woquantization, enable_quantization
    fp = copy.deepcopy(setup.fp)
    with torch.no_grad():
        for layer in fp.model.decoder.layers:
            layer.encoder_attn.q_proj.weight.mul_(q_scale)
            layer.encoder_attn.v_proj.weight.mul_(v_scale)
    m = quantize_model(fp, W_Q, A_Q).to(setup.dev).eval()
    enable_calibration_woquantization(m)
    with torch.no_grad():
        m(setup.ids, setup.mask, decoder_input_ids=setup.dec)
    disable_all(m)
    enable_quantization(m)
    for cfg in (m.config, m.generation_config):
        if cfg is not None:
            cfg.forced_eos_token_id = None
    return m


@pytest.fixture(scope="module")
def apart(setup):
    """A model and generate()'s arguments under which the rows finish on an eos at different steps: the eos ids are taken from
    what the model decodes without one (a row's tokens up to its first eos do not depend on the eos set), one or two of them
    such that two rows meet theirs at different positions before the last, and the call lasts long enough to capture a step."""
    base = dict(max_length=L, min_length=0, no_repeat_ngram_size=2, pad_token_id=1)
    tried = []
    for q_scale, v_scale in ((100, 30), (300, 100), (1000, 300)):
        m = _encoder_sensitive(setup, q_scale, v_scale)
        with torch.no_grad():
            free = m.generate(setup.ids, attention_mask=setup.mask, eos_token_id=[119], **base).cpu()
        tried.append(free.tolist())
        seen = sorted(set(free[:, 1:].flatten().tolist()) - {1, 119})
        for eos in [[t] for t in seen] + [list(p) for p in itertools.combinations(seen, 2)]:
            every = _finish_steps(free, eos)
            ends = [s for s in every if s is not None and s < L - 1]
            if len(set(ends)) >= 2 and max(L - 1 if s is None else s for s in every) >= 5:
                return NS(model=m, kw=dict(base, eos_token_id=eos))
    pytest.fail(f"no eos set makes rows of {tried} finish at different steps")


def _kw(name, setup, unforced, apart):
    """(the model, generate()'s arguments) of a configuration."""
    plain, kw = CONFIGS[name]
    if kw is None:
        return apart.model, apart.kw
    return (unforced if plain else setup.q), kw


@pytest.mark.parametrize("name", list(CONFIGS))
@pytest.mark.parametrize("variant", VARIANTS, ids=("plain", "codes", "graph", "graph-codes", "no-cache"))
def test_a_same_tokens_same_steps(setup, unforced, switches, apart, variant, name):
    m, kw = _kw(name, setup, unforced, apart)
    kw = dict(kw, **variant)
    with torch.no_grad():
        want = m.generate(setup.ids, attention_mask=setup.mask, greedy_advance=False, **kw)
        info, steps = m.last_greedy_advance, want.shape[1] - 1
        assert (info.advanced, info.eager, info.reason) == (0, steps, "not asked for"), info
        got = m.generate(setup.ids, attention_mask=setup.mask, greedy_advance=True, **kw)
    info = m.last_greedy_advance
    assert got.shape == want.shape and got.dtype == want.dtype and torch.equal(got, want), (got, want)
    assert (info.advanced, info.eager, info.reason) == (steps, 0, None), info
    assert m.last_greedy_graph.reason == "not asked for"
    if variant.get("graph"):
        assert m.last_decode_graph.captured == 1 and m.last_decode_graph.reason is None, m.last_decode_graph
        assert m.last_decode_graph.capture_seconds > 0 and m.last_greedy_graph.capture_seconds == 0
    if name == "rows-finish-apart":                       # asserted on the torch result: rows end apart, pad is written after
        ends = _finish_steps(want.cpu(), kw["eos_token_id"])
        early = [e for e in ends if e is not None and e < want.shape[1] - 1]
        assert len(set(ends)) >= 2 and early, ends
        rows = want.cpu().tolist()
        assert all(set(rows[r][e + 1:]) == {1} for r, e in enumerate(ends) if e is not None and e + 1 < want.shape[1])
    if name == "forced-eos":
        assert steps == L - 1 and (want[:, -1] == 2).all()
    if name == "ngram-min-length-forced-bos":
        assert (want[:, 1] == 0).all()


@pytest.mark.parametrize("name", list(CONFIGS))
@pytest.mark.parametrize("codes", (False, True), ids=("fp32-cache", "codes"))
def test_b_whole_step_as_one_graph(setup, unforced, switches, apart, codes, name):
    m, kw = _kw(name, setup, unforced, apart)
    kw = dict(kw, cache_codes=codes)
    with torch.no_grad():
        want = m.generate(setup.ids, attention_mask=setup.mask, graph=True, **kw)      # the same model step, replayed alone
        steps = want.shape[1] - 1
        assert m.last_greedy_graph.reason == m.last_greedy_advance.reason == "not asked for"
        assert (m.last_decode_graph.captured, m.last_decode_graph.replays) == (1, steps - 2)
        assert m.last_decode_graph.capture_seconds > 0
        got = m.generate(setup.ids, attention_mask=setup.mask, greedy_graph=True, **kw)
    info = m.last_greedy_graph
    assert got.shape == want.shape and torch.equal(got, want), (got, want)
    assert steps >= 4 and info.reason is None and info.captured == 1 and info.replays >= 1, info
    # steps 0 and 1 run as before; every later one is a replay, the one on which the forced eos fires included
    assert info.replays == steps - 2, (info, steps)
    assert (m.last_greedy_advance.advanced, m.last_greedy_advance.eager) == (steps, 0)
    assert (m.last_decode_graph.captured, m.last_decode_graph.replays, m.last_decode_graph.reason) == (1, steps - 2, None)
    assert info.capture_seconds > 0 and m.last_decode_graph.capture_seconds > 0      # the one capture path times into both
    if name == "forced-eos":
        assert steps == L - 1 and (want[:, -1] == 2).all()


def test_c_where_the_whole_step_is_not_captured(setup, unforced, switches):
    s = setup
    with torch.no_grad():
        for max_length in (2, 3):                          # too short to reach the third step
            short = dict(max_length=max_length, min_length=max_length)              # no row ends on an eos before
            want = unforced.generate(s.ids, attention_mask=s.mask, **short)
            got = unforced.generate(s.ids, attention_mask=s.mask, greedy_graph=True, **short)
            info = unforced.last_greedy_graph
            assert torch.equal(got, want) and info.captured == 0 and "before a step could be captured" in info.reason, info
            assert unforced.last_greedy_advance.advanced == max_length - 1
        kw = dict(max_length=L, min_length=8)
        want = unforced.generate(s.ids, attention_mask=s.mask, **kw)
        for given in ("graph", "greedy_advance"):
            got = unforced.generate(s.ids, attention_mask=s.mask, greedy_graph=True, **{given: False}, **kw)
            assert torch.equal(got, want) and unforced.last_greedy_graph.reason == f"{given}=False was passed"
            assert unforced.last_greedy_graph.captured == 0
        uncached = unforced.generate(s.ids, attention_mask=s.mask, use_cache=False, **kw)
        got = unforced.generate(s.ids, attention_mask=s.mask, greedy_graph=True, use_cache=False, **kw)
        assert torch.equal(got, uncached) and "use_cache=False" in unforced.last_greedy_graph.reason
        assert unforced.last_greedy_advance.reason == "not asked for"
        unforced.generate(s.ids, attention_mask=s.mask, greedy_graph=True, greedy_advance=True, num_beams=3, **kw)
        assert "beam search" in unforced.last_greedy_graph.reason and "beam search" in unforced.last_greedy_advance.reason


def test_d_the_switches(setup, unforced, switches):
    import outlier_suppression_amd as osq
    s, kw = setup, dict(max_length=L, min_length=8)
    with torch.no_grad():
        want = unforced.generate(s.ids, attention_mask=s.mask, **kw)                  # unset: the torch lines
        assert unforced.last_greedy_advance.advanced == 0 and unforced.last_greedy_advance.reason == "not asked for"
        osq.set_greedy_advance(True)
        got = unforced.generate(s.ids, attention_mask=s.mask, **kw)
        assert torch.equal(got, want) and unforced.last_greedy_advance.advanced == want.shape[1] - 1
        assert unforced.last_greedy_advance.eager == 0 and unforced.last_decode_graph.reason == "not asked for"
        off = unforced.generate(s.ids, attention_mask=s.mask, greedy_advance=False, **kw)
        assert torch.equal(off, want) and unforced.last_greedy_advance.advanced == 0
        osq.set_greedy_advance(False)
        osq.set_greedy_graph(True)
        got = unforced.generate(s.ids, attention_mask=s.mask, **kw)
        assert torch.equal(got, unforced.generate(s.ids, attention_mask=s.mask, greedy_graph=False, graph=True, **kw))
        assert unforced.last_greedy_graph.reason == "not asked for"
        got = unforced.generate(s.ids, attention_mask=s.mask, **kw)
        assert unforced.last_greedy_graph.captured == 1 and unforced.last_greedy_graph.reason is None
        assert unforced.last_greedy_graph.capture_seconds > 0 and unforced.last_decode_graph.capture_seconds > 0
        off = unforced.generate(s.ids, attention_mask=s.mask, greedy_graph=False, **kw)
        assert torch.equal(off, want) and unforced.last_greedy_graph.reason == "not asked for"
        assert unforced.last_greedy_advance.advanced == 0 and unforced.last_decode_graph.reason == "not asked for"


def test_e_beam_graph_at_one_beam_answers_what_it_did(setup, unforced, switches):
    s = setup
    with torch.no_grad():
        want = unforced.generate(s.ids, attention_mask=s.mask, max_length=8, num_beams=1)
        got = unforced.generate(s.ids, attention_mask=s.mask, beam_graph=True, max_length=8, num_beams=1)
    assert torch.equal(got, want)
    assert "greedy" in unforced.last_beam_graph.reason and unforced.last_decode_graph.reason == "not asked for"
    assert unforced.last_greedy_advance.reason == unforced.last_greedy_graph.reason == "not asked for"

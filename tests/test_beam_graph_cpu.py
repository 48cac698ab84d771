"""What a machine without a GPU can say about generate(beam_graph=True): the divisor tables of ops.beam_advance_at
(ops.beam_div_tables) hold, bit for bit, float32 of the Python expressions of generation._beam_search_advanced; the switch is
off by default and reaches the environment; on the CPU a call decodes as without it and says why; the two entry points are
listed in the header and bound."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _words(t):
    return t.numpy().view(np.uint32)


@pytest.mark.parametrize("reciprocal", [False, True], ids=["divide", "reciprocal"])
@pytest.mark.parametrize("early_stopping", [False, True, "never"], ids=str)
@pytest.mark.parametrize("length_penalty", [0.0, 0.8, 1.0, 2.0])
@pytest.mark.parametrize("max_length", [2, 8, 70])
def test_tables_are_float32_of_the_search_expressions(max_length, length_penalty, early_stopping, reciprocal):
    from outlier_suppression_amd import ops
    len_table, best_table = ops.beam_div_tables(max_length, length_penalty, early_stopping, reciprocal, torch.device("cpu"))
    for t in (len_table, best_table):
        assert t.dtype == torch.float32 and tuple(t.shape) == (max_length,) and t.is_contiguous()
    prompt = 1
    for cur in range(1, max_length):
        # the lines of _beam_search_advanced, then what osq_beam_advance makes of the two doubles
        best_len = (max_length - prompt) if (early_stopping == "never" and length_penalty > 0.0) else (cur + 1 - prompt)
        len_div, best_div = (cur + 1 - prompt) ** length_penalty, best_len ** length_penalty
        want = [np.float32(1.0 / float(d)) if reciprocal else np.float32(float(d)) for d in (len_div, best_div)]
        got = [len_table[cur], best_table[cur]]
        for g, w in zip(got, want):
            assert _words(g.reshape(1))[0] == np.array([w], dtype=np.float32).view(np.uint32)[0], (cur, float(g), float(w))


def test_tables_follow_the_prompt():
    from outlier_suppression_amd import ops
    one = ops.beam_div_tables(12, 0.8, False, True, torch.device("cpu"))
    three = ops.beam_div_tables(12, 0.8, False, True, torch.device("cpu"), prompt=3)
    for a, b in zip(one, three):
        assert np.array_equal(_words(a[1:10]), _words(b[3:12]))
        assert bool(torch.isnan(b[:3]).all()) and bool(torch.isnan(a[:1]).all())


def test_entry_points_are_listed_and_bound():
    from outlier_suppression_amd import _hip
    header = open(os.path.join(ROOT, "include", "osq_hip.h")).read()
    above = header[:header.index("#define OSQ_ABI_VERSION")]
    added = set(re.findall(r"osq_\w+", re.search(r"Added within 10 \(no existing signature changed\):(.*?)\*/", above, re.S).group(1)))
    for name, count in (("osq_beam_select_at", 21), ("osq_beam_advance_at", 35)):
        assert name in added
        decl = re.search(r"^int %s\((.*?)\);" % name, header, re.M | re.S)
        assert decl, name
        assert len(decl.group(1).split(",")) == len(_hip.SIGNATURES[name][1]) == count
    assert re.search(r"#define OSQ_ABI_VERSION 10\b", header) and _hip.ABI_VERSION == 10


@pytest.fixture()
def switch():
    from outlier_suppression_amd import util_layernorm as UL
    old = UL.BEAM_GRAPH
    yield UL
    UL.BEAM_GRAPH = old


@pytest.mark.parametrize("value, want", [(None, False), ("", False), ("0", False), ("1", True), ("yes", True)])
def test_environment_variable(value, want):
    import outlier_suppression_amd as osq
    env = {} if value is None else {"OSQ_BEAM_GRAPH": value}
    assert osq.beam_graph_from_environment(env) is want


def test_switch_is_off_by_default_and_reaches_reset_tier(switch, monkeypatch):
    import outlier_suppression_amd as osq
    from outlier_suppression_amd import ops
    assert switch.BEAM_GRAPH is False or os.environ.get("OSQ_BEAM_GRAPH", "") not in ("", "0")
    osq.set_beam_graph()
    assert switch.BEAM_GRAPH is True
    osq.set_beam_graph(False)
    assert switch.BEAM_GRAPH is False
    monkeypatch.setattr(ops, "set_tuning", lambda key, value, lib=None: None)
    monkeypatch.setenv("OSQ_BEAM_GRAPH", "1")
    osq.reset_tier()
    assert switch.BEAM_GRAPH is True
    monkeypatch.delenv("OSQ_BEAM_GRAPH")
    osq.reset_tier()
    assert switch.BEAM_GRAPH is False


def test_generate_on_the_cpu_decodes_as_without_the_switch_and_says_why(switch):
    from test_bart_decode_cpu import batch, tiny_bart, wrapped
    q = wrapped(tiny_bart())
    ids, mask = batch()
    kw = dict(attention_mask=mask, max_length=12, num_beams=3, min_length=5, no_repeat_ngram_size=2)
    with torch.no_grad():
        want = q.generate(ids, **kw)
        info = q.last_beam_graph
        assert (info.captured, info.replays, info.issued, info.reason) == (0, 0, 0, "not asked for"), info
        got = q.generate(ids, beam_graph=True, **kw)
        assert torch.equal(got, want)
        info = q.last_beam_graph
        assert (info.captured, info.replays, info.issued) == (0, 0, 0) and "CPU" in info.reason, info
        # the call fell back to what it is without the switch: the three it would have implied were not asked for
        assert q.last_decode_graph.reason == q.last_beam_select.reason == q.last_beam_advance.reason == "not asked for"
        switch.BEAM_GRAPH = True                       # the package switch asks as the argument does
        assert torch.equal(q.generate(ids, **kw), want) and "CPU" in q.last_beam_graph.reason
        assert torch.equal(q.generate(ids, beam_graph=False, **kw), want) and q.last_beam_graph.reason == "not asked for"
        assert torch.equal(q.generate(ids, beam_advance=False, **kw), want)
        assert "beam_advance=False" in q.last_beam_graph.reason
        q.generate(ids, attention_mask=mask, max_length=6, num_beams=1)
        assert "greedy" in q.last_beam_graph.reason

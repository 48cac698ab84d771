"""CPU side of the nucleus over the whole vocabulary (csrc/sample_nucleus.hip, ops.sample_nucleus, sample(sample_nucleus=True)):
the numpy restatement of the kernel's SEARCH (tests/_sample_nucleus.py: bisections over keys, the tie arithmetic) returns the
token of the sort-and-cumulate restatement (tests/_sample_advance.py) on the cases the GPU file plants, and so do the torch
lines (sampling.select_torch): the cases' margins guarantee it.  The header lists and declares the entry points, the switch
parses as the others do, and on the CPU sample(sample_nucleus=True) returns the torch lines' tokens with a reason."""
import os
import re

import numpy as np
import pytest
import torch

import _sample_advance as SA
import _sample_nucleus as NU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def planted_cases():
    """(label, case, draws, tokens): what tests/test_gpu_sample_nucleus.py plants, at the sizes it uses."""
    out = []
    rng = np.random.default_rng(21)
    for vocab in (50265, NU.MAX_VOCAB):
        for label, place in NU.places(vocab):
            out.append((f"cut at {label}, vocab {vocab}",) + NU.cut_case(rng, vocab, place))
    out.append(("dense",) + NU.dense_case(np.random.default_rng(22)))
    for vocab, top_p in ((4097, 0.25), (4097, 0.5), (50265, 0.999)):
        out.append((f"flat {vocab} {top_p}",) + NU.flat_case(rng, vocab, top_p))
    out.append(("tie group",) + NU.tie_group_case(rng))
    return out


CASES = planted_cases()


@pytest.mark.parametrize("label, case, u, want", CASES, ids=[c[0] for c in CASES])
def test_the_search_and_the_torch_lines_return_the_planted_tokens(label, case, u, want):
    from outlier_suppression_amd.model import sampling
    sv = SA.row(case, 0)
    for b, (draw, token) in enumerate(zip(u, want)):
        assert SA.pick(sv, draw)[0] == token, (label, b)
        got, kept = NU.search(case["logits"][b], SA.banned(case, b), case["temperature"], case["top_p"], draw)
        assert (got, kept) == (token, sv.tokens.size), (label, b, got, kept)
    lines = sampling.select_torch(torch.from_numpy(case["logits"]), torch.from_numpy(u), case["temperature"], 0, case["top_p"])
    assert lines.tolist() == list(want), label


def test_the_search_equals_the_restatement_on_random_rows():
    from outlier_suppression_amd.model import sampling
    rng = np.random.default_rng(23)
    checked = 0
    for vocab in (1, 2, 65, 1025, 4097):
        case = SA.make(rng, 3, vocab, 9, 5, 0.8, 0, 0.9, ngram=2, eos=(min(2, vocab - 1),), pad=0, min_length=7)
        for seed in range(8):
            u = sampling.uniforms(seed, 3, 5).numpy()
            for b in range(3):
                sv = SA.row(case, b)
                if not SA.away_from_boundaries(sv, u[b]) or (np.abs(sv.above - 0.9) < SA.MARGIN).any():
                    continue
                checked += 1
                got, kept = NU.search(case["logits"][b], SA.banned(case, b), 0.8, 0.9, u[b])
                assert (got, kept) == (SA.pick(sv, u[b])[0], sv.tokens.size), (vocab, seed, b)
    assert checked >= 60, checked


def test_degenerate_rows_of_the_search():
    x = np.full(37, -np.inf, dtype=np.float32)
    assert NU.search(x, set(), 1.0, 0.9, 0.5) == (0, 0)
    x[[4, 30]] = np.inf                                                   # +inf weighs 1 each
    assert NU.search(x, set(), 1.0, 0.9, 0.25)[0] == 4 and NU.search(x, set(), 1.0, 0.9, 0.75)[0] == 30
    assert NU.search(x, {4}, 1.0, 0.9, 0.25) == (30, 1)
    x = np.array([0.0, 3.0, -0.0, 1.0], dtype=np.float32)                 # signed zeros are one value
    assert [NU.search(x, set(), 1.0, 1.0, u)[0] for u in (0.0, 0.9, 0.93, NU.LAST_U)] == [1, 3, 0, 2]
    assert NU.search(x, set(), 1.0, 1e-6, NU.LAST_U) == (1, 1)            # rank 0 always stays


def test_entry_points_are_listed_and_bound():
    from outlier_suppression_amd import _hip
    header = open(os.path.join(ROOT, "include", "osq_hip.h")).read()
    above = header[:header.index("#define OSQ_ABI_VERSION")]
    added = re.search(r"Added within 10 \(no existing signature changed\):(.*?)\*/", above, re.S).group(1)
    for name, count in (("osq_sample_nucleus_workspace_bytes", 2), ("osq_sample_nucleus", 25), ("osq_sample_nucleus_at", 28)):
        assert name in set(re.findall(r"osq_\w+", added)), name
        decl = re.search(r"^(?:int|size_t) %s\((.*?)\);" % name, header, re.M | re.S)
        assert decl, f"{name} is not declared"
        assert len(decl.group(1).split(",")) == len(_hip.SIGNATURES[name][1]) == count, name
    assert "#define OSQ_ABI_VERSION 10" in header
    makefile = open(os.path.join(ROOT, "outlier_suppression_amd", "csrc", "Makefile")).read()
    assert makefile.count("sample_nucleus.hip") == 2        # the library and its development build
    lib = _hip.load()
    assert int(lib.osq_sample_nucleus_workspace_bytes(3, 50265)) == 12
    assert int(lib.osq_sample_nucleus_workspace_bytes(3, NU.MAX_VOCAB)) == 12
    assert int(lib.osq_sample_nucleus_workspace_bytes(3, NU.MAX_VOCAB + 1)) == 0
    assert int(lib.osq_sample_nucleus_workspace_bytes(0, 50)) == 0


@pytest.fixture()
def switch():
    from outlier_suppression_amd import util_layernorm as UL
    old = UL.SAMPLE_ADVANCE, UL.SAMPLE_GRAPH, UL.SAMPLE_NUCLEUS
    yield UL
    UL.SAMPLE_ADVANCE, UL.SAMPLE_GRAPH, UL.SAMPLE_NUCLEUS = old


def test_switch_and_environment_reach_reset_tier(switch, monkeypatch):
    import outlier_suppression_amd as osq
    from outlier_suppression_amd import ops
    from_env = osq.sample_nucleus_from_environment
    name = "OSQ_SAMPLE_NUCLEUS"
    assert [from_env(e) for e in ({}, {name: ""}, {name: "0"}, {name: "1"})] == [False, False, False, True]
    assert switch.SAMPLE_NUCLEUS is False                                  # off by default
    osq.set_sample_nucleus()
    assert switch.SAMPLE_NUCLEUS is True
    osq.set_sample_nucleus(False)
    assert switch.SAMPLE_NUCLEUS is False
    monkeypatch.setattr(ops, "set_tuning", lambda key, value, lib=None: None)
    monkeypatch.setenv(name, "1")
    osq.reset_tier()
    assert switch.SAMPLE_NUCLEUS is True
    monkeypatch.delenv(name)
    osq.reset_tier()
    assert switch.SAMPLE_NUCLEUS is False


def test_why_not():
    from types import SimpleNamespace as NS
    from outlier_suppression_amd.model import generation as G
    plan = NS(reason=None)
    assert G._sample_why_not(plan, 0, 0.9) == "top_p below 1 without top_k"
    assert G._sample_why_not(plan, 0, 0.9, False, 50265) == "top_p below 1 without top_k"
    assert G._sample_why_not(plan, 0, 0.9, True, 50265) is None
    assert G._sample_why_not(plan, 0, 0.9, True, NU.MAX_VOCAB + 1) == f"vocab above {NU.MAX_VOCAB}"
    assert G._sample_why_not(plan, 100, 0.9, True, 50265) == "top_k above 64"
    assert G._sample_why_not(plan, 0, 1.0, True, NU.MAX_VOCAB + 1) is None   # the whole vocabulary without a cut: sample_advance's
    assert G._sample_why_not(NS(reason="autograd is on"), 0, 0.9, True, 50265) == "autograd is on"


def test_sample_on_the_cpu_takes_the_torch_lines_and_says_why(switch):
    from test_bart_decode_cpu import batch, tiny_bart, wrapped
    q, (ids, mask) = wrapped(tiny_bart()), batch()
    kw = dict(attention_mask=mask, max_length=10, min_length=10, seed=4, top_k=0, top_p=0.9)
    want = q.sample(ids, **kw)
    assert torch.equal(q.sample(ids, sample_nucleus=True, **kw), want) and q.last_sample_advance.reason == "not asked for"
    assert torch.equal(q.sample(ids, sample_nucleus=True, sample_advance=True, **kw), want)
    assert "CPU" in q.last_sample_advance.reason and q.last_sample_advance.advanced == 0
    assert torch.equal(q.sample(ids, sample_nucleus=True, sample_graph=True, **kw), want) and "CPU" in q.last_sample_graph.reason
    switch.SAMPLE_NUCLEUS = switch.SAMPLE_ADVANCE = True
    assert torch.equal(q.sample(ids, **kw), want) and "CPU" in q.last_sample_advance.reason

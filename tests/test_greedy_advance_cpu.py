"""CPU: what greedy decoding in one kernel call (csrc/greedy_advance.hip, ops.greedy_advance, generate(greedy_advance=True),
generate(greedy_graph=True)) needs where no GPU is involved: the numpy restatement of tests/_greedy_advance.py against the
torch lines it restates -- transformers' processors as generation._processors builds them, torch.argmax, the pad / isin lines
and the loop condition of generation._greedy, on CPU tensors -- with all four outputs exactly equal, NaN, ties and signed
zeros included; the entry points in the header's list and in ``_hip.SIGNATURES``; the two switches and their environment
variables; and generate() on CPU tensors: the tokens of the torch lines, and a reason.
The kernel runs on the GPU (tests/test_gpu_greedy_advance.py, tests/test_gpu_greedy_advance_model.py)."""
import os
import re

import numpy as np
import pytest
import torch

import _greedy_advance as GA

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def torch_step(case, device="cpu"):
    """The body of generation._greedy's loop on ``device`` from a case: (token, seq_out, unfinished_out, go_on) as numpy."""
    from outlier_suppression_amd.model import generation as G
    cur, max_length = case["cur"], case["max_length"]
    eos = torch.tensor(list(case["eos"]), device=device) if len(case["eos"]) else None
    procs = G._processors(case["min_length"], eos, case["ngram"], case["forced_bos"], case["forced_eos"], max_length, device)
    seq = torch.from_numpy(case["seq"][:, :cur].copy()).to(device)
    unfinished = torch.from_numpy(case["unfinished"].astype(np.int64)).to(device)
    pad = case["pad"]
    go_on = True
    # ---- the lines of _greedy
    scores = procs(seq, torch.from_numpy(case["logits"].copy()).to(device).to(torch.float32))
    nxt = torch.argmax(scores, dim=-1)
    if eos is not None:
        nxt = nxt * unfinished + pad * (1 - unfinished)
    seq = torch.cat([seq, nxt[:, None]], dim=-1)
    if eos is not None:
        unfinished = unfinished & ~torch.isin(nxt, eos)
        if unfinished.max() == 0:
            go_on = False
    go_on = go_on and seq.shape[1] < max_length
    # ----
    seq_out = case["seq"].copy()
    seq_out[:, :cur + 1] = seq.cpu().numpy()
    return nxt.cpu().numpy(), seq_out, unfinished.cpu().numpy().astype(np.uint8), int(go_on)


def same(got, want, label):
    for name, g, w in zip(("token", "seq", "unfinished", "go_on"), got, want):
        assert np.array_equal(np.asarray(g), np.asarray(w)), (label, name, g, w)


CASES = GA.all_cases()


@pytest.mark.parametrize("label, case", CASES, ids=[label for label, _ in CASES])
def test_reference_restates_the_torch_lines(label, case):
    same(GA.reference_case(case), torch_step(case), label)


def test_cases_cover_what_they_claim():
    """The makers' cases do what their labels say: a ban changes the winner, rows finish, the stopping word takes both values."""
    by = dict(CASES)
    assert GA.reference_case(by["every token banned"])[0].tolist() == [0, 0, 0]
    assert GA.reference_case(by["an all -inf row"])[0].tolist() == [0, 0, 0]
    assert GA.reference_case(by["-0.0 before +0.0"])[0].tolist() == GA.reference_case(by["+0.0 before -0.0"])[0].tolist() == [5] * 3
    assert GA.reference_case(by["two NaNs"])[0].tolist() == [9] * 3 and GA.reference_case(by["one NaN"])[0].tolist() == [20] * 3
    assert GA.reference_case(by["a banned NaN (n-gram)"])[0].tolist() == [3] * 3
    assert GA.reference_case(by["forced bos over NaN rows"])[0].tolist() == [7] * 3
    assert GA.reference_case(by["both forced at max_length 2"])[0].tolist() == [2] * 3
    assert GA.reference_case(by["min-length 6 with 3 eos at cur 5"])[0].tolist() != GA.reference_case(by["min-length 6 with 3 eos at cur 6"])[0].tolist()
    assert GA.reference_case(by["every row finished"])[3] == 0 and GA.reference_case(by["rows already finished"])[3] == 1
    assert GA.reference_case(by["rows finish now"])[2].tolist() == [0, 1, 0]
    assert GA.reference_case(by["the last position, no eos"])[3] == 0
    for n in (1, 2, 3):                                # every n-gram size bans a would-be winner somewhere
        mine = [c for label, c in CASES if label.startswith(f"ngram {n} ")]
        assert len(mine) >= 2
        assert any(GA.reference_case(c)[0].tolist() != GA.reference_case(dict(c, ngram=0))[0].tolist() for c in mine), n
        below = [c for c in mine if c["cur"] < n]      # nothing is banned before a whole n-gram exists
        assert all(GA.reference_case(c)[0].tolist() == GA.reference_case(dict(c, ngram=0))[0].tolist() for c in below)


def test_entry_points_are_listed_and_bound():
    from outlier_suppression_amd import _hip
    header = open(os.path.join(ROOT, "include", "osq_hip.h")).read()
    above = header[:header.index("#define OSQ_ABI_VERSION")]
    added = re.search(r"Added within 10 \(no existing signature changed\):(.*?)\*/", above, re.S).group(1)
    for name, count in (("osq_greedy_advance_workspace_bytes", 2), ("osq_greedy_advance", 21), ("osq_greedy_advance_at", 24)):
        assert name in set(re.findall(r"osq_\w+", added)), name
        decl = re.search(r"^(?:int|size_t) %s\((.*?)\);" % name, header, re.M | re.S)
        assert decl, f"{name} is not declared"
        assert len(decl.group(1).split(",")) == len(_hip.SIGNATURES[name][1]) == count, name
    assert re.search(r"#define OSQ_ABI_VERSION 10\b", header) and _hip.ABI_VERSION == 10
    makefile = open(os.path.join(ROOT, "outlier_suppression_amd", "csrc", "Makefile")).read()
    assert makefile.count("greedy_advance.hip") == 2        # the library and its development build
    assert makefile.count("token_argmax.h") == 1            # the header both searches' kernels share is a dependency
    for source in ("beam_select.hip", "greedy_advance.hip"):
        text = open(os.path.join(ROOT, "outlier_suppression_amd", "csrc", source)).read()
        assert '#include "token_argmax.h"' in text and "void block_argmax(" not in text, source


@pytest.fixture()
def switch():
    from outlier_suppression_amd import util_layernorm as UL
    old = UL.GREEDY_ADVANCE, UL.GREEDY_GRAPH
    yield UL
    UL.GREEDY_ADVANCE, UL.GREEDY_GRAPH = old


@pytest.mark.parametrize("name", ["GREEDY_ADVANCE", "GREEDY_GRAPH"])
@pytest.mark.parametrize("value, want", [(None, False), ("", False), ("0", False), ("1", True), ("yes", True)])
def test_environment_variable(name, value, want):
    import outlier_suppression_amd as osq
    env = {} if value is None else {"OSQ_" + name: value}
    assert getattr(osq, name.lower() + "_from_environment")(env) is want


@pytest.mark.parametrize("name", ["GREEDY_ADVANCE", "GREEDY_GRAPH"])
def test_switch_and_environment_reach_reset_tier(switch, monkeypatch, name):
    import outlier_suppression_amd as osq
    from outlier_suppression_amd import ops
    setter = getattr(osq, "set_" + name.lower())
    assert getattr(switch, name) is False or os.environ.get("OSQ_" + name, "") not in ("", "0")
    setter()
    assert getattr(switch, name) is True
    setter(False)
    assert getattr(switch, name) is False
    monkeypatch.setattr(ops, "set_tuning", lambda key, value, lib=None: None)
    monkeypatch.setenv("OSQ_" + name, "1")
    osq.reset_tier()
    assert getattr(switch, name) is True
    monkeypatch.delenv("OSQ_" + name)
    osq.reset_tier()
    assert getattr(switch, name) is False


def test_generate_on_the_cpu_takes_the_torch_lines_and_says_why(switch):
    from test_bart_decode_cpu import batch, tiny_bart, wrapped
    q = wrapped(tiny_bart())
    ids, mask = batch()
    kw = dict(attention_mask=mask, max_length=12, min_length=5, no_repeat_ngram_size=2)
    with torch.no_grad():
        want = q.generate(ids, **kw)
        info = q.last_greedy_advance
        assert (info.advanced, info.reason) == (0, "not asked for") and info.eager >= 4
        assert q.last_greedy_graph.reason == "not asked for"
        got = q.generate(ids, greedy_advance=True, **kw)
        assert torch.equal(got, want)
        info = q.last_greedy_advance
        assert info.advanced == 0 and info.eager >= 4 and "CPU" in info.reason, info
        switch.GREEDY_ADVANCE = True                   # the package switch asks as the argument does
        assert torch.equal(q.generate(ids, **kw), want) and "CPU" in q.last_greedy_advance.reason
        assert torch.equal(q.generate(ids, greedy_advance=False, **kw), want)
        assert q.last_greedy_advance.reason == "not asked for"
        q.generate(ids, greedy_advance=True, num_beams=3, **kw)
        assert q.last_greedy_advance.advanced == 0 and "beam search" in q.last_greedy_advance.reason


def test_greedy_graph_on_the_cpu_decodes_as_without_it_and_says_why(switch):
    from test_bart_decode_cpu import batch, tiny_bart, wrapped
    q = wrapped(tiny_bart())
    ids, mask = batch()
    kw = dict(attention_mask=mask, max_length=10, min_length=4)
    with torch.no_grad():
        want = q.generate(ids, **kw)
        got = q.generate(ids, greedy_graph=True, **kw)
        info = q.last_greedy_graph
        assert torch.equal(got, want) and info.captured == 0 and "CPU" in info.reason, info
        # the switches it would imply stay as they were given
        assert q.last_decode_graph.reason == q.last_greedy_advance.reason == "not asked for"
        assert torch.equal(q.generate(ids, greedy_graph=True, graph=False, **kw), want)
        assert q.last_greedy_graph.reason == "graph=False was passed"
        assert torch.equal(q.generate(ids, greedy_graph=True, greedy_advance=False, **kw), want)
        assert q.last_greedy_graph.reason == "greedy_advance=False was passed"
        switch.GREEDY_GRAPH = True                     # the package switch asks as the argument does
        assert torch.equal(q.generate(ids, **kw), want) and "CPU" in q.last_greedy_graph.reason
        assert torch.equal(q.generate(ids, greedy_graph=False, **kw), want) and q.last_greedy_graph.reason == "not asked for"
        q.generate(ids, num_beams=3, **kw)
        assert "beam search" in q.last_greedy_graph.reason

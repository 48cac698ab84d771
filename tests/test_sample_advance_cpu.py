"""CPU: what seeded sampling (csrc/sample_advance.hip, ops.sample_advance, model/sampling.py, sample()) needs where no GPU is
involved: the host Philox against its known answers, the uniforms' format, the float64 restatement of tests/_sample_advance.py
against transformers' warpers (the kept set, tie-free inputs) and against the torch lines (sampling.sample_step_torch, draws
away from every boundary), the entry points and switches, and sample() on CPU tensors.
The kernel runs on the GPU (tests/test_gpu_sample_advance.py, tests/test_gpu_sample_advance_model.py)."""
import os
import re

import numpy as np
import pytest
import torch

import _sample_advance as SA

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KNOWN = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
         ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
         ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
          (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


@pytest.mark.parametrize("counter, key, want", KNOWN)
def test_philox_known_answers(counter, key, want):
    from outlier_suppression_amd.model import sampling
    assert sampling.philox4x32(counter, key) == want


def test_uniforms_lie_in_the_unit_interval_with_24_bits():
    from outlier_suppression_amd.model import sampling
    for seed in (0, 1, 2 ** 64 - 1, 0x123456789abcdef):
        u = sampling.uniforms(seed, 66, 31)
        assert u.dtype == torch.float32 and u.shape == (66,)
        scaled = u.double() * 2 ** 24
        assert (u >= 0).all() and (u < 1).all() and torch.equal(scaled, scaled.round())
        key = (seed & 0xffffffff, seed >> 32)
        assert int(scaled[5]) == sampling.philox4x32((5, 31, 0, 0), key)[0] >> 8
    assert not torch.equal(sampling.uniforms(7, 8, 3), sampling.uniforms(7, 8, 4))
    assert len(set(sampling.uniforms(7, 64, 3).tolist())) > 60


def _tie_free(rng, vocab, k):
    """Distinct values: k of them within a range of 2 (each then weighs a few 1e-3 of the k at the least), the rest far below."""
    return SA.spread_logits(rng, 1, vocab, [rng.choice(vocab, min(k, vocab), replace=False)], tail=-8.0)[0]


@pytest.mark.parametrize("vocab", (65, 4097))
@pytest.mark.parametrize("k, p", [(1, 0.9), (2, 0.3), (50, 0.9), (64, 0.95), (50, 1.0)])
def test_restatement_keeps_what_the_warpers_keep(vocab, k, p):
    from transformers.generation.logits_process import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    rng = np.random.default_rng(vocab * 100 + k)
    for T in (0.7, 1.0, 1.3):
        for _ in range(50):                               # drawn again until no threshold lies within the margin of top_p
            x = _tie_free(rng, vocab, k)
            case = SA.make(rng, 1, vocab, 6, 3, T, k, p, logits=x[None, :])
            if p == 1.0 or (np.abs(SA.row(case, 0).above - p) >= SA.MARGIN).all():
                break
        SA.assert_kth_distinct(case)
        SA.assert_top_p_margin(case)
        scores = TemperatureLogitsWarper(T)(None, torch.from_numpy(x)[None, :])
        scores = TopKLogitsWarper(k)(None, scores)
        if p < 1.0:
            scores = TopPLogitsWarper(p)(None, scores)
        theirs = set(torch.nonzero(scores[0] > float("-inf")).flatten().tolist())
        assert set(SA.row(case, 0).tokens.tolist()) == theirs, (T, k, p)


def _step_cases():
    rng = np.random.default_rng(3)
    out = []
    for vocab, k, p in ((37, 0, 1.0), (37, 5, 1.0), (37, 64, 0.8), (4097, 50, 0.9), (4097, 0, 1.0), (37, 0, 0.7), (200, 100, 1.0)):
        # a few heavy tokens over a light tail: a draw can lie MARGIN away from every running sum
        x = SA.spread_logits(rng, 3, vocab, [rng.choice(vocab, 12, replace=False) for _ in range(3)], tail=-12.0)
        out.append((f"vocab {vocab} k {k} p {p}", SA.make(rng, 3, vocab, 9, 4, 0.8, k, p, logits=x, ngram=2, eos=(4,), pad=1,
                                                           min_length=6, unfinished=(1, 0, 1))))
    x = rng.standard_normal((3, 37)).astype(np.float32)
    x[:, 5], x[1, 7], x[2, :] = np.nan, np.inf, -np.inf
    out.append(("NaN, +inf and an all -inf row", SA.make(rng, 3, 37, 9, 4, 1.0, 5, 1.0, logits=x)))
    out.append(("the same, the whole vocabulary", SA.make(rng, 3, 37, 9, 4, 1.0, 0, 1.0, logits=x)))
    out.append(("forced bos", SA.make(rng, 3, 37, 9, 1, 1.0, 5, 1.0, forced_bos=7, forced_eos=2, eos=(2,), pad=1)))
    out.append(("forced eos", SA.make(rng, 3, 37, 9, 8, 1.0, 5, 1.0, forced_bos=7, forced_eos=2, eos=(2,), pad=1)))
    return out


@pytest.mark.parametrize("label, case", _step_cases(), ids=[label for label, _ in _step_cases()])
def test_torch_lines_equal_the_restatement(label, case):
    from outlier_suppression_amd.model import sampling
    import _greedy_advance as GA
    bsz = case["logits"].shape[0]
    kw = GA.kernel_arguments(case)
    checked = 0
    for seed in range(40):
        u = sampling.uniforms(seed, bsz, case["cur"])
        if not all(SA.away_from_boundaries(SA.row(case, b), u[b]) for b in range(bsz)):
            continue
        checked += 1
        want = SA.reference_case(case, u.numpy())
        token, unfinished, go_on = sampling.sample_step_torch(
            torch.from_numpy(case["logits"]), torch.from_numpy(case["seq"]), case["cur"], case["max_length"], u,
            case["temperature"], case["top_k"], case["top_p"], kw["ngram"], kw["ban_ids"], kw["forced"], kw["eos_ids"], kw["pad"],
            torch.from_numpy(case["unfinished"].copy()))
        assert token.tolist() == want[0].tolist(), (label, seed)
        if kw["eos_ids"]:
            assert unfinished.tolist() == want[2].tolist()
        assert go_on == want[3]
    assert checked >= 20, checked


def test_exactly_k_survive_a_tie_and_the_smaller_token_first():
    x = np.zeros((1, 10), dtype=np.float32)
    x[0, [2, 6, 8]] = 3.0
    rng = np.random.default_rng(0)
    sv = SA.row(SA.make(rng, 1, 10, 6, 3, 1.0, 2, 1.0, logits=x), 0)
    assert sv.tokens.tolist() == [2, 6] and sv.C.tolist() == [1.0, 2.0]


def test_entry_points_are_listed_and_bound():
    from outlier_suppression_amd import _hip
    header = open(os.path.join(ROOT, "include", "osq_hip.h")).read()
    above = header[:header.index("#define OSQ_ABI_VERSION")]
    added = re.search(r"Added within 10 \(no existing signature changed\):(.*?)\*/", above, re.S).group(1)
    for name, count in (("osq_sample_advance_workspace_bytes", 3), ("osq_sample_advance", 26), ("osq_sample_advance_at", 29),
                        ("osq_sample_uniforms", 5)):
        assert name in set(re.findall(r"osq_\w+", added)), name
        decl = re.search(r"^(?:int|size_t) %s\((.*?)\);" % name, header, re.M | re.S)
        assert decl, f"{name} is not declared"
        assert len(decl.group(1).split(",")) == len(_hip.SIGNATURES[name][1]) == count, name
    makefile = open(os.path.join(ROOT, "outlier_suppression_amd", "csrc", "Makefile")).read()
    assert makefile.count("sample_advance.hip") == 2        # the library and its development build
    assert "-ffp-contract=off" in makefile


@pytest.fixture()
def switch():
    from outlier_suppression_amd import util_layernorm as UL
    old = UL.SAMPLE_ADVANCE, UL.SAMPLE_GRAPH
    yield UL
    UL.SAMPLE_ADVANCE, UL.SAMPLE_GRAPH = old


@pytest.mark.parametrize("name", ["SAMPLE_ADVANCE", "SAMPLE_GRAPH"])
def test_switch_and_environment_reach_reset_tier(switch, monkeypatch, name):
    import outlier_suppression_amd as osq
    from outlier_suppression_amd import ops
    setter = getattr(osq, "set_" + name.lower())
    from_env = getattr(osq, name.lower() + "_from_environment")
    assert [from_env(e) for e in ({}, {"OSQ_" + name: ""}, {"OSQ_" + name: "0"}, {"OSQ_" + name: "1"})] == [False, False, False, True]
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


@pytest.fixture(scope="module")
def tiny():
    from test_bart_decode_cpu import batch, tiny_bart, wrapped
    return wrapped(tiny_bart()), batch()


def test_sample_is_a_function_of_its_seed(tiny, switch):
    q, (ids, mask) = tiny
    kw = dict(attention_mask=mask, max_length=12, min_length=12, temperature=1.5)
    first = q.sample(ids, seed=11, **kw)
    assert first.shape == (3, 12) and torch.equal(q.sample(ids, seed=11, **kw), first)
    assert not torch.equal(q.sample(ids, seed=12, **kw), first)
    info = q.last_sample_advance
    assert (info.advanced, info.eager, info.reason) == (0, 11, "not asked for") and q.last_sample_graph.reason == "not asked for"
    torch.manual_seed(5)
    drawn = q.sample(ids, **kw)
    torch.manual_seed(5)
    assert torch.equal(q.sample(ids, **kw), drawn)
    assert torch.equal(q.sample(ids, seed=11, use_cache=False, **kw), first)
    assert torch.equal(q.sample(ids, seed=11, top_k=0, **kw), q.sample(ids, seed=11, top_k=0, **kw))
    # asked for on the CPU: the torch lines, and a reason
    assert torch.equal(q.sample(ids, seed=11, sample_advance=True, **kw), first) and "CPU" in q.last_sample_advance.reason
    assert torch.equal(q.sample(ids, seed=11, sample_graph=True, **kw), first) and "CPU" in q.last_sample_graph.reason
    assert q.last_sample_advance.reason == q.last_decode_graph.reason == "not asked for"
    q.sample(ids, seed=11, sample_graph=True, graph=False, **kw)
    assert q.last_sample_graph.reason == "graph=False was passed"
    switch.SAMPLE_ADVANCE = True
    assert torch.equal(q.sample(ids, seed=11, **kw), first) and "CPU" in q.last_sample_advance.reason


def test_top_k_one_is_greedy(tiny):
    q, (ids, mask) = tiny
    for kw in (dict(max_length=12, min_length=5, no_repeat_ngram_size=2),
               dict(max_length=10, min_length=4, forced_bos_token_id=0, forced_eos_token_id=2)):
        want = q.generate(ids, attention_mask=mask, **kw)
        for seed in (0, 1):
            assert torch.equal(q.sample(ids, attention_mask=mask, seed=seed, top_k=1, temperature=0.7, **kw), want)
        assert torch.equal(q.sample(ids, attention_mask=mask, seed=3, top_k=1, use_cache=False, **kw), want)


def test_a_row_that_met_eos_is_padded(tiny):
    q, (ids, mask) = tiny
    kw = dict(attention_mask=mask, max_length=12, seed=21, temperature=1.5, top_k=20, pad_token_id=1, min_length=0)
    free = q.sample(ids, eos_token_id=[119], **kw)                       # decoded without meeting an eos
    assert free.shape[1] == 12 and 119 not in free[:, 1:].flatten().tolist()
    eos = next(int(t) for t in free[0, 3:8] if int(t) != 1)              # a token row 0 draws midway becomes the eos
    got = q.sample(ids, eos_token_id=[eos], **kw)
    ends = []
    for r in range(free.shape[0]):                                       # the draws hang on (seed, row, position) alone
        hits = [i for i in range(1, 12) if int(free[r, i]) == eos]
        end = hits[0] if hits else 11
        ends.append(end)
        upto = min(end + 1, got.shape[1])
        assert torch.equal(got[r, :upto], free[r, :upto]), r
        assert (got[r, end + 1:] == 1).all(), r
    assert got.shape[1] == min(max(ends) + 1, 12) and ends[0] < 8 and got.shape[1] > ends[0] + 1


def test_sample_refuses_what_it_does_not_cover(tiny):
    q, (ids, mask) = tiny
    for kw, error in ((dict(num_beams=2), ValueError), (dict(num_return_sequences=2), ValueError), (dict(min_p=0.1), TypeError),
                      (dict(temperature=0.0), ValueError), (dict(top_p=0.0), ValueError), (dict(top_k=-1), ValueError)):
        with pytest.raises(error):
            q.sample(ids, attention_mask=mask, max_length=5, **kw)

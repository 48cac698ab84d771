"""CPU: what the beam-step selection (csrc/beam_select.hip, ops.beam_select, generate(beam_select=True)) needs where no GPU is
involved: the float64 restatement of tests/_beam_select.py against the pipeline it restates -- torch's log_softmax,
transformers' own NoRepeatNGramLogitsProcessor and MinLengthLogitsProcessor, the score add and torch.topk on the CPU -- on
tie-free cases; the two entry points in the header's list and in ``_hip.SIGNATURES``; the switch and its environment
variable; and generate(beam_select=True) on CPU tensors: the tokens of the torch lines, and a reason.
The kernel runs on the GPU (tests/test_gpu_beam_select.py, tests/test_gpu_beam_select_model.py)."""
import os
import re

import numpy as np
import pytest
import torch

import _beam_select as BS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("osq_beam_select_workspace_bytes", "osq_beam_select")


def _pipeline(logits, running, keep, seq, ngram, ban_ids, cur):
    """Steps a-c of generation._beam_search as they stand, with transformers' processors, in fp32 on the CPU."""
    from transformers.generation.logits_process import (LogitsProcessorList, MinLengthLogitsProcessor,
                                                        NoRepeatNGramLogitsProcessor)
    bsz, nb = running.shape
    vocab = logits.shape[1]
    procs = LogitsProcessorList()
    if ngram:
        procs.append(NoRepeatNGramLogitsProcessor(ngram))
    if len(ban_ids):
        procs.append(MinLengthLogitsProcessor(cur + 1, list(ban_ids)))
    flat = seq if seq is not None else torch.zeros((bsz * nb, cur), dtype=torch.long)
    log_probs = procs(flat, torch.nn.functional.log_softmax(logits, dim=-1))
    log_probs = (log_probs.view(bsz, nb, vocab) + running[:, :, None]).view(bsz, nb * vocab)
    return torch.topk(log_probs, k=keep)


def _repeating(rows, cur):
    """Histories whose suffix occurs several times: a b c a b d a b e a b ... ending in ``a b``."""
    base = [0, 1, 2, 0, 1, 3, 0, 1, 4, 0, 1, 2, 2, 0, 1]
    seq = torch.tensor([[(t + r) % 5 for t in (base * 8)[-cur:]] for r in range(rows)], dtype=torch.long)
    return seq


CASES = [  # (seed, bsz, nb, vocab, cur, ngram, ban_ids, repeating history)
    (0, 3, 2, 255, 7, 1, (), False),
    (1, 3, 2, 255, 7, 2, (), False),
    (2, 3, 6, 1025, 64, 3, (), False),
    (0, 2, 2, 257, 0, 1, (), False),          # cur = n - 1: nothing banned
    (1, 2, 2, 257, 1, 2, (), False),
    (2, 2, 2, 257, 2, 3, (), False),
    (0, 3, 2, 13, 15, 3, (), True),           # the suffix occurs several times
    (1, 3, 1, 257, 30, 2, (), True),
    (0, 3, 2, 1023, 7, 0, (2,), False),       # one and two ban_ids
    (1, 3, 6, 4099, 7, 3, (2, 4098), False),
]


@pytest.mark.parametrize("seed, bsz, nb, vocab, cur, ngram, ban_ids, repeating", CASES)
def test_reference_restates_the_pipeline(seed, bsz, nb, vocab, cur, ngram, ban_ids, repeating):
    logits, running, seq = BS.case(seed, bsz, nb, vocab, cur)
    if repeating:
        seq = _repeating(bsz * nb, cur)
        assert int((BS.banned(seq.numpy(), cur, ngram, (), bsz * nb, vocab).sum(axis=1) >= 2).sum()) == bsz * nb
    keep = min(2 * nb, vocab)
    assert BS.gap(logits.numpy(), running.numpy(), keep, seq, cur, ngram, ban_ids) >= 1e-4
    want_v, want_i = _pipeline(logits, running, keep, seq, ngram, ban_ids, cur)
    got_v, got_i = BS.reference(logits.numpy(), running.numpy(), keep, None if seq is None else seq.numpy(), cur, ngram, ban_ids)
    assert np.array_equal(got_i, want_i.numpy())
    assert np.abs(got_v - want_v.numpy().astype(np.float64)).max() <= 1e-5


def test_reference_order_rule():
    """Ties by smaller index, NaN first, -inf ties in index order: the part torch.topk leaves open."""
    v = np.array([1.0, 3.0, -np.inf, 3.0, np.nan, -np.inf, 2.0, np.nan])
    assert BS.order(v).tolist() == [4, 7, 1, 3, 6, 0, 2, 5]


def test_entry_points_are_listed_and_bound():
    from outlier_suppression_amd import _hip
    header = open(os.path.join(ROOT, "include", "osq_hip.h")).read()
    above = header[:header.index("#define OSQ_ABI_VERSION")]
    added = re.search(r"Added within 10 \(no existing signature changed\):(.*?)\*/", above, re.S).group(1)
    listed = set(re.findall(r"osq_\w+", added))
    for name in SYMBOLS:
        assert name in listed, f"{name} is not in the header's 'Added within 10' list"
        assert re.search(r"^(int|size_t) " + name + r"\(", header, re.M), f"{name} is not declared"
        assert name in _hip.SIGNATURES
    assert re.search(r"#define OSQ_ABI_VERSION 10\b", header) and _hip.ABI_VERSION == 10
    assert len(_hip.SIGNATURES["osq_beam_select"][1]) == 18 and len(_hip.SIGNATURES["osq_beam_select_workspace_bytes"][1]) == 4


@pytest.fixture()
def switch():
    from outlier_suppression_amd import util_layernorm as UL
    old = UL.BEAM_SELECT
    yield UL
    UL.BEAM_SELECT = old


@pytest.mark.parametrize("value, want", [(None, False), ("", False), ("0", False), ("1", True), ("yes", True)])
def test_environment_variable(value, want):
    import outlier_suppression_amd as osq
    env = {} if value is None else {"OSQ_BEAM_SELECT": value}
    assert osq.beam_select_from_environment(env) is want


def test_switch_and_environment_reach_reset_tier(switch, monkeypatch):
    import outlier_suppression_amd as osq
    from outlier_suppression_amd import ops
    assert switch.BEAM_SELECT is False or os.environ.get("OSQ_BEAM_SELECT", "") not in ("", "0")
    osq.set_beam_select()
    assert switch.BEAM_SELECT is True
    osq.set_beam_select(False)
    assert switch.BEAM_SELECT is False
    monkeypatch.setattr(ops, "set_tuning", lambda key, value, lib=None: None)
    monkeypatch.setenv("OSQ_BEAM_SELECT", "1")
    osq.reset_tier()
    assert switch.BEAM_SELECT is True
    monkeypatch.delenv("OSQ_BEAM_SELECT")
    osq.reset_tier()
    assert switch.BEAM_SELECT is False


def test_generate_on_the_cpu_takes_the_torch_lines_and_says_why(switch):
    from test_bart_decode_cpu import batch, tiny_bart, wrapped
    q = wrapped(tiny_bart())
    ids, mask = batch()
    kw = dict(attention_mask=mask, max_length=12, num_beams=3, min_length=5, no_repeat_ngram_size=2)
    with torch.no_grad():
        want = q.generate(ids, beam_select=False, **kw)
        info = q.last_beam_select
        assert (info.selected, info.reason) == (0, "not asked for") and info.eager >= 4
        got = q.generate(ids, beam_select=True, **kw)
        assert torch.equal(got, want)
        info = q.last_beam_select
        assert info.selected == 0 and info.eager >= 4 and "CPU" in info.reason, info
        switch.BEAM_SELECT = True                      # the package switch asks as the argument does
        assert torch.equal(q.generate(ids, **kw), want) and "CPU" in q.last_beam_select.reason
        q.generate(ids, attention_mask=mask, max_length=6, num_beams=1)
        assert q.last_beam_select.selected == 0 and "greedy" in q.last_beam_select.reason

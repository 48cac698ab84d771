"""CPU: several seeded samples per input and the drawn tokens' log-probabilities (include/osq_hip.h, "seeded sampling";
model/sampling.py; sample(num_samples=, return_logprobs=)) where no GPU is involved: the grouped uniforms against the Philox
words, sampling.token_logprob against the float64 restatement of tests/_sample_group.py on the restatement's own cases, the
entry points' listing and binding, and sample() on the tiny BART of test_bart_decode_cpu.
The kernels run on the GPU (tests/test_gpu_sample_group.py, tests/test_gpu_sample_group_model.py)."""
import os
import re

import numpy as np
import pytest
import torch

import _sample_advance as SA
import _sample_group as SG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("group", (1, 2, 3, 8))
def test_grouped_uniforms_are_the_philox_words(group):
    from outlier_suppression_amd.model import sampling
    for seed in (0, 2 ** 64 - 1, 0x123456789abcdef):
        for inputs, cur in ((1, 1), (3, 31), (5, 4095)):
            u = sampling.uniforms(seed, inputs, cur, group)
            assert u.dtype == torch.float32 and u.shape == (inputs * group,)
            words = SG.uniform_words(seed, inputs, cur, group)
            assert (u.double() * 2 ** 24).tolist() == [float(w) for w in words]
            key = (seed & 0xffffffff, seed >> 32)
            b, j = inputs - 1, group - 1
            assert words[b * group + j] == sampling.philox4x32((b, cur, j, 0), key)[0] >> 8
            if group == 1:
                assert torch.equal(u, sampling.uniforms(seed, inputs, cur))
            # a sequence's draw hangs on (seed, b, j, cur) alone: not on the group or the number of inputs
            wider = sampling.uniforms(seed, inputs + 2, cur, group + 3)
            assert all(u[b * group + j] == wider[b * (group + 3) + j] for b in range(inputs) for j in range(group))
    assert len(set(sampling.uniforms(7, 4, 3, 8).tolist())) > 28


@pytest.mark.parametrize("label, x, T, k, p", SG.lp_cases(), ids=[c[0] for c in SG.lp_cases()])
def test_token_logprob_is_the_restatement(label, x, T, k, p):
    from outlier_suppression_amd.model import sampling
    sv = SA.survivors(x, (), T, k, p)
    rows = torch.from_numpy(x)[None, :]
    if sv.tokens.size == 0:
        got = sampling.token_logprob(rows, torch.zeros(1, dtype=torch.long), T, k, p)
        assert got.dtype == torch.float32 and float(got[0]) == float("-inf")
        return
    if "cut" in label:
        assert sv.tokens.size < sv.ranked.size and (np.abs(sv.above - p) >= SA.MARGIN).all()      # weight is removed
    if "ties" in label:
        z = np.sort(x)[::-1]
        assert z[k - 1] == z[k]
    tokens = torch.from_numpy(sv.tokens.astype(np.int64))
    got = sampling.token_logprob(rows.expand(tokens.numel(), -1).contiguous(), tokens, T, k, p)
    assert got.dtype == torch.float32 and got.shape == tokens.shape
    for t, lp in zip(sv.tokens.tolist(), got.tolist()):
        SG.within(lp, SG.logprob64(x, (), T, k, p, t), (label, t))
    total = sum(np.exp(SG.logprob64(x, (), T, k, p, t)[0]) for t in sv.tokens.tolist())
    assert abs(total - 1.0) < 1e-9                         # the restatement is a distribution over the kept survivors
    out = np.setdiff1d(np.arange(x.size), sv.tokens)
    if out.size:                                           # a token that is not kept was drawn with probability 0
        assert float(sampling.token_logprob(rows, torch.tensor([int(out[0])]), T, k, p)[0]) == float("-inf")


def test_entry_points_are_listed_and_bound():
    from outlier_suppression_amd import _hip
    header = open(os.path.join(ROOT, "include", "osq_hip.h")).read()
    above = header[:header.index("#define OSQ_ABI_VERSION")]
    added = re.search(r"Added within 10 \(no existing signature changed\):(.*?)\*/", above, re.S).group(1)
    assert re.search(r"#define OSQ_ABI_VERSION 10\b", header) and _hip.ABI_VERSION == 10
    for name, namesake, count in (("osq_sample_advance_group", "osq_sample_advance", 29),
                                  ("osq_sample_advance_group_at", "osq_sample_advance_at", 32),
                                  ("osq_sample_nucleus_group", "osq_sample_nucleus", 28),
                                  ("osq_sample_nucleus_group_at", "osq_sample_nucleus_at", 31),
                                  ("osq_sample_uniforms_group", "osq_sample_uniforms", 6)):
        assert name in set(re.findall(r"osq_\w+", added)), name
        decl = re.search(r"^int %s\((.*?)\);" % name, header, re.M | re.S)
        assert decl, f"{name} is not declared"
        args = [a.strip() for a in decl.group(1).split(",")]
        assert len(args) == len(_hip.SIGNATURES[name][1]) == count, name
        theirs = _hip.SIGNATURES[namesake][1]
        if name != "osq_sample_uniforms_group":            # the namesake's list, then group, logprobs, logprobs_stride, the stream
            assert args[-4:] == ["int64_t group", "float* logprobs", "int64_t logprobs_stride", "osq_stream stream"], name
            assert _hip.SIGNATURES[name][1] == theirs[:-1] + [_hip._L, _hip._P, _hip._L] + theirs[-1:], name
    assert "seeded sampling" in header and "(b, cur, j, 0)" in header


@pytest.fixture(scope="module")
def tiny():
    from test_bart_decode_cpu import batch, tiny_bart, wrapped
    return wrapped(tiny_bart()), batch()


KW = dict(max_length=12, min_length=12, temperature=1.5, seed=11)


def test_three_samples_are_the_repeated_batch_under_the_grouped_uniforms(tiny, monkeypatch):
    from outlier_suppression_amd.model import sampling
    q, (ids, mask) = tiny
    got = q.sample(ids, attention_mask=mask, num_samples=3, **KW)
    assert got.shape == (9, 12) and got.dtype == torch.long
    assert torch.equal(q.sample(ids, attention_mask=mask, num_samples=3, use_cache=False, **KW), got)
    assert len({tuple(r) for r in got[:3].tolist()}) > 1   # the sequences of an input differ
    # a sequence does not hang on how many are drawn beside it, nor on the batch
    two = q.sample(ids, attention_mask=mask, num_samples=2, **KW)
    assert torch.equal(two.view(3, 2, 12), got.view(3, 3, 12)[:, :2])
    assert torch.equal(q.sample(ids[:1], attention_mask=mask[:1], num_samples=3, **KW), got[:3])
    one = q.sample(ids, attention_mask=mask, **KW)
    assert torch.equal(q.sample(ids, attention_mask=mask, num_samples=1, **KW), one) and torch.equal(got[::3], one)
    host = sampling.uniforms
    monkeypatch.setattr(sampling, "uniforms", lambda seed, bsz, cur, group=1: host(seed, bsz // 3, cur, 3))
    by_hand = q.sample(ids.repeat_interleave(3, 0), attention_mask=mask.repeat_interleave(3, 0), **KW)
    assert torch.equal(by_hand, got)


def test_sharing_on_the_cpu_decodes_expanded_with_a_reason(tiny):
    q, (ids, mask) = tiny
    want = q.sample(ids, attention_mask=mask, num_samples=3, **KW)
    assert q.last_share_cross_kv.reason == "not asked for"
    assert torch.equal(q.sample(ids, attention_mask=mask, num_samples=3, share_cross_kv=True, **KW), want)
    info = q.last_share_cross_kv
    assert (info.shared, info.eager) == (0, 11) and "CPU" in info.reason
    q.sample(ids, attention_mask=mask, num_samples=3, share_cross_kv=True, use_cache=False, **KW)
    assert "use_cache=False" in q.last_share_cross_kv.reason
    q.sample(ids, attention_mask=mask, max_length=3, seed=1, num_samples=65, share_cross_kv=True)
    assert "64" in q.last_share_cross_kv.reason


def _recorded(q, monkeypatch, ids, mask, **kw):
    """sample(return_logprobs=True) with every step's scores and draws recorded where the step itself saw them."""
    from outlier_suppression_amd.model import sampling
    steps = []
    select = sampling.select_torch

    def recording(scores, u, temperature=1.0, top_k=0, top_p=1.0):
        token = select(scores, u, temperature, top_k, top_p)
        steps.append((scores.clone().numpy(), token.clone().numpy()))
        return token
    monkeypatch.setattr(sampling, "select_torch", recording)
    seq, lps = q.sample(ids, attention_mask=mask, return_logprobs=True, **kw)
    monkeypatch.setattr(sampling, "select_torch", select)
    return seq, lps, steps


@pytest.mark.parametrize("top_k, top_p", [(50, 1.0), (0, 1.0), (8, 0.8), (0, 0.9)])
def test_logprobs_are_the_restatement_on_the_scores_the_step_saw(tiny, monkeypatch, top_k, top_p):
    q, (ids, mask) = tiny
    kw = dict(KW, num_samples=3, top_k=top_k, top_p=top_p, no_repeat_ngram_size=2)
    seq, lps, steps = _recorded(q, monkeypatch, ids, mask, **kw)
    assert torch.equal(seq, q.sample(ids, attention_mask=mask, **kw))                   # asking for them changes no token
    assert seq.shape == lps.shape == (9, 12) and lps.dtype == torch.float32 and len(steps) == 11
    assert (seq[:, 11] == 2).all()                         # the tiny model's own forced_eos_token_id fires at the last position
    assert (lps[:, 0] == 0).all() and (lps[:, 1:11] < 0).all() and (lps[:, 11] == 0).all()
    for cur, (scores, token) in enumerate(steps, start=1):
        assert token.tolist() == seq[:, cur].tolist()
        for r in range(9):
            SG.within(float(lps[r, cur]), SG.logprob64(scores[r], (), 1.5, top_k, top_p, token[r]), (cur, r))


def test_logprobs_are_zero_where_nothing_was_drawn(tiny, monkeypatch):
    q, (ids, mask) = tiny
    base = dict(max_length=12, seed=21, temperature=1.5, top_k=20, pad_token_id=1, num_samples=3)
    free = q.sample(ids, attention_mask=mask, eos_token_id=[119], min_length=0, **base)
    eos = next(int(t) for t in free[0, 3:8] if int(t) != 1)                              # a token row 0 draws midway becomes the eos
    seq, lps, steps = _recorded(q, monkeypatch, ids, mask, eos_token_id=[eos], min_length=0, forced_bos_token_id=0, **base)
    assert (lps[:, 0] == 0).all() and (lps[:, 1] == 0).all() and (seq[:, 1] == 0).all()  # the start column, the forced bos
    ended = 0
    for r in range(9):
        hits = [i for i in range(2, seq.shape[1]) if int(seq[r, i]) == eos]
        end = hits[0] if hits else seq.shape[1] - 1
        drawn = min(end, 10)                               # the model's own forced eos fires at position 11
        assert (lps[r, 2:drawn + 1] < 0).all() and (lps[r, drawn + 1:end + 1] == 0).all(), r
        assert (lps[r, end + 1:] == 0).all() and (seq[r, end + 1:] == 1).all(), r
        ended += bool(hits) and end + 1 < seq.shape[1]
        for cur in range(2, drawn + 1):
            scores, token = steps[cur - 1]
            SG.within(float(lps[r, cur]), SG.logprob64(scores[r], (), 1.5, 20, 1.0, token[r]), (cur, r))
    assert ended >= 1
    kw = dict(max_length=6, min_length=0, seed=3, forced_eos_token_id=2, attention_mask=mask, num_samples=2, return_logprobs=True)
    seq, lps = q.sample(ids, **kw)
    assert (seq[:, 5] == 2).all() and (lps[:, 5] == 0).all() and (lps[:, 1:5] < 0).all()
    one, lp_one = q.sample(ids, **dict(kw, num_samples=1))                               # one sample, with its log-probs
    assert torch.equal(one, seq[::2]) and torch.equal(lp_one, lps[::2])


def test_num_return_sequences_still_raises_and_points_to_num_samples(tiny):
    q, (ids, mask) = tiny
    with pytest.raises(ValueError, match="num_samples"):
        q.sample(ids, attention_mask=mask, max_length=5, num_return_sequences=2)
    with pytest.raises(ValueError, match="num_samples"):
        q.sample(ids, attention_mask=mask, max_length=5, num_samples=0)

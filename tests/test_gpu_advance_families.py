"""What greedy_advance, sample_advance and sample_nucleus (ops.py; csrc/advance_step.h holds their common step record and
tails) have in common, as behaviour: where the choice of the token does not differ, every word they write is the same.

A forced step reads no logit and draws nothing, so all forms write the words of tests/_greedy_advance.py's restatement (the
logits hold NaN everywhere); and a draw with one survivor -- top_k = 1, or a nucleus of top_p = 1e-6 -- is the arg-max, so
both sampling kernels write greedy's words whatever the uniform.  The inputs of the second test hold no NaN: greedy ranks it
first and sampling drops it, which is documented and stays.

Shape: bsz 3, vocab 4100 (two chunks, the second of four tokens), max_length 12 (2 where forced_bos and forced_eos fire
together: only there is length 1 also max_length - 1), unfinished (1, 1, 0), pad 1.  next_tokens, the whole of seq, unfinished
and go_on are compared as words, and every output is pre-filled with a sentinel."""
import numpy as np
import pytest
import torch

import _greedy_advance as GA
import _sample_advance as SA
import _sample_nucleus as NU
from test_greedy_advance_cpu import same

pytestmark = pytest.mark.gpu

BSZ, VOCAB, MAX_LENGTH, CHUNK = 3, 4100, 12, 4096
STATE = dict(unfinished=(1, 1, 0), pad=1)
# (label, the draw's arguments): None is greedy
FORMS = [("greedy", None), ("sample_advance, top_k 3", dict(top_k=3)), ("sample_advance, top_k 0, top_p 1", dict(top_k=0, top_p=1.0)),
         ("sample_nucleus, top_p 0.9", dict(top_p=0.9))]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _ids(ids, dev):
    return torch.tensor(list(ids), dtype=torch.int64, device=dev) if len(ids) else None


def _run(case, dev, draw, at=False, u=None):
    """One step of the case through the form ``draw`` names (static, or ``at``: the position from a device word, the settings
    as generate() has them): (next_tokens, seq, unfinished, go_on) as they lie on the device afterwards."""
    from outlier_suppression_amd import ops
    bsz, max_length = case["seq"].shape
    bufs = ops.GreedyBuffers(bsz, max_length, dev) if draw is None else ops.SampleBuffers(bsz, max_length, dev)
    bufs.seq.copy_(torch.from_numpy(case["seq"]))
    bufs.unfinished.copy_(torch.from_numpy(case["unfinished"]))
    bufs.next_tokens.fill_(-7)
    bufs.go_on.fill_(77)
    logits = torch.from_numpy(case["logits"]).to(dev)
    eos = _ids(case["eos"], dev)
    if at:
        position = (torch.full((1,), case["cur"], dtype=torch.int32, device=dev),)
        settings = dict(ngram=case["ngram"], ban_ids=eos, ban_below=case["min_length"], forced_bos=case["forced_bos"],
                        forced_eos=case["forced_eos"], eos_ids=eos, pad=case["pad"])
    else:
        kw = GA.kernel_arguments(case)
        position = (case["cur"],)
        settings = dict(ngram=kw["ngram"], ban_ids=_ids(kw["ban_ids"], dev), forced=kw["forced"], eos_ids=eos, pad=kw["pad"])
    if draw is None:
        call = ops.greedy_advance_at if at else ops.greedy_advance
    else:
        family = "sample_advance" if "top_k" in draw else "sample_nucleus"
        call = getattr(ops, family + ("_at" if at else ""))
        position += (0,)                                                  # the seed
        settings.update(draw, uniforms=None if u is None else torch.from_numpy(np.asarray(u, dtype=np.float32)).to(dev))
    assert call(logits, bufs, *position, **settings) is bufs
    torch.cuda.synchronize()
    return bufs.next_tokens.cpu().numpy(), bufs.seq.cpu().numpy(), bufs.unfinished.cpu().numpy(), int(bufs.go_on)


FORCED = [("forced = 5", False, MAX_LENGTH, 1, dict(forced_bos=5, eos=(9, 4097))),
          ("forced is an eos id", False, MAX_LENGTH, 1, dict(forced_bos=9, eos=(9, 4097))),
          ("forced_bos at length 1", True, MAX_LENGTH, 1, dict(forced_bos=7, forced_eos=9, eos=(9,))),
          ("forced_eos at max_length - 1", True, MAX_LENGTH, MAX_LENGTH - 1, dict(forced_bos=7, forced_eos=9, eos=(9,))),
          ("both fire", True, 2, 1, dict(forced_bos=7, forced_eos=9, eos=(9,)))]


@pytest.mark.parametrize("label, at, max_length, cur, settings", FORCED, ids=[f[0] for f in FORCED])
def test_a_forced_step_writes_the_same_words_in_every_form(dev, label, at, max_length, cur, settings):
    rng = np.random.default_rng(1)
    nan_rows = np.full((BSZ, VOCAB), np.nan, dtype=np.float32)           # a forced step reads none of them
    case = GA.make(rng, BSZ, VOCAB, max_length, cur, logits=nan_rows, ngram=2, min_length=6, **STATE, **settings)
    want = GA.reference_case(case)
    assert GA.kernel_arguments(case)["forced"] is not None and want[0].tolist()[2] == STATE["pad"]
    for form, draw in FORMS:
        same(_run(case, dev, draw, at), want, (label, form))


def _one_survivor_case():
    """Rows whose arg-max is decided by everything at once: the largest value is the eos id 4097, banned below min_length;
    the next is token 0, which the 2-gram rule bans (the history 1, 0, 1 ends with a 1, and a 0 followed the first 1); then
    rows 0 and 2 hold their maximum twice, in the last token of the first chunk and the first of the second, and row 1 holds
    -0.0 at token 7 and +0.0 in the second chunk over negative numbers.  The first of each pair wins."""
    rng = np.random.default_rng(2)
    x = rng.uniform(-4, -1, size=(BSZ, VOCAB)).astype(np.float32)
    x[:, 4097], x[:, 0] = 50.0, 45.0
    x[0, CHUNK - 1] = x[0, CHUNK] = x[2, CHUNK - 1] = x[2, CHUNK] = 40.0
    x[1, 7], x[1, CHUNK] = -0.0, 0.0
    history = np.tile(np.array([1, 0, 1], dtype=np.int64), (BSZ, 1))
    case = GA.make(rng, BSZ, VOCAB, MAX_LENGTH, 3, logits=x, history=history, ngram=2, min_length=6, eos=(4097,), **STATE)
    assert not GA.has_nan(case)
    want = GA.reference_case(case)
    assert want[0].tolist() == [CHUNK - 1, 7, STATE["pad"]] and want[3] == 1
    # on the CPU, before any launch: the restatements of both sampling rules give greedy's token on these very inputs
    for u in (np.float32(0.0), NU.LAST_U):
        draws = np.full(BSZ, u, dtype=np.float32)
        for top_k, top_p in ((1, 1.0), (0, 1e-6)):
            same(SA.reference_case(dict(case, temperature=1.0, top_k=top_k, top_p=top_p), draws), want, ("restated", top_k, u))
        for b, token in enumerate([CHUNK - 1, 7, CHUNK - 1]):
            ban = SA.banned(dict(case, temperature=1.0, top_k=0, top_p=1e-6), b)
            assert ban == {4097, 0}
            assert NU.search(x[b], ban, 1.0, 1e-6, u) == (token, 1), (b, u)
    return case, want


def test_b_a_draw_with_one_survivor_is_the_arg_max(dev):
    case, want = _one_survivor_case()
    greedy = _run(case, dev, None)
    same(greedy, want, "greedy")
    for u in (np.float32(0.0), NU.LAST_U):
        draws = np.full(BSZ, u, dtype=np.float32)
        for form, draw in (("sample_advance, top_k 1", dict(temperature=1.0, top_k=1)),
                           ("sample_nucleus, top_p 1e-6", dict(temperature=1.0, top_p=1e-6))):
            same(_run(case, dev, draw, u=draws), greedy, (form, float(u)))

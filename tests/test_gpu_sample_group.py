"""osq_sample_advance_group(_at) / osq_sample_nucleus_group(_at) / osq_sample_uniforms_group (csrc/sample_advance.hip,
csrc/sample_nucleus.hip) through ops: several sequences per input and the drawn token's log-probability.

A grouped launch must write the words of the existing entry point fed the host's grouped uniforms, in every family (top-k,
the whole vocabulary in token order, the nucleus) and in both forms.  The log-probabilities are checked on constructed rows
with the draw planted at least 1e-3 W inside a survivor's float64 interval (tests/_sample_advance.py), so that the token and
the kept set are the restatement's; the bound is tests/_sample_group.py's, 2e-5 + 2**-21 * (|z_tok - m| + |ln W|).  The
logprobs buffer is sentinel-filled before every launch and only its [r, cur] words may change; every other output word is
that of the call without a buffer.  The largest excursion per family goes to profiles/sample_group_accuracy.txt when
OSQ_SAMPLE_GROUP_ACCURACY_OUT=<path> is set."""
import math
import os

import numpy as np
import pytest
import torch

import _greedy_advance as GA
import _sample_advance as SA
import _sample_group as SG
from test_greedy_advance_cpu import same

pytestmark = pytest.mark.gpu

MAX_LENGTH = 8
CHUNKED = (1, 50, 4096, 4097, 8200)
NUCLEUS = (50, 51, 3200, 3201, 50265)
FAMILIES = [("top-k", v) for v in CHUNKED] + [("full", v) for v in CHUNKED] + [("nucleus", v) for v in NUCLEUS]
SENTINEL = -77.0
_seen = {}             # family -> (the largest |lp - lp64|, its bound, where)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _ids(ids, dev):
    return torch.tensor(list(ids), dtype=torch.int64, device=dev) if len(ids) else None


def _buffers(case, dev, family):
    from outlier_suppression_amd import ops
    bsz, max_length = case["seq"].shape
    bufs = ops.SampleBuffers(bsz, max_length, dev, top_k=case["top_k"], nucleus=family == "nucleus")
    bufs.seq.copy_(torch.from_numpy(case["seq"]))
    bufs.unfinished.copy_(torch.from_numpy(case["unfinished"]))
    bufs.next_tokens.fill_(-7)
    bufs.go_on.fill_(77)
    return bufs


def _step(case, dev, family, at, bufs, logits, seed=0, u=None, cur=None, **grouped):
    """One step of the family in its static or its _at form on ``bufs``; ``grouped``: group= / logprobs=, or nothing -- the
    existing entry point."""
    from outlier_suppression_amd import ops
    cur = case["cur"] if cur is None else cur
    planted = None if u is None else torch.from_numpy(np.asarray(u, dtype=np.float32)).to(dev)
    draw = dict(temperature=case["temperature"], top_p=case["top_p"], uniforms=planted, **grouped)
    if family != "nucleus":
        draw["top_k"] = case["top_k"]
    if at:
        fn = ops.sample_nucleus_at if family == "nucleus" else ops.sample_advance_at
        word = torch.full((1,), cur, dtype=torch.int32, device=dev)
        out = fn(logits, bufs, word, seed, 0, ngram=case["ngram"], ban_ids=_ids(case["eos"], dev), ban_below=case["min_length"],
                 forced_bos=case["forced_bos"], forced_eos=case["forced_eos"], eos_ids=_ids(case["eos"], dev), pad=case["pad"], **draw)
    else:
        fn = ops.sample_nucleus if family == "nucleus" else ops.sample_advance
        kw = GA.kernel_arguments(dict(case, cur=cur))
        out = fn(logits, bufs, cur, seed, ngram=kw["ngram"], ban_ids=_ids(kw["ban_ids"], dev), forced=kw["forced"],
                 eos_ids=_ids(kw["eos_ids"], dev), pad=kw["pad"], **draw)
    assert out is bufs


def _outputs(bufs):
    torch.cuda.synchronize()
    return bufs.next_tokens.cpu().numpy(), bufs.seq.cpu().numpy(), bufs.unfinished.cpu().numpy(), int(bufs.go_on)


def _run(case, dev, family, at, **kw):
    bufs = _buffers(case, dev, family)
    _step(case, dev, family, at, bufs, torch.from_numpy(case["logits"]).to(dev), **kw)
    return _outputs(bufs)


def _draw_of(family):
    return dict(top_k=5, top_p=0.9) if family == "top-k" else dict(top_k=0, top_p=0.9 if family == "nucleus" else 1.0)


@pytest.mark.parametrize("group", (1, 2, 3, 8))
def test_a_grouped_uniforms_are_the_hosts(dev, group):
    from outlier_suppression_amd import _hip, ops
    for seed in (0, 5, 2 ** 64 - 1):
        for inputs, cur in ((1, 1), (3, 7), (3, 4095), (90, 31)):
            got = ops.sample_uniforms(seed, inputs, cur, dev, group).cpu().numpy()
            assert np.array_equal(got.view(np.uint32), SG.uniforms(seed, inputs, cur, group).view(np.uint32)), (seed, inputs, cur)
    out = torch.full((8,), SENTINEL, device=dev)
    for bsz, g in ((6, 0), (6, -1), (6, 4), (0, 1)):                      # refused: nothing launched
        assert _hip.load().osq_sample_uniforms_group(1, bsz, g, 3, out.data_ptr(), _hip.raw_stream(dev)) == -1
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()


@pytest.mark.parametrize("at", (False, True), ids=("static", "at"))
@pytest.mark.parametrize("family, vocab", FAMILIES)
def test_b_a_grouped_launch_writes_the_words_of_the_planted_one(dev, family, vocab, at):
    rng = np.random.default_rng(vocab)
    settings = dict(eos=(min(4, vocab - 1),), pad=min(1, vocab - 1), min_length=5, ngram=2)
    seen = set()
    for inputs in (1, 3):
        for group in (1, 2, 3, 8):
            cur = int(rng.integers(2, MAX_LENGTH - 1))
            bsz = inputs * group
            unfinished = (rng.uniform(size=bsz) < 0.8).astype(np.uint8)
            case = SA.make(rng, bsz, vocab, MAX_LENGTH, cur, 0.8, unfinished=unfinished, **_draw_of(family), **settings)
            seed = int(rng.integers(0, 2 ** 63))
            got = _run(case, dev, family, at, seed=seed, group=group)
            want = _run(case, dev, family, at, seed=seed + 1, u=SG.uniforms(seed, inputs, cur, group))
            same(got, want, (family, vocab, inputs, group))
            same(got, _run(case, dev, family, not at, seed=seed, group=group), "the other form")
            seen |= {int(t) for t in got[0]}
    assert len(seen) > 1 or vocab == 1


def _seams(vocab):
    return [t for t in dict.fromkeys((0, vocab - 1, 49, 50, 3199, 3200, 4095, 4096)) if 0 <= t < vocab]


def _heavy(rng, vocab, first=()):
    """Six distinct tokens (all of a smaller vocabulary): ``first``, then the layouts' seams, then any."""
    want = min(6, vocab)
    picked = list(dict.fromkeys(list(first) + _seams(vocab)))[:want]
    rest = np.setdiff1d(np.arange(vocab), picked)
    return np.array(picked + rng.choice(rest, want - len(picked), replace=False).tolist(), dtype=np.int64)


def _wide(sv):
    """The kept survivors whose interval is wide enough to plant a draw in."""
    lo = np.concatenate(([0.0], sv.C[:-1]))
    return [i for i in range(sv.tokens.size) if sv.C[i] - lo[i] >= 2.2 * SA.MARGIN * sv.W]


def _rows(case, n):
    rep = lambda a: np.repeat(a[:1], n, axis=0)            # noqa: E731
    return dict(case, logits=rep(case["logits"]), seq=rep(case["seq"]), unfinished=rep(case["unfinished"]))


def _cut(case, kept):
    """The case with a top_p that keeps ``kept`` ranks: midway between two thresholds, MARGIN from both."""
    ranked = dict(case, top_k=case["top_k"] or case["logits"].shape[1], top_p=1.0)
    above = SA.row(ranked, 0).above
    assert kept < above.size and above[kept] - above[kept - 1] >= 2 * SA.MARGIN
    return dict(case, top_p=float(above[kept - 1] + above[kept]) / 2)


def _at_midpoints(case):
    """One row per plantable kept survivor of the case's row 0, and the draws at the midpoints."""
    sv = SA.row(case, 0)
    at = _wide(sv)
    assert at, "no survivor to plant a draw in"
    return _rows(case, len(at)), np.array([SA.midpoint(sv, i) for i in at], dtype=np.float32), sv.tokens[at]


def _lp_cases(family, vocab):
    """(label, case, u, what is asserted of the tokens): every kind of row the rule names."""
    rng = np.random.default_rng(1000 + vocab)
    k = 5 if family == "top-k" else 0
    cuts = family != "full"                                               # the token-order family has no top-p
    inf = np.float32(np.inf)
    out = []
    for T in (0.7, 1.5):                                                  # the maximum and every other heavy survivor; a cut
        x = SA.spread_logits(rng, 1, vocab, [_heavy(rng, vocab)])
        case = SA.make(rng, 1, vocab, MAX_LENGTH, 3, T, k, 1.0, logits=x)
        if cuts and vocab >= 6:
            case = _cut(case, 3)
            assert SA.row(case, 0).tokens.size == 3
        many, u, tokens = _at_midpoints(case)
        assert int(np.argmax(x[0])) in tokens.tolist()
        out.append((f"the maximum and its neighbours, T {T}", many, u, tokens))
    if vocab >= 8:
        heavy = _heavy(rng, vocab)
        x = SA.spread_logits(rng, 1, vocab, [heavy], tail=-3.0)
        tied = heavy[:3].tolist()
        x[0, tied] = inf                                                  # a tie group at +inf; the cut keeps two of the three
        case = SA.make(rng, 1, vocab, MAX_LENGTH, 3, 1.5, k, 0.5 if cuts else 1.0, logits=x)
        many, u, tokens = _at_midpoints(case)
        assert tokens.tolist() == sorted(tied)[:2 if cuts else 3]
        out.append(("a tie group at +inf", many, u, tokens))
        heavy = _heavy(rng, vocab, first=(2, 4))                          # bans: min-length takes the eos 4, the 2-gram rule takes 2
        x = SA.spread_logits(rng, 1, vocab, [heavy])
        x[0, [2, 4]] = 3.0                                                # the would-be winners
        case = SA.make(rng, 1, vocab, MAX_LENGTH, 3, 0.7, k, 1.0, logits=x, history=np.array([[1, 2, 1]]), ngram=2, eos=(4,),
                       pad=1, min_length=6)
        assert SA.banned(case, 0) == {2, 4}
        if cuts:
            case = _cut(case, 2)
        many, u, tokens = _at_midpoints(case)
        assert not {2, 4} & set(tokens.tolist())
        out.append(("banned ids and a no-repeat-ngram ban", many, u, tokens))
    forced = SA.make(rng, 3, vocab, MAX_LENGTH, 1, 1.5, k, 0.9 if cuts else 1.0, forced_bos=vocab - 1,
                     logits=np.full((3, vocab), np.nan, dtype=np.float32))
    out.append(("a forced step", forced, np.full(3, 0.5, dtype=np.float32), np.full(3, vocab - 1)))
    eos, pad = ((vocab - 1,), 0) if vocab < 8 else ((5,), 1)
    x = SA.spread_logits(rng, 1, vocab, [_heavy(rng, vocab)]).repeat(4, axis=0)
    x[2:] = -inf                                                          # rows 2 and 3: without a survivor
    case = SA.make(rng, 4, vocab, MAX_LENGTH, 3, 0.7, k, 0.9 if cuts else 1.0, logits=x, unfinished=(1, 0, 1, 0), eos=eos, pad=pad)
    sv = SA.row(case, 0)
    i = _wide(sv)[0]
    out.append(("a finished row, a row without a survivor, and both", case,
                np.array([SA.midpoint(sv, i), 0.5, 0.5, 0.5], dtype=np.float32), np.array([sv.tokens[i], pad, 0, pad])))
    return out


def _expected_lp(case, b, token):
    kw = GA.kernel_arguments(case)
    if (kw["forced"] is not None and kw["forced"] >= 0) or (kw["eos_ids"] and not case["unfinished"][b]):
        return 0.0, 0.0
    return SG.case_logprob64(case, b, token)


@pytest.mark.parametrize("family, vocab", FAMILIES)
def test_c_logprobs_of_constructed_rows(dev, family, vocab):
    cases = _lp_cases(family, vocab)
    assert len(cases) == (6 if vocab >= 8 else 4)
    for n, (label, case, u, tokens) in enumerate(cases):
        bsz = case["logits"].shape[0]
        group = bsz if n % 2 else 1
        want = SA.reference_case(case, u)
        assert want[0].tolist() == [int(t) for t in tokens], label
        words = []
        for at in (False, True):
            plain = _run(case, dev, family, at, u=u)
            same(plain, want, (label, at))
            bufs = _buffers(case, dev, family)
            wide = torch.full((bsz, MAX_LENGTH + 3), SENTINEL, dtype=torch.float32, device=dev)      # a padded row stride
            _step(case, dev, family, at, bufs, torch.from_numpy(case["logits"]).to(dev), u=u, group=group,
                  logprobs=wide[:, :MAX_LENGTH])
            same(_outputs(bufs), plain, (label, at, "with logprobs"))
            lp = wide.cpu().numpy()
            others = np.delete(lp, case["cur"], axis=1)
            assert (others == SENTINEL).all(), (label, at)
            words.append(lp[:, case["cur"]].copy())
            for b in range(bsz):
                expect = _expected_lp(case, b, plain[0][b])
                off = SG.within(lp[b, case["cur"]], expect, (family, vocab, label, at, b))
                if off >= _seen.get(family, (-1.0,))[0]:
                    _seen[family] = (off, expect[1], f"vocab {vocab}, {label}")
        assert np.array_equal(words[0].view(np.uint32), words[1].view(np.uint32)), label
    none = [c for c in cases if "without a survivor" in c[0]][0]
    assert _expected_lp(none[1], 2, 0)[0] == -math.inf and _expected_lp(none[1], 3, 0)[0] == 0.0


def test_d_accuracy_record():
    path = os.environ.get("OSQ_SAMPLE_GROUP_ACCURACY_OUT")
    if path and _seen:
        with open(path, "w") as f:
            f.write("The log-probability of the drawn token (osq_sample_advance_group, osq_sample_nucleus_group) against the float64\n"
                    "restatement of tests/_sample_group.py on the constructed rows of tests/test_gpu_sample_group.py: the largest\n"
                    "|lp - lp64| per family beside its bound there, 2e-5 + 2**-21 * (|z_tok - m| + |ln W|)\n\n")
            for family, (off, tol, where) in _seen.items():
                f.write(f"{family:10s} largest {off:.3e}   bound {tol:.3e}   ({where})\n")


@pytest.mark.parametrize("what", ["group = 0", "group < 0", "bsz % group", "logprobs stride", "valid"])
@pytest.mark.parametrize("family", ("top-k", "nucleus"))
def test_e_refusals_launch_nothing(dev, family, what):
    from outlier_suppression_amd import _hip
    lib = _hip.load()
    bsz, vocab = 6, 50
    group = {"group = 0": 0, "group < 0": -2, "bsz % group": 4}.get(what, 3)
    stride = MAX_LENGTH - 1 if what == "logprobs stride" else MAX_LENGTH
    logits = torch.zeros((bsz, vocab), dtype=torch.float32, device=dev)
    seq = torch.full((bsz, MAX_LENGTH), 85, dtype=torch.int64, device=dev)
    nxt = torch.full((bsz,), 85, dtype=torch.int64, device=dev)
    go_on = torch.full((1,), 85, dtype=torch.int32, device=dev)
    ws = torch.full((4096,), 85, dtype=torch.uint8, device=dev)
    lp = torch.full((bsz, MAX_LENGTH), SENTINEL, dtype=torch.float32, device=dev)
    head = (logits.data_ptr(), vocab, seq.data_ptr(), MAX_LENGTH, 3, 0, None, 0, -1, None, 0, 0, None, bsz, vocab, MAX_LENGTH,
            nxt.data_ptr(), go_on.data_ptr(), ws.data_ptr(), ws.numel(), 12345, 0.8)
    tail = (0.9, None, group, lp.data_ptr(), stride, _hip.raw_stream(dev))
    rc = lib.osq_sample_advance_group(*head, 4, *tail) if family == "top-k" else lib.osq_sample_nucleus_group(*head, *tail)
    torch.cuda.synchronize()
    if what == "valid":
        assert rc == 0 and (lp[:, 3] != SENTINEL).all() and (nxt != 85).all() and int(go_on) == 1
        return
    assert rc == -1 and lib.osq_last_error()
    assert (seq == 85).all() and (nxt == 85).all() and int(go_on) == 85 and (ws == 85).all() and (lp == SENTINEL).all()


def test_f_ops_wrapper_checks(dev):
    from outlier_suppression_amd import ops
    bufs = ops.SampleBuffers(6, MAX_LENGTH, dev, logprobs=True)
    assert bufs.logprobs.shape == (6, MAX_LENGTH) and bufs.logprobs.dtype == torch.float32 and not bufs.logprobs.any()
    assert ops.SampleBuffers(6, MAX_LENGTH, dev).logprobs is None
    logits = torch.randn(6, 50, device=dev)
    assert ops.sample_advance(logits, bufs, 1, 7, top_k=3, group=3, logprobs=bufs.logprobs) is bufs
    torch.cuda.synchronize()
    assert (bufs.logprobs[:, 1] < 0).all() and not bufs.logprobs[:, 2:].any() and not bufs.logprobs[:, 0].any()
    with pytest.raises(ValueError, match="group"):
        ops.sample_advance(logits, bufs, 1, 7, group=4)
    with pytest.raises(ValueError, match="group"):
        ops.sample_nucleus(logits, bufs, 1, 7, group=0)
    with pytest.raises(ValueError, match="logprobs"):
        ops.sample_advance(logits, bufs, 1, 7, logprobs=torch.zeros(6, MAX_LENGTH - 1, device=dev))
    with pytest.raises(ValueError, match="logprobs"):
        ops.sample_nucleus(logits, bufs, 1, 7, logprobs=torch.zeros(6, MAX_LENGTH, dtype=torch.float64, device=dev))
    with pytest.raises(TypeError):
        ops.sample_advance(logits, bufs, 1, 7, 1.0, 0, 1.0, 0, None, None, None, 0, None, 3)      # keyword-only


@pytest.mark.parametrize("family", ("top-k", "full", "nucleus"))
def test_g_captured_with_logprobs_and_replayed_over_the_positions(dev, family):
    """The _at form with group and logprobs captured into a graph on a side stream (after one issued warm-up there) and
    replayed in place at the positions 1 .. 7, the search's state carried from one to the next: the words of the static
    calls, the log-probabilities included."""
    rng = np.random.default_rng(23)
    inputs, group, vocab, seed = 2, 3, 4100, 2 ** 63 + 29
    bsz = inputs * group
    settings = dict(eos=(4097, 9), pad=1, min_length=4, ngram=2, forced_bos=7, forced_eos=9)
    case = SA.make(rng, bsz, vocab, MAX_LENGTH, 1, 1.2, history=np.full((bsz, 1), 2), **_draw_of(family), **settings)
    logits = torch.zeros((bsz, vocab), dtype=torch.float32, device=dev)
    bufs, static = _buffers(case, dev, family), _buffers(case, dev, family)
    lp = torch.full((bsz, MAX_LENGTH), SENTINEL, dtype=torch.float32, device=dev)
    lp_static = lp.clone()
    word = torch.full((1,), 1, dtype=torch.int32, device=dev)
    eos = _ids(settings["eos"], dev)
    from outlier_suppression_amd import ops
    fn = ops.sample_nucleus_at if family == "nucleus" else ops.sample_advance_at
    draw = dict(temperature=1.2, top_p=case["top_p"], **({} if family == "nucleus" else {"top_k": case["top_k"]}))
    call = lambda: fn(logits, bufs, word, seed, 0, ngram=2, ban_ids=eos, ban_below=4, forced_bos=7, forced_eos=9,  # noqa: E731
                      eos_ids=eos, pad=1, group=group, logprobs=lp, **draw)
    keep = (bufs.seq.clone(), bufs.unfinished.clone())
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        call()
    bufs.seq.copy_(keep[0]), bufs.unfinished.copy_(keep[1]), lp.fill_(SENTINEL)
    for cur in range(1, MAX_LENGTH):
        x = rng.standard_normal((bsz, vocab)).astype(np.float32)
        x[:, 4097] += 10.5                                                # an eos that some row draws once min-length lets it
        logits.copy_(torch.from_numpy(x).to(dev))
        word.fill_(cur)
        bufs.next_tokens.fill_(-7), bufs.go_on.fill_(77)
        graph.replay()
        got = _outputs(bufs)
        static.next_tokens.fill_(-7), static.go_on.fill_(77)
        _step(case, dev, family, False, static, logits, seed=seed, cur=cur, group=group, logprobs=lp_static)
        same(got, _outputs(static), (family, "replay / static", cur))
        assert torch.equal(lp.view(torch.int32), lp_static.view(torch.int32)), cur
    lp = lp.cpu().numpy()
    seq = got[1]
    assert (lp[:, 0] == SENTINEL).all() and (lp[:, 1] == 0).all() and (lp[:, MAX_LENGTH - 1] == 0).all()      # both forced
    assert (seq[:, 1] == 7).all() and (lp[:, 2:4] < 0).all()
    finished = [(r, c) for r in range(bsz) for c in range(3, MAX_LENGTH - 1) if seq[r, c] == 1 and seq[r, c - 1] in (1, 4097, 9)]
    assert finished and all(lp[r, c] == 0 for r, c in finished)
    assert len({tuple(r) for r in seq[:group].tolist()}) > 1              # the sequences of an input differ

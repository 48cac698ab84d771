"""osq_beam_select (csrc/beam_select.hip) through the C ABI and ops.beam_select: the continuations of one beam-search step
against the float64 restatement of tests/_beam_select.py (pinned to torch's and transformers' own pipeline by
tests/test_beam_select_cpu.py).

On every case the indices equal the restatement's exactly and the values agree within 2e-5 absolute: about four fp32
roundings at magnitude <= 64 (ulp 7.6e-6) plus a relative 1e-6 on the row sum.  What entitles a test to exact indices is
asserted first, per case: the smallest distance between two distinct neighbours among ranks 1 .. keep + 1 is at least 1e-4,
five times the value bound.  Exact ties (duplicated logits, identical beams, -inf) are ordered by the contract's index rule,
which the restatement states as well.

Shapes: vocab one element either side of a float4, a wavefront's trip (64), a workgroup's trip (256), a chunk (4096) and two
chunks plus one; vocab == keep; the odd BART vocabulary 50265; a row stride above vocab.
Measured on MI355X: profiles/beam_select_accuracy.txt (written when OSQ_BEAM_SELECT_ACCURACY_OUT=<path> is set)."""
import os

import numpy as np
import pytest
import torch

import _beam_select as BS

pytestmark = pytest.mark.gpu

VALUE_BOUND = 2e-5
MIN_GAP = 1e-4
CHUNK = 4096
WORST = {}          # case id -> largest |value - float64| seen


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _strided(t, stride, dev):
    """``t`` [rows, n] on the device with rows ``stride`` elements apart (NaN between them: nothing may read there)."""
    if stride is None:
        return t.to(dev)
    buf = torch.full((t.shape[0], stride), float("nan") if t.is_floating_point() else -7, dtype=t.dtype, device=dev)
    buf[:, :t.shape[1]] = t.to(dev)
    return buf[:, :t.shape[1]]


def _abi(dev, logits, running, keep, seq=None, cur=0, ngram=0, ban_ids=(), stride=None, seq_stride=None, n_ban=None,
         ws_bytes=None, fill=None):
    """One call through the C ABI.  Returns (rc, top_value, top_index) with the outputs on the CPU."""
    from outlier_suppression_amd import _hip
    lib = _hip.load()
    bsz, nb = running.shape
    vocab = logits.shape[1]
    x = _strided(logits, stride, dev)
    run = running.to(dev).contiguous()
    s = None if seq is None else _strided(seq, seq_stride, dev)
    ban = torch.tensor(list(ban_ids) if len(ban_ids) else [0], dtype=torch.int64, device=dev)
    top_v = torch.full((bsz, keep), -123.0 if fill is None else fill, dtype=torch.float32, device=dev)
    top_i = torch.full((bsz, keep), -123, dtype=torch.int64, device=dev)
    need = int(lib.osq_beam_select_workspace_bytes(bsz, nb, vocab, min(keep, 64)))
    ws = torch.empty(max(need, 8), dtype=torch.uint8, device=dev)
    rc = lib.osq_beam_select(x.data_ptr(), x.stride(0), run.data_ptr(), _hip.ptr(s), 0 if s is None else s.stride(0), cur, ngram,
                             ban.data_ptr(), len(ban_ids) if n_ban is None else n_ban, bsz, nb, vocab, keep,
                             top_v.data_ptr(), top_i.data_ptr(), ws.data_ptr(), need if ws_bytes is None else ws_bytes(need),
                             _hip.raw_stream(dev))
    torch.cuda.synchronize()
    return rc, top_v.cpu(), top_i.cpu()


def _words(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _check(name, got_v, got_i, logits, running, keep, seq=None, cur=0, ngram=0, ban_ids=(), min_gap=MIN_GAP):
    args = (logits.numpy(), running.numpy(), keep, None if seq is None else seq.numpy(), cur, ngram, ban_ids)
    gap = BS.gap(*args)
    assert gap >= min_gap, f"{name}: gap {gap:.3g}: the case does not separate its candidates"
    want_v, want_i = BS.reference(*args)
    got_v = got_v.numpy().astype(np.float64)
    assert np.array_equal(got_i.numpy(), want_i), (name, got_i.numpy(), want_i)
    finite = np.isfinite(want_v)
    assert np.array_equal(got_v[~finite], want_v[~finite], equal_nan=True), (name, got_v, want_v)
    err = float(np.abs(got_v[finite] - want_v[finite]).max()) if finite.any() else 0.0
    WORST[name] = max(WORST.get(name, 0.0), err)
    print(f"{name}: max |value - float64| {err:.3g}, gap {gap:.3g}")
    assert err <= VALUE_BOUND, (name, err)
    return want_v, want_i


# (vocab, bsz, nb, keep, seed, logits row stride or None)
SHAPES = [
    (3, 1, 1, 2, 0, None), (4, 3, 2, 2, 0, None), (5, 1, 6, 2, 0, None),                      # a float4
    (63, 3, 1, 12, 0, None), (64, 1, 2, 64, 0, None), (65, 3, 6, 12, 0, None),                 # a wavefront's trip
    (255, 1, 6, 64, 0, None), (256, 3, 1, 12, 0, None), (257, 3, 2, 2, 0, 300),               # a workgroup's trip
    (4095, 3, 2, 12, 0, None), (4096, 1, 6, 64, 0, None), (4097, 1, 2, 12, 0, 4100), (4097, 3, 1, 2, 1, None),   # a chunk
    (8193, 3, 6, 12, 0, None),                                                                # two chunks plus one
    (2, 3, 1, 2, 0, None), (12, 3, 2, 12, 0, None), (64, 1, 1, 64, 0, None),                   # vocab == keep
    (50265, 2, 6, 12, 0, None),                                                               # the odd BART vocabulary
]


@pytest.mark.parametrize("vocab, bsz, nb, keep, seed, stride", SHAPES)
def test_a_shapes(dev, vocab, bsz, nb, keep, seed, stride):
    logits, running, _ = BS.case(seed, bsz, nb, vocab)
    rc, got_v, got_i = _abi(dev, logits, running, keep, stride=stride)
    assert rc == 0
    _check(f"shape v{vocab} b{bsz} n{nb} k{keep}", got_v, got_i, logits, running, keep)


BAN_VOCAB = 4099
BAN_ALPHABET = (0, CHUNK - 1, CHUNK, BAN_VOCAB - 1, 9)      # element 0, vocab - 1, both sides of the chunk boundary


@pytest.mark.parametrize("ngram", [1, 2, 3])
@pytest.mark.parametrize("cur_of", ["n-1", "n", "7", "64"])
def test_b_ngram_bans(dev, ngram, cur_of):
    cur = {"n-1": ngram - 1, "n": ngram, "7": 7, "64": 64}[cur_of]
    logits, running, seq = BS.case(3, 3, 2, BAN_VOCAB, max(cur, 1), BAN_ALPHABET)
    logits[:, list(BAN_ALPHABET)] += 12.0                     # the history's tokens would rank first
    rc, got_v, got_i = _abi(dev, logits, running, 4, seq, cur, ngram, seq_stride=70)
    assert rc == 0
    _, want_i = _check(f"ngram {ngram} cur {cur}", got_v, got_i, logits, running, 4, seq, cur, ngram)
    n_banned = int(BS.banned(seq.numpy(), cur, ngram, (), 6, BAN_VOCAB).sum())
    assert n_banned == 0 if cur < ngram else n_banned >= (6 if cur == 64 else ngram == 1)


def test_b_banned_token_that_would_have_ranked_first(dev):
    logits, running, _ = BS.case(4, 3, 2, 257)
    _, free_i = BS.reference(logits.numpy(), running.numpy(), 4)
    seq = torch.zeros((6, 1), dtype=torch.int64)
    for b in range(3):
        seq[b * 2 + free_i[b, 0] // 257, 0] = free_i[b, 0] % 257        # the winner's beam has seen the winner's token
    rc, got_v, got_i = _abi(dev, logits, running, 4, seq, 1, 1)
    assert rc == 0
    _check("banned winner", got_v, got_i, logits, running, 4, seq, 1, 1)
    assert not (got_i.numpy() == free_i[:, :1]).any()


def test_b_ids_outside_the_vocabulary_ban_nothing(dev):
    logits, running, seq = BS.case(5, 3, 2, 257, 9, (-1, 257, 3, 4, 5))
    assert (seq == -1).any() and (seq == 257).any()
    for ngram in (1, 2):
        rc, got_v, got_i = _abi(dev, logits, running, 4, seq, 9, ngram)
        assert rc == 0
        _check(f"outside ids ngram {ngram}", got_v, got_i, logits, running, 4, seq, 9, ngram)


@pytest.mark.parametrize("ban_ids", [(2,), (2, BAN_VOCAB - 1)], ids=["one", "two"])
def test_b_ban_ids(dev, ban_ids):
    logits, running, seq = BS.case(6, 3, 2, BAN_VOCAB, 7, BAN_ALPHABET)
    logits[:, list(ban_ids)] += 12.0
    rc, got_v, got_i = _abi(dev, logits, running, 4, seq, 7, 3, ban_ids)
    assert rc == 0
    _check(f"ban_ids {ban_ids}", got_v, got_i, logits, running, 4, seq, 7, 3, ban_ids)
    assert not np.isin(got_i.numpy() % BAN_VOCAB, ban_ids).any()


def test_b_fewer_finite_candidates_than_keep(dev):
    logits, running, seq = BS.case(7, 3, 1, 8, 64)              # the history holds ids 0..4; 5 and 6 are banned as well
    rc, got_v, got_i = _abi(dev, logits, running, 4, seq, 64, 1, (5, 6))
    assert rc == 0
    _check("seven of eight banned", got_v, got_i, logits, running, 4, seq, 64, 1, (5, 6), min_gap=0.0)
    assert got_i.tolist() == [[7, 0, 1, 2]] * 3                 # the one finite value, then -inf in index order
    assert torch.isinf(got_v[:, 1:]).all() and torch.isfinite(got_v[:, 0]).all()


def test_c_exact_ties(dev):
    # duplicated logits in a row: equal values, the smaller index first
    logits, running, _ = BS.case(8, 3, 2, 257)
    logits[:, 200] = 30.0
    logits[:, 17] = 30.0
    rc, got_v, got_i = _abi(dev, logits, running, 4)
    assert rc == 0
    _check("duplicated logits", got_v, got_i, logits, running, 4)
    first = got_i.numpy()[:, :2]
    assert (first[:, 0] % 257 == 17).all() and (first[:, 1] == first[:, 0] + 183).all()
    assert torch.equal(_words(got_v[:, 0]), _words(got_v[:, 1]))
    # two identical beams with equal running scores: every value twice, beam 0 first
    logits, running, _ = BS.case(9, 3, 2, 257)
    logits[1::2] = logits[0::2]
    running[:, 1] = running[:, 0]
    rc, got_v, got_i = _abi(dev, logits, running, 4)
    assert rc == 0
    _check("identical beams", got_v, got_i, logits, running, 4)
    i = got_i.numpy()
    assert (i[:, 1] == i[:, 0] + 257).all() and (i[:, 3] == i[:, 2] + 257).all() and (i[:, 0] < 257).all()
    # the first step: -1e9 on every beam but the first, whose candidates are the only ones in reach
    logits, running, _ = BS.case(10, 3, 6, 257)
    running[:, 0] = 0.0
    running[:, 1:] = -1e9
    rc, got_v, got_i = _abi(dev, logits, running, 12)
    assert rc == 0
    _check("first step", got_v, got_i, logits, running, 12)
    assert (got_i < 257).all()


def test_d_same_words_at_every_batch_size_and_on_every_run(dev):
    logits, running, seq = BS.case(16, 3, 2, 8193, 7)
    full = _abi(dev, logits, running, 12, seq, 7, 2)
    again = _abi(dev, logits, running, 12, seq, 7, 2)
    assert full[0] == 0 and again[0] == 0
    assert torch.equal(_words(full[1]), _words(again[1])) and torch.equal(full[2], again[2])
    _check("determinism", full[1], full[2], logits, running, 12, seq, 7, 2)
    for b in range(3):      # the batch row alone: other addresses and alignments (the odd row length), the same words
        one = _abi(dev, logits[2 * b:2 * b + 2].clone(), running[b:b + 1], 12, seq[2 * b:2 * b + 2].clone(), 7, 2)
        assert one[0] == 0
        assert torch.equal(_words(one[1]), _words(full[1][b:b + 1])) and torch.equal(one[2], full[2][b:b + 1])


def test_d_one_nan_logit(dev):
    logits, running, _ = BS.case(12, 3, 2, 4099)
    clean = _abi(dev, logits, running, 4)
    bad = logits.clone()
    bad[2, 4097] = float("nan")                                   # batch row 1, beam 0, second chunk
    rc, got_v, got_i = _abi(dev, bad, running, 4)
    assert rc == 0 and clean[0] == 0
    assert torch.isnan(got_v[1]).all() and got_i[1].tolist() == [0, 1, 2, 3]      # NaN first, by index
    want_v, want_i = BS.reference(bad.numpy(), running.numpy(), 4)
    assert np.array_equal(got_i.numpy(), want_i) and np.isnan(want_v[1]).all()
    for b in (0, 2):
        assert torch.equal(_words(got_v[b]), _words(clean[1][b])) and torch.equal(got_i[b], clean[2][b])


@pytest.mark.parametrize("what", ["keep > 64", "nb > 64", "keep > vocab", "cur > 4096", "n_ban > 16", "workspace too small"])
def test_e_invalid_arguments_launch_nothing(dev, what):
    from outlier_suppression_amd import _hip
    bsz, nb, vocab, keep, kw = 2, 2, 257, 4, {}
    if what == "keep > 64":
        keep = 65
    elif what == "nb > 64":
        bsz, nb = 1, 65
    elif what == "keep > vocab":
        vocab, keep = 3, 4
    elif what == "n_ban > 16":
        kw = dict(ban_ids=tuple(range(17)))
    elif what == "workspace too small":
        kw = dict(ws_bytes=lambda need: need - 1)
    logits, running, _ = BS.case(0, bsz, nb, vocab)
    if what == "cur > 4096":
        kw = dict(seq=torch.zeros((bsz * nb, 4097), dtype=torch.int64), cur=4097, ngram=2)
    rc, got_v, got_i = _abi(dev, logits, running, keep, **kw)
    assert rc == -1 and _hip.load().osq_last_error()
    assert (got_v == -123.0).all() and (got_i == -123).all()
    if what == "cur > 4096":        # the limit itself is taken
        kw = dict(seq=torch.zeros((bsz * nb, 4096), dtype=torch.int64), cur=4096, ngram=2)
        assert _abi(dev, logits, running, keep, **kw)[0] == 0


def test_f_ops_wrapper_and_capture(dev):
    """ops.beam_select on views as generate() hands them, then captured on a side stream after one issued warm-up there and
    replayed once over new inputs: the words of the issued call."""
    from outlier_suppression_amd import ops
    vocab, bsz, nb, keep, cur = 4099, 3, 2, 4, 7
    logits, running, seq = BS.case(13, bsz, nb, vocab, cur, BAN_ALPHABET)
    other, other_running, _ = BS.case(14, bsz, nb, vocab)
    ban = torch.tensor([2], dtype=torch.int64, device=dev)
    wide = torch.zeros((bsz * nb, 3, vocab), device=dev)           # the use_cache=False path: a [:, -1, :] view
    wide[:, -1, :] = logits.to(dev)
    history = torch.full((bsz * nb, 20), 1, dtype=torch.int64, device=dev)
    history[:, :cur] = seq.to(dev)
    run = running.to(dev)
    got_v, got_i = ops.beam_select(wide[:, -1, :], run, keep, history[:, :cur], cur, 3, ban)
    assert got_v.shape == (bsz, keep) and got_v.dtype == torch.float32 and got_i.dtype == torch.int64
    _check("ops", got_v.cpu(), got_i.cpu(), logits, running, keep, seq, cur, 3, (2,))
    with pytest.raises(RuntimeError, match="status -1"):
        ops.beam_select(wide[:, -1, :], run, 65, history[:, :cur], cur, 3, ban)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.beam_select(logits, running, keep)
    with pytest.raises(TypeError):
        ops.beam_select(wide[:, -1, :].double(), run, keep)

    x = wide[:, -1, :]
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        ops.beam_select(x, run, keep, history[:, :cur], cur, 3, ban)          # issued: nothing is allocated first in the capture
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        cap_v, cap_i = ops.beam_select(x, run, keep, history[:, :cur], cur, 3, ban)
    x.copy_(other.to(dev))
    run.copy_(other_running.to(dev))
    graph.replay()
    torch.cuda.synchronize()
    want_v, want_i = ops.beam_select(x, run, keep, history[:, :cur], cur, 3, ban)
    assert torch.equal(_words(cap_v), _words(want_v)) and torch.equal(cap_i, want_i)
    _check("captured", cap_v.cpu(), cap_i.cpu(), other, other_running, keep, seq, cur, 3, (2,))


AT = dict(bsz=2, nb=2, vocab=70, keep=4, ngram=2, cur_max=9)


def _at_case(dev):
    logits, running, seq = BS.case(24, AT["bsz"], AT["nb"], AT["vocab"], AT["cur_max"])
    ban = torch.tensor([35], dtype=torch.int64, device=dev)         # this seed's best token; a 2-gram bans another winner
    return logits.to(dev), running.to(dev), seq.to(dev), ban


@pytest.mark.parametrize("own", [True, False], ids=["caller-owned", "new"])
def test_g_select_at_gives_the_words_of_select(dev, own):
    """ops.beam_select_at and ops.beam_select share one Python body: at the positions 0 and cur_max the words of
    ops.beam_select at that position, one past cur_max NaN in every top_lp and 0 in every top_idx -- into the caller's
    top_lp / top_idx / workspace, and with None for new ones."""
    from outlier_suppression_amd import ops
    bsz, nb, vocab, keep, ngram, cur_max = (AT[k] for k in ("bsz", "nb", "vocab", "keep", "ngram", "cur_max"))
    logits, running, seq, ban = _at_case(dev)
    word = torch.zeros(1, dtype=torch.int32, device=dev)
    outs = {}
    if own:
        outs = dict(top_lp=torch.empty((bsz, keep), device=dev), top_idx=torch.empty((bsz, keep), dtype=torch.int64, device=dev),
                    workspace=torch.empty(ops.beam_select_workspace_bytes(bsz, nb, vocab, keep), dtype=torch.uint8, device=dev))
    for cur in (0, cur_max, cur_max + 1):
        word.fill_(cur)
        if own:
            outs["top_lp"].fill_(5.0)
            outs["top_idx"].fill_(-9)
        got_v, got_i = ops.beam_select_at(logits, running, keep, word, 0, cur_max, seq=seq, ngram=ngram, ban_ids=ban,
                                          ban_below=cur_max + 1, **outs)
        assert (got_v is outs["top_lp"] and got_i is outs["top_idx"]) if own else got_v.shape == got_i.shape == (bsz, keep)
        if cur > cur_max:
            assert bool(torch.isnan(got_v).all()) and bool((got_i == 0).all()), (cur, got_v, got_i)
            continue
        want_v, want_i = ops.beam_select(logits, running, keep, seq, cur, ngram, ban)
        assert torch.equal(_words(got_v), _words(want_v)) and torch.equal(got_i, want_i), (cur, got_v, want_v, got_i, want_i)
        assert bool(torch.isfinite(got_v).all())
    free = ops.beam_select(logits, running, keep, seq, cur_max, 0, None)
    assert not torch.equal(free[1], want_i)                       # at cur_max the windows and the banned id did remove a winner


def test_g_running_scores_with_a_stride(dev):
    """A non-contiguous running_scores: ops.beam_select copies it and gives the words of the contiguous call;
    ops.beam_select_at, which a captured step calls on static buffers, copies nothing and refuses."""
    from outlier_suppression_amd import ops
    bsz, nb, keep, ngram, cur_max = (AT[k] for k in ("bsz", "nb", "keep", "ngram", "cur_max"))
    logits, running, seq, ban = _at_case(dev)
    wide = torch.full((bsz, 2 * nb), float("nan"), device=dev)
    wide[:, ::2] = running
    strided = wide[:, ::2]
    assert not strided.is_contiguous() and torch.equal(strided, running)
    want_v, want_i = ops.beam_select(logits, running, keep, seq, cur_max, ngram, ban)
    got_v, got_i = ops.beam_select(logits, strided, keep, seq, cur_max, ngram, ban)
    assert torch.equal(_words(got_v), _words(want_v)) and torch.equal(got_i, want_i)
    word = torch.full((1,), cur_max, dtype=torch.int32, device=dev)
    with pytest.raises(ValueError, match=r"beam_select_at: logits must be \[bsz \* nb, vocab\] and running_scores a contiguous \[bsz, nb\]"):
        ops.beam_select_at(logits, strided, keep, word, 0, cur_max, seq=seq, ngram=ngram, ban_ids=ban, ban_below=cur_max + 1)


def test_z_report():
    """The largest error of this run, per group and overall (the bound is 2e-5)."""
    if not WORST:           # run on its own: nothing to report
        return
    lines = ["osq_beam_select against the float64 restatement (tests/_beam_select.py): max |value - float64| per case;",
             f"bound {VALUE_BOUND:g}, every case's gap between distinct neighbours among ranks 1 .. keep + 1 >= {MIN_GAP:g}", ""]
    lines += [f"{name:<40s} {err:.3e}" for name, err in WORST.items()]
    lines += ["", f"largest: {max(WORST.values()):.3e}"]
    print("\n".join(lines))
    out = os.environ.get("OSQ_BEAM_SELECT_ACCURACY_OUT")
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")

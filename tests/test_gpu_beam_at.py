"""The position-from-device forms of a beam step, through ``ops``: ops.beam_select_at (osq_beam_select_at) and
ops.beam_advance_at (osq_beam_advance_at).

The contract is one sentence each: for any position, an _at launch produces the words of the static entry point called with
that position (and, for the selection, with ban_ids present while the position is below ban_below).  So every case captures
ONE hipGraph of the _at call and replays it once per position; between two replays the test rewrites the device word (and
the inputs held in static buffers); each replay is compared with the static call at that position word for word -- no
tolerance, no oracle: the static calls have their own tests (test_gpu_beam_select.py, test_gpu_beam_advance.py).

Selection: a vocabulary below, just below and just above one 4096-token chunk; positions either side of the n-gram size and
of one trip of the 256-thread window loop, up to cur_max; a history over five ids, so that windows ban tokens, poisoned
beyond the position; duplicated logits, identical beams and a NaN row; ban_below at 0, inside the range (both sides of it
are positions) and above it; the positions -1 and cur_max + 1 give NaN / 0.
Bookkeeping: every position of a short search and the positions either side of the 64 lanes the row copy strides; every
early_stopping, three length penalties, both forms of the division; eos hits, ties among the -1e9 sentinels, -inf; outputs
pre-filled with a sentinel pattern; the positions 0 and max_length leave them untouched and give go_on == -1."""
import numpy as np
import pytest
import torch

import _beam_advance as BA
from conftest import same_f32

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from outlier_suppression_amd import _hip
    _hip.load()
    return torch.device("cuda:0")


def captured(dev, launch):
    """``launch`` issued once on a side stream, then captured there: the graph."""
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        launch()
    torch.cuda.current_stream(dev).wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        launch()
    return graph


# ------------------------------------------------------------------------------------------------ selection

BSZ, NB, KEEP, CUR_MAX = 2, 3, 6, 300
CANONICAL_NAN = 0x7FC00000


def select_positions(ngram):
    return sorted({p for p in (0, 1, ngram - 1, ngram, ngram + 1, 255, 256, 257, CUR_MAX) if 0 <= p <= CUR_MAX})


@pytest.mark.parametrize("ban_below", [0, 256, CUR_MAX + 700], ids=lambda b: f"below{b}")
@pytest.mark.parametrize("ngram", [0, 2, 3])
@pytest.mark.parametrize("vocab", [50, 4095, 4097])
def test_select_at_equals_static_at_every_position(dev, vocab, ngram, ban_below):
    from outlier_suppression_amd import ops
    g = torch.Generator().manual_seed(vocab * 10 + ngram)
    rows = BSZ * NB
    logits = torch.randn(rows, vocab, generator=g) * 4
    logits[:, 7] = logits[:, 3] = logits.max(dim=1).values + 1.0       # duplicated logits at the top of every row
    logits[1] = logits[0]                                              # two identical beams (their running scores too)
    logits[5, vocab - 2] = float("nan")                                # batch row 1: a NaN row
    running = torch.randn(BSZ, NB, generator=g)
    running[0, 1] = running[0, 0]
    seq0 = torch.randint(0, 5, (rows, CUR_MAX), generator=g)           # five ids: windows repeat, and they ban
    seq0[2, 10:14] = seq0[2, 250:254]                                  # a planted repeat across the 256-window boundary
    logits, running, seq0 = logits.to(dev), running.to(dev), seq0.to(dev)
    ban_ids = torch.tensor([3, vocab - 1], dtype=torch.int64, device=dev)
    seq = seq0.clone()
    word = torch.zeros(1, dtype=torch.int32, device=dev)
    top_lp = torch.empty(BSZ, KEEP, device=dev)
    top_idx = torch.empty(BSZ, KEEP, dtype=torch.int64, device=dev)
    workspace = torch.empty(ops.beam_select_workspace_bytes(BSZ, NB, vocab, KEEP), dtype=torch.uint8, device=dev)

    def launch():
        got = ops.beam_select_at(logits, running, KEEP, word, 1, CUR_MAX, seq=seq, ngram=ngram, ban_ids=ban_ids,
                                 ban_below=ban_below, top_lp=top_lp, top_idx=top_idx, workspace=workspace)
        assert got[0] is top_lp and got[1] is top_idx

    graph = captured(dev, launch)
    seen_banned, seen_free = False, False
    for cur in reversed(select_positions(ngram)):                      # longest first: the poisoned tail only grows
        word.fill_(cur - 1)                                            # the launch adds 1
        seq[:, cur:] = 2                                               # an id of the alphabet: read, it would ban
        top_lp.fill_(5.0)
        top_idx.fill_(-9)
        graph.replay()
        banned = cur < ban_below
        want_lp, want_idx = ops.beam_select(logits, running, KEEP, seq0, cur, ngram, ban_ids if banned else None)
        assert same_f32(top_lp.cpu().numpy(), want_lp.cpu().numpy()), (cur, top_lp, want_lp)
        assert torch.equal(top_idx, want_idx), (cur, top_idx, want_idx)
        assert bool(torch.isnan(top_lp[1]).all()) and not bool(torch.isnan(top_lp[0]).any())
        seen_banned, seen_free = seen_banned or banned, seen_free or not banned
    assert seen_free == (ban_below <= CUR_MAX) and seen_banned == (ban_below > 0)
    if ngram:                                                          # the windows did ban something the n-gram-free call keeps
        free = ops.beam_select(logits, running, KEEP, seq0, CUR_MAX, 0, None)
        with_windows = ops.beam_select(logits, running, KEEP, seq0, CUR_MAX, ngram, None)
        assert not torch.equal(free[1], with_windows[1])
    for bad in (-1, CUR_MAX + 1):
        word.fill_(bad - 1)
        top_lp.fill_(5.0)
        top_idx.fill_(-9)
        graph.replay()
        assert bool((top_lp.cpu().view(torch.int32) == CANONICAL_NAN).all()), (bad, top_lp)
        assert bool((top_idx == 0).all()), (bad, top_idx)


def test_select_at_checks_its_arguments(dev):
    from outlier_suppression_amd import ops
    logits = torch.randn(BSZ * NB, 50, device=dev)
    running = torch.zeros(BSZ, NB, device=dev)
    word = torch.zeros(1, dtype=torch.int32, device=dev)
    seq = torch.zeros(BSZ * NB, 20, dtype=torch.int64, device=dev)
    with pytest.raises(TypeError):
        ops.beam_select_at(logits, running, KEEP, word.to(torch.int64), 0, 10)
    with pytest.raises(ValueError):
        ops.beam_select_at(logits, running, KEEP, word, 0, 21, seq=seq, ngram=2)       # rows shorter than cur_max
    with pytest.raises(RuntimeError):
        ops.beam_select_at(logits, running, KEEP, word, 0, 4097)                       # cur_max above 4096
    with pytest.raises(ValueError):
        ops.beam_select_at(logits, running, KEEP, word, 0, 10, workspace=torch.empty(8, dtype=torch.uint8, device=dev))


# ------------------------------------------------------------------------------------------------ bookkeeping

ABSZ, ANB, AKEEP, AVOCAB, EOS = 3, 3, 6, 11, (2, 5)
KINDS = ("nothing", "some", "all", "stale")


def advance_positions(max_length):
    return list(range(1, max_length)) if max_length <= 8 else [1, 63, 64, 65, 69]


def _load(buffers, state, dev):
    for name in BA.STATE:
        getattr(buffers, name).copy_(torch.from_numpy(state[name]).to(dev).reshape(getattr(buffers, name).shape))


def _prefill(buffers):
    for name in ("running", "finished", "finished_len", "beam_idx", "next_tokens"):
        getattr(buffers, name).fill_(-3)
    for name in ("running_scores", "scores"):
        getattr(buffers, name).fill_(7.5)
    buffers.done.fill_(True)
    buffers.improvable.fill_(False)
    buffers.go_on.fill_(77)


def _outputs(buffers):
    return {name: getattr(buffers, name).cpu() for name in BA.OUTPUTS}


def _same(a, b):
    for name in BA.OUTPUTS:
        x, y = a[name], b[name]
        ok = same_f32(x.numpy(), y.numpy()) if x.dtype == torch.float32 else torch.equal(x, y)
        if not ok:
            return name
    return None


@pytest.mark.parametrize("reciprocal", [True, False], ids=["reciprocal", "divide"])
@pytest.mark.parametrize("length_penalty", [0.8, 1.0, 2.0])
@pytest.mark.parametrize("early_stopping", [False, True, "never"], ids=str)
@pytest.mark.parametrize("max_length", [8, 70])
def test_advance_at_equals_static_at_every_position(dev, max_length, early_stopping, length_penalty, reciprocal):
    from outlier_suppression_amd import ops
    rng = np.random.default_rng(1000 * max_length + int(10 * length_penalty) + len(str(early_stopping)))
    now, out_at, out_static = (ops.BeamBuffers(ABSZ, ANB, max_length, dev) for _ in range(3))
    top_lp = torch.zeros(ABSZ, AKEEP, device=dev)
    top_idx = torch.zeros(ABSZ, AKEEP, dtype=torch.int64, device=dev)
    eos_ids = torch.tensor(EOS, dtype=torch.int64, device=dev)
    word = torch.ones(1, dtype=torch.int32, device=dev)
    len_table, best_table = ops.beam_div_tables(max_length, length_penalty, early_stopping, reciprocal, dev)

    def launch():
        ops.beam_advance_at(top_lp, top_idx, now, out_at, word, -2, AVOCAB, len_table, best_table, eos_ids, early_stopping,
                            reciprocal)

    word.fill_(3)
    _load(now, BA.random_state(rng, ABSZ, ANB, max_length, 1, AVOCAB, "nothing", EOS), dev)
    graph = captured(dev, launch)
    stopped = set()
    for i, cur in enumerate(advance_positions(max_length)):
        kind = KINDS[i % len(KINDS)]
        _load(now, BA.random_state(rng, ABSZ, ANB, max_length, cur, AVOCAB, kind, EOS), dev)
        lp, idx = BA.random_selection(rng, ABSZ, ANB, AKEEP, AVOCAB, EOS, wide=bool(i & 1), hits=True)
        if i % 3 == 1:
            lp[0, AKEEP - 1] = -np.inf                                 # a continuation that cannot be
            lp[1, 1] = lp[1, 0]                                        # and a tie among the real ones
        top_lp.copy_(torch.from_numpy(lp))
        top_idx.copy_(torch.from_numpy(idx))
        word.fill_(cur + 2)                                            # the launch adds -2
        _prefill(out_at)
        _prefill(out_static)
        graph.replay()
        len_div, best_div = BA.divisors(cur, max_length, early_stopping, length_penalty)
        ops.beam_advance(top_lp, top_idx, now, out_static, cur, AVOCAB, eos_ids, early_stopping, len_div, best_div, reciprocal)
        got, want = _outputs(out_at), _outputs(out_static)
        assert _same(got, want) is None, (cur, kind, _same(got, want), got, want)
        assert int(got["go_on"]) in (0, 1)
        assert not bool((got["running"] == -3).any()) and not bool((got["scores"] == 7.5).any())      # the step was written
        if kind == "nothing" and cur + 1 < max_length:                                      # ties among the -1e9 sentinels were there to be ordered
            assert int((want["scores"] <= -1.0e9).sum()) >= 2
        stopped.add(int(got["go_on"]))
    assert 0 in stopped                                                # the last position stops: every candidate hits
    for bad in (0, max_length):
        word.fill_(bad + 2)
        _prefill(out_at)
        before = _outputs(out_at)
        graph.replay()
        after = _outputs(out_at)
        assert int(after["go_on"]) == -1, bad
        after["go_on"], before["go_on"] = None, None
        for name in BA.STATE + ("beam_idx", "next_tokens"):
            x, y = after[name], before[name]
            assert same_f32(x.numpy(), y.numpy()) if x.dtype == torch.float32 else torch.equal(x, y), (bad, name)


def test_advance_at_checks_its_arguments(dev):
    from outlier_suppression_amd import ops
    now, out = ops.BeamBuffers(ABSZ, ANB, 8, dev), ops.BeamBuffers(ABSZ, ANB, 8, dev)
    top_lp = torch.zeros(ABSZ, AKEEP, device=dev)
    top_idx = torch.zeros(ABSZ, AKEEP, dtype=torch.int64, device=dev)
    word = torch.ones(1, dtype=torch.int32, device=dev)
    tables = ops.beam_div_tables(8, 1.0, False, True, dev)
    with pytest.raises(TypeError):
        ops.beam_advance_at(top_lp, top_idx, now, out, word.to(torch.int64), 0, AVOCAB, *tables)
    with pytest.raises(ValueError):
        ops.beam_advance_at(top_lp, top_idx, now, out, word, 0, AVOCAB, tables[0][:7], tables[1])     # a short table
    with pytest.raises(ValueError):
        ops.beam_advance_at(top_lp, top_idx, now, now, word, 0, AVOCAB, *tables)                      # an output is its input

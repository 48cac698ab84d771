"""osq_greedy_advance / osq_greedy_advance_at (csrc/greedy_advance.hip) through ops.greedy_advance(_at) and the C ABI: one
greedy decoding step against the numpy restatement of tests/_greedy_advance.py (pinned to the torch lines by
tests/test_greedy_advance_cpu.py).

Every output -- next_tokens, the whole of seq, unfinished, go_on -- is compared as words with no tolerance, and every output
is pre-filled with a sentinel, so that a word that must not be written is seen.  Over the launch shapes (vocab around the
lane, wave, workgroup and chunk sizes, bsz around one trip of the go_on reduction, padded rows), the winner planted at every
boundary, ties and special values across chunks, the bans, the n-gram windows at the loop's trip boundary and at the longest
history, finishing and stopping, the forced token, the invalid arguments between guard bands, the position-from-device form at
every position and outside the range, a capture, and twice the same call.  Against the torch lines on the same GPU every
case without NaN is compared too (ties and signed zeros included: torch.argmax documents the first maximum); for the NaN cases
torch's GPU argmax is printed and the restatement stays the contract."""
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import _greedy_advance as GA
from test_greedy_advance_cpu import same, torch_step

pytestmark = pytest.mark.gpu

CHUNK = 4096          # tokens one workgroup turns into a candidate
GO_ROWS = 64          # rows one trip of the go_on reduction covers
VOCABS = (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8193, 50265)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _ids(ids, dev):
    return torch.tensor(list(ids), dtype=torch.int64, device=dev) if len(ids) else None


def _buffers(case, dev, seq_pad=0):
    """The case's state on the device; next_tokens and go_on hold sentinels, seq rows lie ``seq_pad`` words apart beyond
    max_length (the gaps hold -9)."""
    bsz, max_length = case["seq"].shape
    wide = torch.full((bsz, max_length + seq_pad), -9, dtype=torch.int64, device=dev)
    wide[:, :max_length] = torch.from_numpy(case["seq"]).to(dev)
    return NS(seq=wide[:, :max_length], wide=wide, unfinished=torch.from_numpy(case["unfinished"].copy()).to(dev),
              next_tokens=torch.full((bsz,), -7, dtype=torch.int64, device=dev),
              go_on=torch.full((1,), 77, dtype=torch.int32, device=dev), workspace=None, room=None)


def _attach_room(bufs):
    from outlier_suppression_amd import ops
    bufs.room = lambda vocab: ops.GreedyBuffers.room(bufs, vocab)
    return bufs


def _logits(case, dev, pad=0):
    """The case's logits on the device; rows ``pad`` floats apart beyond vocab, the gaps holding NaN."""
    bsz, vocab = case["logits"].shape
    wide = torch.full((bsz, vocab + pad), float("nan"), dtype=torch.float32, device=dev)
    wide[:, :vocab] = torch.from_numpy(case["logits"]).to(dev)
    return wide[:, :vocab]


def _outputs(bufs):
    torch.cuda.synchronize()
    assert (bufs.wide[:, bufs.seq.shape[1]:] == -9).all()
    return bufs.next_tokens.cpu().numpy(), bufs.seq.cpu().numpy(), bufs.unfinished.cpu().numpy(), int(bufs.go_on)


def _kernel(case, dev, logits_pad=0, seq_pad=0):
    from outlier_suppression_amd import ops
    bufs = _attach_room(_buffers(case, dev, seq_pad))
    kw = GA.kernel_arguments(case)
    ops.greedy_advance(_logits(case, dev, logits_pad), bufs, case["cur"], kw["ngram"], _ids(kw["ban_ids"], dev), kw["forced"],
                       _ids(kw["eos_ids"], dev), kw["pad"])
    return _outputs(bufs)


def check(case, dev, label, **pads):
    """The kernel against the restatement, and, without NaN, against the torch lines on the GPU.  Returns the tokens."""
    got = _kernel(case, dev, **pads)
    same(got, GA.reference_case(case), label)
    if not GA.has_nan(case):
        same(got, torch_step(case, dev), (label, "torch on the GPU"))
    return got[0]


def test_a_every_case_of_the_cpu_test(dev):
    for label, case in GA.all_cases():
        check(case, dev, label)


def _positions(vocab):
    at = {0, vocab - 1, 63, 64, 255, 256}
    for c in range(CHUNK, vocab + 1, CHUNK):
        at |= {c - 1, c}
    return sorted(p for p in at if 0 <= p < vocab)


@pytest.mark.parametrize("vocab", VOCABS)
def test_b_shapes_with_the_winner_at_every_boundary(dev, vocab):
    """bsz 1 and 3; every row of a call has its winner planted at another boundary position."""
    rng = np.random.default_rng(vocab)
    for bsz in (1, 3):
        at = _positions(vocab)
        for k in range(0, len(at), bsz):
            rows = [at[(k + r) % len(at)] for r in range(bsz)]
            x = rng.uniform(-4, 4, size=(bsz, vocab)).astype(np.float32)
            x[np.arange(bsz), rows] = 50.0
            case = GA.make(rng, bsz, vocab, 6, 3, logits=x, eos=(0,), pad=0)
            assert check(case, dev, (vocab, bsz, rows)).tolist() == rows


@pytest.mark.parametrize("bsz", (GO_ROWS - 1, GO_ROWS, GO_ROWS + 1))
def test_c_rows_around_one_trip_of_the_go_on_reduction(dev, bsz):
    rng = np.random.default_rng(bsz)
    x = GA.planted(rng, bsz, 5, 4)                                       # every unfinished row picks the eos 4
    for alive, want in (((), 0), ((0,), 0), ((bsz - 1,), 0)):
        unfinished = np.zeros(bsz, dtype=np.uint8)
        unfinished[list(alive)] = 1
        case = GA.make(rng, bsz, 5, 6, 3, logits=x, unfinished=unfinished, eos=(4,), pad=1)
        check(case, dev, (bsz, alive))
        assert GA.reference_case(case)[3] == want
    for alive in ((0,), (bsz - 1,), (min(GO_ROWS, bsz) - 1,), tuple(range(bsz))):   # they go on: the winner 3 is no eos
        unfinished = np.zeros(bsz, dtype=np.uint8)
        unfinished[list(alive)] = 1
        case = GA.make(rng, bsz, 5, 6, 3, logits=GA.planted(rng, bsz, 5, 3), unfinished=unfinished, eos=(4,), pad=1)
        check(case, dev, (bsz, alive, "go on"))
        assert GA.reference_case(case)[3] == 1
    check(GA.make(rng, bsz, 5, 6, 3), dev, (bsz, "no eos"))


def test_d_padded_rows(dev):
    """A logits row stride above vocab with NaN in the gaps, a seq row stride above max_length."""
    rng = np.random.default_rng(4)
    for vocab in (5, 4097):
        case = GA.make(rng, 3, vocab, 7, 4, ngram=2, eos=(2,), pad=1)
        check(case, dev, (vocab, "padded"), logits_pad=3, seq_pad=5)
        check(case, dev, (vocab, "padded logits"), logits_pad=1)
        check(case, dev, (vocab, "padded seq"), seq_pad=1)


def test_e_ties_and_special_values_across_chunks(dev):
    rng = np.random.default_rng(5)
    vocab, bsz, nan, inf = 2 * CHUNK + 1, 2, np.float32(np.nan), np.float32(np.inf)
    base = lambda: rng.uniform(-4, 4, size=(bsz, vocab)).astype(np.float32)   # noqa: E731
    mk = lambda x, **kw: GA.make(rng, bsz, vocab, 6, 3, logits=x, **kw)       # noqa: E731
    x = base()
    x[:, CHUNK - 1] = x[:, CHUNK] = 9.0
    assert check(mk(x), dev, "equal maxima in two chunks").tolist() == [CHUNK - 1] * bsz
    x[:, 2 * CHUNK] = 9.0
    assert check(mk(x), dev, "equal maxima in three chunks").tolist() == [CHUNK - 1] * bsz
    assert check(mk(np.full((bsz, vocab), 2.5, dtype=np.float32)), dev, "a constant row").tolist() == [0] * bsz
    for a, b in ((7, 300), (CHUNK - 2, CHUNK + 5), (300, 2 * CHUNK)):
        for first, second in ((-0.0, 0.0), (0.0, -0.0)):
            x = np.full((bsz, vocab), -3.0, dtype=np.float32)
            x[:, a], x[:, b] = first, second
            assert check(mk(x), dev, ("signed zeros", a, b, first)).tolist() == [a] * bsz
    x = base()
    x[:, 5], x[:, vocab - 1] = 1e30, nan
    assert check(mk(x), dev, "NaN last against a large number first").tolist() == [vocab - 1] * bsz
    x[:, CHUNK + 1] = nan
    assert check(mk(x), dev, "two NaNs in two chunks").tolist() == [CHUNK + 1] * bsz
    x = base()
    x[:, CHUNK + 1], x[:, 17] = nan, 30.0
    assert check(mk(x, eos=(CHUNK + 1,), pad=1, min_length=5), dev, "a banned NaN").tolist() == [17] * bsz
    assert check(mk(np.full((bsz, vocab), -inf, dtype=np.float32)), dev, "all -inf").tolist() == [0] * bsz
    x = np.full((bsz, vocab), -inf, dtype=np.float32)
    x[:, 2 * CHUNK] = -3e38
    assert check(mk(x), dev, "all -inf but the last").tolist() == [2 * CHUNK] * bsz


def test_f_banned_ids_take_the_would_be_winner(dev):
    rng = np.random.default_rng(6)
    vocab, ids = 4099, (0, 4095, 4096, 4098, 9)
    for t in ids:
        x = GA.planted(rng, 2, vocab, t)
        x[:, 2000] = 40.0
        case = GA.make(rng, 2, vocab, 8, 3, logits=x, eos=ids, pad=1, min_length=4)
        assert check(case, dev, ("banned", t)).tolist() == [2000, 2000]
        assert check(dict(case, min_length=3), dev, ("free", t)).tolist() == [t, t]
    x = np.full((2, vocab), 1.0, dtype=np.float32)
    assert check(GA.make(rng, 2, vocab, 8, 3, logits=x, eos=ids, pad=1, min_length=4), dev, "banned, constant").tolist() == [1, 1]


@pytest.mark.parametrize("cur, max_length", [(300, 302), (4095, 4096)])
def test_g_ngram_windows_at_the_trip_boundary_and_the_longest_history(dev, cur, max_length):
    """A history of distinct tokens with one repeated window planted first, around index 255 / 256 (the second trip of the
    window loop), late, and last; the window's last token is the would-be winner."""
    rng = np.random.default_rng(cur)
    vocab, n, W = 8200, 3, 8190
    for p in (0, 254, 255, 256, cur - 40, "last"):
        history = np.tile(rng.permutation(np.arange(10, 8000))[:cur], (2, 1)).astype(np.int64)
        if p == "last":
            history[:, cur - n:] = W                                    # the last window is its own suffix
        else:
            history[:, p:p + n - 1] = history[:, cur - n + 1:]
            history[:, p + n - 1] = W
        history[1] = np.arange(10, 10 + cur)                            # the second row repeats nothing
        x = GA.planted(rng, 2, vocab, W)
        x[:, 3] = 40.0
        case = GA.make(rng, 2, vocab, max_length, cur, logits=x, history=history, ngram=n)
        assert check(case, dev, ("window", p)).tolist() == [3, W]
        assert check(dict(case, ngram=1), dev, ("window, n = 1", p)).tolist() == [3, W]


def test_h_sixteen_eos_ids(dev):
    rng = np.random.default_rng(8)
    eos = tuple(range(20, 36))
    for winner, unfinished in ((35, (1, 1, 0)), (20, (1, 0, 1)), (19, (1, 1, 1)), (36, (0, 0, 1))):
        x = GA.planted(rng, 3, 70, winner)
        case = GA.make(rng, 3, 70, 9, 4, logits=x, unfinished=unfinished, eos=eos, pad=1, min_length=0)
        check(case, dev, ("16 eos", winner))
        check(dict(case, min_length=5), dev, ("16 eos banned", winner))


GUARD = 64
INVALID = ["bsz = 0", "vocab = 0", "max_length = 0", "vocab = 2^31", "max_length > 4096", "cur < 1", "cur >= max_length",
           "n_ban > 16", "n_eos > 16", "null unfinished", "forced >= vocab", "pad >= vocab", "pad < 0", "logits stride",
           "seq stride", "ngram without seq", "workspace too small", "forced_bos >= vocab", "forced_eos >= vocab",
           "null cur_dev", "valid", "valid at"]


@pytest.mark.parametrize("what", INVALID)
def test_i_invalid_arguments_launch_nothing(dev, what):
    """Every invalid-argument case returns OSQ_ERR_INVALID_ARGUMENT and writes nothing: each output lies between guard bands
    and keeps its fill.  The same calls with valid arguments write their outputs and leave the bands alone."""
    from outlier_suppression_amd import _hip
    lib = _hip.load()
    a = dict(bsz=2, vocab=50, max_length=8, cur=3, n_ban=1, n_eos=1, forced=-1, pad=1, ngram=2, logits_stride=50, seq_stride=8,
             forced_bos=-1, forced_eos=-1)
    at = what in ("forced_bos >= vocab", "forced_eos >= vocab", "null cur_dev", "valid at")
    change = {"bsz = 0": dict(bsz=0), "vocab = 0": dict(vocab=0, logits_stride=0), "max_length = 0": dict(max_length=0),
              "vocab = 2^31": dict(vocab=2 ** 31, logits_stride=2 ** 31), "max_length > 4096": dict(max_length=4097, seq_stride=4097),
              "cur < 1": dict(cur=0), "cur >= max_length": dict(cur=8), "n_ban > 16": dict(n_ban=17), "n_eos > 16": dict(n_eos=17),
              "forced >= vocab": dict(forced=50), "pad >= vocab": dict(pad=50), "pad < 0": dict(pad=-1),
              "logits stride": dict(logits_stride=49), "seq stride": dict(seq_stride=7), "forced_bos >= vocab": dict(forced_bos=50),
              "forced_eos >= vocab": dict(forced_eos=50)}
    a.update(change.get(what, {}))
    logits = torch.zeros(2 * 50, dtype=torch.float32, device=dev)
    ids = torch.arange(2, 19, dtype=torch.int64, device=dev)
    word = torch.full((1,), 3, dtype=torch.int32, device=dev)
    sizes = dict(seq=(2 * 8, torch.int64), unfinished=(2, torch.uint8), next_tokens=(2, torch.int64), go_on=(1, torch.int32),
                 ws=(64, torch.uint8))
    outs = {k: torch.full((n + 2 * GUARD,), 85, dtype=dt, device=dev) for k, (n, dt) in sizes.items()}
    ptr = {k: t[GUARD:].data_ptr() for k, t in outs.items()}
    if what == "null unfinished":
        ptr["unfinished"] = None
    if what == "ngram without seq":
        ptr["seq"] = None
    ws_bytes = int(lib.osq_greedy_advance_workspace_bytes(2, 50)) - (1 if what == "workspace too small" else 0)
    assert ws_bytes in (23, 24)
    head = (logits.data_ptr(), a["logits_stride"], ptr["seq"], a["seq_stride"])
    tail = (ids.data_ptr(), a["n_eos"], a["pad"], ptr["unfinished"], a["bsz"], a["vocab"], a["max_length"], ptr["next_tokens"],
            ptr["go_on"], ptr["ws"], ws_bytes, _hip.raw_stream(dev))
    if at:
        rc = lib.osq_greedy_advance_at(*head, None if what == "null cur_dev" else word.data_ptr(), 0, a["ngram"], ids.data_ptr(),
                                       a["n_ban"], 5, a["forced_bos"], a["forced_eos"], *tail)
    else:
        rc = lib.osq_greedy_advance(*head, a["cur"], a["ngram"], ids.data_ptr(), a["n_ban"], a["forced"], *tail)
    torch.cuda.synchronize()
    if what in ("valid", "valid at"):
        assert rc == 0
        seq = outs["seq"][GUARD:GUARD + 16].view(2, 8)
        assert (seq[:, 3] != 85).all() and (seq[:, :3] == 85).all() and (seq[:, 4:] == 85).all()
        for k, used in (("unfinished", 2), ("next_tokens", 2), ("go_on", 1)):
            t = outs[k]
            assert (t[:GUARD] == 85).all() and (t[GUARD + used:] == 85).all() and (t[GUARD:GUARD + used] != 85).all(), k
        for k, used in (("seq", 16), ("ws", 24)):
            assert (outs[k][:GUARD] == 85).all() and (outs[k][GUARD + used:] == 85).all(), k
        return
    assert rc == -1 and lib.osq_last_error()
    for k, t in outs.items():
        assert (t == 85).all(), k


def test_j_ops_wrapper_checks(dev):
    from outlier_suppression_amd import ops
    bufs = ops.GreedyBuffers(2, 8, dev)
    logits = torch.randn(2, 50, device=dev)
    assert ops.greedy_advance(logits, bufs, 1) is bufs
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.greedy_advance(logits.cpu(), bufs, 1)
    with pytest.raises(TypeError, match="float32"):
        ops.greedy_advance(logits.double(), bufs, 1)
    with pytest.raises(ValueError, match="seq"):
        ops.greedy_advance(logits[:1], bufs, 1)
    with pytest.raises(ValueError, match="eos_ids"):
        ops.greedy_advance(logits, bufs, 1, eos_ids=torch.zeros(1, dtype=torch.int32, device=dev))
    with pytest.raises(RuntimeError, match="status -1"):
        ops.greedy_advance(logits, bufs, 8)
    with pytest.raises(TypeError, match="cur"):
        ops.greedy_advance_at(logits, bufs, torch.zeros(1, dtype=torch.int64, device=dev))


AT = dict(bsz=3, vocab=4100, max_length=12)


def _at_case(rng, cur, **settings):
    x = GA.planted(rng, AT["bsz"], AT["vocab"], 4097)                    # the winner is an eos id: banned below min_length
    x[:, 0], x[:, 1], x[:, 4] = 45.0, 44.0, 40.0                          # then 0, 1 (the n-gram rule bans one of them), then 4
    x[1, 4097] = -5.0
    history = np.array([[(b + i) % 2 for i in range(cur)] for b in range(AT["bsz"])], dtype=np.int64)
    return GA.make(rng, AT["bsz"], AT["vocab"], AT["max_length"], cur, logits=x, history=history, unfinished=(1, 1, 0), **settings)


def _at_kernel(case, dev, word_value, cur_add):
    from outlier_suppression_amd import ops
    bufs = _attach_room(_buffers(case, dev))
    word = torch.full((1,), word_value, dtype=torch.int32, device=dev)
    ops.greedy_advance_at(_logits(case, dev), bufs, word, cur_add, ngram=case["ngram"], ban_ids=_ids(case["eos"], dev),
                          ban_below=case["min_length"], forced_bos=case["forced_bos"], forced_eos=case["forced_eos"],
                          eos_ids=_ids(case["eos"], dev), pad=case["pad"])
    return _outputs(bufs)


@pytest.mark.parametrize("settings", [dict(eos=(4097, 9), pad=1, min_length=6, ngram=2, forced_bos=7, forced_eos=9),
                                      dict(eos=(4097,), pad=1, min_length=6), dict(forced_eos=5), dict(ngram=1, forced_bos=7)],
                         ids=["all", "min-length", "forced eos", "ngram, forced bos"])
def test_k_position_from_the_device_equals_the_static_call(dev, settings):
    rng = np.random.default_rng(11)
    tokens = []
    for cur in range(1, AT["max_length"]):
        case = _at_case(rng, cur, **settings)
        static = _kernel(case, dev)
        same(static, GA.reference_case(case), ("static", cur))
        same(_at_kernel(case, dev, cur, 0), static, ("at", cur))
        same(_at_kernel(case, dev, cur + 2, -2), static, ("at, cur_add", cur))
        tokens.append(static[0].tolist())
    assert len({tuple(t) for t in tokens}) >= 2                          # the settings change the step along the way


@pytest.mark.parametrize("position", (-5, 0, 12, 2 ** 30))
def test_l_refused_position_writes_go_on_only(dev, position):
    rng = np.random.default_rng(12)
    case = _at_case(rng, 3, eos=(4097, 9), pad=1, min_length=6, ngram=2, forced_bos=7, forced_eos=9)
    for word, add in ((position, 0), (position - 7, 7)):
        token, seq, unfinished, go_on = _at_kernel(case, dev, word, add)
        assert go_on == -1
        assert (token == -7).all() and np.array_equal(seq, case["seq"]) and np.array_equal(unfinished, case["unfinished"])


def test_m_captured_and_replayed_in_place(dev):
    """The _at call captured into a graph on a side stream (after one issued warm-up there) and replayed while the device word
    advances over five positions, in place on one seq buffer: the static calls' words, forced eos on the last step included."""
    from outlier_suppression_amd import ops
    rng = np.random.default_rng(13)
    bsz, vocab, max_length, first = 3, 4100, 9, 4
    settings = dict(eos=(4097, 9), pad=1, min_length=6, ngram=2, forced_eos=9)
    start = GA.make(rng, bsz, vocab, max_length, first, **settings)
    bufs = _attach_room(_buffers(start, dev))
    logits = _logits(start, dev).contiguous()
    word = torch.full((1,), first, dtype=torch.int32, device=dev)
    eos = _ids(settings["eos"], dev)
    call = lambda: ops.greedy_advance_at(logits, bufs, word, 0, ngram=2, ban_ids=eos, ban_below=6, forced_eos=9, eos_ids=eos,  # noqa: E731
                                         pad=1)
    keep = (bufs.seq.clone(), bufs.unfinished.clone())
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        call()
    bufs.seq.copy_(keep[0]), bufs.unfinished.copy_(keep[1])
    case = start
    for cur in range(first, max_length):
        x = rng.standard_normal((bsz, vocab)).astype(np.float32)
        x[:, 4097 if cur == 5 else 1] += 30.0                               # at 5 the eos 4097 is still banned
        case = dict(case, logits=x, cur=cur)
        logits.copy_(torch.from_numpy(x).to(dev))
        word.fill_(cur)
        bufs.next_tokens.fill_(-7), bufs.go_on.fill_(77)
        graph.replay()
        got = _outputs(bufs)
        want = GA.reference_case(case)
        same(got, want, ("replay", cur))
        same(got, _kernel(case, dev), ("replay / static", cur))
        alive = case["unfinished"] != 0
        case = dict(case, seq=want[1], unfinished=want[2])
    assert want[3] == 0 and alive.any() and (want[0][alive] == 9).all() and (want[0][~alive] == 1).all()


def test_n_the_same_call_twice_gives_the_same_words(dev):
    rng = np.random.default_rng(14)
    x = rng.integers(-2, 3, size=(3, 50265)).astype(np.float32)          # thousands of tied maxima in every chunk
    x[1, 777] = np.nan
    case = GA.make(rng, 3, 50265, 40, 20, logits=x, ngram=2, eos=(2,), pad=1, min_length=30)
    first, second = _kernel(case, dev), _kernel(case, dev)
    same(first, second, "twice")
    same(first, GA.reference_case(case), "twice / reference")


def test_o_what_torch_does_with_nan_on_this_gpu(dev):
    """Not a contract: torch's GPU argmax on the NaN cases, printed beside the restatement (which is numpy's and torch's CPU
    order, pinned by the CPU test)."""
    for label, case in GA.all_cases():
        if GA.has_nan(case) and GA.kernel_arguments(case)["forced"] is None:
            print(f"{label}: torch on the GPU {torch_step(case, dev)[0].tolist()}, the restatement {GA.reference_case(case)[0].tolist()}")

"""osq_sample_advance / osq_sample_advance_at / osq_sample_uniforms (csrc/sample_advance.hip) through ops.sample_advance(_at),
ops.sample_uniforms and the C ABI: one sampling step against the float64 restatement of tests/_sample_advance.py (pinned to
transformers' warpers and to the torch lines by tests/test_sample_advance_cpu.py).

next_tokens, the whole of seq, unfinished and go_on are compared as words; every output is pre-filled with a sentinel.  A
planted uniform lies at the midpoint of a survivor's float64 interval, at least 1e-3 W from its ends, so the token is exact;
the Philox draws are held to the band of the fp32 sums (2e-5 W, profiles/beam_select_accuracy.txt: the same sums), the largest
excursion measured going to profiles/sample_advance_accuracy.txt when OSQ_SAMPLE_ADVANCE_ACCURACY_OUT=<path> is set."""
import os

import numpy as np
import pytest
import torch

import _greedy_advance as GA
import _sample_advance as SA
from test_greedy_advance_cpu import same

pytestmark = pytest.mark.gpu

CHUNK = 4096
VOCABS = (1, 63, 64, 65, 4095, 4096, 4097, 8193)
TOP_KS = (1, 2, 63, 64)
LAST_U = np.float32(1 - 2.0 ** -24)
_seen = {}             # label -> the largest excursion of a Philox draw, in units of W


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _ids(ids, dev):
    return torch.tensor(list(ids), dtype=torch.int64, device=dev) if len(ids) else None


def _buffers(case, dev, seq_pad=0):
    """The case's state in an ops.SampleBuffers; next_tokens and go_on hold sentinels, seq rows lie ``seq_pad`` words apart
    beyond max_length (the gaps hold -9)."""
    from outlier_suppression_amd import ops
    bsz, max_length = case["seq"].shape
    bufs = ops.SampleBuffers(bsz, max_length, dev, top_k=case["top_k"])
    bufs.wide = torch.full((bsz, max_length + seq_pad), -9, dtype=torch.int64, device=dev)
    bufs.wide[:, :max_length] = torch.from_numpy(case["seq"]).to(dev)
    bufs.seq = bufs.wide[:, :max_length]
    bufs.unfinished = torch.from_numpy(case["unfinished"].copy()).to(dev)
    bufs.next_tokens.fill_(-7)
    bufs.go_on.fill_(77)
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


def _draw(case):
    return dict(temperature=case["temperature"], top_k=case["top_k"], top_p=case["top_p"])


def _kernel(case, dev, u=None, seed=0, logits_pad=0, seq_pad=0):
    from outlier_suppression_amd import ops
    bufs = _buffers(case, dev, seq_pad)
    kw = GA.kernel_arguments(case)
    planted = None if u is None else torch.from_numpy(np.asarray(u, dtype=np.float32)).to(dev)
    assert ops.sample_advance(_logits(case, dev, logits_pad), bufs, case["cur"], seed, ngram=kw["ngram"],
                              ban_ids=_ids(kw["ban_ids"], dev), forced=kw["forced"], eos_ids=_ids(kw["eos_ids"], dev),
                              pad=kw["pad"], uniforms=planted, **_draw(case)) is bufs
    return _outputs(bufs)


def check(case, dev, u, label, **pads):
    """The kernel with the planted draws ``u`` against the restatement, all four outputs.  Returns the tokens."""
    got = _kernel(case, dev, u, **pads)
    same(got, SA.reference_case(case, u), label)
    return got[0]


def _one_row_per_survivor(case):
    """The case with its one row repeated once per kept survivor, and the draws at the midpoints of their intervals."""
    sv = SA.row(case, 0)
    n = sv.tokens.size
    u = np.array([SA.midpoint(sv, i) for i in range(n)], dtype=np.float32)
    rep = lambda a: np.repeat(a[:1], n, axis=0)            # noqa: E731
    return dict(case, logits=rep(case["logits"]), seq=rep(case["seq"]), unfinished=rep(case["unfinished"])), u, sv


def _boundary_tokens(vocab):
    at = {0, vocab - 1}
    for c in range(CHUNK, vocab + 1, CHUNK):
        at |= {c - 1, c}
    return sorted(t for t in at if 0 <= t < vocab)


def _heavy(rng, vocab, n, where):
    """n distinct tokens: the chunk boundaries first (``where`` == "chunks": one winner per chunk's first and last token), or
    all of them inside the last whole chunk."""
    n = min(n, vocab)
    if where == "chunks":
        first = _boundary_tokens(vocab)[:n]
        rest = np.setdiff1d(np.arange(vocab), first)
        return np.concatenate([first, rng.choice(rest, n - len(first), replace=False)]).astype(np.int64)
    c = (vocab - 1) // CHUNK
    if vocab - c * CHUNK < n:                                            # the last chunk is too short: the one before it
        c -= 1
    return (c * CHUNK + rng.choice(min(CHUNK, vocab - c * CHUNK), n, replace=False)).astype(np.int64)


def test_a_uniforms_are_the_hosts(dev):
    from outlier_suppression_amd import ops
    from outlier_suppression_amd.model import sampling
    for seed in (0, 1, 2 ** 64 - 1):
        for cur in (1, 31, 4095):
            got = ops.sample_uniforms(seed, 66, cur, dev).cpu()
            assert torch.equal(got.view(torch.int32), sampling.uniforms(seed, 66, cur).view(torch.int32)), (seed, cur)


@pytest.mark.parametrize("vocab", VOCABS)
def test_b_every_survivor_of_the_top_k_form_at_its_midpoint(dev, vocab):
    rng = np.random.default_rng(vocab)
    for top_k in TOP_KS + ((vocab + 1,) if vocab < 64 else ()):          # vocab 1 and 63: top_k above vocab
        for where in ("chunks", "one chunk") if vocab > CHUNK else ("chunks",):
            n = min(top_k, vocab)
            x = SA.spread_logits(rng, 1, vocab, [_heavy(rng, vocab, n, where)])
            case = SA.make(rng, 1, vocab, 6, 3, 0.9, top_k, 1.0, logits=x, eos=(0,), pad=0)
            SA.assert_kth_distinct(case)
            many, u, sv = _one_row_per_survivor(case)
            assert sv.tokens.size == n
            assert check(many, dev, u, (vocab, top_k, where)).tolist() == sv.tokens.tolist()
    if vocab > 1:                                                        # a padded row stride, NaN in the gaps
        check(many, dev, u, (vocab, "padded"), logits_pad=3, seq_pad=5)


def test_c_equal_values_across_a_chunk_boundary(dev):
    rng = np.random.default_rng(3)
    vocab = 2 * CHUNK + 1
    x = SA.spread_logits(rng, 1, vocab, [[7]], hi=1.0)
    x[0, [CHUNK - 1, CHUNK, 2 * CHUNK]] = 3.0
    one = SA.make(rng, 1, vocab, 6, 3, 1.0, 1, 1.0, logits=x)
    for u in (0.0, 0.5, LAST_U):
        assert check(one, dev, np.array([u], dtype=np.float32), ("tie, k 1", u)).tolist() == [CHUNK - 1]
    many, u, sv = _one_row_per_survivor(dict(one, top_k=2))
    assert sv.tokens.tolist() == [CHUNK - 1, CHUNK] and check(many, dev, u, "tie, k 2").tolist() == [CHUNK - 1, CHUNK]
    many, u, sv = _one_row_per_survivor(dict(one, top_k=4))
    assert sv.tokens.tolist() == [CHUNK - 1, CHUNK, 2 * CHUNK, 7] and check(many, dev, u, "tie, k 4").tolist() == sv.tokens.tolist()
    x[0, 9] = -0.0                                                        # signed zeros are one value: the smaller token first
    x[0, 5000] = 0.0
    zeros = SA.make(rng, 1, vocab, 6, 3, 1.0, 5, 1.0, logits=np.where(x == 3.0, np.float32(-1.0), x))
    many, u, sv = _one_row_per_survivor(zeros)
    assert sv.tokens.tolist()[:3] == [7, 9, 5000] and check(many, dev, u, "zeros").tolist() == sv.tokens.tolist()


@pytest.mark.parametrize("vocab", VOCABS)
def test_d_heavy_tokens_of_the_full_vocabulary_form_at_their_midpoints(dev, vocab):
    rng = np.random.default_rng(vocab + 1)
    heavy = np.array(_boundary_tokens(vocab) + ([vocab // 3] if vocab > 3 else []))
    x = SA.spread_logits(rng, 1, vocab, [heavy])
    case = SA.make(rng, 1, vocab, 6, 3, 1.1, 0, 1.0, logits=x, eos=(0,), pad=0)
    sv = SA.row(case, 0)
    at = [int(np.flatnonzero(sv.tokens == t)[0]) for t in sorted(heavy)]
    u = np.array([SA.midpoint(sv, i) for i in at] + [0.0, LAST_U], dtype=np.float32)
    rep = lambda a: np.repeat(a[:1], len(u), axis=0)                      # noqa: E731
    many = dict(case, logits=rep(case["logits"]), seq=rep(case["seq"]), unfinished=rep(case["unfinished"]))
    got = check(many, dev, u, (vocab, "full")).tolist()
    assert got[:len(at)] == sorted(heavy.tolist()) and got[-2] == 0 and got[-1] == vocab - 1
    check(many, dev, u, (vocab, "full, padded"), logits_pad=1, seq_pad=2)


def test_e_top_p_cut_either_side_of_every_threshold(dev):
    rng = np.random.default_rng(5)
    vocab, k = 4100, 16
    x = SA.spread_logits(rng, 1, vocab, [_heavy(rng, vocab, k, "chunks")])
    base = SA.make(rng, 1, vocab, 6, 3, 1.0, k, 1.0, logits=x)
    above = SA.row(base, 0).above
    assert (np.diff(above) >= 4 * SA.MARGIN).all()
    for r in range(1, k):
        for side, kept in ((-1.5 * SA.MARGIN, r), (1.5 * SA.MARGIN, r + 1)):
            case = dict(base, top_p=float(above[r] + side))
            SA.assert_top_p_margin(case)
            sv = SA.row(case, 0)
            assert sv.tokens.size == kept
            two = dict(case, logits=np.repeat(x, 2, axis=0), seq=np.repeat(case["seq"], 2, axis=0),
                       unfinished=np.repeat(case["unfinished"], 2))
            u = np.array([SA.midpoint(sv, kept - 1), LAST_U], dtype=np.float32)
            assert check(two, dev, u, ("top-p", r, side)).tolist() == [int(sv.tokens[-1])] * 2
    tiny = dict(base, top_p=1e-6)                                         # rank 0 always stays
    assert check(tiny, dev, np.array([LAST_U]), "top-p, rank 0 alone").tolist() == [int(SA.row(base, 0).tokens[0])]


def test_f_banned_ids_nan_and_infinities(dev):
    rng = np.random.default_rng(6)
    vocab, ids = 4099, (0, 4095, 4096, 4098, 9)
    for top_k in (0, 3):
        for t in ids:                                                    # the would-be winner banned by id
            x = SA.spread_logits(rng, 2, vocab, [[t, 2000, 77]] * 2)
            x[:, t] = 9.0
            case = SA.make(rng, 2, vocab, 8, 3, 1.0, top_k, 1.0, logits=x, eos=ids, pad=1, min_length=4)
            u = np.array([0.01, 0.99], dtype=np.float32)
            assert set(check(case, dev, u, ("banned", top_k, t)).tolist()) <= {2000, 77}
            free = check(dict(case, min_length=3), dev, np.array([0.3, 0.6], dtype=np.float32), ("free", top_k, t))
            assert free.tolist() == [t, t]
        x = SA.spread_logits(rng, 3, vocab, [[5, 4096, 4098]] * 3)
        x[0, 5], x[1, 4096], x[2, :] = np.nan, np.inf, -np.inf
        x[1, 11] = np.inf
        case = SA.make(rng, 3, vocab, 8, 3, 1.0, top_k, 1.0, logits=x)
        got = check(case, dev, np.array([0.99, 0.75, 0.5], dtype=np.float32), ("NaN, +inf, all -inf", top_k)).tolist()
        assert got[0] != 5 and got[1] == 4096 and got[2] == 0
        assert check(case, dev, np.array([0.01, 0.25, 0.0], dtype=np.float32), ("NaN, +inf, all -inf, low", top_k)).tolist()[1] == 11
        history = np.tile(np.array([0, 1, 2, 1], dtype=np.int64), (2, 1))
        banned = SA.make(rng, 2, 3, 9, 4, 1.0, min(top_k, 3), 1.0, history=history, ngram=1)
        assert check(banned, dev, np.array([0.2, 0.9], dtype=np.float32), ("every token banned", top_k)).tolist() == [0, 0]


@pytest.mark.parametrize("cur, max_length", [(300, 302), (4095, 4096)])
def test_g_the_ngram_rule_takes_the_would_be_winner(dev, cur, max_length):
    rng = np.random.default_rng(cur)
    vocab, n, W = 8200, 3, 8190
    for top_k in (0, 2):
        for p in (0, 255, 256, "last"):
            history = np.tile(rng.permutation(np.arange(10, 8000))[:cur], (2, 1)).astype(np.int64)
            if p == "last":
                history[:, cur - n:] = W
            else:
                history[:, p:p + n - 1] = history[:, cur - n + 1:]
                history[:, p + n - 1] = W
            history[1] = np.arange(10, 10 + cur)                          # the second row repeats nothing
            x = SA.spread_logits(rng, 2, vocab, [[W, 3]] * 2)
            x[:, W], x[:, 3] = 9.0, 1.0
            case = SA.make(rng, 2, vocab, max_length, cur, 1.0, top_k, 1.0, logits=x, history=history, ngram=n)
            assert check(case, dev, np.array([0.5, 0.5], dtype=np.float32), ("window", top_k, p)).tolist() == [3, W]


SHAPES = [(v, k, p) for v in VOCABS for k, p in ((0, 1.0), (2, 1.0), (64, 0.9))] + [(50265, 50, 0.95), (50265, 0, 1.0)]


@pytest.mark.parametrize("vocab, top_k, top_p", SHAPES)
def test_h_philox_draws_within_the_band(dev, vocab, top_k, top_p):
    """uniforms=None: the kernel's own draws.  Its token at survivor position i passes iff C_{i-1} - eps W <= u W <= C_i + eps W."""
    from outlier_suppression_amd.model import sampling
    rng = np.random.default_rng(vocab * 7 + top_k)
    bsz, cur, seed = 64, 5, 0x9e3779b97f4a7c15 + vocab
    case = SA.make(rng, bsz, vocab, 9, cur, 0.8, top_k, top_p, ngram=2, eos=(min(2, vocab - 1),), pad=0, min_length=7)
    got = _kernel(case, dev, None, seed=seed)
    u = sampling.uniforms(seed, bsz, cur).numpy()
    worst = max(SA.excursion(SA.row(case, b), int(got[0][b]), u[b]) for b in range(bsz))
    print(f"vocab {vocab} top_k {top_k} top_p {top_p}: largest excursion {worst:.3e} W")
    _seen[f"v{vocab} k{top_k} p{top_p}"] = worst
    assert worst <= SA.EPS, worst
    planted = _kernel(case, dev, u, seed=seed + 1)                        # the same draws planted: the same words
    same(got, planted, "Philox / planted")
    if len({int(t) for t in got[0]}) > 1:
        assert not np.array_equal(_kernel(case, dev, None, seed=seed + 1)[0], got[0]) or vocab < 4


def test_i_accuracy_record():
    path = os.environ.get("OSQ_SAMPLE_ADVANCE_ACCURACY_OUT")
    if path and _seen:
        with open(path, "w") as f:
            f.write("osq_sample_advance with its own Philox draws against the float64 restatement (tests/_sample_advance.py): how far\n"
                    f"u * W lies outside the float64 interval of the kernel's token, in units of W (0: inside); bound {SA.EPS:g},\n"
                    "64 rows per shape, temperature 0.8, n-gram 2 and a min-length ban on\n\n")
            for label, worst in _seen.items():
                f.write(f"{label:40s} {worst:.3e}\n")
            f.write(f"\nlargest: {max(_seen.values()):.3e}\n")


@pytest.mark.parametrize("bsz", (63, 64, 65))
def test_j_finishing_and_stopping(dev, bsz):
    rng = np.random.default_rng(bsz)
    eos = tuple(range(20, 36))                                            # sixteen eos ids
    for top_k in (0, 4):
        for winner, alive, go_on in ((35, (bsz - 1,), 0), (19, (bsz - 1,), 1), (20, (), 0), (19, (0,), 1), (19, range(bsz), 1)):
            x = SA.spread_logits(rng, bsz, 70, [[winner]] * bsz)
            unfinished = np.zeros(bsz, dtype=np.uint8)
            unfinished[list(alive)] = 1
            case = SA.make(rng, bsz, 70, 9, 4, 1.0, top_k, 1.0, logits=x, unfinished=unfinished, eos=eos, pad=1)
            u = rng.uniform(0.001, 0.999, bsz).astype(np.float32)          # one survivor weighs everything
            got = _kernel(case, dev, u)
            same(got, SA.reference_case(case, u), (bsz, winner, top_k))
            assert (got[0][unfinished != 0] == winner).all()
            assert got[3] == go_on
        forced = SA.make(rng, bsz, 70, 9, 8, 1.0, top_k, 1.0, logits=np.full((bsz, 70), np.nan, dtype=np.float32),
                         forced_eos=21, eos=eos, pad=1)
        got = check(forced, dev, np.zeros(bsz, dtype=np.float32), ("forced", top_k))
        assert got.tolist() == [21] * bsz


GUARD = 64
INVALID = ["top_k < 0", "top_k > 64", "top_p = 0", "top_p > 1", "top_p NaN", "temperature = 0", "temperature < 0",
           "temperature inf", "temperature NaN", "bsz = 0", "cur >= max_length", "n_eos > 16", "forced >= vocab", "logits stride",
           "workspace too small", "null cur_dev", "nucleus without top_k", "valid", "valid at"]


@pytest.mark.parametrize("what", INVALID)
def test_k_invalid_and_unsupported_arguments_launch_nothing(dev, what):
    from outlier_suppression_amd import _hip
    lib = _hip.load()
    a = dict(bsz=2, vocab=50, max_length=8, cur=3, n_ban=1, n_eos=1, forced=-1, pad=1, ngram=2, logits_stride=50, seq_stride=8,
             top_k=4, top_p=0.9, temperature=0.8)
    nan, inf = float("nan"), float("inf")
    change = {"top_k < 0": dict(top_k=-1), "top_k > 64": dict(top_k=65), "top_p = 0": dict(top_p=0.0), "top_p > 1": dict(top_p=1.5),
              "top_p NaN": dict(top_p=nan), "temperature = 0": dict(temperature=0.0), "temperature < 0": dict(temperature=-1.0),
              "temperature inf": dict(temperature=inf), "temperature NaN": dict(temperature=nan), "bsz = 0": dict(bsz=0),
              "cur >= max_length": dict(cur=8), "n_eos > 16": dict(n_eos=17), "forced >= vocab": dict(forced=50),
              "logits stride": dict(logits_stride=49), "nucleus without top_k": dict(top_k=0)}
    a.update(change.get(what, {}))
    at = what in ("null cur_dev", "valid at")
    logits = torch.zeros(2 * 50, dtype=torch.float32, device=dev)
    ids = torch.arange(2, 19, dtype=torch.int64, device=dev)
    word = torch.full((1,), 3, dtype=torch.int32, device=dev)
    ws_full = int(lib.osq_sample_advance_workspace_bytes(2, 50, 4))
    assert ws_full == 2 * 1 * 4 * 8 + 2 * 4 and int(lib.osq_sample_advance_workspace_bytes(2, 50, 0)) == 2 * 8 + 2 * 4
    sizes = dict(seq=(2 * 8, torch.int64), unfinished=(2, torch.uint8), next_tokens=(2, torch.int64), go_on=(1, torch.int32),
                 ws=(ws_full, torch.uint8))
    outs = {k: torch.full((n + 2 * GUARD,), 85, dtype=dt, device=dev) for k, (n, dt) in sizes.items()}
    ptr = {k: t[GUARD:].data_ptr() for k, t in outs.items()}
    ws_bytes = ws_full - (1 if what == "workspace too small" else 0)
    head = (logits.data_ptr(), a["logits_stride"], ptr["seq"], a["seq_stride"])
    tail = (ids.data_ptr(), a["n_eos"], a["pad"], ptr["unfinished"], a["bsz"], a["vocab"], a["max_length"], ptr["next_tokens"],
            ptr["go_on"], ptr["ws"], ws_bytes, 12345, a["temperature"], a["top_k"], a["top_p"], None, _hip.raw_stream(dev))
    if at:
        rc = lib.osq_sample_advance_at(*head, None if what == "null cur_dev" else word.data_ptr(), 0, a["ngram"], ids.data_ptr(),
                                       a["n_ban"], 5, -1, -1, *tail)
    else:
        rc = lib.osq_sample_advance(*head, a["cur"], a["ngram"], ids.data_ptr(), a["n_ban"], a["forced"], *tail)
    torch.cuda.synchronize()
    if what in ("valid", "valid at"):
        assert rc == 0
        seq = outs["seq"][GUARD:GUARD + 16].view(2, 8)
        assert (seq[:, 3] != 85).all() and (seq[:, :3] == 85).all() and (seq[:, 4:] == 85).all()
        for k, used in (("unfinished", 2), ("next_tokens", 2), ("go_on", 1)):
            t = outs[k]
            assert (t[:GUARD] == 85).all() and (t[GUARD + used:] == 85).all() and (t[GUARD:GUARD + used] != 85).all(), k
        for k, used in (("seq", 16), ("ws", ws_full)):
            assert (outs[k][:GUARD] == 85).all() and (outs[k][GUARD + used:] == 85).all(), k
        return
    assert rc == (-3 if what == "nucleus without top_k" else -1) and lib.osq_last_error()
    for k, t in outs.items():
        assert (t == 85).all(), k


def test_l_ops_wrapper_checks(dev):
    from outlier_suppression_amd import ops
    bufs = ops.SampleBuffers(2, 8, dev)
    logits = torch.randn(2, 50, device=dev)
    assert ops.sample_advance(logits, bufs, 1, 7, top_k=3) is bufs
    assert ops.sample_advance(logits, bufs, 1, 7, top_k=0, top_p=0.9) is None          # the library does not take it
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.sample_advance(logits.cpu(), bufs, 1, 7)
    with pytest.raises(TypeError, match="SampleBuffers"):
        ops.sample_advance(logits, ops.GreedyBuffers(2, 8, dev), 1, 7)
    with pytest.raises(ValueError, match="top_k"):
        ops.sample_advance(logits, bufs, 1, 7, top_k=65)
    with pytest.raises(ValueError, match="uniforms"):
        ops.sample_advance(logits, bufs, 1, 7, uniforms=torch.zeros(3, device=dev))
    with pytest.raises(RuntimeError, match="status -1"):
        ops.sample_advance(logits, bufs, 1, 7, temperature=0.0)
    with pytest.raises(TypeError, match="cur"):
        ops.sample_advance_at(logits, bufs, torch.zeros(1, dtype=torch.int64, device=dev), 7)


AT = dict(bsz=3, vocab=4100, max_length=12)
AT_SETTINGS = dict(eos=(4097, 9), pad=1, min_length=6, ngram=2, forced_bos=7, forced_eos=9)


def _at_case(rng, cur, top_k, top_p):
    x = SA.spread_logits(rng, AT["bsz"], AT["vocab"], [[4097, 0, 1, 4, 4095, 4096]] * AT["bsz"])
    history = np.array([[(b + i) % 2 for i in range(cur)] for b in range(AT["bsz"])], dtype=np.int64)
    return SA.make(rng, AT["bsz"], AT["vocab"], AT["max_length"], cur, 0.9, top_k, top_p, logits=x, history=history,
                   unfinished=(1, 1, 0), **AT_SETTINGS)


def _at_kernel(case, dev, word_value, cur_add, seed):
    from outlier_suppression_amd import ops
    bufs = _buffers(case, dev)
    word = torch.full((1,), word_value, dtype=torch.int32, device=dev)
    ops.sample_advance_at(_logits(case, dev), bufs, word, seed, cur_add, ngram=case["ngram"], ban_ids=_ids(case["eos"], dev),
                          ban_below=case["min_length"], forced_bos=case["forced_bos"], forced_eos=case["forced_eos"],
                          eos_ids=_ids(case["eos"], dev), pad=case["pad"], **_draw(case))
    return _outputs(bufs)


@pytest.mark.parametrize("top_k, top_p", [(0, 1.0), (4, 0.8)])
def test_m_position_from_the_device_equals_the_static_call(dev, top_k, top_p):
    rng = np.random.default_rng(11)
    tokens = []
    for cur in range(1, AT["max_length"]):
        case = _at_case(rng, cur, top_k, top_p)
        static = _kernel(case, dev, None, seed=99)
        same(_at_kernel(case, dev, cur, 0, 99), static, ("at", cur))
        same(_at_kernel(case, dev, cur + 2, -2, 99), static, ("at, cur_add", cur))
        same(_kernel(case, dev, None, seed=99), static, ("twice", cur))   # the same call twice: the same words
        tokens.append(static[0].tolist())
    assert tokens[0] == [7, 7, 1] and tokens[-1] == [9, 9, 1] and len({tuple(t) for t in tokens}) >= 3


@pytest.mark.parametrize("position", (-5, 0, 12, 2 ** 30))
def test_n_refused_position_writes_go_on_only(dev, position):
    rng = np.random.default_rng(12)
    case = _at_case(rng, 3, 4, 0.8)
    for word, add in ((position, 0), (position - 7, 7)):
        token, seq, unfinished, go_on = _at_kernel(case, dev, word, add, 5)
        assert go_on == -1
        assert (token == -7).all() and np.array_equal(seq, case["seq"]) and np.array_equal(unfinished, case["unfinished"])


@pytest.mark.parametrize("top_k", (0, 8))
def test_o_captured_and_replayed_in_place(dev, top_k):
    """The _at call captured into a graph on a side stream (after one issued warm-up there) and replayed in place at three
    positions: the words of the static calls at those positions, the draws moving with the position."""
    from outlier_suppression_amd import ops
    rng = np.random.default_rng(13)
    bsz, vocab, max_length, first, seed = 3, 4100, 9, 4, 2 ** 63 + 17
    settings = dict(eos=(4097, 9), pad=1, min_length=6, ngram=2)
    case = SA.make(rng, bsz, vocab, max_length, first, 1.2, top_k, 1.0, **settings)
    bufs = _buffers(case, dev)
    logits = _logits(case, dev).contiguous()
    word = torch.full((1,), first, dtype=torch.int32, device=dev)
    eos = _ids(settings["eos"], dev)
    call = lambda: ops.sample_advance_at(logits, bufs, word, seed, 0, 1.2, top_k, 1.0, ngram=2, ban_ids=eos, ban_below=6,  # noqa: E731
                                         eos_ids=eos, pad=1)
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
    for cur in range(first, first + 3):
        x = rng.standard_normal((bsz, vocab)).astype(np.float32)
        case = dict(case, logits=x, cur=cur)
        logits.copy_(torch.from_numpy(x).to(dev))
        word.fill_(cur)
        bufs.next_tokens.fill_(-7), bufs.go_on.fill_(77)
        graph.replay()
        got = _outputs(bufs)
        same(got, _kernel(case, dev, None, seed=seed), ("replay / static", cur))
        case = dict(case, seq=got[1], unfinished=got[2])

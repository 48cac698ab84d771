"""osq_sample_nucleus / osq_sample_nucleus_at (csrc/sample_nucleus.hip) through ops.sample_nucleus(_at) and the C ABI: one
sampling step from a nucleus over the whole vocabulary (top_k == 0, top_p < 1) against the float64 restatement of
tests/_sample_advance.py (``survivors`` ranks every token for this form), with the cases of tests/_sample_nucleus.py aimed at
the kernel's layout: 1024 threads of 50 consecutive tokens, 64 threads to a wave, at most 51200 tokens.

next_tokens, the whole of seq, unfinished and go_on are compared as words; every output is pre-filled with a sentinel.  A
planted uniform lies at the midpoint of a kept rank's float64 interval and top_p midway between two ranks' thresholds, each at
least 1e-3 W (2e-4 W in the dense case) from a boundary, so the token is exact: one rank too many or too few kept moves every
target by a whole interval.  The Philox draws are held to the band of the fp32 sums (EPS = 2e-5 W, tests/_sample_advance.py);
the largest excursion seen is printed and, when the file runs with -s, written to profiles/sample_nucleus_accuracy.txt.

Rows: 1 to 3, but one row per planted draw (up to 8) where a case plants several draws on the same logits."""
import os

import numpy as np
import pytest
import torch

import _greedy_advance as GA
import _sample_advance as SA
import _sample_nucleus as NU
from test_greedy_advance_cpu import same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOCABS = (1, 2, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, NU.PER - 1, NU.PER, NU.PER + 1, 50265, NU.MAX_VOCAB)
SEEDS = (0, 0x9e3779b97f4a7c15, 2 ** 64 - 1)
LAST_U = NU.LAST_U
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
    bufs = ops.SampleBuffers(bsz, max_length, dev, nucleus=True)
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


def _kernel(case, dev, u=None, seed=0, logits_pad=0, seq_pad=0):
    from outlier_suppression_amd import ops
    bufs = _buffers(case, dev, seq_pad)
    kw = GA.kernel_arguments(case)
    planted = None if u is None else torch.from_numpy(np.asarray(u, dtype=np.float32)).to(dev)
    assert ops.sample_nucleus(_logits(case, dev, logits_pad), bufs, case["cur"], seed, case["temperature"], case["top_p"],
                              ngram=kw["ngram"], ban_ids=_ids(kw["ban_ids"], dev), forced=kw["forced"],
                              eos_ids=_ids(kw["eos_ids"], dev), pad=kw["pad"], uniforms=planted) is bufs
    assert bufs.workspace.numel() >= 4 * case["seq"].shape[0]
    return _outputs(bufs)


def check(case, dev, u, label, **pads):
    """The kernel with the planted draws ``u`` against the restatement, all four outputs.  Returns the tokens."""
    assert case["top_k"] == 0 and case["top_p"] < 1.0                    # the form ``survivors`` ranks
    got = _kernel(case, dev, u, **pads)
    same(got, SA.reference_case(case, u), label)
    return got[0]


def _seams(vocab):
    return sorted({t for _, t in NU.places(vocab)} | {vocab // 3})


@pytest.mark.parametrize("vocab", VOCABS)
def test_a_every_kept_rank_at_its_midpoint_at_every_launch_shape(dev, vocab):
    """Up to eight heavy tokens on the seams of the layout, the cut keeping all but the last two of them (top_p between two
    thresholds), one row per kept rank; again with padded row strides -- with an odd vocab the second row is 4-byte aligned
    only -- and seq rows wider than max_length."""
    rng = np.random.default_rng(vocab)
    heavy = np.array(_seams(vocab)[:8], dtype=np.int64)
    if heavy.size < min(8, vocab):
        rest = np.setdiff1d(np.arange(vocab), heavy)
        heavy = np.concatenate([heavy, rng.choice(rest, min(8, vocab) - heavy.size, replace=False)])
    x = SA.spread_logits(rng, 1, vocab, [heavy])
    case = SA.make(rng, 1, vocab, 6, 3, 0.9, 0, 0.5, logits=x, eos=(0,), pad=0)
    everyone = SA.survivors(x[0], set(), 0.9, 0, 1.0 - 1e-12)
    kept = max(1, heavy.size - 2)
    if vocab > kept:
        case["top_p"] = NU.between(everyone.above, kept)
    SA.assert_top_p_margin(case)
    sv = SA.row(case, 0)
    assert sv.tokens.size == kept
    u = np.array([NU.midpoint(sv, i) for i in range(kept)] + [LAST_U], dtype=np.float32)
    many = NU.repeat_rows(case, len(u))
    want = sv.tokens.tolist() + [int(sv.tokens[-1])]
    assert check(many, dev, u, (vocab, "dense rows")).tolist() == want
    assert check(many, dev, u, (vocab, "padded rows"), logits_pad=3 if vocab % 2 else 2, seq_pad=5).tolist() == want


def test_b_a_vocabulary_above_the_limit_is_refused_with_nothing_written(dev):
    from outlier_suppression_amd import _hip, ops
    lib = _hip.load()
    vocab = NU.MAX_VOCAB + 1
    assert int(lib.osq_sample_nucleus_workspace_bytes(2, vocab)) == 0
    logits = torch.zeros(2, vocab, device=dev)
    outs = {k: torch.full((n,), 85, dtype=dt, device=dev) for k, (n, dt) in
            dict(seq=(16, torch.int64), unfinished=(2, torch.uint8), next_tokens=(2, torch.int64), go_on=(1, torch.int32),
                 ws=(64, torch.uint8)).items()}
    eos = torch.tensor([3], dtype=torch.int64, device=dev)
    rc = lib.osq_sample_nucleus(logits.data_ptr(), vocab, outs["seq"].data_ptr(), 8, 3, 2, None, 0, -1, eos.data_ptr(), 1, 1,
                                outs["unfinished"].data_ptr(), 2, vocab, 8, outs["next_tokens"].data_ptr(),
                                outs["go_on"].data_ptr(), outs["ws"].data_ptr(), 64, 5, 1.0, 0.9, None, _hip.raw_stream(dev))
    torch.cuda.synchronize()
    assert rc == -3 and b"51200" in lib.osq_last_error()
    for k, t in outs.items():
        assert (t == 85).all(), k
    assert ops.sample_nucleus(logits, ops.SampleBuffers(2, 8, dev), 3, 5, top_p=0.9) is None
    assert ops.sample_nucleus_at(logits, ops.SampleBuffers(2, 8, dev), torch.full((1,), 3, dtype=torch.int32, device=dev), 5,
                                 top_p=0.9) is None


@pytest.mark.parametrize("vocab", (50265, NU.MAX_VOCAB))
def test_c_the_cut_at_every_seam_of_the_layout(dev, vocab):
    rng = np.random.default_rng(vocab + 1)
    for label, place in NU.places(vocab):
        case, u, want = NU.cut_case(rng, vocab, place)
        assert check(case, dev, u, (vocab, label)).tolist() == want, label


def test_d_a_dense_nucleus(dev):
    case, u, want = NU.dense_case(np.random.default_rng(22))
    assert check(case, dev, u, "dense").tolist() == want


@pytest.mark.parametrize("vocab, top_p", [(4097, 0.25), (4097, 0.5), (50265, 0.999)])
def test_e_every_logit_equal(dev, vocab, top_p):
    case, u, want = NU.flat_case(np.random.default_rng(vocab), vocab, top_p)
    assert check(case, dev, u, ("flat", vocab, top_p)).tolist() == want


def test_f_tie_groups_and_signed_zeros(dev):
    rng = np.random.default_rng(31)
    case, u, want = NU.tie_group_case(rng)
    assert check(case, dev, u, "a group of 5 across a wave boundary").tolist() == want
    vocab = 2 * NU.WAVE * NU.PER + 1
    x = SA.spread_logits(rng, 1, vocab, [[7]], lo=1.0, hi=1.0)
    x[0, 9], x[0, 5000] = -0.0, 0.0                                       # signed zeros are one value: the smaller token first
    zeros = SA.make(rng, 1, vocab, 6, 3, 1.0, 0, 0.95, logits=x)
    SA.assert_top_p_margin(zeros)
    sv = SA.row(zeros, 0)
    assert sv.tokens.tolist() == [7, 9, 5000]
    u = np.array([NU.midpoint(sv, i) for i in range(3)] + [LAST_U], dtype=np.float32)
    assert check(NU.repeat_rows(zeros, 4), dev, u, "zeros").tolist() == [7, 9, 5000, 5000]
    x[0, 9], x[0, 5000] = 0.0, -0.0
    assert check(NU.repeat_rows(dict(zeros, logits=x), 4), dev, u, "zeros, swapped").tolist() == [7, 9, 5000, 5000]


def test_g_degenerate_rows(dev):
    rng = np.random.default_rng(32)
    vocab = 4099
    x = SA.spread_logits(rng, 3, vocab, [[5, 4096, 4098]] * 3)
    tiny = SA.make(rng, 3, vocab, 8, 3, 1.0, 0, 1e-6, logits=x)           # rank 0 always stays, alone here
    first = [int(SA.row(tiny, b).tokens[0]) for b in range(3)]
    assert all(SA.row(tiny, b).tokens.size == 1 for b in range(3))
    assert check(tiny, dev, np.array([0.0, 0.5, LAST_U], dtype=np.float32), "rank 0 alone").tolist() == first
    x = np.full((3, vocab), -np.inf, dtype=np.float32)
    x[0, 4098], x[1, :] = 0.25, np.nan                                    # one survivor; no survivor: NaN, -inf
    x[2, [11, 4096]] = np.inf                                             # +inf weighs 1 each
    case = SA.make(rng, 3, vocab, 8, 3, 1.0, 0, 0.9, logits=x)
    assert check(case, dev, np.array([0.7, 0.7, 0.25], dtype=np.float32), "one, none, +inf").tolist() == [4098, 0, 11]
    assert check(case, dev, np.array([LAST_U, 0.0, 0.75], dtype=np.float32), "one, none, +inf, high").tolist() == [4098, 0, 4096]
    history = np.tile(np.array([0, 1, 2, 1], dtype=np.int64), (2, 1))
    banned = SA.make(rng, 2, 3, 9, 4, 1.0, 0, 0.9, history=history, ngram=1)
    assert check(banned, dev, np.array([0.2, 0.9], dtype=np.float32), "every token banned").tolist() == [0, 0]


def test_h_bans_take_the_would_be_rank_0(dev):
    rng = np.random.default_rng(33)
    vocab, ids = 6500, (0, NU.PER - 1, NU.PER, NU.WAVE * NU.PER, 6499)
    u = np.array([0.01, 0.99], dtype=np.float32)
    for t in ids:                                                         # the min-length ids
        x = SA.spread_logits(rng, 2, vocab, [[t, 2000, 77]] * 2)
        x[:, t] = 9.0
        case = SA.make(rng, 2, vocab, 8, 3, 1.0, 0, 0.9, logits=x, eos=ids, pad=1, min_length=4)
        assert set(check(case, dev, u, ("banned", t)).tolist()) <= {2000, 77}
        free = check(dict(case, min_length=3), dev, np.array([0.3, 0.6], dtype=np.float32), ("free", t))
        assert free.tolist() == [t, t]
    x = SA.spread_logits(rng, 2, vocab, [[3200, 2000, 77]] * 2)
    x[:, 3200] = np.nan                                                   # a NaN at rank 0's place
    assert set(check(SA.make(rng, 2, vocab, 8, 3, 1.0, 0, 0.9, logits=x), dev, u, "NaN").tolist()) <= {2000, 77}
    cur, n, W = 300, 3, 6490                                              # the no-repeat-ngram rule
    for p in (0, 255, 256, "last"):
        history = np.tile(rng.permutation(np.arange(10, 6000))[:cur], (2, 1)).astype(np.int64)
        if p == "last":
            history[:, cur - n:] = W
        else:
            history[:, p:p + n - 1] = history[:, cur - n + 1:]
            history[:, p + n - 1] = W
        history[1] = np.arange(10, 10 + cur)                              # the second row repeats nothing
        x = SA.spread_logits(rng, 2, vocab, [[W, 3]] * 2)
        x[:, W], x[:, 3] = 9.0, 1.0
        case = SA.make(rng, 2, vocab, cur + 2, cur, 1.0, 0, 0.9, logits=x, history=history, ngram=n)
        assert check(case, dev, np.array([0.5, 0.5], dtype=np.float32), ("window", p)).tolist() == [3, W]


def test_i_uniforms_are_the_hosts(dev):
    from outlier_suppression_amd import ops
    from outlier_suppression_amd.model import sampling
    for seed in SEEDS:
        got = ops.sample_uniforms(seed, 66, 31, dev).cpu()
        assert torch.equal(got.view(torch.int32), sampling.uniforms(seed, 66, 31).view(torch.int32)), seed


@pytest.mark.parametrize("vocab", VOCABS)
def test_j_philox_draws_within_the_band(dev, vocab):
    """uniforms=None: the kernel's own draws.  Its token at kept rank i passes iff C_{i-1} - eps W <= u W <= C_i + eps W."""
    from outlier_suppression_amd.model import sampling
    rng = np.random.default_rng(vocab * 7)
    bsz, cur = 3, 5
    case = SA.make(rng, bsz, vocab, 9, cur, 0.8, 0, 0.9, ngram=2, eos=(min(2, vocab - 1),), pad=0, min_length=7)
    rows = [SA.row(case, b) for b in range(bsz)]
    worst = 0.0
    for seed in SEEDS:
        got = _kernel(case, dev, None, seed=seed + vocab)
        u = sampling.uniforms(seed + vocab, bsz, cur).numpy()
        worst = max([worst] + [SA.excursion(rows[b], int(got[0][b]), u[b]) for b in range(bsz)])
        same(got, _kernel(case, dev, u, seed=1), ("Philox / planted", vocab, seed))      # the same draws planted: the same words
    print(f"vocab {vocab} top_p 0.9: largest excursion {worst:.3e} W")
    _seen[f"v{vocab} p0.9"] = worst
    assert worst <= SA.EPS, worst


def test_k_accuracy_record(request):
    if not _seen:                                                         # run without test_j: nothing to record
        return
    print(f"largest excursion over all shapes: {max(_seen.values()):.3e} W (bound {SA.EPS:g})")
    if request.config.getoption("capture") == "no":                       # run with -s: the record is rewritten
        with open(os.path.join(ROOT, "profiles", "sample_nucleus_accuracy.txt"), "w") as f:
            f.write("osq_sample_nucleus with its own Philox draws against the float64 restatement (tests/_sample_advance.py): how far\n"
                    f"u * W lies outside the float64 interval of the kernel's token, in units of W (0: inside); bound {SA.EPS:g},\n"
                    "3 rows x 3 seeds per shape, top_p 0.9, temperature 0.8, n-gram 2 and a min-length ban on\n\n")
            for label, worst in _seen.items():
                f.write(f"{label:40s} {worst:.3e}\n")
            f.write(f"\nlargest: {max(_seen.values()):.3e}\n")


def test_l_finishing_stopping_and_forced_steps(dev):
    rng = np.random.default_rng(34)
    bsz, eos = 3, tuple(range(20, 36))                                    # sixteen eos ids
    for winner, alive, go_on in ((35, (2,), 0), (19, (2,), 1), (20, (), 0), (19, (0,), 1), (19, range(bsz), 1)):
        x = SA.spread_logits(rng, bsz, 70, [[winner]] * bsz)
        unfinished = np.zeros(bsz, dtype=np.uint8)
        unfinished[list(alive)] = 1
        case = SA.make(rng, bsz, 70, 9, 4, 1.0, 0, 0.9, logits=x, unfinished=unfinished, eos=eos, pad=1)
        u = rng.uniform(0.001, 0.999, bsz).astype(np.float32)             # one survivor weighs everything
        got = _kernel(case, dev, u)
        same(got, SA.reference_case(case, u), (winner, tuple(alive)))
        assert (got[0][unfinished != 0] == winner).all() and (got[0][unfinished == 0] == 1).all() and got[3] == go_on
    nan_rows = np.full((bsz, 70), np.nan, dtype=np.float32)               # a forced step reads no logit
    forced = SA.make(rng, bsz, 70, 9, 8, 1.0, 0, 0.9, logits=nan_rows, forced_eos=21, eos=eos, pad=1)
    assert check(forced, dev, np.zeros(bsz, dtype=np.float32), "forced eos").tolist() == [21] * bsz
    forced = SA.make(rng, bsz, 70, 9, 1, 1.0, 0, 0.9, logits=nan_rows, forced_bos=7, forced_eos=21, eos=eos, pad=1)
    assert check(forced, dev, np.zeros(bsz, dtype=np.float32), "forced bos").tolist() == [7] * bsz
    last = SA.make(rng, bsz, 70, 9, 8, 1.0, 0, 0.9)                       # the last position stops the search
    assert _kernel(last, dev, np.full(bsz, 0.5, dtype=np.float32))[3] == 0


def test_m_top_p_one_is_the_draw_in_rank_order(dev):
    rng = np.random.default_rng(35)
    vocab = 4097
    x = SA.spread_logits(rng, 1, vocab, [[4096, 3, 3200]])
    case = SA.make(rng, 1, vocab, 6, 3, 1.0, 0, 1.0, logits=x)
    ranked = SA.survivors(x[0], set(), 1.0, vocab, 1.0)                   # every token, in rank order, nothing cut
    assert ranked.tokens.size == vocab and ranked.tokens[:3].tolist() != sorted(ranked.tokens[:3].tolist())
    u = np.array([NU.midpoint(ranked, i) for i in range(3)], dtype=np.float32)
    got = _kernel(NU.repeat_rows(case, 3), dev, u)[0].tolist()
    assert got == ranked.tokens[:3].tolist() == [NU.search(x[0], set(), 1.0, 1.0, v)[0] for v in u]


GUARD = 64
INVALID = ["top_p = 0", "top_p > 1", "top_p NaN", "temperature = 0", "temperature < 0", "temperature inf", "temperature NaN",
           "bsz = 0", "cur >= max_length", "n_eos > 16", "forced >= vocab", "logits stride", "workspace too small", "null cur_dev",
           "valid", "valid at"]


@pytest.mark.parametrize("what", INVALID)
def test_n_invalid_arguments_launch_nothing_and_guard_bands_stay(dev, what):
    from outlier_suppression_amd import _hip
    lib = _hip.load()
    a = dict(bsz=2, vocab=51, max_length=8, cur=3, n_ban=1, n_eos=1, forced=-1, pad=1, ngram=2, logits_stride=51, seq_stride=8,
             top_p=0.9, temperature=0.8)
    nan, inf = float("nan"), float("inf")
    change = {"top_p = 0": dict(top_p=0.0), "top_p > 1": dict(top_p=1.5), "top_p NaN": dict(top_p=nan),
              "temperature = 0": dict(temperature=0.0), "temperature < 0": dict(temperature=-1.0),
              "temperature inf": dict(temperature=inf), "temperature NaN": dict(temperature=nan), "bsz = 0": dict(bsz=0),
              "cur >= max_length": dict(cur=8), "n_eos > 16": dict(n_eos=17), "forced >= vocab": dict(forced=51),
              "logits stride": dict(logits_stride=50)}
    a.update(change.get(what, {}))
    at = what in ("null cur_dev", "valid at")
    logits = torch.randn(2 * 51, dtype=torch.float32, device=dev)
    ids = torch.arange(2, 19, dtype=torch.int64, device=dev)
    word = torch.full((1,), 3, dtype=torch.int32, device=dev)
    ws_full = int(lib.osq_sample_nucleus_workspace_bytes(2, 51))
    assert ws_full == 2 * 4
    sizes = dict(seq=(2 * 8, torch.int64), unfinished=(2, torch.uint8), next_tokens=(2, torch.int64), go_on=(1, torch.int32),
                 ws=(ws_full, torch.uint8))
    outs = {k: torch.full((n + 2 * GUARD,), 85, dtype=dt, device=dev) for k, (n, dt) in sizes.items()}
    ptr = {k: t[GUARD:].data_ptr() for k, t in outs.items()}
    ws_bytes = ws_full - (1 if what == "workspace too small" else 0)
    head = (logits.data_ptr(), a["logits_stride"], ptr["seq"], a["seq_stride"])
    tail = (ids.data_ptr(), a["n_eos"], a["pad"], ptr["unfinished"], a["bsz"], a["vocab"], a["max_length"], ptr["next_tokens"],
            ptr["go_on"], ptr["ws"], ws_bytes, 12345, a["temperature"], a["top_p"], None, _hip.raw_stream(dev))
    if at:
        rc = lib.osq_sample_nucleus_at(*head, None if what == "null cur_dev" else word.data_ptr(), 0, a["ngram"], ids.data_ptr(),
                                       a["n_ban"], 5, -1, -1, *tail)
    else:
        rc = lib.osq_sample_nucleus(*head, a["cur"], a["ngram"], ids.data_ptr(), a["n_ban"], a["forced"], *tail)
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
    assert rc == -1 and lib.osq_last_error()
    for k, t in outs.items():
        assert (t == 85).all(), k


def test_o_ops_wrapper_checks(dev):
    from outlier_suppression_amd import ops
    bufs = ops.SampleBuffers(2, 8, dev)
    logits = torch.randn(2, 50, device=dev)
    assert ops.sample_nucleus(logits, bufs, 1, 7, top_p=0.9) is bufs and bufs.nucleus
    assert ops.sample_advance(logits, bufs, 1, 7, top_k=0, top_p=0.9) is None          # that entry point keeps refusing the form
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.sample_nucleus(logits.cpu(), bufs, 1, 7)
    with pytest.raises(TypeError, match="SampleBuffers"):
        ops.sample_nucleus(logits, ops.GreedyBuffers(2, 8, dev), 1, 7)
    with pytest.raises(ValueError, match="uniforms"):
        ops.sample_nucleus(logits, bufs, 1, 7, uniforms=torch.zeros(3, device=dev))
    with pytest.raises(RuntimeError, match="status -1"):
        ops.sample_nucleus(logits, bufs, 1, 7, temperature=0.0)
    with pytest.raises(TypeError, match="cur"):
        ops.sample_nucleus_at(logits, bufs, torch.zeros(1, dtype=torch.int64, device=dev), 7)


AT = dict(bsz=3, vocab=4100, max_length=8)
AT_SETTINGS = dict(eos=(4097, 9), pad=1, min_length=5, ngram=2, forced_bos=7, forced_eos=9)


def _at_case(rng, cur):
    x = SA.spread_logits(rng, AT["bsz"], AT["vocab"], [[4097, 0, 1, 4, 4095, 4096]] * AT["bsz"])
    history = np.array([[(b + i) % 2 for i in range(cur)] for b in range(AT["bsz"])], dtype=np.int64)
    return SA.make(rng, AT["bsz"], AT["vocab"], AT["max_length"], cur, 0.9, 0, 0.8, logits=x, history=history,
                   unfinished=(1, 1, 0), **AT_SETTINGS)


def _at_kernel(case, dev, word_value, cur_add, seed):
    from outlier_suppression_amd import ops
    bufs = _buffers(case, dev)
    word = torch.full((1,), word_value, dtype=torch.int32, device=dev)
    ops.sample_nucleus_at(_logits(case, dev), bufs, word, seed, cur_add, case["temperature"], case["top_p"], ngram=case["ngram"],
                          ban_ids=_ids(case["eos"], dev), ban_below=case["min_length"], forced_bos=case["forced_bos"],
                          forced_eos=case["forced_eos"], eos_ids=_ids(case["eos"], dev), pad=case["pad"])
    return _outputs(bufs)


def test_p_position_from_the_device_equals_the_static_call(dev):
    rng = np.random.default_rng(11)
    tokens = []
    for cur in range(1, AT["max_length"]):
        case = _at_case(rng, cur)
        static = _kernel(case, dev, None, seed=99)
        same(_at_kernel(case, dev, cur, 0, 99), static, ("at", cur))
        same(_at_kernel(case, dev, cur + 2, -2, 99), static, ("at, cur_add", cur))
        same(_kernel(case, dev, None, seed=99), static, ("twice", cur))   # the same call twice: the same words
        tokens.append(static[0].tolist())
    assert tokens[0] == [7, 7, 1] and tokens[-1] == [9, 9, 1] and len({tuple(t) for t in tokens}) >= 3


@pytest.mark.parametrize("position", (-5, 0, 8, 2 ** 30))
def test_q_refused_position_writes_go_on_only(dev, position):
    rng = np.random.default_rng(12)
    case = _at_case(rng, 3)
    for word, add in ((position, 0), (position - 7, 7)):
        token, seq, unfinished, go_on = _at_kernel(case, dev, word, add, 5)
        assert go_on == -1
        assert (token == -7).all() and np.array_equal(seq, case["seq"]) and np.array_equal(unfinished, case["unfinished"])


def test_r_captured_and_replayed_in_place(dev):
    """The _at call captured into a graph on a side stream (after one issued warm-up there) and replayed in place at three
    positions: the words of the static calls at those positions, the draws moving with the position."""
    from outlier_suppression_amd import ops
    rng = np.random.default_rng(13)
    bsz, vocab, max_length, first, seed = 3, 4100, 9, 4, 2 ** 63 + 17
    settings = dict(eos=(4097, 9), pad=1, min_length=6, ngram=2)
    case = SA.make(rng, bsz, vocab, max_length, first, 1.2, 0, 0.9, **settings)
    bufs = _buffers(case, dev)
    logits = _logits(case, dev).contiguous()
    word = torch.full((1,), first, dtype=torch.int32, device=dev)
    eos = _ids(settings["eos"], dev)
    call = lambda: ops.sample_nucleus_at(logits, bufs, word, seed, 0, 1.2, 0.9, ngram=2, ban_ids=eos, ban_below=6,  # noqa: E731
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


def test_s_a_rows_token_does_not_depend_on_the_batch(dev):
    """Planted uniforms: the same row gives the same token alone, as any row of three, with any row stride."""
    rng = np.random.default_rng(14)
    vocab = 50265
    one = SA.make(rng, 1, vocab, 6, 3, 0.8, 0, 0.9)
    u = np.float32(0.37)
    alone = _kernel(one, dev, np.array([u]))[0].tolist()
    other = rng.standard_normal((1, vocab)).astype(np.float32)
    for at in range(3):
        x = np.repeat(other, 3, axis=0)
        x[at] = one["logits"][0]
        three = dict(NU.repeat_rows(one, 3), logits=x)
        got = _kernel(three, dev, np.full(3, u, dtype=np.float32), logits_pad=at)
        assert got[0][at] == alone[0] and (got[0][[b for b in range(3) if b != at]] == got[0][(at + 1) % 3]).all(), at
    assert SA.excursion(SA.row(one, 0), alone[0], u) <= SA.EPS

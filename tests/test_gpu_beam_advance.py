"""osq_beam_advance (csrc/beam_advance.hip) through ops.beam_advance and the C ABI: one beam-search step's bookkeeping against
the numpy restatement of tests/_beam_advance.py (pinned to the torch lines by tests/test_beam_advance_cpu.py).

Kernel and restatement share the strict order of ties, so EVERY output word is compared, undone slots included: over the launch
shapes (bsz, nb / keep, the copy loop's lane boundaries in max_length, the first, last-but-one and last step), with planted
ties, -inf, NaN, -0.0, eos among and beyond the first nb candidates, every beam done and a row that is no longer improvable,
and over a 12-step walk through the two alternating buffer sets.  Against generation._advance_beams_torch on the same GPU the
comparison is the CPU test's (tie-free inputs, finished / finished_len where done): it runs under the division flag
generate() passes, and so settles it.  Then the call inside a captured graph, and the invalid arguments between guard bands."""
import itertools

import numpy as np
import pytest
import torch

import _beam_advance as BA
from test_beam_advance_cpu import EOS, KINDS, compare_with_torch, tie_free, torch_step

pytestmark = pytest.mark.gpu

VOCAB = 50
MODES = (False, True, "never")
PENALTIES = (0, 0.8, 1, 2)
EOS_SETS = {0: (), 1: (2,), 2: (2, 7), 16: tuple(range(2, 18))}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _buffers(state, dev, fill=False):
    """ops.BeamBuffers of the state's geometry: holding it, or (``fill``) holding -7 / NaN / True everywhere."""
    from outlier_suppression_amd import ops
    bsz, nb, L = state["running"].shape
    buf = ops.BeamBuffers(bsz, nb, L, dev)
    for name in BA.STATE:
        t = getattr(buf, name)
        if fill:
            t.fill_(float("nan") if t.dtype == torch.float32 else (True if t.dtype == torch.bool else -7))
        else:
            t.copy_(torch.from_numpy(state[name]).view(t.shape))
    if fill:
        buf.beam_idx.fill_(-7), buf.next_tokens.fill_(-7), buf.go_on.fill_(-7)
    return buf


def _numpy(buf):
    out = {name: getattr(buf, name).cpu().numpy() for name in BA.OUTPUTS}
    out["improvable"] = out["improvable"].reshape(-1)
    return out


def _kernel(dev, top_lp, top_idx, state, cur, vocab, eos, early_stopping, length_penalty, reciprocal, now=None, out=None):
    from outlier_suppression_amd import ops
    L = state["running"].shape[2]
    now = _buffers(state, dev) if now is None else now
    out = _buffers(state, dev, fill=True) if out is None else out
    eos_t = torch.tensor(list(eos), dtype=torch.int64, device=dev) if len(eos) else None
    len_div, best_div = BA.divisors(cur, L, early_stopping, length_penalty)
    ops.beam_advance(torch.from_numpy(top_lp).to(dev), torch.from_numpy(top_idx).to(dev), now, out, cur, vocab, eos_t,
                     early_stopping, len_div, best_div, reciprocal)
    return out


def _same_words(got, want, label):
    for name in BA.OUTPUTS:
        g, w = np.ascontiguousarray(got[name]), np.ascontiguousarray(want[name])
        assert g.shape == w.shape and g.dtype == w.dtype, (label, name, g.dtype, w.dtype)
        if g.dtype == np.float32:
            both_nan = np.isnan(g) & np.isnan(w)
            same = (g.view(np.uint32) == w.view(np.uint32)) | both_nan
        else:
            same = g == w
        assert same.all(), (label, name, np.argwhere(~same)[:4].tolist(), g[~same][:4], w[~same][:4])


def _against_reference(dev, top_lp, top_idx, state, cur, eos, early_stopping, length_penalty, reciprocal, label, vocab=VOCAB):
    got = _numpy(_kernel(dev, top_lp, top_idx, state, cur, vocab, eos, early_stopping, length_penalty, reciprocal))
    want = BA.reference(top_lp, top_idx, state, cur, vocab, eos, early_stopping, length_penalty, reciprocal)
    _same_words(got, want, label)
    return want


@pytest.mark.parametrize("max_length", [2, 3, 63, 64, 65, 129, 4096])
@pytest.mark.parametrize("nb, keep", [(1, 2), (2, 4), (6, 12), (6, 18), (21, 63), (32, 64)])
def test_a_launch_shapes(dev, nb, keep, max_length):
    """Every nb / keep at every lane boundary of the copy loop, at the first, the last-but-one and the last step; the batch
    sizes, eos counts, early-stopping modes, length penalties, state kinds and the two divisions rotate through the cases."""
    L = max_length
    rng = np.random.default_rng(100 * L + keep)
    turn = itertools.count(L + keep)
    for cur in sorted({1, max(1, L - 2), L - 1}):
        i = next(turn)
        bsz = (1, 3, 70)[i % 3] if L <= 129 and nb * L <= 2048 else (1, 3)[i % 2]
        eos = EOS_SETS[(0, 1, 2, 16)[i % 4]]
        state = BA.random_state(rng, bsz, nb, L, cur, VOCAB, KINDS[(i // 2) % 4], eos)
        top_lp, top_idx = BA.random_selection(rng, bsz, nb, keep, VOCAB, eos, wide=bool(i % 2))
        _against_reference(dev, top_lp, top_idx, state, cur, eos, MODES[i % 3], PENALTIES[(i // 3) % 4], bool((i // 4) % 2),
                           (bsz, nb, keep, L, cur))


@pytest.mark.parametrize("early_stopping", MODES)
@pytest.mark.parametrize("length_penalty", PENALTIES)
def test_b_every_mode_and_penalty(dev, early_stopping, length_penalty):
    """All three early-stopping modes with all four penalties, every state kind, both divisions, 0 to 16 eos ids, 70 rows."""
    rng = np.random.default_rng(11)
    nb, keep, L = 6, 12, 20
    for kind, n_eos, reciprocal in itertools.product(KINDS, (0, 1, 2, 16), (False, True)):
        cur = (3, 18, 19)[(n_eos + reciprocal) % 3]
        eos = EOS_SETS[n_eos]
        state = BA.random_state(rng, 70, nb, L, cur, VOCAB, kind, eos)
        top_lp, top_idx = BA.random_selection(rng, 70, nb, keep, VOCAB, eos)
        want = _against_reference(dev, top_lp, top_idx, state, cur, eos, early_stopping, length_penalty, reciprocal,
                                  (kind, n_eos, reciprocal))
        if kind == "stale":
            assert not want["improvable"][1]


def test_c_planted_values(dev):
    """Ties (pairs and a whole row), -inf, NaN, -0.0 / +0.0, eos among the first nb candidates and only beyond them, every
    beam done, a row that is no longer improvable: the strict order decides, kernel and restatement agree on every word."""
    nb, keep, L, cur, eos = 6, 12, 16, 5, (2, 7)
    rng = np.random.default_rng(5)
    inf, nan = np.float32("inf"), np.float32("nan")
    for kind, early_stopping, length_penalty, reciprocal in itertools.product(KINDS, MODES, (0.8, 2), (False, True)):
        state = BA.random_state(rng, 8, nb, L, cur, VOCAB, kind, eos)
        top_lp, top_idx = BA.random_selection(rng, 8, nb, keep, VOCAB, eos, hits=False)
        top_lp = -np.sort(-top_lp, axis=1)                          # descending, as a selection hands them over
        top_lp[0, 3], top_lp[0, 9] = top_lp[0, 2], top_lp[0, 8]    # equal pairs, inside and beyond the first nb
        top_lp[1, :] = np.float32(-1.5)                             # an all-equal row
        top_lp[2, 4:] = -inf                                        # banned tokens: -inf, fewer finite candidates than nb
        top_lp[3, 1], top_lp[3, 7] = nan, nan                       # NaN goes first
        top_lp[4, :3] = np.float32(0.0), np.float32(-0.0), np.float32(0.0)
        beam, token = top_idx // VOCAB, top_idx % VOCAB
        token[5, 1], token[5, 4] = 2, 7                             # eos among the first nb candidates
        token[6, nb + 1], token[6, keep - 1] = 7, 2                 # eos only beyond them
        token[1, 0], token[3, 1], token[4, 1] = 2, 7, 2             # ... and on a tie, a NaN and a zero
        top_idx = beam * VOCAB + token
        if kind == "all":
            state["scores"][7] = np.float32(-0.001) * np.arange(1, nb + 1, dtype=np.float32)   # row 7: nothing gets in
        want = _against_reference(dev, top_lp, top_idx, state, cur, eos, early_stopping, length_penalty, reciprocal,
                                  (kind, early_stopping, length_penalty, reciprocal))
        # the all-equal row keeps candidates 1 .. nb (candidate 0 is a hit); the NaNs lead row 3, hit or not
        assert want["beam_idx"][nb:2 * nb].tolist() == (beam[1, 1:nb + 1] + nb).tolist()
        assert np.isnan(want["running_scores"][3, :2]).all() and want["next_tokens"][3 * nb] == 7


def test_d_twelve_step_walk(dev):
    """Random selections chained through the kernel (two alternating buffer sets) and through the restatement (its own
    chain): every word of every step, beams finishing along the way."""
    bsz, nb, keep, L, eos = 3, 6, 12, 14, (2,)
    rng = np.random.default_rng(21)
    state = BA.random_state(rng, bsz, nb, L, 1, VOCAB, "nothing", eos)
    now, spare = _buffers(state, dev), _buffers(state, dev, fill=True)
    finished_rows = 0
    for step in range(12):
        cur = step + 1
        top_lp, top_idx = BA.random_selection(rng, bsz, nb, keep, VOCAB, eos, hits=step % 3 == 1)
        if step % 4 == 3:
            top_lp[:, 1] = top_lp[:, 0]                              # a tie on the way
        _kernel(dev, top_lp, top_idx, state, cur, VOCAB, eos, False, 0.8, True, now, spare)
        now, spare = spare, now
        state = BA.reference(top_lp, top_idx, state, cur, VOCAB, eos, False, 0.8, True)
        _same_words(_numpy(now), state, ("walk", step))
        finished_rows += int(state["done"].sum())
    assert finished_rows >= 1


def test_e_same_words_as_the_torch_lines_on_this_gpu(dev):
    """generation._advance_beams_torch run on the GPU against the kernel under the division flag generate() passes
    (generation._ADVANCE_RECIPROCAL), on the CPU test's tie-free cases.  The other form of the division must differ somewhere
    on these cases, else they would settle nothing."""
    from outlier_suppression_amd.model import generation as G
    flag = G._ADVANCE_RECIPROCAL
    bsz, L = 3, 8
    differs = 0
    for i, (nb, n_eos, length_penalty) in enumerate(itertools.product((1, 2, 6), (0, 1, 2), PENALTIES)):
        eos, early_stopping = EOS[n_eos], MODES[i % 3]
        keep = max(2, 1 + n_eos) * nb
        rng = np.random.default_rng(1000 * nb + 100 * n_eos + 9)
        compared = 0
        for kind, last in itertools.product(KINDS, (False, True)):
            cur = L - 1 if last else 3
            state = BA.random_state(rng, bsz, nb, L, cur, VOCAB, kind, eos)
            top_lp, top_idx = BA.random_selection(rng, bsz, nb, keep, VOCAB, eos, wide=last)
            tie_free(state, top_lp, top_idx, cur, VOCAB, eos, early_stopping, length_penalty, nb, flag)
            got = _numpy(_kernel(dev, top_lp, top_idx, state, cur, VOCAB, eos, early_stopping, length_penalty, flag))
            want = torch_step(state, top_lp, top_idx, cur, VOCAB, eos, early_stopping, length_penalty, device=dev)
            compared += compare_with_torch(got, want, (nb, n_eos, length_penalty, kind, last))
            other = BA.reference(top_lp, top_idx, state, cur, VOCAB, eos, early_stopping, length_penalty, not flag)
            differs += int((other["scores"].view(np.uint32) != got["scores"].view(np.uint32)).any())
        assert compared >= 1
    print(f"reciprocal={flag}: word-equal to the torch lines on this GPU; the other division differs on {differs} cases")
    assert differs >= 1


def test_f_captured_and_replayed(dev):
    """The call captured into a graph on a side stream (after one issued warm-up there) and replayed twice over new inputs:
    the words of the issued call."""
    bsz, nb, keep, L, cur, eos = 3, 6, 12, 14, 6, (2, 7)
    rng = np.random.default_rng(31)
    state = BA.random_state(rng, bsz, nb, L, cur, VOCAB, "some", eos)
    first = BA.random_selection(rng, bsz, nb, keep, VOCAB, eos)
    from outlier_suppression_amd import ops
    now, out = _buffers(state, dev), _buffers(state, dev, fill=True)
    lp, idx = torch.from_numpy(first[0]).to(dev), torch.from_numpy(first[1]).to(dev)
    eos_t = torch.tensor(list(eos), dtype=torch.int64, device=dev)
    len_div, best_div = BA.divisors(cur, L, True, 0.8)
    call = lambda: ops.beam_advance(lp, idx, now, out, cur, VOCAB, eos_t, True, len_div, best_div, True)  # noqa: E731
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        call()
    for _ in range(2):
        top_lp, top_idx = BA.random_selection(rng, bsz, nb, keep, VOCAB, eos)
        lp.copy_(torch.from_numpy(top_lp).to(dev)), idx.copy_(torch.from_numpy(top_idx).to(dev))
        for name in BA.STATE:
            t = getattr(out, name)
            t.fill_(float("nan") if t.dtype == torch.float32 else (True if t.dtype == torch.bool else -7))
        graph.replay()
        torch.cuda.synchronize()
        replayed = _numpy(out)
        issued = _numpy(_kernel(dev, top_lp, top_idx, state, cur, VOCAB, eos, True, 0.8, True))
        _same_words(replayed, issued, "replay")
        _same_words(replayed, BA.reference(top_lp, top_idx, state, cur, VOCAB, eos, True, 0.8, True), "replay / reference")


GUARD = 64
INVALID = ["keep > 64", "nb > 64", "nb > keep", "n_eos > 16", "max_length > 4096", "cur < 1", "cur >= max_length",
           "bsz = 0", "vocab = 0", "running_out is running", "scores_out is scores", "done_out is done",
           "improvable_out is improvable", "workspace too small", "valid"]


@pytest.mark.parametrize("what", INVALID)
def test_g_invalid_arguments_launch_nothing(dev, what):
    """Every invalid-argument case returns OSQ_ERR_INVALID_ARGUMENT and writes nothing: each output lies between guard bands
    and the whole buffer, output included, keeps its fill.  The same call with valid arguments writes every output and leaves
    the bands alone."""
    from outlier_suppression_amd import _hip
    lib = _hip.load()
    bsz, nb, keep, L, cur, vocab, n_eos = 2, 2, 4, 8, 3, VOCAB, 1
    alloc = dict(bsz=2, nb=65, keep=65, L=4097)                       # every buffer is large enough for every case
    if what == "keep > 64":
        keep = 65
    elif what == "nb > 64":
        nb, keep = 65, 65
    elif what == "nb > keep":
        nb, keep = 4, 3
    elif what == "n_eos > 16":
        n_eos = 17
    elif what == "max_length > 4096":
        L = 4097
    elif what == "cur < 1":
        cur = 0
    elif what == "cur >= max_length":
        cur = L
    elif what == "bsz = 0":
        bsz = 0
    elif what == "vocab = 0":
        vocab = 0
    rows, wide = alloc["bsz"] * alloc["nb"], alloc["bsz"] * alloc["nb"] * alloc["L"]
    sizes = dict(running=(wide, torch.int64), running_scores=(rows, torch.float32), finished=(wide, torch.int64),
                 scores=(rows, torch.float32), finished_len=(rows, torch.int64), done=(rows, torch.uint8),
                 improvable=(alloc["bsz"], torch.uint8))
    ins = {k: torch.zeros(n, dtype=dt, device=dev) for k, (n, dt) in sizes.items()}
    sizes.update(beam_idx=(rows, torch.int64), next_tokens=(rows, torch.int64), go_on=(1, torch.int32))
    outs = {k: torch.full((n + 2 * GUARD,), 85, dtype=dt, device=dev) for k, (n, dt) in sizes.items()}
    top_lp = -torch.arange(1, alloc["bsz"] * alloc["keep"] + 1, dtype=torch.float32, device=dev)
    top_idx = torch.arange(alloc["bsz"] * alloc["keep"], dtype=torch.int64, device=dev) % 7 + 10
    eos = torch.arange(2, 19, dtype=torch.int64, device=dev)
    ws = torch.full((64 + 2 * GUARD,), 85, dtype=torch.uint8, device=dev)
    ptr = {k: t[GUARD:].data_ptr() for k, t in outs.items()}
    for name in BA.STATE:
        if what == f"{name}_out is {name}":
            ptr[name] = ins[name].data_ptr()
    ws_bytes = 4 * bsz - 1 if what == "workspace too small" else 64
    rc = lib.osq_beam_advance(top_lp.data_ptr(), top_idx.data_ptr(), *(ins[k].data_ptr() for k in BA.STATE), eos.data_ptr(), n_eos,
                              bsz, nb, keep, vocab, L, cur, 1, 2.0, 3.0, 1, *(ptr[k] for k in BA.STATE), ptr["beam_idx"],
                              ptr["next_tokens"], ptr["go_on"], ws[GUARD:].data_ptr(), ws_bytes, _hip.raw_stream(dev))
    torch.cuda.synchronize()
    if what == "valid":
        assert rc == 0
        used = dict(running=bsz * nb * L, running_scores=bsz * nb, finished=bsz * nb * L, scores=bsz * nb, finished_len=bsz * nb,
                    done=bsz * nb, improvable=bsz, beam_idx=bsz * nb, next_tokens=bsz * nb, go_on=1)
        for k, t in outs.items():
            assert (t[:GUARD] == 85).all() and (t[GUARD + used[k]:] == 85).all(), k
            assert (t[GUARD:GUARD + used[k]] != 85).all(), k
        assert (ws[:GUARD] == 85).all() and (ws[GUARD + 4 * bsz:] == 85).all()
        return
    assert rc == -1 and lib.osq_last_error()
    for k, t in outs.items():
        assert (t == 85).all(), k
    assert (ws == 85).all()
    assert all((t == 0).all() for t in ins.values())


def test_h_ops_wrapper_checks(dev):
    """ops.beam_advance refuses what it cannot hand on: CPU tensors, a wrong dtype or shape, two sets that share memory, a
    shape the library does not take."""
    from outlier_suppression_amd import ops
    rng = np.random.default_rng(3)
    state = BA.random_state(rng, 2, 2, 8, 3, VOCAB)
    top_lp, top_idx = (torch.from_numpy(t).to(dev) for t in BA.random_selection(rng, 2, 2, 4, VOCAB))
    now, out = _buffers(state, dev), _buffers(state, dev, fill=True)
    ops.beam_advance(top_lp, top_idx, now, out, 3, VOCAB)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.beam_advance(top_lp.cpu(), top_idx.cpu(), now, out, 3, VOCAB)
    with pytest.raises(ValueError, match="top_lp"):
        ops.beam_advance(top_lp.double(), top_idx, now, out, 3, VOCAB)
    with pytest.raises(ValueError, match="shares memory"):
        ops.beam_advance(top_lp, top_idx, now, now, 3, VOCAB)
    other = ops.BeamBuffers(2, 3, 8, dev)
    with pytest.raises(ValueError, match="out.running"):
        ops.beam_advance(top_lp, top_idx, now, other, 3, VOCAB)
    with pytest.raises(ValueError, match="early_stopping"):
        ops.beam_advance(top_lp, top_idx, now, out, 3, VOCAB, early_stopping="always")
    with pytest.raises(RuntimeError, match="status -1"):
        ops.beam_advance(top_lp, top_idx, now, out, 8, VOCAB)

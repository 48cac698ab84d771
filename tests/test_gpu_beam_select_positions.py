"""osq_beam_select and osq_beam_select_at (csrc/beam_select.hip, csrc/token_argmax.h) through the C ABI with the winners
planted where the kernels' state machine turns: the table of tests/_beam_select_positions.py, whose cases
tests/test_beam_select_positions_cpu.py entitles to exact indices (gap >= 1e-4, winners = plants, magnitudes <= 64).

    A  a chunk's first and last token, registers 0 and 15, lanes 0 and 63      E  the merge: slots 0, 255, 256, n - 1, trips,
    B  all winners in the 16 registers of one thread (the owner's rescan)         nb = keep = 64, two rows planted differently
    C  all winners in one wave; lane 0 of the four waves                       F  exact ties, over chunks, beams, threads, slots
    D  every chunk's edges, the ragged last chunk, a chunk shorter than keep   G  -inf, +inf and NaN as logits and as scores
                                                                               H  ban_ids that ban planted winners

Every call: outputs pre-filled with sentinels, the workspace with 0xFF bytes (as candidates: NaN keys, which would rank
first -- a slot the chunk kernel did not write shows), logits rows ``vocab`` or ``vocab + 3`` apart in turn with NaN between
them.  Compared as tests/test_gpu_beam_select.py::_check does, with its bound: indices exactly the restatement's, finite
values within VALUE_BOUND, non-finite values equal (a NaN as the canonical quiet NaN), values that tie in float64 as equal
words.  The same table then runs through osq_beam_select_at, the position in a device word: the words of the static call.
Measured on MI355X: profiles/beam_select_positions.txt (written when OSQ_BEAM_SELECT_POSITIONS_OUT=<path> is set)."""
import os

import numpy as np
import pytest
import torch

import _beam_select_positions as P
from test_gpu_beam_select import MIN_GAP, VALUE_BOUND, _strided, _words

pytestmark = pytest.mark.gpu

CUR = 3                             # the position of every call: no history is read (ngram 0), ban_ids apply
CANONICAL_NAN = 0x7FC00000
WORST = {}                          # group -> largest |value - float64| seen
STRIDE = {c.label: c.vocab + 3 * (n & 1) for n, c in enumerate(P.TABLE)}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _call(dev, case, at=False, ws_fill=0xFF):
    """One call through the C ABI: (top_value, top_index) on the CPU.  ``at``: osq_beam_select_at with CUR as a device word
    plus an addend, cur_max above it and ban_below above it."""
    from outlier_suppression_amd import _hip
    lib = _hip.load()
    logits, running = P.inputs(case)
    bsz, nb, vocab, keep = case.bsz, case.nb, case.vocab, case.keep
    x = _strided(logits, STRIDE[case.label], dev)
    run = running.to(dev).contiguous()
    ban = torch.tensor(list(case.ban_ids) or [0], dtype=torch.int64, device=dev)
    top_v = torch.full((bsz, keep), -123.0, dtype=torch.float32, device=dev)
    top_i = torch.full((bsz, keep), -123, dtype=torch.int64, device=dev)
    need = int(lib.osq_beam_select_workspace_bytes(bsz, nb, vocab, keep))
    ws = torch.full((need,), ws_fill, dtype=torch.uint8, device=dev)
    if at:
        word = torch.tensor([CUR + 2], dtype=torch.int32, device=dev)
        rc = lib.osq_beam_select_at(x.data_ptr(), x.stride(0), run.data_ptr(), None, 0, word.data_ptr(), -2, CUR + 4, 0,
                                    ban.data_ptr(), len(case.ban_ids), CUR + 1, bsz, nb, vocab, keep, top_v.data_ptr(),
                                    top_i.data_ptr(), ws.data_ptr(), need, _hip.raw_stream(dev))
    else:
        rc = lib.osq_beam_select(x.data_ptr(), x.stride(0), run.data_ptr(), None, 0, CUR, 0, ban.data_ptr(), len(case.ban_ids),
                                 bsz, nb, vocab, keep, top_v.data_ptr(), top_i.data_ptr(), ws.data_ptr(), need,
                                 _hip.raw_stream(dev))
    torch.cuda.synchronize()
    assert rc == 0, (case.label, lib.osq_last_error())
    return top_v.cpu(), top_i.cpu()


def _check(case, got_v, got_i):
    want_v, want_i, gap = P.expected(case)
    assert gap >= MIN_GAP, f"{case.label}: gap {gap:.3g}: the case does not separate its candidates"
    words = _words(got_v).numpy()
    got = got_v.numpy().astype(np.float64)
    assert np.array_equal(got_i.numpy(), want_i), (case.label, got_i.numpy(), want_i)
    finite = np.isfinite(want_v)
    assert np.array_equal(got[~finite], want_v[~finite], equal_nan=True), (case.label, got, want_v)
    assert (words[np.isnan(want_v)] == CANONICAL_NAN).all(), (case.label, words)
    tied = want_v[:, :-1] == want_v[:, 1:]
    assert np.array_equal(words[:, :-1][tied], words[:, 1:][tied]), (case.label, "tied values differ", words)
    err = float(np.abs(got[finite] - want_v[finite]).max()) if finite.any() else 0.0
    WORST[case.group] = max(WORST.get(case.group, 0.0), err)
    print(f"{case.label}: max |value - float64| {err:.3g}, gap {gap:.3g}")
    assert err <= VALUE_BOUND, (case.label, err)
    if case.index is not None:
        for b, want in enumerate(case.index):
            assert want is None or got_i[b].tolist() == want, (case.label, b, got_i[b].tolist(), want)


def _group(letter):
    return pytest.mark.parametrize("label", [c.label for c in P.cases(letter)])


def _run(dev, label):
    case = P.BY_LABEL[label]
    got_v, got_i = _call(dev, case)
    _check(case, got_v, got_i)
    return case, got_v, got_i


@_group("A")
def test_a_positions_in_one_chunk(dev, label):
    _run(dev, label)


@_group("B")
def test_b_one_thread_owns_them_all(dev, label):
    _run(dev, label)


@_group("C")
def test_c_one_wave_one_lane(dev, label):
    _run(dev, label)


@_group("D")
def test_d_chunks(dev, label):
    _run(dev, label)


@_group("E")
def test_e_merge(dev, label):
    _run(dev, label)


@_group("F")
def test_f_exact_ties(dev, label):
    case, got_v, _ = _run(dev, label)
    want_v = P.expected(case)[0]
    assert (want_v[:, :-1] == want_v[:, 1:]).any()              # the tie is among the values returned


@_group("G")
def test_g_special_values(dev, label):
    case, got_v, got_i = _run(dev, label)
    if label == P.NAN_CASE:                                     # the batch rows without the NaN keep the clean run's words
        clean_v, clean_i = _call(dev, P.BY_LABEL[P.CLEAN_CASE])
        assert torch.isnan(got_v[1]).all() and not torch.isnan(clean_v).any()
        for b in (0, 2):
            assert torch.equal(_words(got_v[b]), _words(clean_v[b])) and torch.equal(got_i[b], clean_i[b])


@_group("H")
def test_h_bans_on_plants(dev, label):
    case, _, got_i = _run(dev, label)
    assert not np.isin(got_i.numpy() % case.vocab, case.ban_ids).any()


@pytest.mark.parametrize("label", ["D 4097, token 4096 first of 12", "E 288 slots, slots 0..6 and 252..256",
                                   "G all but three tokens of a row -inf"])
def test_i_workspace_contents_do_not_matter(dev, label):
    """The absent candidates of a chunk shorter than keep, the slots of two merge trips, -inf candidates: over a workspace
    of zero bytes the words of the run over 0xFF bytes."""
    case = P.BY_LABEL[label]
    ones = _call(dev, case)
    zeros = _call(dev, case, ws_fill=0)
    assert torch.equal(_words(ones[0]), _words(zeros[0])) and torch.equal(ones[1], zeros[1])
    _check(case, *zeros)


@pytest.mark.parametrize("group", list(P.GROUPS))
def test_j_position_from_a_device_word(dev, group):
    """osq_beam_select_at over the table: the three kernels are the static form's, so what is new is only that reading the
    position (and comparing it with ban_below, which is above it: the ban_ids of H apply) leaves the selection alone."""
    for case in P.cases(group):
        static = _call(dev, case)
        at = _call(dev, case, at=True)
        assert torch.equal(_words(at[0]), _words(static[0])) and torch.equal(at[1], static[1]), case.label


def test_z_report():
    """The largest error of this run per group (the bound is VALUE_BOUND)."""
    if not WORST:           # run on its own: nothing to report
        return
    lines = ["osq_beam_select with planted winners (tests/_beam_select_positions.py) against the float64 restatement",
             f"(tests/_beam_select.py): max |value - float64| per group; bound {VALUE_BOUND:g}, every case's gap between distinct",
             f"neighbours among ranks 1 .. keep + 1 >= {MIN_GAP:g}", ""]
    titles = {"A": "positions in one chunk", "B": "one thread owns them all", "C": "one wave, one lane", "D": "chunks",
              "E": "merge", "F": "exact ties", "G": "special values", "H": "bans on plants"}
    lines += [f"{g} {titles[g]:<28s} {len(P.cases(g)):3d} cases   {WORST[g]:.3e}" for g in P.GROUPS if g in WORST]
    lines += ["", f"largest: {max(WORST.values()):.3e}"]
    print("\n".join(lines))
    out = os.environ.get("OSQ_BEAM_SELECT_POSITIONS_OUT")
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")

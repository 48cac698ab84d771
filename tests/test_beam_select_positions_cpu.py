"""CPU: the case table of tests/_beam_select_positions.py on the float64 restatement alone (tests/_beam_select.py) -- what
entitles tests/test_gpu_beam_select_positions.py to compare indices exactly and values within the bound that
tests/test_gpu_beam_select.py derives for magnitude <= 64.

For every case: the gap between distinct neighbours among ranks 1 .. keep + 1 is at least 1e-4 (exact ties and non-finite
values do not count, as BS.gap says); in the planted groups A-E and H the reference's first N elements, N the number of
plants no ban_id bans (N >= keep), are exactly those plants, so its top ``keep`` are plants and the plants not taken still
outrank all noise; every compared finite value, the winners' x - m and every L involved stay within 64; where a case states
an order, the reference gives it; and on the tie-free, all-finite cases the reference agrees with torch's and transformers'
own pipeline on the CPU (``_pipeline`` of tests/test_beam_select_cpu.py: exact indices, values within its 1e-5).
Then the coverage, by the ownership model and not by hand: every class of ``P.CLASSES`` is hit by the winners of some case,
and every case hits the classes it is there for."""
import numpy as np
import pytest
import torch

import _beam_select as BS
import _beam_select_positions as P
from test_beam_select_cpu import _pipeline
from test_gpu_beam_select import MIN_GAP       # the module imports without a GPU; its tests are not collected from here

MAGNITUDE = 64.0            # what VALUE_BOUND of tests/test_gpu_beam_select.py is derived for

LABELS = [c.label for c in P.TABLE]


def test_ownership_model():
    for t, want in ((0, (0, 0, 0, 0, 0, 0)), (63, (0, 63, 63, 0, 0, 63)), (64, (0, 64, 64, 0, 1, 0)), (255, (0, 255, 255, 0, 3, 63)),
                    (256, (0, 256, 0, 1, 0, 0)), (3839, (0, 3839, 255, 14, 3, 63)), (3840, (0, 3840, 0, 15, 0, 0)),
                    (4095, (0, 4095, 255, 15, 3, 63)), (4096, (1, 0, 0, 0, 0, 0)), (50264, (12, 1112, 88, 4, 1, 24))):
        assert tuple(P.owner(t)) == want, t
        o = P.owner(t)
        assert P.tok(o.chunk, o.thread, o.register) == t
    assert [P.chunks_of(v) for v in (1, 4096, 4097, 8193, 50265)] == [1, 1, 2, 3, 13]
    assert P.chunk_len(50265, 12) == 1113 and P.chunk_len(8193, 2) == 1 and P.chunk_len(8193, 1) == 4096
    assert P.merge_slot(7, 0, 4, 3, 12) == 256 and P.merge_owner(256) == (0, 1) and P.merge_owner(255) == (255, 0)


def test_the_table_has_every_group_and_the_issue_s_shapes():
    assert sorted({c.group for c in P.TABLE}) == list(P.GROUPS)
    shapes = {(c.nb, c.vocab, c.keep) for c in P.TABLE}
    assert {(64, 4097, 64), (64, 50265, 64), (4, 4096, 64)} <= shapes
    slots = {c.nb * P.chunks_of(c.vocab) * c.keep for c in P.cases("E")}
    assert min(slots) < 256 and 256 in slots and max(slots) > 256
    for c in P.TABLE:
        assert 1 <= c.keep <= min(64, c.vocab) and 1 <= c.nb <= 64 and len(c.ban_ids) <= 16, c.label
        assert c.bsz * c.nb * c.vocab <= 2 * 64 * 50265, c.label


@pytest.mark.parametrize("label", LABELS)
def test_case_separates_its_candidates(label):
    case = P.BY_LABEL[label]
    logits, running = P.inputs(case)
    want_v, want_i, gap = P.expected(case)
    assert gap >= MIN_GAP, f"{label}: gap {gap:.3g}"
    print(f"{label}: gap {gap:.3g}")

    # ---- magnitudes: the compared values, the winners' x - m, the L of every row that supplies a winner
    x = logits.numpy().astype(np.float64)
    finite = np.isfinite(want_v)
    assert finite.any() or case.group == "G"
    if finite.any():
        assert np.abs(want_v[finite]).max() <= MAGNITUDE, (label, np.abs(want_v[finite]).max())
    for b in range(case.bsz):
        for value, idx in zip(want_v[b], want_i[b].tolist()):
            if not np.isfinite(value):
                continue
            row = x[b * case.nb + idx // case.vocab]
            m = row.max()
            big_l = np.log(np.exp(row - m).sum())
            assert abs(row[idx % case.vocab] - m) <= MAGNITUDE and abs(big_l) <= MAGNITUDE, (label, b, idx)

    # ---- the winners are the plants
    if case.group in P.PLANTED_GROUPS:
        v = BS.values(logits.numpy(), running.numpy(), ban_ids=case.ban_ids)
        for b, plants in enumerate(P.unbanned_plants(case)):
            assert len(plants) >= case.keep, (label, "fewer plants than keep")
            first = sorted(BS.order(v[b])[:len(plants)].tolist())
            assert first == plants, (label, b, sorted(set(first) ^ set(plants)))
            assert set(want_i[b].tolist()) <= set(plants)
            if len(plants) == case.keep:
                assert sorted(want_i[b].tolist()) == plants
        if case.ban_ids:
            banned = [t for row in P.per_row(case.plants, case.bsz) for _, t in row if t in case.ban_ids]
            assert banned and not np.isin(want_i % case.vocab, case.ban_ids).any(), (label, "no plant is banned")

    # ---- a stated order
    if case.index is not None:
        for b, want in enumerate(case.index):
            assert want is None or want_i[b].tolist() == want, (label, b, want_i[b].tolist(), want)
    if case.group == "F":                                   # a tie is there: two of the first keep + 1 values are one word
        v = BS.values(logits.numpy(), running.numpy())
        for b in range(case.bsz):
            top = v[b][BS.order(v[b])[:case.keep + 1]]
            assert (top[:-1] == top[1:]).any(), (label, b)

    # ---- torch's own pipeline
    if case.pipeline:
        assert torch.isfinite(logits).all() and torch.isfinite(running).all()
        assert all(len(np.unique(row)) == row.size for row in want_v), (label, "a tie")
        torch_v, torch_i = _pipeline(logits, running, case.keep, None, 0, case.ban_ids, 0)
        assert np.array_equal(want_i, torch_i.numpy()), label
        assert np.abs(want_v - torch_v.numpy().astype(np.float64)).max() <= 1e-5, label


def test_special_value_cases_say_what_the_issue_says():
    inf_v, _, _ = P.expected(P.BY_LABEL["G one +inf logit"])
    assert np.isnan(inf_v[1]).all() and np.isfinite(inf_v[[0, 2]]).all()
    ninf_v, _, _ = P.expected(P.BY_LABEL["G a row of -inf only"])
    assert np.isnan(ninf_v[2]).all() and np.isfinite(ninf_v[[0, 1]]).all()
    nan_v, nan_i, _ = P.expected(P.BY_LABEL[P.NAN_CASE])
    clean_v, clean_i, _ = P.expected(P.BY_LABEL[P.CLEAN_CASE])
    assert np.isnan(nan_v[1]).all()
    assert np.array_equal(nan_v[[0, 2]], clean_v[[0, 2]]) and np.array_equal(nan_i[[0, 2]], clean_i[[0, 2]])
    assert np.isnan(P.expected(P.BY_LABEL["G a running score of NaN"])[0][0]).all()
    assert np.isfinite(P.expected(P.BY_LABEL["G a running score of -inf"])[0]).all()
    assert (P.expected(P.BY_LABEL["G a running score of +inf"])[0][2] == np.inf).all()
    # all but three tokens -inf: the six finite values of a batch row, then -inf by flat index over chunks and beams
    case = P.BY_LABEL["G all but three tokens of a row -inf"]
    v, i, _ = P.expected(case)
    assert np.isfinite(v[:, :6]).all() and (v[:, 6:] == -np.inf).all()
    assert i[0, 6:].tolist() == [0, 2, 3, 5, 6, 7] and i[1, 6:].tolist() == [0, 1, 2, 4, 6, 7]
    assert {t // P.CHUNK for t in (i[0, :6] % case.vocab).tolist()} == {0, 1}
    for name in ("first", "middle", "ragged last"):
        case = P.BY_LABEL[f"G the {name} chunk of beam 1 holds only -inf"]
        logits, _ = P.inputs(case)
        per_chunk = [bool(torch.isinf(logits[1, c * P.CHUNK:(c + 1) * P.CHUNK]).all()) for c in range(3)]
        assert per_chunk == [name == "first", name == "middle", name == "ragged last"]
        assert np.isfinite(P.expected(case)[0]).all()


def test_the_winners_hit_every_ownership_class():
    hit = set()
    for case in P.TABLE:
        here = P.classes_hit(case)
        assert here <= set(P.CLASSES), here - set(P.CLASSES)
        missing = [name for name in case.classes if name not in here]
        assert not missing, f"{case.label}: its winners miss {missing}"
        hit |= here
    missing = [name for name in P.CLASSES if name not in hit]
    assert not missing, f"no case of the table puts a winner into: {missing}"
    print("classes hit: " + ", ".join(P.CLASSES))

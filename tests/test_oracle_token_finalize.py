"""What the tables of tests/_token_finalize.py reach, asserted from the models (no GPU): every branch class of the three
implementations of osq_token_range_finalize has a case, every case's oracle result is finite (or NaN where it says so), every
placement is dispatched to the implementation it is aimed at, and the models agree with each other and with a plain walk of the
slots."""
import numpy as np
import pytest

import _fused_select as FS
import _token_finalize as TF
from _minmax_positions import case_seed

F32 = np.float32
CASES = TF.value_cases()
IMPLS = ("select", "single", "wide")


def problem(case, side, impl, n):
    B, T, L, knobs = TF.value_geometry(impl, case["vals"].size, n)
    tmin, tmax, ok = TF.place(case["vals"], case["other"], side, B, T, L, case_seed(case["name"]) + side, ("nan", "huge")[n % 2])
    return B, T, L, knobs, tmin, tmax, ok


def sides_of(tmin, tmax, ok):
    return tmax[ok], -tmin[ok]


@pytest.fixture(scope="module")
def reached():
    """{impl: {class: [case names]}} over the value cases (both sides) and the size classes."""
    out = {impl: {} for impl in IMPLS}

    def note(impl, classes, name):
        for c in classes:
            out[impl].setdefault(c, []).append(name)

    for n, case in enumerate(CASES):
        for side in (0, 1):
            name = "%s/side%d" % (case["name"], side)
            B, T, L, _, tmin, tmax, ok = problem(case, side, "select", n)
            for s, v in enumerate(sides_of(tmin, tmax, ok)):
                note("select", TF.select_classes_of(TF.select_report(v, case["p"]), TF.select_side_model(B, T, L)), name)
            B, T, L, _, tmin, tmax, ok = problem(case, side, "single", n)
            note("single", TF.single_classes_of(TF.single_path(*sides_of(tmin, tmax, ok), case["p"], B * T)), name)
            B, T, L, _, tmin, tmax, ok = problem(case, side, "wide", n)
            for v in sides_of(tmin, tmax, ok):
                note("wide", TF.wide_classes_of(TF.wide_path(v, case["p"]), TF.wide_geometry(B, T, L)), name)
    for B, T in TF.SELECT_SIZES:
        for pattern, L, kind, pad in TF.size_problems("select", B, T):
            vals, p = TF.scalable_values(kind, sum(TF.clamp_lengths(L, T)))
            name = "size %dx%d/%s/%s" % (B, T, pattern, kind)
            note("select", TF.select_classes_of(TF.select_report(vals, p), TF.select_side_model(B, T, L)), name)
    for B, T, how in TF.SINGLE_SIZES:
        for pattern, L, kind, pad in TF.size_problems("single", B, T):
            vals, p = TF.scalable_values(kind, sum(TF.clamp_lengths(L, T)))
            note("single", TF.single_classes_of(TF.single_path(vals, TF.default_other(vals.size), p, B * T)), "size %dx%d/%s/%s/%s" % (B, T, how, pattern, kind))
    for B, T in TF.WIDE_SIZES:
        for pattern, L, kind, pad in TF.size_problems("wide", B, T):
            vals, p = TF.scalable_values(kind, sum(TF.clamp_lengths(L, T)))
            note("wide", TF.wide_classes_of(TF.wide_path(vals, p), TF.wide_geometry(B, T, L)), "size %dx%d/%s/%s" % (B, T, pattern, kind))
    return out


@pytest.mark.parametrize("impl,classes", [("select", TF.SELECT_CLASSES), ("single", TF.SINGLE_CLASSES), ("wide", TF.WIDE_CLASSES)])
def test_every_class_is_reached(impl, classes, reached):
    missing = [c for c in classes if not reached[impl].get(c)]
    assert not missing, (impl, missing)


def test_a_class_without_cases_is_noticed(reached):
    """The check above looks at the models' reports, not at a list kept by hand: a class nothing reaches is reported."""
    assert not reached["wide"].get(("hi_source", "no such source"))
    assert not reached["single"].get(("SLOTS", 64))


def test_the_fused_cases_keep_their_branches():
    """The cases taken over from tests/_fused_select.py take, without a window, the branches their names say."""
    by_name = {c["name"]: c for c in FS.path_cases()}
    for case in CASES:
        if case["name"] not in by_name:
            continue
        rep = TF.select_report(case["vals"], case["p"])
        for k, v in by_name[case["name"]]["expect"].items():
            if k in TF.WINDOW_FIELDS:
                continue
            if by_name[case["name"]]["expect"].get("window") is not False and k not in ("k_eq", "w_lt_half", "reaches_hi", "pos"):
                continue                                            # a hinted first level is not the full-range one: other bins
            assert rep[k] == v, (case["name"], k, rep[k], v)


def test_named_aims():
    """The classes the new cases are named after, per implementation, from the models."""
    by = {c["name"]: c for c in CASES}

    def wide(name, side=0):
        c = by[name]
        return TF.wide_path(c["vals"], c["p"])

    def single(name):
        c = by[name]
        return TF.single_path(c["vals"], c["other"], c["p"], c["vals"].size)

    r = wide("edge_next_coarse_bin")
    assert r["last_of_coarse"] and r["hi_source"] == "next_inv" and r["source_decides"] and r["coarse_count"] > TF.LIST_CAP
    assert wide("edge_first_of_coarse_bin")["first_of_coarse"]
    r = wide("edge_next_first_level_bin")
    assert r["hi_source"] == "s_above" and r["source_decides"]
    r = wide("edge_same_first_level_bin")
    assert r["hi_source"] == "same_bin" and r["source_decides"]
    assert wide("dense_no_next")["all_in_list"]
    r = single("edge_next_level0_bin")[0]
    assert r["exit"] == "listed" and r["hi_source"] == "s_next" and r["source_decides"]
    r = single("edge_same_first_level_bin")[0]
    assert r["exit"] == "listed" and r["hi_source"] == "list" and r["source_decides"]
    r = single("dups_rank_inside")[0]
    assert r["exit"] == "listed" and r["mixed"] == "this_done" and r["hi_source"] == "dups"
    r = single("dups_rank_last")[0]
    assert r["exit"] == "listed" and r["mixed"] == "this_done" and r["hi_source"] == "s_next" and r["source_decides"]
    r = single("dups_rank_last_beside_constant")[0]
    assert r["exit"] == "all_levels" and r["hi_source"] == "s_next" and r["source_decides"]
    r = single("dups_rank_last_wide_range")[0]
    assert r["levels"] == 3 and r["exit"] == "all_levels" and r["hi_source"] == "s_next" and r["source_decides"]
    r = single("all_levels_inner")[0]
    assert r["levels"] == 3 and r["exit"] == "all_levels" and r["hi_source"] == "dups"
    r = single("dups_rank_below")[0]
    assert r["hi_source"] == "s_next" and r["source_decides"]
    a, b = single("crowded_beside_constant")
    assert a["exit"] == "listed" and a["mixed"] == "other_done" and b["mixed"] == "this_done" and b["hi_source"] == "dups" and b["levels"] == 1
    a, b = single("crowded_beside_two_keys")
    assert a["mixed"] == "other_done" and b["mixed"] == "this_done" and b["hi_source"] == "s_next" and b["source_decides"]
    a, b = single("duplicates_beside_sparse")
    assert a["mixed"] == "this_done" and a["hi_source"] == "dups" and b["mixed"] == "other_done" and b["hi_source"] == "list"
    assert single("sign_tie_at_rank")[0]["list_sign_tie"] and single("zeros_of_both_signs")[0]["sign_tie"]


def test_oracle_results():
    """Every case's oracle result is finite on both sides; a NaN at a valid slot poisons the oracle (the quantile is NaN), one
    in the padding does not."""
    for n, case in enumerate(CASES):
        for side in (0, 1):
            B, T, L, _, tmin, tmax, ok = problem(case, side, "select", n)
            cur = TF.expected_cur(tmin[ok], tmax[ok], case["p"])
            assert case["finite"] and np.isfinite(cur).all(), (case["name"], side, cur)
            assert cur[0] <= cur[1]
            first, last = np.flatnonzero(ok)[[0, -1]]
            for where, arr in ((first, tmax), (last, tmin)):
                bad = arr.copy()
                bad[where] = np.nan
                got = TF.expected_cur(*((tmin[ok], bad[ok]) if arr is tmax else (bad[ok], tmax[ok])), case["p"])
                assert np.isnan(got).all(), (case["name"], side, where)
            if not ok.all():
                pad = tmax.copy()
                pad[np.flatnonzero(~ok)[0]] = np.nan
                assert np.array_equal(TF.expected_cur(tmin[ok], pad[ok], case["p"]), cur)
    c = {c["name"]: c for c in CASES}["clip_rule_lo_above_up"]
    B, T, L, _, tmin, tmax, ok = problem(c, 0, "select", 0)
    lo, up = TF.OB.prune_thresholds(tmin[ok], tmax[ok], c["p"])
    assert lo > up and TF.expected_cur(tmin[ok], tmax[ok], c["p"]).tolist() == [up, up]


def test_value_placements_are_dispatched_as_aimed():
    for n, case in enumerate(CASES):
        N = case["vals"].size
        for impl in IMPLS:
            B, T, L, knobs = TF.value_geometry(impl, N, n)
            assert sum(TF.clamp_lengths(L, T)) == N and len(L) == B
            assert TF.dispatch(B, T, knobs["final_fast"], knobs["wide_min"])[0] == impl, (case["name"], impl, B, T)
            if impl == "single" and knobs["final_fast"]:
                assert not TF.select_fast_ok(B, T)
            if impl == "single" and not knobs["final_fast"]:
                assert TF.select_fast_ok(B, T)                      # only the knob keeps select away


def test_size_classes_are_dispatched_as_aimed():
    got = {}
    for B, T in TF.SELECT_SIZES:
        impl, r4 = TF.dispatch(B, T)
        assert impl == "select" and TF.select_side_model(B, T, None)["R4"] == r4
        got.setdefault("select", set()).add(r4)
    assert sorted(B * T for B, T in TF.SELECT_SIZES[:8]) == [4, 4096, 4100, 8192, 8196, 16384, 16388, 32768]
    assert {T for _, T in TF.SELECT_SIZES[8:]} == {5, 6, 7, 101}
    for B, T, how in TF.SINGLE_SIZES:
        k = TF.single_knobs(how)
        impl, slots = TF.dispatch(B, T, k["final_fast"], k["wide_min"], k["off_min"], k["off_max"])
        assert impl == "single", (B, T, how)
        got.setdefault("single", set()).add(slots)
        # the stated reason is THE reason: with the knobs at their defaults and aligned arrays it alone decides
        plain = TF.dispatch(B, T)[0]
        assert {"t_below_4": T < 4 and plain == "single", "odd_slots": T >= 4 and (B * T) % 4 != 0 and plain == "single",
                "final_fast_0": plain == "select", "tmin_off_16": plain == "select", "tmax_off_16": plain == "select",
                "wide_min_raised": plain == "wide"}[how], (B, T, how)
    assert {B * T for B, T, _ in TF.SINGLE_SIZES} >= {1, 3, 4095, 4096, 4097, 8193, 16385, 32768, 32769}
    assert {how for _, _, how in TF.SINGLE_SIZES} == {"t_below_4", "odd_slots", "final_fast_0", "tmin_off_16", "tmax_off_16", "wide_min_raised"}
    for B, T in TF.WIDE_SIZES:
        impl, wgs = TF.dispatch(B, T, wide_min=TF.WIDE_FLOOR)
        assert impl == "wide"
        got.setdefault("wide", set()).add(wgs)
    assert {B * T for B, T in TF.WIDE_SIZES} == {1024, 1025, 12288}
    assert got["select"] == {1, 2, 4, 8} and got["single"] == {4, 8, 16, 32, 0} and {2, 3, 24} <= got["wide"]


@pytest.mark.parametrize("B,T", [s for s in TF.SELECT_SIZES if s[0] * s[1] <= 8196 or s[1] in (7, 101)])
def test_select_side_validity_is_the_mask(B, T):
    """rem_a / rem_b / wrap give every slot the validity of t < lengths[b], at every length pattern."""
    for pattern in TF.LENGTH_PATTERNS:
        L = TF.pattern_lengths(pattern, B, T)
        assert np.array_equal(TF.select_side_model(B, T, L)["ok"], TF.valid_mask(B, T, L)), (B, T, pattern)


def test_models_agree_on_the_ranks():
    """select_path, the single model and the wide model compute one rank arithmetic: k_lo / k_hi / w agree per case, and the key
    the single model's narrowing ends on is the sorted array's (asserted inside single_path)."""
    for n, case in enumerate(CASES):
        N = case["vals"].size
        sel, wide = TF.select_report(case["vals"], case["p"]), TF.wide_path(case["vals"], case["p"])
        one = TF.single_path(case["vals"], case["other"], case["p"], N)[0]
        ref = FS.select_path(case["vals"], case["p"], np.inf)
        for rep in (sel, wide, one):
            assert (rep["k_lo"], rep["k_hi"]) == (wide["k_lo"], wide["k_hi"]) and rep["w"] == wide["w"], case["name"]
            assert rep["k_eq"] == ref["k_eq"] and rep["w_lt_half"] == ref["w_lt_half"], case["name"]
        if ref["exit"] == "listed" and ref["reaches_hi"] is not None and not ref["k_eq"]:
            assert ref["reaches_hi"] == wide["reaches_hi"] == one["reaches_hi"], case["name"]


def test_scalable_values_are_distinct_where_they_say():
    for kind in TF.SCALABLE_KINDS:
        for V in (1, 2, 3, 4, 7, 4095, 32769):
            vals, p = TF.scalable_values(kind, V)
            assert vals.size == V and np.isfinite(vals).all() and (np.diff(vals) >= 0).all() and 0 <= p <= 1
            if kind != "dups":
                assert np.unique(vals).size == V

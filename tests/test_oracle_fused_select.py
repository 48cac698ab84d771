"""What the cases of tests/_fused_select.py reach, asserted on the CPU: the chunk-geometry model of fused_select<CH>
(csrc/fused_step.h) against a brute-force walk of its loads, the (CH, lt) classes, grids and planted positions of the
case tables, the branch of select_from_registers (csrc/token_select.h) every selection-path case names, and the condition
that makes a dropped extremum visible: with the planted token poisoned the oracle's (lo, up) changes, for every planted
case.  tests/test_gpu_fused_select.py runs the same tables on the device."""
import numpy as np
import pytest

import _fused_select as FS
import _minmax_positions as MP
from conftest import bits_equal
from oracle import observer_oracle as OB

RELEASE_NWG = 254           # an MI355X: 256 CUs, two of them selectors
ALL21 = {(ch, lt) for ch in (1, 2, 3) for lt in range(7)}


def release_geometries(nwg):
    out = {}
    for name in FS.RELEASE_CLASSES:
        c = FS.release_case(name, nwg)
        if c is not None:
            V, B, T = c
            out[name] = FS.geometry(nwg, B * T, V)
    return out


def knob_geometries():
    return [FS.geometry(nwg, B * T, V) for nwg in FS.KNOB_NWG for V, B, T in FS.knob_cases(nwg)]


def test_constants_restate_the_header():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "outlier_suppression_amd", "csrc", "fused_step.h")).read()
    obs = open(os.path.join(root, "outlier_suppression_amd", "csrc", "observer.hip")).read()
    for text in ("#define OSQ_FUSED_GROUPS %d" % FS.NG, "const unsigned int nwg = gridDim.x - 2u;", "qt = total / nwg, rt = total - qt * nwg;",
                 "qv = V / nwg, rv = V - qv * nwg;", "cmax = qv + (rv ? 1u : 0u);", "tlen = cmax - static_cast<unsigned int>(OSQ_WAVE * (CH - 1));",
                 "ntg = static_cast<unsigned int>(GC) / cpr;", "constexpr int kFusedMaxBatch = %d;" % FS.MAX_BATCH,
                 "constexpr int kFusedHoldRegs = %d;" % MP.FUSED_HOLD_REGS, "constexpr int kFusedHoldLds = %d;" % MP.FUSED_HOLD_LDS):
        assert text in src, text
    for text in ("constexpr int kSelBins = %d;" % FS.SEL_BINS, "constexpr int kSelBits = %d;" % FS.SEL_BITS, "constexpr int kListCap = %d;" % FS.LIST_CAP,
                 "> 3 * OSQ_WAVE || grid - 2 > kFusedWaves * kFusedWaves", "slots <= 4 * 8 * kSelThreads"):
        assert text in obs, text
    assert FS.NC == 16 and FS.GC == 8 and FS.MAX_NWG == 256


@pytest.mark.parametrize("nwg", [1, 2, 3, 15, 16, 17, 33, 130, 254, 256])
def test_release_classes_reach_every_chunk_shape(nwg):
    """The V list of the release-grid test on nwg streaming workgroups (254 on an MI355X; the formula for any CUs >= 3)."""
    geos = release_geometries(nwg)
    got = {(g["CH"], g["lt"]) for g in geos.values()}
    cap = min(FS.MAX_SLOTS, 192 * nwg)
    want = {(ch, lt) for ch in (1, 2) for lt in range(7) if (64 * (ch - 1) + FS.TAILS[lt] - 1) * nwg + 1 <= cap}
    want |= {(3, lt) for lt, t in ((0, 1), (1, 2)) if (128 + t - 1) * nwg + 4 <= cap}
    assert want <= got, sorted(want - got)
    for name, g in geos.items():
        if name.startswith("ch"):
            ch, k = int(name[2]), int(name.rsplit("t", 1)[1])
            assert g["CH"] == ch and g["tlen"] == (FS.TAILS[k] if ch < 3 else k), (name, g)
        assert FS.eligible(g["total"] // FS.release_case(name, nwg)[2], FS.release_case(name, nwg)[2], 768, nwg), name
    if nwg == RELEASE_NWG:
        assert set(geos) == set(FS.RELEASE_CLASSES)                                     # none is missing on the real grid
        assert got == {(ch, lt) for ch in (1, 2) for lt in range(7)} | {(3, 0), (3, 1)}
        assert {g["tlen"] for g in geos.values() if g["CH"] == 3} == {1, 2}
        assert {g["rv"] == 0 for g in geos.values()} == {True, False} and {g["rt"] == 0 for g in geos.values()} == {True, False}
        V = {n: g["V"] for n, g in geos.items()}
        assert V["v1"] == 1 and V["below_nwg"] < nwg and geos["below_nwg"]["qv"] == 0
        assert (V["v64n"], V["v64n+1"], V["v128n"], V["v128n+1"]) == (64 * nwg, 64 * nwg + 1, 128 * nwg, 128 * nwg + 1)
        assert geos["v64n"]["CH"] == 1 and geos["v64n+1"]["CH"] == 2 and geos["v128n"]["CH"] == 2 and geos["v128n+1"]["CH"] == 3
        assert max(g["total"] for g in geos.values()) == FS.MAX_SLOTS


def test_knob_grids_reach_all_21_classes():
    geos = knob_geometries()
    assert {(g["CH"], g["lt"]) for g in geos} == ALL21
    assert {(g["CH"], g["lt"]) for g in geos if g["nwg"] == 1} == ALL21              # in tensors of at most 192 tokens
    assert {(g["CH"], g["lt"]) for g in geos if 1 < g["nwg"] < 130} == ALL21
    assert {g["nwg"] for g in geos} == {1, 2, 15, 16, 17, 33, 130}
    assert max(g["tlen"] for g in geos if g["CH"] == 3) == 64
    assert {g["ntg"] for g in geos} == {1, 2, 4, 8}
    for g in geos:
        assert g["total"] % 4 == 0 and g["V"] <= g["total"] <= 192 * g["nwg"], g
    big = [g for g in geos if g["nwg"] >= 129]
    assert big and any(g["cpr"] > 1 for g in big)                                       # tails of several chunks share a register
    for g in big:                                                                       # ... and a wave holds chunks of both groups
        assert {FS.locate(g, j)["group"] for j in range(g["nwg"])} == {0, 1}, g
    assert any(g["rv"] == 0 for g in geos) and any(g["rv"] > 0 for g in geos) and any(g["rt"] > 0 for g in geos)


def all_geometries():
    out = [g for nwg in (RELEASE_NWG, 3, 62) for g in release_geometries(nwg).values()] + knob_geometries()
    return out


def test_locate_equals_the_brute_force_walk():
    """Every j < V lies in exactly one (register, lane) of exactly one selector wave; the slots the walk absorbs as valid are
    exactly those with local < nv(g); locate() names the same place."""
    for geo in all_geometries():
        walk = FS.walk_selector(geo)
        written = FS.written_slots(geo)
        assert len(written) == geo["V"] and sorted(written.values()) == list(range(geo["V"])), geo
        valid = {}
        for (wv, reg, lane), (slot, ok) in walk.items():
            if ok:
                assert slot not in valid, (geo, "slot absorbed twice", slot)
                valid[slot] = (wv, reg, lane)
        assert set(valid) == set(written), (geo, sorted(set(valid) ^ set(written))[:8])
        assert geo["V"] == 0 or max(written) < geo["total"]
        step = max(1, geo["V"] // 997)
        for j in list(range(0, geo["V"], step)) + FS.plant_positions(geo):
            at = FS.locate(geo, j)
            assert written[at["slot"]] == j and valid[at["slot"]] == (at["wave"], at["reg"], at["lane"]), (geo, j, at)
            assert at["local"] < FS.nv_of(geo, at["g"])
        R = FS.NC * (geo["CH"] - 1) + FS.NC
        assert all(reg < R for _, reg, _ in walk)


def test_planted_positions_cover_every_place():
    for geo in all_geometries():
        if geo["V"] == 0:
            continue
        pos = FS.plant_positions(geo)
        assert len(set(pos)) == len(pos) and all(0 <= j < geo["V"] for j in pos)
        at = [FS.locate(geo, j) for j in pos]
        nwg, rv, CH, tlen = geo["nwg"], geo["rv"], geo["CH"], geo["tlen"]
        chunks = {a["g"] for a in at}
        want_chunks = {g for g in (0, rv - 1, rv, nwg - 1) if 0 <= g < nwg and FS.nv_of(geo, g) > 0}
        assert want_chunks <= chunks, (geo, want_chunks - chunks)
        if geo["V"] >= nwg >= FS.NC:
            assert any(a["wave"] == FS.NC - 1 for a in at), geo
        if geo["V"] >= nwg > FS.NC * FS.GC:
            assert any(a["group"] == 1 for a in at), geo
        for g in want_chunks:
            mine = [a for a in at if a["g"] == g]
            nvg = FS.nv_of(geo, g)
            mains = {(a["c"], a["lane"]) for a in mine if a["kind"] == "main"}
            assert mains == {(c, l) for c in range(CH - 1) for l in (0, 63)}, (geo, g)
            tails = {a["tl"] for a in mine if a["kind"] == "tail"}
            assert tails == {t for t in (0, tlen - 2, tlen - 1) if 0 <= t and 64 * (CH - 1) + t < nvg}, (geo, g, tails)
        launches = FS.plant_launches(geo)
        assert {l[0] for l in launches} == set(pos) and {l[1] for l in launches} == set(pos)      # both sides visit every place
        if len(launches) > 1:
            assert {l[4] for l in launches} == {True, False}


def test_a_dropped_planted_extremum_changes_the_oracle():
    """The omission design as a condition: for EVERY planted launch of every geometry, the oracle's (lo, up) with the planted
    token's extremum poisoned differs from the one with it -- on each side.  Also: the planted threshold is the planted token's
    own extremum, and the hinted launches' windows hold the rank."""
    n = 0
    for geo in list(release_geometries(RELEASE_NWG).values()) + knob_geometries():      # every geometry the GPU file runs
        V = geo["V"]
        if V == 0:
            continue
        a, m = FS.grids(V, V + geo["nwg"])
        launches = FS.plant_launches(geo)
        for j0, j1, k, p, hinted in launches:
            tmax, tmin = FS.plant(a, j0, k), -FS.plant(m, j1, k)
            lo, up = OB.prune_thresholds(tmin, tmax, p)
            assert up == tmax[j0] and lo == tmin[j1], (geo, j0, j1, k)
            for side, j in ((0, j0), (1, j1)):
                lo2, up2 = FS.poisoned_thresholds(tmin, tmax, p, j, side)
                got, was = (up2, up) if side == 0 else (lo2, lo)
                assert not bits_equal(np.array([got], np.float32), np.array([was], np.float32)), (geo, side, j, k)
            if hinted:
                for side, hint in ((0, FS.HINT_MAX), (1, -FS.HINT_MIN)):
                    rep = FS.select_path(FS.side_values(tmin, tmax, side), p, hint)
                    assert rep["window"] and rep["prehist"] and rep["k_eq"], (geo, side, rep)
            n += 1
    assert n > 900


def test_selection_path_cases_reach_the_branches_they_name():
    cases = FS.path_cases()
    assert len({c["name"] for c in cases}) == len(cases)
    for side in (0, 1):
        met = set()
        for c in cases:
            tmin, tmax, state, cnt = FS.path_tokens(c, side, MP.case_seed(c["name"]))
            assert (tmin <= tmax).all() and 8 <= tmin.size <= 3000
            hint = abs(state[1] if side == 0 else state[0])
            rep = FS.select_path(FS.side_values(tmin, tmax, side), c["p"], hint)
            for key, want in c["expect"].items():
                assert rep[key] == want, (c["name"], side, key, rep)
            met |= {(k, rep[k]) for k in rep if rep[k] is not None}
            if c["name"].startswith("off_"):
                assert not FS.hint_window(hint)["on"]
        missing = [cl for cl in FS.PATH_CLASSES if cl not in met]
        assert not missing, (side, missing)


def test_select_path_threshold_agrees_with_the_oracle_quantile():
    """The model's rank arithmetic is the oracle's: where the path is `listed`, lerp of the two keys it finds equals
    torch_quantile_linear of |values| (a check of the MODEL, so that its branch claims can be trusted)."""
    for c in FS.path_cases():
        v = c["vals"]
        s = np.sort(np.abs(v))
        rank = np.float32(c["p"]) * np.float32(v.size - 1)
        assert int(np.floor(rank)) < v.size
        q = OB.torch_quantile_linear(np.abs(v), c["p"])
        assert s[int(np.floor(rank))] <= q <= s[int(np.ceil(rank))]


def test_enumeration_and_row_mapping_tables():
    rows, V = FS.enumeration_rows([2, 0, 3, 1], 3)
    assert V == 6 and rows.tolist() == [0, 1, 6, 7, 8, 9, 2, 3, 4, 5, 10, 11]
    for B in FS.ROW_B:
        for pattern in FS.ROW_PATTERNS:
            L = FS.pattern_lengths(pattern, B, 8)
            rows, V = FS.enumeration_rows(L, 8)
            assert sorted(rows.tolist()) == list(range(B * 8)) and V == sum(L)
    nwg = RELEASE_NWG
    for nv in (4, 12, 16):
        for B in FS.ROW_B:
            for pattern in FS.ROW_PATTERNS:
                T = FS.row_mapping_T(B, pattern, nv, nwg)
                assert T is not None and B * T <= FS.MAX_SLOTS and FS.eligible(B, T, 256 * nv, nwg), (nv, B, pattern, T)
                V = sum(FS.pattern_lengths(pattern, B, T))
                assert B * T > FS.held_tokens(nv, nwg)                                  # something is streamed
    # both kinds streamed where the pattern has both
    for B, pattern in ((64, "alternating"), (1024, "leading"), (65, "trailing"), (63, "alternating")):
        T = FS.row_mapping_T(B, pattern, 12, nwg)
        V = sum(FS.pattern_lengths(pattern, B, T))
        assert V > FS.held_tokens(12, nwg) and B * T > V
    assert FS.row_mapping_T(64, "full", 3, nwg) is None                                 # NV = 3 holds every token of a full grid
    assert not FS.eligible(1025, 4, 768, nwg) and not FS.eligible(12, 2731, 768, nwg) and FS.eligible(1024, 32, 768, nwg)
    assert not FS.eligible(49, 4, 768, 1) and FS.eligible(48, 4, 768, 1)                # 192 nwg + 4 slots fall back


def test_exact_percentile_is_exact():
    for N in (2, 3, 8, 255, 4097, 16257, 32767, 32768):
        for f in (0.9, 0.5, 0.97):
            k = int(f * (N - 1))
            p = FS.exact_percentile(N, k)
            r = np.float32(p) * np.float32(N - 1)
            assert r == k and np.floor(r) == np.ceil(r)

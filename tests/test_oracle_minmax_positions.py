"""tests/_minmax_positions.py on the CPU: every index model equals a brute-force walk of the kernel's loops, the listed
shapes reach every class of every kernel (what they cannot reach is named, with the reason), the expected values known by
construction are the oracle's, and no case is vacuous: with the planted element removed the oracle's answer changes."""
import numpy as np
import pytest

import _minmax_positions as MP
from conftest import f32_bits

ITEMSIZES = (4, 2)


def word(v):
    return int(f32_bits(np.array([v], np.float32))[0])


# ----------------------------------------------------------------------------------- constants

def test_constants_restate_the_sources():
    """Each constant against the source line quoted beside it."""
    import os
    import re
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "outlier_suppression_amd", "csrc")
    obs = open(os.path.join(root, "observer.hip")).read()
    dev = open(os.path.join(root, "osq_device.h")).read()
    host = open(os.path.join(root, "osq_host.h")).read()
    assert "constexpr int kThreads = %d;" % MP.THREADS in obs and "#define OSQ_WAVE %d" % MP.WAVE in dev
    assert "OSQ_AB_KNOB(int, g_obs_blocks, %d);" % MP.OBS_BLOCKS in obs and "constexpr int kMaxBlocks = %d;" % MP.MAX_BLOCKS in host
    assert "constexpr int kTokPerWave = %d;" % MP.TOK_PER_WAVE in obs
    assert "constexpr int kWavesPerBlock = kThreads / OSQ_WAVE;" in obs and MP.WAVES == MP.THREADS // MP.WAVE
    assert "constexpr int kTokPerBlock = kTokPerWave * kWavesPerBlock;" in obs and MP.TOK_PER_BLOCK == MP.TOK_PER_WAVE * MP.WAVES
    assert "constexpr int kPer = kMaxBlocks / kThreads;" in obs and MP.FINISH_PER == MP.MAX_BLOCKS // MP.THREADS
    fused = open(os.path.join(root, "fused_step.h")).read()
    assert "constexpr int kFusedThreads = %d;" % MP.FUSED_THREADS in fused and "constexpr int kFusedWaves = kFusedThreads / OSQ_WAVE;" in fused
    assert "constexpr int kFusedHoldRegs = %d;" % MP.FUSED_HOLD_REGS in fused and "constexpr int kFusedHoldLds = %d;" % MP.FUSED_HOLD_LDS in fused
    # what tests/test_gpu_minmax_positions.py derives its LDS-held and streamed tokens from: the split of a wave's tokens, the
    # enumeration k * nwv + wave * G + workgroup, 16 G streaming waves, and a grid of one workgroup per CU
    assert "constexpr int SR = kFusedHoldRegs / NV;" in fused and "constexpr int SL = kFusedHoldLds / NV;" in fused
    assert "const unsigned int nwv = (gridDim.x - 2u) * kFusedWaves;" in fused and "const unsigned int nwg = gridDim.x - 2u;" in fused
    assert "const unsigned int gwi = static_cast<unsigned int>(wv) * nwg + bp;" in fused
    assert "#define OSQ_FUSED_TOKEN(k) (static_cast<unsigned int>(k) * nwv + gwi)" in fused
    assert "hipDeviceAttributeMultiprocessorCount" in obs and "    return cus[dev];\n}\nstatic int fused_grid_for" in obs
    assert "for (; i + 3 * stride < ng; i += 4 * stride)" in obs and "kThreads * 4, g_obs_blocks" in obs
    assert "for (; j + 2 * OSQ_WAVE < inner_g; j += 3 * OSQ_WAVE)" in obs and obs.count("j += 3 * OSQ_WAVE") == 3
    assert "grid_for(channels, kWavesPerBlock, kMaxBlocks * 4)" in obs and obs.count("kWavesPerBlock, kMaxBlocks * 8)") == 2
    assert "while ((1 << lgG) < inner_g && lgG < 6) ++lgG;" in obs
    per = [int(v) for v in re.findall(r"static constexpr int kPer = (\d+);", dev)]
    loads = [int(v) for v in re.findall(r"static constexpr int kRowLoads = (\d+);", dev)]
    assert per == [MP.GRANULE[2], MP.GRANULE[4]] and loads == [MP.ROW_LOADS[2], MP.ROW_LOADS[4]]
    assert MP.grid_for(0, 4) == 1 and MP.grid_for(5, 4) == 2 and MP.grid_for(10 ** 9, 4, 7) == 7
    assert [MP.lg_group(g) for g in MP.TOKEN_HEAD_INNER_G] == [0, 1, 2, 2, 4, 6, 6]


# ----------------------------------------------------------------------------------- observe_flat_kernel

@pytest.fixture(scope="module", params=ITEMSIZES)
def flat_tables(request):
    isz = request.param
    per = MP.GRANULE[isz]
    out = []
    for name, size, aligned in MP.FLAT_SIZES:
        n = size(per)
        table = MP.flat_model(n, isz, aligned)
        out.append((name, n, aligned, table, MP.flat_representatives(n, isz, aligned, table=table)))
    return isz, out


def test_flat_model_equals_the_walker(flat_tables):
    isz, tables = flat_tables
    for name, n, aligned, table, reps in tables:
        assert np.array_equal(table, MP.flat_walk(n, isz, aligned)), name
        for idx, cls in reps:
            assert MP.flat_class_of(idx, n, isz, aligned) == cls, (name, idx)


def test_flat_shapes_reach_every_class(flat_tables):
    """Nothing is unreachable for the flat kernel on the release grid: the misaligned case takes the scalar loop through every
    workgroup class, the capped cases the unrolled body's second trip and all three remainder trips."""
    isz, tables = flat_tables
    got = set()
    for name, n, aligned, table, reps in tables:
        got |= MP.flat_classes(reps)
        assert len(reps) <= 120, (name, len(reps))                 # times the kinds: several hundred launches per size at most
    want = MP.flat_all_classes(isz)
    assert got == want, (sorted(want - got, key=str), sorted(got - want, key=str))


def test_flat_knob_sizes_reach_later_trips_on_small_grids():
    for isz in ITEMSIZES:
        per = MP.GRANULE[isz]
        for blocks in (1, 2, 3):
            got = set()
            for n in MP.flat_knob_sizes(blocks, per):
                assert n < 65536                                   # a few thousand granules
                table = MP.flat_model(n, isz, True, blocks)
                assert np.array_equal(table, MP.flat_walk(n, isz, True, blocks))
                got |= {p for p, _, _ in MP.flat_classes(MP.flat_representatives(n, isz, True, blocks, table))}
            assert {"body2+a", "body2+d", "rem1", "rem2", "rem3", "tail1"} <= got, (blocks, got)
        n, = MP.flat_knob_sizes(MP.MAX_BLOCKS, per)
        assert MP.flat_geometry(n, isz, True, MP.MAX_BLOCKS)[2] == MP.MAX_BLOCKS
        wgs = {v for _, a, v in MP.flat_classes(MP.flat_representatives(n, isz, True, MP.MAX_BLOCKS)) if a == "wg"}
        assert {str(m * 256 + d) for m in range(1, 8) for d in (-1, 0, 1)} <= wgs, wgs


def test_flat_construction_oracle_and_dropped_element(flat_tables):
    """Every (representative pair, kind) of every size: the expected pair known by construction is the oracle's, and removing
    the planted maximum (minimum) changes the oracle's maximum (minimum) word.  Small sizes: the oracle runs over the whole
    planted array.  Large sizes (millions of elements, hundreds of pairs): min and max are associative, so the oracle runs
    over [min of the rest, max of the rest, the planted values], the rest being the array without the two planted places; its
    ends come from the three smallest and three largest elements of the base, found once per sign and held against the
    oracle's pass over the whole base."""
    isz, tables = flat_tables
    kinds = MP.kinds_for(isz)
    for name, n, aligned, table, reps in tables:
        base = MP.flat_base(n, MP.case_seed(name))
        pairs = MP.flat_pairs(reps)
        large = name in MP.FLAT_LARGE
        if large:
            signed = {s: MP.signed_base(base, s) for s in (0, 1, -1)}
            ends = {s: MP.flat_ends(signed[s]) for s in signed}
            for s in signed:
                want = MP.expected_pair(signed[s])
                got = MP.flat_rest_pair(signed[s], ends[s], ())
                assert (word(got[0]), word(got[1])) == (word(want[0]), word(want[1])), (name, s)
        for imax, imin in pairs:
            cls = (MP.flat_class_of(imax, n, isz, aligned), None if imin is None else MP.flat_class_of(imin, n, isz, aligned))
            for kind in kinds:
                kname, sign, vmax, vmin = kind
                two = imin is not None and vmin is not None
                if large:
                    assert imin is not None
                    rest = list(MP.flat_rest_pair(signed[sign], ends[sign], (imax, imin) if two else (imax,)))
                    emin, emax = (np.float32(np.nan),) * 2 if kname == "nan" else ((vmin, vmax) if two else (None, vmax))
                    planted = [vmax] + ([vmin] if two else [])
                    omin, omax = MP.expected_pair(np.array(rest + planted, np.float32))
                    dmax = MP.expected_pair(np.array(rest + planted[1:], np.float32))[1]
                    dmin = MP.expected_pair(np.array(rest + planted[:1], np.float32))[0]
                    if emin is None:
                        emin = omin
                else:
                    x, emin, emax = MP.plant_flat(base, kind, imax, imin)
                    omin, omax = MP.expected_pair(x)
                    if n > 1:
                        dmax = MP.expected_pair(np.delete(x, imax))[1]
                        dmin = MP.expected_pair(np.delete(x, imin))[0] if two else None
                assert (word(omin), word(omax)) == (word(emin), word(emax)), (name, kname, cls)
                if n == 1:
                    continue
                assert word(dmax) != word(emax), (name, kname, "max", cls[0])
                if two:
                    assert word(dmin) != word(emin), (name, kname, "min", cls[1])


# ----------------------------------------------------------------------------------- the per-row kernels

def test_column_models_equal_their_walkers():
    for isz in ITEMSIZES:
        L = MP.ROW_LOADS[isz]
        for ig in set(MP.rows_inner_g(L)) | {2 * L * 64 + 130}:
            assert MP.column_parts(ig, L) == MP.column_parts_walk(ig, L), ig
    for ig in set(MP.TOKEN_SINGLE_INNER_G) | {577, 640}:
        assert MP.column_parts(ig, MP.TOK_STEP, "012") == MP.column_parts_walk(ig, MP.TOK_STEP, "012"), ig
    for inner in MP.CHANNELS_INNER:
        for outer in MP.CHANNELS_OUTER:
            walk = MP.channels_column_walk(outer, inner)
            assert len(walk) == outer * inner
            for (o, j), (trip, t) in walk.items():
                p = "trip%s" % ("1" if trip == 0 else ("2" if trip == 1 else "3+"))
                want = {(p, "lane", MP.edge(t % 64, 64)), (p, "wave", t // 64), (p, "outer", MP.edge(o, outer))}
                assert MP.channels_column_class(o, j, outer, inner) == want
    for ig in MP.TOKEN_HEAD_INNER_G:
        for fo in MP.head_feat_outers(ig):
            walk = MP.head_walk(fo, ig)
            assert len(walk) == fo * ig                              # every granule read, by exactly one lane
            for (o, g), (lane, ot, jt) in walk.items():
                lg, mlane, part, grp, li = MP.head_column(o, g, fo, ig)
                assert (mlane, part) == (lane, "seg%s_g%s" % (MP.trip_name(ot), MP.trip_name(jt))), (ig, fo, o, g)


def test_row_and_token_slot_models_equal_their_walkers():
    for rows in MP.ROWS_COUNTS + (MP.ROWS_TRIP2,):
        grid = MP.grid_for(rows, MP.WAVES, MP.ROWS_CAP)
        seen = {}
        for wg in range(grid):                                   # for (r = wave; r < rows; r += nwaves)
            for w in range(MP.WAVES):
                r, trip = wg * MP.WAVES + w, 0
                while r < rows:
                    seen[r] = {("row", "wave", w), ("row", "wg", MP.edge(wg, grid)), ("row", "trip", MP.trip_name(trip))}
                    r += grid * MP.WAVES
                    trip += 1
        assert len(seen) == rows
        step = 1 if rows < 100 else 997
        assert all(seen[r] == MP.rows_row_class(r, rows) for r in list(range(0, rows, step)) + [rows - 1])
    for _, kind, lengths, T, fo, fi in MP.token_cases(4):
        walk = MP.token_slot_walk(lengths, T)
        assert sorted(walk) == [(b, t) for b, l in enumerate(lengths) for t in range(min(l, T))]     # every valid token stored once, no padded one
        chunks = (T + 15) // 16
        for (b, t), (k, ntok, w, chunk, bx) in walk.items():
            want = {("tok", "slot", (k, ntok)), ("tok", "wave", w), ("tok", "chunk", MP.edge(chunk, chunks)), ("tok", "rotated", bx != chunk)}
            assert MP.token_slot_class(b, t, min(lengths[b], T), T) == want


@pytest.fixture(scope="module", params=ITEMSIZES)
def row_runs(request):
    """Every launch of every per-row case, planted once and shared by the tests below."""
    isz = request.param
    kinds = MP.kinds_for(isz)
    return isz, kinds, [(c, list(MP.case_launches(c, kinds))) for c in MP.row_cases(isz)]


def test_row_cases_reach_every_class_with_every_kind(row_runs):
    """Per kernel: the union over its cases of the classes of the columns that held a planted maximum and of those that held a
    planted minimum is the kernel's full class list, and every kind met every STAGE -- each (axis, value): granule element, lane class, wave, outer index -- as a maximum.  Token kernels: every slot
    class (k, ntok), wave, chunk position and rotation has a valid token, and every loop part met every slot k."""
    isz, kinds, runs = row_runs
    reached = {}
    for case, launches in runs:
        cols = MP.column_classes(case, isz)
        rows = np.flatnonzero(case["valid"])
        r = reached.setdefault(case["kernel"], dict(max=set(), min=set(), kind=set(), slot=set(), part_slot=set(), row=set()))
        for x, emin, emax, cmax, cmin, kidx in launches:
            for c in np.unique(cmax[rows]):
                r["max"] |= cols[c]
            for c in np.unique(cmin[rows]):
                r["min"] |= cols[c]
            if "shifts" not in case:
                for c, k in set(zip(cmax[rows].tolist(), kidx[rows].tolist())):
                    r["kind"] |= {(kinds[k][0],) + cl[1:] for cl in cols[c]}
            if case["kernel"] in ("single", "head"):
                T = case["T"]
                for row in rows:
                    b, t = divmod(int(row), T)
                    sc = MP.token_slot_class(b, t, min(case["lengths"][b], T), T)
                    r["slot"] |= sc
                    r["part_slot"] |= {(cl[0], t % 4) for cl in cols[cmax[row]]}
        if case["kernel"] == "rows":
            for row in (0, case["R"] // 2, case["R"] - 1, min(case["R"] - 1, 5)):
                r["row"] |= MP.rows_row_class(row, case["R"])
    want = {"rows": MP.rows_all_classes(isz) - {c for c in MP.rows_all_classes(isz) if c[0] == "row"}, "channels": MP.channels_all_classes(),
            "single": MP.single_all_classes(isz)}
    for kernel, full in want.items():
        for side in ("max", "min"):
            assert reached[kernel][side] == full, (kernel, side, sorted(full - reached[kernel][side], key=str), sorted(reached[kernel][side] - full, key=str))
        missing = {(k[0],) + cl[1:] for k in kinds for cl in full} - reached[kernel]["kind"]
        assert not missing, (kernel, sorted(missing, key=str)[:12], len(missing))
    assert reached["rows"]["row"] == {c for c in MP.rows_all_classes(isz) if c[0] == "row"}
    # head split: every lgG 0..6 with a first and a later segment trip, a second granule trip where inner_g exceeds the group
    # (lgG = 6, inner_g = 65), first / last / interior groups and lanes-in-group wherever the group count allows them
    head = reached["head"]["max"]
    assert {v for p, a, v in head if a == "lgG"} == {0, 1, 2, 4, 6}, "lgG 3 and 5 need inner_g 5..8 / 17..32: not in the listed sizes"
    for lg in (0, 1, 2, 4, 6):
        parts = {p for p, a, v in head if a == "lgG" and v == lg}
        assert {"seg1_g1", "seg2+_g1"} <= parts, (lg, parts)
    assert {"seg1_g2+", "seg2+_g2+"} <= {p for p, a, v in head if a == "lgG" and v == 6}
    assert {("head", "elem", e) for e in range(MP.GRANULE[isz])} <= head
    for axis in ("grp", "li", "lane"):
        assert {v for p, a, v in head if a == axis} == {"first", "last", "mid"}, axis
    assert reached["head"]["min"] == head
    for kernel in ("head", "generic"):                      # every kind met every stage these kernels have, as the three above
        stages = {cl[1:] for cl in reached[kernel]["max"]}
        missing = {(k[0],) + st for k in kinds for st in stages} - reached[kernel]["kind"]
        assert not missing, (kernel, sorted(missing, key=str)[:12], len(missing))
    assert {cl[0] for cl in reached["generic"]["max"]} == {"trip1", "trip2", "trip3+"}
    assert {v for p, a, v in reached["generic"]["max"] if a == "lane"} == {"first", "last", "mid"}
    for kernel in ("single", "head"):
        assert reached[kernel]["slot"] == MP.token_all_slot_classes(), (kernel, MP.token_all_slot_classes() - reached[kernel]["slot"])
        parts = {p for p, _ in reached[kernel]["part_slot"]}
        assert reached[kernel]["part_slot"] == {(p, k) for p in parts for k in range(4)}, kernel


def test_row_construction_oracle_and_dropped_element(row_runs):
    isz, kinds, runs = row_runs
    for case, launches in runs:
        v = case["valid"]
        for x, emin, emax, cmax, cmin, kidx in launches:
            omin, omax = MP.oracle_rows(x[v])
            assert np.array_equal(f32_bits(omin), f32_bits(emin[v])) and np.array_equal(f32_bits(omax), f32_bits(emax[v])), case["name"]
            assert not MP.dropped_rows_unchanged(x, emin, emax, cmax, cmin, v), case["name"]
            pad = x[~v]
            assert (np.isnan(pad) | (np.abs(pad) >= 1e30)).all()                  # padding holds only values that would show


def test_multi_planted_columns_reach_every_loop_part():
    """The loop parts of token_minmax_multi_kernel that hold a planted maximum, and those that hold a planted minimum, over the
    table launches tests/test_gpu_minmax_positions.py::test_multi_site_table runs: all of them, for both vector loops and
    the scalar loop."""
    kinds = MP.kinds_for(4)
    cases = [c for c in MP.row_cases(4) if c["kernel"] in ("single", "head", "generic") and "shifts" not in c]
    runs = [list(MP.case_launches(c, kinds)) for c in cases]
    got = {"max": set(), "min": set()}
    for l in range(MP.multi_launch_count(runs)):
        for c, launches in zip(cases, runs):
            parts = MP.multi_column_parts(c["kernel"] != "generic", c["feat_outer"], c["feat_inner"])
            assert len(parts) == c["F"]
            _, _, _, cmax, cmin, _ = launches[l % len(launches)]
            rows = np.flatnonzero(c["valid"])
            got["max"] |= {parts[j] for j in cmax[rows]}
            got["min"] |= {parts[j] for j in cmin[rows]}
    assert got["max"] == MP.multi_all_parts() and got["min"] == MP.multi_all_parts(), \
        (MP.multi_all_parts() - got["max"], MP.multi_all_parts() - got["min"])

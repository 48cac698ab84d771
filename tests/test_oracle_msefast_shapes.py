"""tests/_msefast_shapes.py on the CPU: the constants and threshold expressions still stand in the launchers, the predictors
equal a walk of the kernels' loops, the case tables reach every instantiation and loop part (each assertion lists what was
reached), every planted element decides the oracle's search, and the two lane widths of the row order can be told apart."""
import os

import numpy as np
import pytest

import _msefast_shapes as MS
from conftest import f32_bits
from oracle import observer_oracle as OB

F32 = np.float32
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "outlier_suppression_amd", "csrc")


def scheme(table, name):
    return next((b, s) for n, b, s in table if n == name)


# ----------------------------------------------------------------------------------- constants, launcher text

def test_constants_and_thresholds_restate_the_launchers():
    """A plain text search: a threshold that moves breaks this test before it silently moves a boundary out of the GPU cases."""
    hip = open(os.path.join(CSRC, "msefast.hip")).read()
    host = open(os.path.join(CSRC, "osq_host.h")).read()
    dev = open(os.path.join(CSRC, "osq_device.h")).read()
    assert "#define OSQ_WAVE %d" % MS.WAVE in dev
    assert "constexpr int kThreads = %d;" % MS.THREADS in hip and "constexpr int kWavesPerBlock = kThreads / OSQ_WAVE;" in hip
    assert MS.ROW_WAVES == MS.THREADS // MS.WAVE
    assert "constexpr int kMaxBlocks = %d;" % MS.MAX_BLOCKS in host
    assert "constexpr int kResidentMaxSites = %d;" % MS.RES_MAX_SITES in host
    assert "constexpr int kResidentMaxBlocks = %d;" % MS.RES_MAX_BLOCKS in host
    assert ("int64_t b = (work_items + per_block - 1) / per_block;\n    if (b < 1) b = 1;\n    if (b > max_blocks) b = max_blocks;") in host
    # rows
    rows = hip[hip.index('extern "C" int osq_msefast_rows('):hip.index('extern "C" int osq_msefast_tensor_begin(')]
    for text in ("const int grid = static_cast<int>((rows + kWavesPerBlock - 1) / kWavesPerBlock);",
                 "const bool forced = g_mse_sum_order == 8 || g_mse_sum_order == 16;",
                 "const int order = forced ? g_mse_sum_order : g_mse_rows_order;",
                 "if (order && cols > 64 * 48 && cols < 32768) {",
                 "hipFuncAttributeMaxDynamicSharedMemorySize, 32768 * 4)",
                 "dim3(static_cast<unsigned int>(rows)), dim3(OSQ_WAVE), static_cast<size_t>(c) * sizeof(float)",
                 "if (forced && cols >= 32768) return OSQ_ERR_UNSUPPORTED;",
                 "if (order && cols <= 64 * 48) {",
                 "if (cols <= 64 * 4) OSQ_ROWS_ATEN(4);", "else if (cols <= 64 * 16) OSQ_ROWS_ATEN(16);", "else OSQ_ROWS_ATEN(48);",
                 "if (cols <= 64 * 4) OSQ_ROWS(4);", "else if (cols <= 64 * 16) OSQ_ROWS(16);", "else if (cols <= 64 * 48) OSQ_ROWS(48);",
                 "else OSQ_ROWS(0);"):
        assert text in rows, text
    assert MS.ROW_MAXV == (4, 16, 48) and MS.ROW_LONG_MAX == 32768 - 1 and MS.ROW_FALLBACK == 32768
    assert "cols >= sum_width ? aten_mean_wave(sq, cols, sum_width) : aten_sum_short(sq, cols) / static_cast<float>(cols)" in hip
    assert "const int j = lane + k * OSQ_WAVE;" in hip and "for (int j = lane; j < cols; j += OSQ_WAVE)" in hip
    # streaming flat
    for text in ("const int grid = grid_for(n4, kThreads * 2, kMaxBlocks);",
                 "const int64_t stride = static_cast<int64_t>(gridDim.x) * kThreads;",
                 "i < n4; i += 2 * stride) {", "const bool two = (i + stride) < n4;",
                 "if (blockIdx.x == 0 && static_cast<int>(threadIdx.x) < tail)",
                 "n4, x + n4 * 4, static_cast<int>(n - n4 * 4), n,"):
        assert text in hip, text
    # streaming tokens
    for text in ("const int grid = grid_for(v.batch * v.tokens, kWavesPerBlock, kMaxBlocks);",
                 "const int vec = v.stride_inner == 1 && v.feat_inner % 4 == 0 && aligned16(x) && v.stride_batch % 4 == 0 &&\n"
                 "                    v.stride_token % 4 == 0 && (v.feat_outer == 1 || v.stride_outer % 4 == 0);",
                 "const int64_t nwaves = static_cast<int64_t>(gridDim.x) * kWavesPerBlock;",
                 "for (int64_t tok = wave0; tok < ntok; tok += nwaves) {", "if (lengths && t >= lengths[b]) continue;"):
        assert text in hip, text
    # resident
    for text in ("constexpr int kResThreads = %d;" % MS.RES_THREADS, "constexpr int kResStage = %d;" % MS.RES_STAGE,
                 "constexpr int kResMaxSlots = %d;" % MS.RES_MAX_SLOTS, "constexpr int kResMaxBatch = kResThreads;",
                 "const int64_t per_k = static_cast<int64_t>(grid) * kResThreads * 4;",
                 "const int64_t need = (elems + per_k - 1) / per_k;", "if (need > kResMaxSlots) return OSQ_ERR_UNSUPPORTED;",
                 "if (v.batch > kResMaxBatch) return OSQ_ERR_UNSUPPORTED;",
                 "for (int c0 = 0; c0 < slots; c0 += kResStage) {",
                 "constexpr int KR = KT > 24 ? 24 : KT, KL = KT - KR;",
                 "if (slot > kResMaxSlots) return OSQ_ERR_UNSUPPORTED;",
                 "if (!g_mse_resident || g_mse_sum_order != 0 || n_sites > kResidentMaxSites) return OSQ_ERR_UNSUPPORTED;"):
        assert text in hip, text
    assert MS.RES_MAX_BATCH == MS.RES_THREADS and MS.RES_MULTI_REG_SLOTS == 24
    ladder = ["if (need <= %d) OSQ_RESIDENT(%d);" % (MS.RES_LADDER[0], MS.RES_LADDER[0])]
    ladder += ["else if (need <= %d) OSQ_RESIDENT(%d);" % (k, k) for k in MS.RES_LADDER[1:-1]] + ["else OSQ_RESIDENT(%d);" % MS.RES_LADDER[-1]]
    multi = ["if (slot <= %d) OSQ_RESIDENT_MULTI(%d);" % (MS.RES_MULTI_LADDER[0], MS.RES_MULTI_LADDER[0])]
    multi += ["else if (slot <= %d) OSQ_RESIDENT_MULTI(%d);" % (k, k) for k in MS.RES_MULTI_LADDER[1:-1]] + ["else OSQ_RESIDENT_MULTI(%d);" % MS.RES_MULTI_LADDER[-1]]
    assert "\n    ".join(ladder) in hip and "\n    ".join(multi) in hip
    assert hip.count("OSQ_RESIDENT(") == len(MS.RES_LADDER) + 1 and hip.count("OSQ_RESIDENT_MULTI(") == len(MS.RES_MULTI_LADDER) + 1


# ----------------------------------------------------------------------------------- predictors against a walk of the loops

def walk_flat(n):
    """msefast_flat_loss_kernel's loop, thread by thread: parts reached and how often each element is added."""
    n4, tail = n // 4, n % 4
    grid = MS.grid_for(n4, MS.THREADS * 2)
    stride = grid * MS.THREADS
    seen, parts = np.zeros(n, dtype=np.int64), set()
    for t in range(stride):
        i, trip = t, 0
        while i < n4:
            two = i + stride < n4
            parts.add("pair" if two else "single")
            if trip:
                parts.add("second trip")
            seen[4 * i:4 * i + 4] += 1
            if two:
                seen[4 * (i + stride):4 * (i + stride) + 4] += 1
            i, trip = i + 2 * stride, trip + 1
    if tail:
        parts.add("tail%d" % tail)
        seen[4 * n4:] += 1
    return grid, parts, seen


def test_flat_predictor_equals_a_walk_of_the_loop():
    for n in [n for n in MS.FLAT_LENGTHS] + [1024, 2048, 2052, 4096, 4100, 8191]:
        grid, parts, seen = walk_flat(n)
        assert (grid, parts) == MS.predict_flat(n), n
        assert (seen == 1).all(), n
    # the capped grid: the walk of one thread column is the walk of all (every thread of a trip takes the same branch but
    # those round n4 % stride)
    n = MS.FLAT_BIG
    grid, parts = MS.predict_flat(n)
    n4, stride = n // 4, grid * MS.THREADS
    assert grid == MS.MAX_BLOCKS and stride == MS.flat_stride(n) and n4 == 2 * stride + 300
    assert parts == {"pair", "single", "second trip", "tail3"}


def test_row_predictor():
    assert MS.predict_rows(256) == ("ordered", 4, False) and MS.predict_rows(257) == ("ordered", 16, False)
    assert MS.predict_rows(1024) == ("ordered", 16, False) and MS.predict_rows(1025) == ("ordered", 48, False)
    assert MS.predict_rows(3072) == ("ordered", 48, False) and MS.predict_rows(3073) == ("ordered-long", 0, False)
    assert MS.predict_rows(32767) == ("ordered-long", 0, False) and MS.predict_rows(32768) == ("order-free", 0, False)
    assert MS.predict_rows(32768, 8, 8) == ("unsupported", None, False) and MS.predict_rows(32767, 0, 16) == ("ordered-long", 0, False)
    assert MS.predict_rows(7) == ("ordered", 4, True) and MS.predict_rows(8) == ("ordered", 4, False)
    assert MS.predict_rows(15, 16) == ("ordered", 4, True) and MS.predict_rows(16, 16) == ("ordered", 4, False)
    assert MS.predict_rows(3073, 0) == ("order-free", 0, False) and MS.predict_rows(7, 0) == ("order-free", 4, False)


# ----------------------------------------------------------------------------------- coverage of the case tables

def test_row_cases_reach_every_instantiation():
    forms = {}
    for cols, order, _ in MS.row_units():
        forms.setdefault(MS.predict_rows(cols, order), []).append(cols)
    inst = {(f[0] != "order-free", f[1]) for f in forms}
    print("rows instantiations (ordered, MAXV):", sorted(inst))
    assert inst == {(o, m) for o in (True, False) for m in (4, 16, 48, 0)}                       # 8 instantiations
    short = {order for cols, order, _ in MS.row_units() if MS.predict_rows(cols, order)[2]}
    print("short paths at widths:", sorted(short))
    assert short == {8, 16}                                                                   # 2 short paths
    assert {c for c in MS.ROW_COLS if MS.predict_rows(c, 16)[2] and not MS.predict_rows(c, 8)[2]} == set(range(8, 16))
    # every threshold as a pair, the longest row of the long form, a partly filled last workgroup
    for a in (256, 1024, 3072, 32767):
        assert a in MS.ROW_COLS and a + 1 in MS.ROW_COLS and MS.predict_rows(a) != MS.predict_rows(a + 1)
    assert all(r % MS.ROW_WAVES for r in (1, 3, 5)) and set(MS.row_counts(257)) == {1, 3, 4, 5} and set(MS.row_counts(32767)) == {1, 2}
    planted = {MS.predict_rows(c, o)[:2] for c, o, _ in MS.row_planted_units()}
    assert {(f != "order-free", m) for f, m in planted} == inst
    for cols in MS.ROW_PLANTED_COLS:
        for order in MS.ROW_ORDERS:
            pos = MS.row_positions(cols, order)
            assert pos[0] == 0 and pos[-1] == cols - 1 and all(64 * m - 1 in pos for m in MS.ROW_MAXV if 64 * m <= cols)


def test_flat_cases_reach_every_loop_part():
    reached = set()
    for n in MS.FLAT_LENGTHS + (MS.FLAT_BIG,):
        reached |= MS.predict_flat(n)[1]
    print("flat loop parts:", sorted(reached))
    assert reached == {"pair", "single", "second trip", "tail1", "tail2", "tail3"}
    assert {"pair", "single"} <= MS.predict_flat(MS.FLAT_SINGLE_AND_PAIR)[1]
    s = MS.flat_stride(MS.FLAT_SINGLE_AND_PAIR)
    assert s < MS.FLAT_SINGLE_AND_PAIR // 4 < 2 * s
    assert MS.predict_flat(MS.FLAT_BIG)[0] == MS.MAX_BLOCKS and "second trip" in MS.predict_flat(MS.FLAT_BIG)[1]
    assert {n % 4 for n in MS.FLAT_PLANTED_LENGTHS} == {0, 1, 2, 3}
    planted = set()
    for n in MS.FLAT_PLANTED_LENGTHS:
        pos, s = MS.flat_planted_positions(n), MS.flat_stride(n)
        assert n - 1 in pos
        planted |= {("first", 0 in pos), ("4s", 4 * s in pos and 4 * s - 1 in MS.flat_positions(n)), ("8s", 8 * s in pos and 8 * s - 1 in pos)}
    assert {("first", True), ("4s", True), ("8s", True)} <= planted
    assert sum(n > 300000 for n in MS.FLAT_LENGTHS + (MS.FLAT_BIG,)) == 1


def test_token_cases_reach_both_load_forms_and_both_trip_counts():
    reached = set()
    for name, case in MS.TOKEN_CASES.items():
        vec, grid, parts = MS.predict_tokens(case.geometry())
        reached.add(("vector" if vec else "scalar", "second trip" if parts else "one trip"))
        T = case.view(case.mem()).shape[case.seq_pos]
        assert 0 in case.lengths and T in case.lengths and case.lengths.max() > T, name
        b, t, _ = case.last_valid()
        assert 0 <= t < T - 1, name                                    # a padded token follows the last valid one
    print("token forms:", sorted(reached))
    assert reached == {(a, b) for a in ("vector", "scalar") for b in ("one trip", "second trip")}           # 2 x 2 forms
    geo = {n: MS.predict_tokens(c.geometry()) for n, c in MS.TOKEN_CASES.items()}
    assert [geo[n][0] for n in ("dense_F4", "dense_F6", "dense_F64", "dense_F68", "head_split", "key_view")] == [True, False, True, True, True, False]
    assert MS.TOKEN_CASES["head_split"].geometry()["feat_outer"] == 3 and MS.TOKEN_CASES["key_view"].geometry()["stride_inner"] != 1
    assert MS.TOKEN_CASES["zip_3d"].geometry()["batch"] == 4 < 12
    g = MS.TOKEN_CASES["grid_cap"].geometry()
    assert g["batch"] * g["tokens"] == 8192 + 5 and geo["grid_cap"][1] == MS.MAX_BLOCKS
    assert geo["grid_cap_F6"] == (False, MS.MAX_BLOCKS, {"second trip"})


def test_resident_cases_reach_every_k():
    per_k = MS.NOMINAL_PER_K
    sizes = MS.resident_sizes(per_k)
    reached = {}
    for k, ns in sizes.items():
        for n in ns:
            assert MS.predict_resident(n, per_k) == k, (k, n)
            reached.setdefault(k, []).append(n)
    print("resident K:", sorted(reached))
    assert sorted(reached) == list(MS.RES_LADDER)                                              # 7 forms
    assert MS.predict_resident(32 * per_k + 1, per_k) == 0
    # every boundary of the position list is planted under some K, once from either side
    planted = set()
    for (kp, k) in zip((0,) + MS.RES_LADDER, MS.RES_LADDER):
        for n in sizes[k]:
            planted |= set(MS.resident_planted_positions(n, per_k, kp))
    for k in (1, 2, 4, 8, 16, 24):
        assert k * per_k - 1 in planted and k * per_k in planted, k
    kts, lds = {}, {}
    for name, slots in MS.MULTI_GROUPS.items():
        kt, in_lds = MS.predict_resident_multi(slots)
        kts.setdefault(kt, []).append(name)
        lds[name] = in_lds
    print("multi-site KT:", {k: v for k, v in sorted(kts.items())}, "LDS sites:", {k: v for k, v in lds.items() if v})
    assert sorted(kts) == list(MS.RES_MULTI_LADDER)                                            # 4 forms
    assert [sum(MS.MULTI_GROUPS[n]) for n in ("sum8", "sum9", "sum16", "sum17", "sum24", "sum25_straddle", "sum32_lds_site")] == [8, 9, 16, 17, 24, 25, 32]
    assert lds["sum25_straddle"] == (1,) and sum(MS.MULTI_GROUPS["sum25_straddle"][:1]) == 23   # slots 23 and 24
    assert lds["sum32_lds_site"] == (2,) and sum(MS.MULTI_GROUPS["sum32_lds_site"][:2]) == 24   # wholly in 24 .. 31
    assert len(lds["sixteen_twos"]) == 4 and lds["sixteen_ones"] == ()
    assert all(MS.predict_resident_multi(s) == (0, ()) for s in MS.MULTI_REJECTED.values())
    assert len(MS.MULTI_REJECTED["seventeen_sites"]) == 17 and sum(MS.MULTI_REJECTED["sum33"]) == 33
    # a site's slots: multi_site_elems stays inside them
    for slots in (1, 2, 9, 23):
        for i in range(3):
            assert MS.ceil_div(MS.multi_site_elems(slots, i, per_k), per_k) == slots


# ----------------------------------------------------------------------------------- sensitivity: a planted element decides

def test_every_planted_row_element_decides_the_search():
    worst = (np.inf, None)
    for cols, order, name in MS.row_planted_units():
        bit, sym = scheme(MS.ROW_SCHEMES, name)
        for p, w in MS.row_planted_cases(cols, order):
            st = MS.scheme_state(bit, sym, w, 0)
            for r in (0, -1):
                ratio = MS.decides(w[r], p, st, MS.row_vec(order))
                worst = min(worst, (ratio, (cols, order, name, p, r)))
                assert ratio >= 1.5, (cols, order, name, p, r, ratio)
    print("smallest decides ratio, rows:", worst)


def test_every_planted_flat_element_decides_the_search():
    worst = (np.inf, None)
    for n in MS.FLAT_PLANTED_LENGTHS:
        for p, x in MS.planted(n, MS.flat_planted_positions(n), 1.0, MS.plant_value(n), 3):
            ratio = MS.decides(x, p, MS.scheme_state(6, True, x))
            worst = min(worst, (ratio, (n, p)))
            assert ratio >= 1.5, (n, p, ratio)
    print("smallest decides ratio, flat:", worst)


def token_planted(case):
    """(dense array with the element planted in the last valid token, its observed form, the element's flat index there)."""
    V = MS.plant_value(MS.token_observed(case).size)
    mem = case.mem()
    case.plant(mem, "valid", V)
    obs = MS.token_observed(case, mem)
    pos = np.flatnonzero(obs.reshape(-1) == F32(V))
    assert pos.size == 1 and pos[0] == obs.size - 1                 # the last feature of the last valid token
    return mem, obs, int(pos[0])


def test_every_planted_token_element_decides_the_search():
    worst = (np.inf, None)
    for name, case in MS.TOKEN_CASES.items():
        mem, obs, pos = token_planted(case)
        for _, bit, sym in MS.FLAT_SCHEMES:
            ratio = MS.decides(obs.reshape(-1), pos, MS.scheme_state(bit, sym, obs))
            worst = min(worst, (ratio, (name, sym)))
            assert ratio >= 1.5, (name, sym, ratio)
        # the padded plant is invisible to the reference: the observed values do not change
        mem2 = case.mem()
        case.plant(mem2, "padded", 1e4)
        assert (mem2 != case.mem()).sum() == 1 and np.array_equal(MS.token_observed(case, mem2), MS.token_observed(case))
    print("smallest decides ratio, tokens:", worst)


# ----------------------------------------------------------------------------------- the oracle on the row cases

def test_lane_widths_can_be_told_apart():
    """The oracle's row results on 8 and on 16 lanes differ in at least one word over the width-16 cases: a kernel that
    summed on eight lanes under "mse_rows_order" 16 could not pass them."""
    differing = []
    for cols in MS.ROW_COLS:
        if cols < 8 or cols >= MS.ROW_FALLBACK:
            continue
        w = MS.row_weights(cols)
        a, b = MS.oracle_rows(w, 4, True, 8), MS.oracle_rows(w, 4, True, 16)
        if not (np.array_equal(f32_bits(a[0]), f32_bits(b[0])) and np.array_equal(f32_bits(a[1]), f32_bits(b[1])) and np.array_equal(a[2], b[2])):
            differing.append(cols)
    print("column counts whose 8- and 16-lane results differ:", differing)
    assert differing
    assert any(8 <= c < 16 for c in differing), "the short path of the 16-lane order must be told from the 8-lane vector path"


def test_oracle_rows_is_observe_msefast():
    """oracle_rows (row by row, memoised) gives what one observe_msefast call on the whole tensor gives."""
    for w, bit, sym, vec in ((MS.row_weights(33), 4, True, 8), (MS.row_weights(257), 4, False, 16), (MS.degenerate_rows(), 4, True, None),
                             (np.abs(MS.row_weights(17)), 4, False, 8)):
        st = OB.ObserverState(bit=bit, symmetric=sym, ch_axis=0)
        counter = [0]
        old = OB.ROW_SUM_VEC
        OB.ROW_SUM_VEC = vec
        try:
            OB.observe_msefast(st, w, counter=counter)
        finally:
            OB.ROW_SUM_VEC = old
        mn, mx, nfev = MS.oracle_rows(w, bit, sym, vec)
        assert np.array_equal(f32_bits(mn), f32_bits(st.min_val)) and np.array_equal(f32_bits(mx), f32_bits(st.max_val))
        assert int(nfev.sum()) == counter[0]


def test_oracle_takes_the_degenerate_rows():
    w = MS.degenerate_rows()
    assert not w[1].any() and (w[2] == w[2, 0]).all() and w[2, 0] > 0 and (w[4] == w[4, 0]).all() and w[4, 0] < 0
    assert np.count_nonzero(w[5]) == 1
    for _, bit, sym in MS.ROW_SCHEMES:
        for vec in (8, 16, None):
            mn, mx, nfev = MS.oracle_rows(w, bit, sym, vec)
            assert np.isfinite(mn).all() and np.isfinite(mx).all() and (nfev > 0).all()


def test_planted_is_one_element():
    base = MS.normal(1027, 1.0, 3)
    for p, x in MS.planted(1027, (0, 1026), 1.0, 40.0, 3):
        assert x[p] == F32(40) and (x != base).sum() == 1
    assert MS.flat_positions(4 * 512 * 3 + 3) == (0, 3071, 3072, 6143, 6144, 6146)
    assert MS.resident_positions(3 * 100 + 1, 100) == (99, 100, 199, 200, 300)
    assert MS.row_positions(300, 16) == (0, 63, 64, 255, 256, 288, 299) and MS.row_positions(300, 0) == (0, 63, 64, 255, 299)

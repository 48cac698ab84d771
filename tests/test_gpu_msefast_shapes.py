"""The MSEFast searches of csrc/msefast.hip at every launch form and loop boundary (case tables, predictors and planted
elements: tests/_msefast_shapes.py, whose promises tests/test_oracle_msefast_shapes.py checks on the CPU).

Every comparison covers an observer's FIRST call: fp32 arithmetic, the mean rounded to fp32 once -- min_val and max_val
bit-equal, evaluation counts equal.

  a. msefast_rows_kernel<MAXV, ATEN> against the oracle: every column count round a form boundary and a lane-width edge under
     "mse_rows_order" 8, 16 and 0 (ROW_SUM_VEC 8, 16, None), 1 / 3 / 4 / 5 rows, a planted element in the first and the last row;
  b. the streaming flat form against the oracle: every tail, the `single` branch, the capped grid's second trip;
  c. the streaming token form against the oracle: vector and scalar loads, the views of the model, the grid cap;
  d. msefast_resident_kernel<K> at every K against the streaming form (which b and c pin to the oracle);
  e. msefast_resident_multi_kernel<KT> at every KT, site by site against the streaming form.
b and c also run the float64 second call under "mse_sum_order" 64 against the oracle's exact mean, bit for bit."""
import contextlib

import numpy as np
import pytest
import torch

import _msefast_shapes as MS
from conftest import bits_equal
from oracle import observer_oracle as OB

pytestmark = pytest.mark.gpu

F32 = np.float32
SWITCHES = ("mse_resident", "mse_rows_order", "mse_sum_order")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from outlier_suppression_amd import _hip
    _hip.load()          # fail loudly if the HIP library is missing
    return torch.device("cuda:0")


def shipped(key):
    from test_abi_and_host import SHIPPED_SWITCHES
    return SHIPPED_SWITCHES[key][1]


@pytest.fixture(autouse=True)
def switches_are_back_at_their_shipped_values():
    """After every test of this file, passed or failed."""
    yield
    from outlier_suppression_amd import ops
    assert {k: ops._tuning.get(k, shipped(k)) for k in SWITCHES} == {k: shipped(k) for k in SWITCHES}


@contextlib.contextmanager
def switches(**values):
    """osq_set_tuning for the duration; the shipped values afterwards, also after a failure."""
    from outlier_suppression_amd import ops
    try:
        for k, v in values.items():
            ops.set_tuning(k, v)
        yield
    finally:
        for k in values:
            ops.set_tuning(k, shipped(k))


def N(t):
    return t.detach().cpu().numpy()


def T(a, dev):
    return torch.from_numpy(np.array(a, order="C")).to(dev)          # a copy: the shared case arrays are read-only


def same_search(got, want):
    """(min, max, evaluations): words and counts."""
    return bits_equal(np.float64(got[0]), np.float64(want[0])) and bits_equal(np.float64(got[1]), np.float64(want[1])) and int(got[2]) == int(want[2])


# =========================================================================================== a. rows

def device_rows(w, bit, symmetric, side="no"):
    """side: the sidedness an observer decided on its first tensor (every row tensor of the tables is two-sided; a slice of
    one or two elements of it need not be)."""
    from outlier_suppression_amd import ops
    quant_min, quant_max = OB.quant_range(bit, symmetric)
    mn, mx, nfev = ops.msefast_rows(w, 0, quant_min, quant_max, symmetric, side, not (side != "no" or symmetric))
    return N(mn), N(mx), N(nfev)


def rows_equal(got, want, rows=None):
    rows = slice(None) if rows is None else rows
    return bits_equal(got[0], want[0][rows]) and bits_equal(got[1], want[1][rows]) and np.array_equal(got[2], want[2][rows])


@pytest.mark.parametrize("cols", MS.ROW_COLS)
def test_rows_equal_the_oracle(cols, dev):
    """One wave per row, four rows per workgroup: 1, 3, 4 and 5 rows (1 and 2 at the two longest lengths), every summation
    order, the 1-D and the nested search."""
    w = MS.row_weights(cols)
    assert OB.one_side_dist(w) == "no"
    wd = T(w, dev)
    fails = []
    for order in MS.ROW_ORDERS:
        with switches(mse_sum_order=0, mse_rows_order=order):
            for name, bit, sym in MS.ROW_SCHEMES:
                if name == "asym" and cols > MS.ROW_ASYM_MAX_COLS:
                    continue
                want = MS.oracle_rows(w, bit, sym, MS.row_vec(order))
                for rows in MS.row_counts(cols):
                    got = device_rows(wd[:rows], bit, sym)
                    if not rows_equal(got, want, slice(0, rows)):
                        fails.append((order, name, rows, MS.predict_rows(cols, order), got, [v[:rows] for v in want]))
    assert not fails, fails


@pytest.mark.parametrize("cols", MS.ROW_PLANTED_COLS)
def test_rows_with_a_planted_element_equal_the_oracle(cols, dev):
    """The element that decides the search (test_every_planted_row_element_decides_the_search) at columns 0, 63, 64,
    64 * MAXV - 1, cols - 1 and the first column of the ordered forms' tails, in the first and in the last row."""
    fails = []
    for order in MS.ROW_ORDERS:
        with switches(mse_sum_order=0, mse_rows_order=order):
            for name, bit, sym in MS.ROW_SCHEMES:
                if name == "asym" and cols not in MS.ROW_PLANTED_ASYM_COLS:
                    continue
                for p, w in MS.row_planted_cases(cols, order):
                    got = device_rows(T(w, dev), bit, sym)
                    want = MS.oracle_rows(w, bit, sym, MS.row_vec(order))
                    if not rows_equal(got, want):
                        fails.append((order, name, p, got, want))
    assert not fails, fails


def test_degenerate_rows_equal_the_oracle(dev):
    """An all-zero row, a constant positive row, a constant negative row and a row with one non-zero element beside normal rows."""
    w = MS.degenerate_rows()
    fails = []
    for order in MS.ROW_ORDERS:
        with switches(mse_sum_order=0, mse_rows_order=order):
            for name, bit, sym in MS.ROW_SCHEMES:
                got = device_rows(T(w, dev), bit, sym)
                want = MS.oracle_rows(w, bit, sym, MS.row_vec(order))
                if not rows_equal(got, want):
                    fails.append((order, name, got, want))
    assert not fails, fails


def test_rows_beyond_the_serial_grain_are_refused_under_the_strict_order(dev):
    """ "mse_sum_order" 8 and a row of 32768 columns: OSQ_ERR_UNSUPPORTED, the outputs untouched."""
    from outlier_suppression_amd import _hip
    lib = _hip.load()
    w = T(MS.row_weights(MS.ROW_FALLBACK), dev)
    rows = w.shape[0]
    mn = torch.full((rows,), 123.5, device=dev)
    mx = torch.full((rows,), -77.25, device=dev)
    nfev = torch.full((rows,), -9, dtype=torch.int32, device=dev)
    assert MS.predict_rows(MS.ROW_FALLBACK, 8, 8)[0] == "unsupported"
    with switches(mse_sum_order=8):
        rc = lib.osq_msefast_rows(_hip.ptr(w), rows, MS.ROW_FALLBACK, -8, 7, 1, 0, 0, _hip.ptr(mn), _hip.ptr(mx), _hip.ptr(nfev), _hip.stream_ptr(dev))
    torch.cuda.synchronize()
    assert rc == _hip.ERR_UNSUPPORTED
    assert (N(mn) == F32(123.5)).all() and (N(mx) == F32(-77.25)).all() and (N(nfev) == -9).all()


# =========================================================================================== b. / c. streaming forms through the observer

def observe(x, lengths, seq_pos, bit, symmetric, calls=1, grow=1.5):
    """[(min_val, max_val, evaluations)] after each call of a fresh MSEFastObserver; call k observes x * grow^k."""
    from outlier_suppression_amd.quantization.observer import MSEFastObserver
    ob = MSEFastObserver(bit=bit, symmetric=symmetric).to(x.device)
    out = []
    for k in range(calls):
        xi = x if k == 0 else x * float(F32(grow ** k))
        if lengths is None:
            ob(xi)
        else:
            ob(xi, lengths, seq_pos)
        out.append((float(N(ob.min_val)), float(N(ob.max_val)), int(ob.last_nfev.sum().item())))
    return out


def oracle_calls(x, lengths, seq_pos, bit, symmetric, calls=1, grow=1.5, mean=None):
    st = OB.ObserverState(bit=bit, symmetric=symmetric)
    old = OB.MEAN_LIKE_TORCH
    OB.MEAN_LIKE_TORCH = mean
    out = []
    try:
        for k in range(calls):
            counter = [0]
            xi = x if k == 0 else (x * F32(grow ** k)).astype(F32)
            OB.observe_msefast(st, xi, lengths, seq_pos, counter=counter)
            out.append((float(st.min_val), float(st.max_val), counter[0]))
    finally:
        OB.MEAN_LIKE_TORCH = old
    return out


@pytest.mark.parametrize("n", MS.FLAT_LENGTHS)
def test_streaming_flat_equals_the_oracle(n, dev, order_free):
    """Every tail length, one float4 per thread (`single`), two (`pair`), both in one launch."""
    x = MS.flat_data(n)
    with switches(mse_resident=0):
        for name, bit, sym in MS.FLAT_SCHEMES:
            got = observe(T(x, dev), None, -1, bit, sym)[0]
            want = oracle_calls(x, None, -1, bit, sym)[0]
            assert same_search(got, want), (n, name, MS.predict_flat(n), got, want)


@pytest.mark.parametrize("n", [n for n in MS.FLAT_PLANTED_LENGTHS if n != MS.FLAT_BIG])
def test_streaming_flat_with_a_planted_element_equals_the_oracle(n, dev, order_free):
    """Element 0, the last element of every tail, either side of 4 * stride and of 8 * stride."""
    fails = []
    with switches(mse_resident=0):
        for p, x in MS.planted(n, MS.flat_planted_positions(n), 1.0, MS.plant_value(n), 3):
            got = observe(T(x, dev), None, -1, 6, True)[0]
            want = oracle_calls(x, None, -1, 6, True)[0]
            if not same_search(got, want):
                fails.append((p, got, want))
    assert not fails, fails


@pytest.mark.parametrize("position", MS.flat_planted_positions(MS.FLAT_BIG))
def test_streaming_flat_second_trip_equals_the_oracle(position, dev, order_free):
    """4 * (2 * 2048 * 256) + 1203 elements: the capped grid, 300 float4s in a second trip, a tail of 3; the planted element
    in a thread's second float4, at the end of the first trip, at the start of the second and in the tail."""
    n = MS.FLAT_BIG
    assert MS.predict_flat(n) == (MS.MAX_BLOCKS, {"pair", "single", "second trip", "tail3"})
    (p, x), = MS.planted(n, (position,), 1.0, MS.plant_value(n), 3)
    with switches(mse_resident=0):
        got = observe(T(x, dev), None, -1, 6, True)[0]
    want = oracle_calls(x, None, -1, 6, True)[0]
    assert same_search(got, want), (p, got, want)


def test_streaming_flat_misaligned_base_is_copied_once(dev, order_free):
    """A buffer 4 bytes off a 16-byte boundary through the observer: the same words as the oracle (and as the aligned tensor)."""
    n = MS.FLAT_MISALIGNED
    x = MS.flat_data(n)
    base = torch.empty(n + 4, dtype=torch.float32, device=dev)
    t = base[1:1 + n]
    t.copy_(T(x, dev))
    assert base.data_ptr() % 16 == 0 and t.data_ptr() % 16 == 4
    for resident in (0, 1):
        with switches(mse_resident=resident):
            for name, bit, sym in MS.FLAT_SCHEMES:
                got = observe(t, None, -1, bit, sym)[0]
                want = oracle_calls(x, None, -1, bit, sym)[0]
                assert same_search(got, want), (resident, name, got, want)
                assert same_search(got, observe(T(x, dev), None, -1, bit, sym)[0])


@pytest.mark.parametrize("n", MS.FLAT_LENGTHS)
def test_streaming_flat_float64_second_call_equals_the_oracle_with_exact_sums(n, dev):
    """ "mse_sum_order" 64 against OB.exact_mean: both calls of an observer bit-equal, the second in float64 arithmetic."""
    x = MS.flat_data(n)
    with switches(mse_sum_order=64):
        for name, bit, sym in MS.FLAT_SCHEMES:
            got = observe(T(x, dev), None, -1, bit, sym, calls=2)
            want = oracle_calls(x, None, -1, bit, sym, calls=2, mean=OB.exact_mean)
            assert all(same_search(g, w) for g, w in zip(got, want)), (n, name, got, want)


def token_inputs(case, mem, dev):
    return case.view(T(mem, dev)), T(case.lengths, dev)


@pytest.mark.parametrize("name", list(MS.TOKEN_CASES))
def test_streaming_tokens_equal_the_oracle(name, dev, order_free):
    """Plain data; the deciding element in the last feature of the last valid token of the last non-empty sample; an element
    of 10^4 in the first padded token, which must not move a word."""
    case = MS.TOKEN_CASES[name]
    mem = case.mem()
    valid = case.mem()
    case.plant(valid, "valid", MS.plant_value(MS.token_observed(case).size))
    padded = case.mem()
    case.plant(padded, "padded", 1e4)
    with switches(mse_resident=0):
        for sname, bit, sym in MS.FLAT_SCHEMES:
            got = {}
            for what, m in (("plain", mem), ("valid", valid), ("padded", padded)):
                x, L = token_inputs(case, m, dev)
                got[what] = observe(x, L, case.seq_pos, bit, sym)[0]
                want = oracle_calls(case.view(m), case.lengths, case.seq_pos, bit, sym)[0]
                assert same_search(got[what], want), (name, sname, what, MS.predict_tokens(case.geometry()), got[what], want)
            assert same_search(got["padded"], got["plain"]) and not same_search(got["valid"], got["plain"])


@pytest.mark.parametrize("name", list(MS.TOKEN_CASES))
def test_streaming_tokens_float64_second_call_equals_the_oracle_with_exact_sums(name, dev):
    case = MS.TOKEN_CASES[name]
    mem = case.mem()
    with switches(mse_sum_order=64):
        for sname, bit, sym in MS.FLAT_SCHEMES:
            x, L = token_inputs(case, mem, dev)
            got = observe(x, L, case.seq_pos, bit, sym, calls=2)
            want = oracle_calls(case.view(mem), case.lengths, case.seq_pos, bit, sym, calls=2, mean=OB.exact_mean)
            assert all(same_search(g, w) for g, w in zip(got, want)), (name, sname, got, want)


@pytest.mark.parametrize("name", list(MS.TOKEN_CASES))
def test_gathered_tokens_equal_the_oracle_in_the_reference_order(name, dev):
    """ "mse_sum_order" 8: gather_valid_tokens_kernel lays the valid tokens out as remove_padding does, the strict kernel adds
    them in torch's one-thread order; the oracle's mean is oracle/aten_sum.py on 8 lanes."""
    from conftest import aten_order_mean
    case = MS.TOKEN_CASES[name]
    valid = case.mem()
    case.plant(valid, "valid", MS.plant_value(MS.token_observed(case).size))
    with switches(mse_sum_order=8):
        for m in (case.mem(), valid):
            for sname, bit, sym in MS.FLAT_SCHEMES:
                x, L = token_inputs(case, m, dev)
                got = observe(x, L, case.seq_pos, bit, sym)[0]
                want = oracle_calls(case.view(m), case.lengths, case.seq_pos, bit, sym, mean=aten_order_mean)[0]
                assert same_search(got, want), (name, sname, got, want)


# =========================================================================================== d. / e. resident forms

def begin(x, lengths, seq_pos, bit, symmetric, float64_input=False, cur=None):
    from outlier_suppression_amd import ops
    quant_min, quant_max = OB.quant_range(bit, symmetric)
    cur = ops.batch_minmax(x, lengths, seq_pos) if cur is None else cur
    return ops.msefast_tensor_begin(x, cur, lengths, seq_pos, quant_min, quant_max, symmetric, "no", not symmetric, float64_input)


def commit(r):
    from outlier_suppression_amd import ops
    mn = torch.full((1,), float("inf"), dtype=torch.float64, device=r.x.device)
    mx = torch.full((1,), float("-inf"), dtype=torch.float64, device=r.x.device)
    nfev = ops.msefast_tensor_commit(r, ops.UPDATE_RUNNING, 0, mn, mx)
    return float(N(mn)[0]), float(N(mx)[0]), int(nfev.item())


def search(x, lengths, seq_pos, bit, symmetric, resident, float64_input=False, cur=None):
    """One per-tensor search (two-sided data) -> ((min, max, evaluations), took the persistent launch)."""
    from outlier_suppression_amd import ops
    ops.check_persistent()
    with switches(mse_resident=resident):
        r = begin(x, lengths, seq_pos, bit, symmetric, float64_input, cur)
        ops.msefast_tensor_run(r, None, not symmetric)
        persistent = bool(ops._persistent_dirty)
        out = commit(r)
    ops.check_persistent()
    return out, persistent


@pytest.fixture(scope="module")
def per_k(dev):
    """Elements one float4 slot of the resident grid holds: the largest tensor msefast_resident_slots gives one slot."""
    import outlier_suppression_amd as osq
    from outlier_suppression_amd import ops
    osq.set_strict(False)
    try:
        if ops.msefast_resident_slots(1) == 0:
            pytest.skip("msefast_resident_slots: this device has no persistent grid")
        lo, hi = 1, 1 << 27                         # slots(lo) == 1 < slots(hi) or 0
        assert ops.msefast_resident_slots(hi) != 1
        while lo + 1 < hi:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if ops.msefast_resident_slots(mid) == 1 else (lo, mid)
        assert ops.msefast_resident_slots(2 * lo) == 2 and ops.msefast_resident_slots(2 * lo + 1) == 3
        assert lo % (MS.RES_THREADS * 4) == 0 and lo // (MS.RES_THREADS * 4) <= MS.RES_MAX_BLOCKS
    finally:
        osq.reset_tier()
    print("per_k:", lo)
    return lo


def device_normal(n, dev, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    return torch.randn(n, device=dev, generator=g)


def decides_on_device(x, p, cur):
    """The 1.5 condition with the streaming form: the search on x against the search on x without the element (extrema of x kept)."""
    keep = x[p].clone()
    full = search(x, None, -1, 6, True, 0, cur=cur)[0]
    x[p] = 0.0
    try:
        without = search(x, None, -1, 6, True, 0, cur=cur)[0]
    finally:
        x[p] = keep
    a, b = full[1] - full[0], without[1] - without[0]
    return max(a / b, b / a)


@pytest.mark.parametrize("K", MS.RES_LADDER)
def test_resident_form_equals_the_streaming_form_at_every_k(K, dev, per_k, order_free):
    """K_prev * per_k + 1, K * per_k - 3 and K * per_k elements: the first size of msefast_resident_kernel<K>, a last slot with
    a tail, the last size.  The deciding element on either side of every slot boundary this K adds and in the last valid
    element; 6 bit symmetric; the second call (float64) within the bounds of test_msefast_resident_search_equals_launch_per_evaluation."""
    from outlier_suppression_amd import ops
    k_prev = ((0,) + MS.RES_LADDER)[MS.RES_LADDER.index(K)]
    fails, worst = [], np.inf
    for n in MS.resident_sizes(per_k)[K]:
        assert MS.predict_resident(n, per_k) == K and ops.msefast_resident_slots(n) == MS.ceil_div(n, per_k) > k_prev
        x = device_normal(n, dev, 100 + K)
        if n < 257:                                 # K = 1 begins at ONE element: nothing to plant among, the forms must still agree
            got, persistent = search(x, None, -1, 6, True, 1)
            want, streamed = search(x, None, -1, 6, True, 0)
            assert persistent and not streamed and same_search(got, want), (n, got, want)
            continue
        for p in MS.resident_planted_positions(n, per_k, k_prev):
            keep = x[p].clone()
            x[p] = MS.plant_value(n)
            cur = ops.batch_minmax(x)
            got, persistent = search(x, None, -1, 6, True, 1)
            want, streamed = search(x, None, -1, 6, True, 0)
            assert persistent and not streamed
            ratio = decides_on_device(x, p, cur)
            worst = min(worst, ratio)
            print("K", K, "n", n, "position", p, "decides", ratio)
            if not same_search(got, want) or ratio < 1.5:
                fails.append((n, p, got, want, ratio))
            x[p] = keep
    print("K", K, "sizes", MS.resident_sizes(per_k)[K], "smallest decides ratio", worst)
    assert not fails, fails
    n = MS.resident_sizes(per_k)[K][1]
    x = device_normal(n, dev, 200 + K)
    for sym in (True, False) if K <= 2 else (True,):
        a = search(x, None, -1, 6, sym, 1, float64_input=True)[0]
        b = search(x, None, -1, 6, sym, 0, float64_input=True)[0]
        assert a[2] == b[2] or abs(a[2] - b[2]) <= 0.35 * b[2], (K, sym, a, b)
        np.testing.assert_allclose(a[:2], b[:2], rtol=2e-3 if sym else 3e-2, atol=1e-9)
    ops.check_persistent()


def test_one_element_past_32_slots_falls_back_by_itself(dev, per_k, order_free):
    from outlier_suppression_amd import ops
    n = MS.RES_MAX_SLOTS * per_k + 1
    assert MS.predict_resident(n, per_k) == 0 and ops.msefast_resident_slots(n) == 0
    x = device_normal(n, dev, 300)
    x[n - 1] = MS.plant_value(n)
    got, persistent = search(x, None, -1, 6, True, 1)
    want, _ = search(x, None, -1, 6, True, 0)
    assert not persistent and same_search(got, want), (got, want)
    assert decides_on_device(x, n - 1, ops.batch_minmax(x)) >= 1.5


@pytest.mark.parametrize("K,vec", [(1, True), (1, False), (2, True), (2, False)])
def test_masked_resident_form_and_its_batch_limit(K, vec, dev, per_k, order_free):
    """A batch of 512 samples (kResMaxBatch), zero lengths among them, stays resident; 513 fall back; both agree with the
    streaming form.  Vector (F % 4 == 0) and scalar loads, one slot and two."""
    from outlier_suppression_amd import ops
    Tn = 8
    F = 8 if K == 1 else 4 * MS.ceil_div(per_k + per_k // 16, MS.RES_MAX_BATCH * Tn * 4)
    F += 0 if vec else 2
    rng = np.random.default_rng([7104, K, vec])
    for B in (MS.RES_MAX_BATCH, MS.RES_MAX_BATCH + 1):
        L = np.full(B, Tn, dtype=np.int64)
        L[rng.choice(B, 5, replace=False)] = 0
        L[7], L[B - 1] = Tn + 3, Tn - 2
        valid = int(np.minimum(L, Tn).sum()) * F
        assert MS.predict_resident(B * Tn * F, per_k) == K and (K == 1 or valid > per_k)
        x = device_normal(B * Tn * F, dev, 400 + K).view(B, Tn, F)
        x[B - 1, Tn - 3, F - 1] = MS.plant_value(valid)          # the last valid element
        Ld = T(L, dev)
        g = MS.token_geometry(np.empty((B, Tn, F), F32), 1, B)
        assert MS.predict_tokens(g)[0] == vec
        got, persistent = search(x, Ld, 1, 6, True, 1)
        want, _ = search(x, Ld, 1, 6, True, 0)
        assert persistent == (B <= MS.RES_MAX_BATCH) and same_search(got, want), (B, persistent, got, want)
    ops.check_persistent()


def run_group(sites):
    """[(x, lengths)] -> ([(min, max, evaluations)] of ONE osq_msefast_tensor_search_multi launch, or None when the group was
    refused -- then with the states as they were), [the same sites one by one through the streaming form]."""
    from outlier_suppression_amd import ops
    ops.check_persistent()
    recs = [begin(x, L, 1 if L is not None else -1, 6, True) for x, L in sites]
    before = [N(ops.msefast_tensor_stats(r)) for r in recs]
    took = ops.msefast_tensor_run_group(recs)
    if not took:
        assert all(np.array_equal(N(ops.msefast_tensor_stats(r)), b) for r, b in zip(recs, before))
        assert all(int(b[3]) == 0 for b in before)                     # no search had finished
        together = None
    else:
        together = [commit(r) for r in recs]
    ops.check_persistent()
    alone = [search(x, L, 1 if L is not None else -1, 6, True, 0)[0] for x, L in sites]
    return together, alone


def group_sites(name, per_k, dev):
    """The group's sites: flat normal tensors of multi_site_elems elements, the deciding element in each at its last element,
    its first, or either side of its first slot boundary, in turn."""
    sites, plants = [], []
    for i, slots in enumerate(MS.MULTI_GROUPS.get(name) or MS.MULTI_REJECTED[name]):
        n = MS.multi_site_elems(slots, i, per_k) if slots > 1 or i % 3 != 2 else per_k - 5 * i
        x = device_normal(n, dev, 500 + 17 * i + len(name)) * (1.0 + 0.25 * (i % 4))
        p = [q for q in (n - 1, 0, per_k - 1, per_k) if q < n][i % (4 if n > per_k else 2)]
        x[p] = MS.plant_value(n) * (1.0 + 0.25 * (i % 4))
        sites.append((x, None))
        plants.append(p)
    return sites, plants


@pytest.mark.parametrize("name", list(MS.MULTI_GROUPS))
def test_multi_site_resident_form_equals_each_site_alone(name, dev, per_k, order_free):
    """Groups whose slots add up to 8, 9, 16, 17, 24, 25 and 32, sixteen sites of one and of two slots, a site over slots 23
    and 24, a site wholly in the LDS-kept slots 24 .. 31 with the deciding element in it, a masked site inside a group: every
    site bit-equal to its own run through the streaming form, counts included."""
    from outlier_suppression_amd import ops
    slots = MS.MULTI_GROUPS[name]
    kt, in_lds = MS.predict_resident_multi(slots)
    sites, plants = group_sites(name, per_k, dev)
    if name == "masked_inside":
        B, Tn, F = 64, 8, 40
        L = np.full(B, Tn, dtype=np.int64)
        L[[0, 5, 63]] = (0, Tn + 2, 3)
        x = device_normal(B * Tn * F, dev, 600).view(B, Tn, F)
        x[63, 2, F - 1] = MS.plant_value(int(np.minimum(L, Tn).sum()) * F)
        sites[1], plants[1] = (x, T(L, dev)), None
    elif name == "sum25_straddle":               # site 1: the element at the end of slot 23 (registers) ...
        x, p = sites[1][0], plants[1]
        x[p] = 0.5
        plants[1] = per_k - 1
        x[per_k - 1] = MS.plant_value(x.numel())
    assert [ops.msefast_resident_slots(x.numel()) for x, _ in sites] == list(slots) and kt in MS.RES_MULTI_LADDER
    together, alone = run_group(sites)
    assert together is not None, "the group must fit one launch"
    assert all(same_search(a, b) for a, b in zip(together, alone)), (name, kt, together, alone)
    check = {len(sites) - 1} | set(in_lds[:1])
    if name == "sum25_straddle":                 # ... and at the start of slot 24 (LDS)
        x = sites[1][0]
        x[per_k - 1] = 0.5
        x[per_k] = MS.plant_value(x.numel())
        plants[1] = per_k
        together, alone = run_group(sites)
        assert together is not None and all(same_search(a, b) for a, b in zip(together, alone)), (name, together, alone)
    for i in sorted(check):
        if plants[i] is not None:
            x = sites[i][0]
            ratio = decides_on_device(x, plants[i], ops.batch_minmax(x))
            print(name, "site", i, "elements", x.numel(), "position", plants[i], "decides", ratio)
            assert ratio >= 1.5, (name, i, ratio)
    ops.check_persistent()


@pytest.mark.parametrize("name", list(MS.MULTI_REJECTED))
def test_groups_that_do_not_fit_are_refused_untouched(name, dev, per_k, order_free):
    """17 sites, and slots that add up to 33: False, every state as osq_msefast_tensor_begin left it."""
    from outlier_suppression_amd import ops
    assert MS.predict_resident_multi(MS.MULTI_REJECTED[name]) == (0, ())
    sites, _ = group_sites(name, per_k, dev)
    if name == "seventeen_sites":
        sites = [(x[:1000 + 4 * i].clone(), None) for i, (x, _) in enumerate(sites)]
    together, alone = run_group(sites)
    assert together is None
    ops.check_persistent()

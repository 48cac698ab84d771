"""The selectors of the one-launch observe + fake-quant step (csrc/fused_step.h: fused_select<CH>; select_from_registers of
csrc/token_select.h behind them) at every chunk shape, select path, row mapping and parameter form of tests/_fused_select.py
(tests/test_oracle_fused_select.py asserts what those tables reach).  The calls go through the C ABI with the test's own
buffers: the per-token extrema arrays are NaN before every launch (a slot absorbed as valid that no streaming workgroup wrote
this launch poisons the statistics), y holds one NaN payload word before every launch (an unwritten word stays), the
statistics are the oracle's, y is the three-launch fake-quant kernel's for every launch and the oracle's for the first and
the last launch of a case, every launch is repeated with the three-launch form, and all comparisons are of words.
The test_knobs_* cases need the tunable build: tests/test_gpu_tunable_build.py runs them in a child process."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import _fused_select as FS
import _minmax_positions as MP
from conftest import bits_equal
from oracle import fake_quant_oracle as FQ
from oracle import observer_oracle as OB

pytestmark = pytest.mark.gpu
F32 = np.float32
MODES = ("fixed", "lsq", "lsqplus")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from outlier_suppression_amd import _hip
    _hip.load()
    return torch.device("cuda:0")


def cus_of(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def fused_status(dev):
    from outlier_suppression_amd import _hip
    st = ctypes.c_int(-1)
    _hip.check(_hip.load().osq_fused_step_status(_hip.ptr(_hip.workspace(dev)), ctypes.byref(st), _hip.stream_ptr(dev)), "status")
    return st.value


def finish(dev, where):
    from outlier_suppression_amd import ops
    ops.check_persistent(where)
    assert fused_status(dev) == 0, where


def fused_launch_seen(call):
    """Whether `call` ran a launch of the one-launch kernel family (as tests/test_gpu_minmax_positions.py does)."""
    from outlier_suppression_amd import _hip
    lib = _hip.load()
    a, b = ctypes.c_void_p(), ctypes.c_void_p()
    _hip.check(lib.osq_timing_events_create(ctypes.byref(a), ctypes.byref(b)), "events")
    lib.osq_time_next_launch(_hip.TIME_FUSED_STEP, a, b)
    call()
    torch.cuda.synchronize()
    us = ctypes.c_float()
    seen = lib.osq_timing_elapsed_us(a, b, ctypes.byref(us)) == 0
    lib.osq_time_next_launch(0, None, None)
    lib.osq_timing_events_destroy(a, b)
    return seen


def nan_filled(n, dev):
    return torch.full((n,), float("nan"), dtype=torch.float32, device=dev)


def same_words(a, b):
    """Word equality of two fp32 device tensors, NaN equal to NaN whatever its payload."""
    return bool(((a.view(torch.int32) == b.view(torch.int32)) | (torch.isnan(a) & torch.isnan(b))).all())


def expected_stats(tmin, tmax, prune, p, rule, cnt, state, bit, sym):
    """(cur, min_val, max_val, scale, zero_point) of the oracle for one batch whose per-token extrema are tmin / tmax."""
    from outlier_suppression_amd import _hip
    vals = np.concatenate([tmin, tmax]).astype(F32)
    if prune:
        lo, up = OB.prune_thresholds(tmin, tmax, p)
        vals = OB.zminimum(OB.zmaximum(vals, lo), up)            # prune_token's clip; aminmax of it is aminmax of the clipped extrema
    cur = OB.aminmax(vals)
    st = OB.ObserverState(bit=bit, symmetric=sym)
    st.min_val, st.max_val, st.cnt = np.asarray(F32(state[0])), np.asarray(F32(state[1])), cnt
    with np.errstate(all="ignore"):
        if rule == _hip.UPDATE_AVERAGE:
            st._avg_update(*cur)
        elif rule == _hip.UPDATE_RUNNING:
            st._running_update(*cur)
        else:
            st.min_val, st.max_val = np.asarray(cur[0]), np.asarray(cur[1])
        scale, zp = st.qparams()
    return np.array(cur, F32), F32(st.min_val), F32(st.max_val), F32(scale), F32(zp)


def oracle_y(x, scale, zp, qmin, qmax, mode, g):
    with np.errstate(all="ignore"):
        if mode == "lsqplus":
            return FQ.fake_quantize_learnableplus_per_tensor(x, scale, zp, qmin, qmax, g)[1]
        if mode == "lsq":
            return FQ.fake_quantize_learnable_per_tensor(x, scale, zp, qmin, qmax, g)[1]
        return FQ.fake_quantize_per_tensor_affine(x, scale, zp, qmin, qmax)[1]


class Tensor:
    """One [B, T, H] input on the device with its lengths, the enumeration of its tokens and the test's own buffers."""

    def __init__(self, dev, rows_host, lengths, T, nwg):
        self.dev, self.T, self.B = dev, T, len(lengths)
        self.total, self.H = rows_host.shape
        assert self.total == self.B * T
        self.rows, self.V = FS.enumeration_rows(lengths, T)
        self.host = rows_host
        self.x = torch.from_numpy(rows_host).to(dev).view(self.B, T, self.H)
        self.xf = self.x.view(self.total, self.H)
        self.L = torch.tensor(lengths, dtype=torch.int64, device=dev)
        self.vrows = torch.from_numpy(self.rows[:self.V]).to(dev)
        self.geo = FS.geometry(nwg, self.total, self.V)
        self.fused = FS.eligible(self.B, T, self.H, nwg)
        self.y = {p: torch.empty_like(self.x) for p in (True, False)}
        cap = (self.total + 3) // 4 * 4
        self.tok = {p: (nan_filled(cap, dev), nan_filled(cap, dev)) for p in (True, False)}
        self.lst = torch.empty(2 * cap, dtype=torch.float32, device=dev) if self.total > FS.MAX_SLOTS else None    # the wide finaliser's list (as ops._scratch)
        j = np.arange(self.V, dtype=np.int64)
        g, local = j % nwg, j // nwg
        self.slot = g * self.geo["qt"] + np.minimum(g, self.geo["rt"]) + local          # fused_step.h:429, 504
        self.launches = 0

    def set_extrema(self, tmin, tmax):
        """Column 0 of the valid tokens carries their maxima, column 1 their minima (in enumeration order)."""
        self.host[self.rows[:self.V], 0], self.host[self.rows[:self.V], 1] = tmax, tmin
        self.xf[self.vrows, 0] = torch.from_numpy(np.ascontiguousarray(tmax)).to(self.dev)
        self.xf[self.vrows, 1] = torch.from_numpy(np.ascontiguousarray(tmin)).to(self.dev)

    def launch(self, persistent, prune, p, rule, cnt, state, bit, sym, mode="fixed", g=1.0, zp_dtype=torch.float32, old=(0.125, 3.0),
               probe=False):
        """One call of osq_observe_tokens_fake_quant on fresh parameter buffers.  Returns dict(cur, mn, mx, scale, zp, y)."""
        from outlier_suppression_amd import ops, _hip
        lib, dev = _hip.load(), self.dev
        qmin, qmax = OB.quant_range(bit, sym)
        o = dict(mn=torch.tensor([float(state[0])], device=dev), mx=torch.tensor([float(state[1])], device=dev),
                 cur=torch.full((2,), 77.0, device=dev), scale=torch.tensor([old[0]], device=dev),
                 zp=torch.tensor([old[1]], device=dev).to(zp_dtype))
        y = self.y[persistent]
        y.view(torch.int32).fill_(FS.SENTINEL_Y)
        tmin, tmax = self.tok[persistent]
        tmin.fill_(float("nan"))
        tmax.fill_(float("nan"))
        view = ops.token_view(self.x, 1, self.L.numel())
        m = MODES.index(mode) | (0 if persistent else _hip.PARAM_NO_PERSISTENT)

        def call():
            rc = lib.osq_observe_tokens_fake_quant(self.x.data_ptr(), ctypes.byref(view), self.L.data_ptr(), tmin.data_ptr(), tmax.data_ptr(),
                                                   1 if prune else 0, float(p) if prune else 1.0, rule, cnt, o["mn"].data_ptr(),
                                                   o["mx"].data_ptr(), o["cur"].data_ptr(), qmin, qmax, 1 if sym else 0, o["scale"].data_ptr(),
                                                   o["zp"].data_ptr(), ops._zp_type(o["zp"]), y.data_ptr(), self.x.numel(), m, g,
                                                   _hip.workspace(dev).data_ptr(), _hip.ptr(self.lst), _hip.raw_stream(dev))
            _hip.check(rc, "observe_tokens_fake_quant")
            ops._persistent_dirty.add((dev.index, _hip.raw_stream(dev)))
        if probe:      # the entry point falls back to three launches without a word: see that it did (not)
            assert fused_launch_seen(call) == (persistent and self.fused), (self.geo, "persistent" if persistent else "three launches")
        else:
            call()
        self.launches += 1
        o.update(y=y, qmin=qmin, qmax=qmax, mode=mode, g=g)
        return o

    def check(self, o, persistent, tmin_h, tmax_h, prune, p, rule, cnt, state, bit, sym, old=(0.125, 3.0), oracle=False, tag=None):
        """Everything one launch left, against the oracle."""
        from outlier_suppression_amd import ops, _hip
        tag = (tag, self.geo, "persistent" if persistent else "three launches")
        if self.V:
            cur, mn, mx, scale, zp = expected_stats(tmin_h, tmax_h, prune, p, rule, cnt, state, bit, sym)
            if rule == _hip.UPDATE_NONE:
                mn, mx = F32(state[0]), F32(state[1])                        # no running statistic: the buffers stay
        else:                                                                # nothing observed: nothing moves
            cur, mn, mx, scale, zp = np.array([77.0, 77.0], F32), F32(state[0]), F32(state[1]), F32(old[0]), F32(old[1])
        got = {k: o[k].cpu().numpy() for k in ("cur", "mn", "mx", "scale", "zp")}
        assert bits_equal(got["cur"], cur), (tag, "cur", got["cur"].tolist(), cur.tolist())
        assert bits_equal(got["mn"], np.array([mn], F32)) and bits_equal(got["mx"], np.array([mx], F32)), (tag, "min_val / max_val", got["mn"], got["mx"], mn, mx)
        assert bits_equal(got["scale"], np.array([scale], F32)), (tag, "scale", got["scale"], scale)
        if got["zp"].dtype == np.int32:
            assert got["zp"][0] == int(zp), (tag, "zero_point", got["zp"], zp)
        else:
            assert bits_equal(got["zp"], np.array([zp], F32)), (tag, "zero_point", got["zp"], zp)
        y = o["y"]
        assert not bool((y.view(torch.int32) == FS.SENTINEL_Y).any()), (tag, "a word of y was never written",
                                                                           torch.nonzero((y.view(torch.int32) == FS.SENTINEL_Y).view(self.total, -1).any(1)).flatten()[:8].tolist())
        ref = ops.fake_quant_per_tensor(self.x, o["scale"], o["zp"], o["qmin"], o["qmax"], MODES.index(o["mode"]), o["g"])
        assert same_words(y, ref), (tag, "y differs from the fake-quant kernel's", torch.nonzero((y != ref).view(self.total, -1).any(1)).flatten()[:8].tolist())
        if persistent and self.fused:                                        # what the streaming workgroups published, and where
            for arr, vals, what in ((self.tok[True][0], tmin_h, "token_min"), (self.tok[True][1], tmax_h, "token_max")):
                want = np.full(arr.numel(), np.nan, F32)
                want[self.slot] = vals
                assert bits_equal(arr.cpu().numpy(), want), (tag, what, "the compact array is not the published chunks")
        if oracle:
            want = oracle_y(self.host, scale, F32(int(zp)) if got["zp"].dtype == np.int32 else zp, o["qmin"], o["qmax"], o["mode"], o["g"])
            yh = y.view(self.total, self.H).cpu().numpy()
            assert bits_equal(yh, want), (tag, "y differs from the oracle")

    def both(self, tmin_h, tmax_h, prune, p, rule, cnt, state, bit=6, sym=False, probe=False, oracle=False, tag=None, **kw):
        """The launch in the one-launch form and as three launches: each against the oracle, and word-equal to each other."""
        out = {}
        for persistent in (True, False):
            o = self.launch(persistent, prune, p, rule, cnt, state, bit, sym, probe=probe, **kw)
            self.check(o, persistent, tmin_h, tmax_h, prune, p, rule, cnt, state, bit, sym, oracle=oracle and persistent, tag=tag,
                       **({"old": kw["old"]} if "old" in kw else {}))
            out[persistent] = o
        for k in ("cur", "mn", "mx", "scale", "zp"):
            assert torch.equal(out[True][k].view(torch.int32), out[False][k].view(torch.int32)), (tag, k)
        assert same_words(out[True]["y"], out[False]["y"]), (tag, "y of the two forms")
        return out[True]


# ----------------------------------------------------------------------------------- chunk geometry

def run_geometry(dev, nwg, V, B, T, H=768, max_launches=None, record=None):
    """Every planted launch of one geometry (tests/_fused_select.py, plant_launches): the key at the wanted rank sits at the
    planted position of each side, p makes the rank integral, so `up` / `lo` ARE those tokens' extrema."""
    from outlier_suppression_amd import _hip
    seed = V + nwg
    L = FS.lengths_for(B, T, V)
    rows, _ = FS.enumeration_rows(L, T)
    xh = FS.base_rows(B * T, H, seed)
    FS.fill_padding(xh, rows, V)
    t = Tensor(dev, xh, L, T, nwg)
    assert t.V == V
    a, m = FS.grids(V, seed)
    launches = FS.plant_launches(t.geo, max_launches)
    for n, (j0, j1, k, p, hinted) in enumerate(launches):
        tmax_h, tmin_h = FS.plant(a, j0, k), -FS.plant(m, j1, k)
        t.set_extrema(tmin_h, tmax_h)
        ends = n in (0, len(launches) - 1)
        rule, cnt, state = (_hip.UPDATE_AVERAGE, 1, (FS.HINT_MIN, FS.HINT_MAX)) if hinted else (_hip.UPDATE_NONE, 0, (-7.0, 7.0))
        t.both(tmin_h, tmax_h, True, p, rule, cnt, state, probe=ends, oracle=ends,
               tag=("planted", n, FS.locate(t.geo, j0), FS.locate(t.geo, j1), k, float(p), hinted))
    if record is not None:
        record.append((nwg, B * T, V, t.geo["CH"], t.geo["tlen"], t.geo["ntg"], len(launches), t.fused))
    return t


@pytest.mark.parametrize("name", FS.RELEASE_CLASSES)
def test_chunk_geometry_release_grid(name, dev):
    """One workgroup per CU (nwg = CUs - 2, read from the device): CH = 1 and 2 with every tail size class, CH = 3 with
    tails of 1 and 2, V = 1, V < nwg, V either side of 64 nwg and 128 nwg; the planted rank at the first and last lane of
    every main block and tail positions 0 / tlen - 2 / tlen - 1 of chunks 0, rv - 1, rv, nwg - 1, one of wave 15 and one of
    the second group."""
    nwg = cus_of(dev) - 2
    case = FS.release_case(name, nwg)
    assert case is not None, (name, nwg, "this device cannot hold the class")
    V, B, T = case
    t = run_geometry(dev, nwg, V, B, T)
    assert t.fused and t.launches >= 2
    print("geometry", name, "nwg", nwg, "total", B * T, "V", V, "CH", t.geo["CH"], "tlen", t.geo["tlen"], "ntg", t.geo["ntg"], "launches", t.launches)
    finish(dev, name)


# ----------------------------------------------------------------------------------- selection paths

PATH_CASES = {c["name"]: c for c in FS.path_cases()}


def path_tensor(dev, case, side, nwg, H=768):
    tmin, tmax, state, cnt = FS.path_tokens(case, side, MP.case_seed(case["name"]))
    V = tmin.size
    B, T = FS.shape_for(V + 5)                                               # at least five padded slots
    L = FS.lengths_for(B, T, V)
    rows, _ = FS.enumeration_rows(L, T)
    xh = np.zeros((B * T, H), F32)
    xh[rows[:V]] = FS.token_rows(tmin, tmax, H, V + side)
    FS.fill_padding(xh, rows, V)
    return Tensor(dev, xh, L, T, nwg), tmin, tmax, state, cnt


@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("name", list(PATH_CASES))
def test_selection_paths(name, side, dev):
    """Every branch class of select_from_registers behind the fused gathering pass, on either side, with the shortcut of the
    threshold pass on and off: the hinted window off (first batch, zero / denormal / 1e31 hints), hit, missed from below and
    from above and at the two equalities, a crowded bin behind the pre-built level, the all-levels exit, `listed` with and
    without the next key, the shortcut taken and refused, thresholds that reach the upper key, integral ranks, p = 0 and 1,
    all-negative values.  (Which branches a case takes: tests/test_oracle_fused_select.py.)"""
    from outlier_suppression_amd import ops, _hip
    case = PATH_CASES[name]
    t, tmin, tmax, state, cnt = path_tensor(dev, case, side, cus_of(dev) - 2)
    outs = []
    try:
        for shortcut in (1, 0):
            ops.set_tuning("select_shortcut", shortcut)
            outs.append(t.both(tmin, tmax, True, case["p"], _hip.UPDATE_AVERAGE, cnt, state, probe=True, oracle=shortcut == 1,
                               tag=(name, side, "shortcut", shortcut)))
            outs[-1] = {k: outs[-1][k].clone() for k in ("cur", "mn", "mx", "scale", "zp", "y")}
    finally:
        ops.set_tuning("select_shortcut", 1)
    for k in outs[0]:
        assert same_words(outs[0][k], outs[1][k]), (name, side, k)
    assert t.fused
    finish(dev, name)


# ----------------------------------------------------------------------------------- token -> row mapping

def run_rows(dev, nwg, B, T, pattern, H, expect_fused=True):
    from outlier_suppression_amd import _hip
    L = FS.pattern_lengths(pattern, B, T)
    rows, V = FS.enumeration_rows(L, T)
    seed = B * 7 + T + H
    xh = FS.base_rows(B * T, H, seed)
    FS.fill_padding(xh, rows, V)
    t = Tensor(dev, xh, L, T, nwg)
    assert t.fused == expect_fused, (B, T, H, nwg)
    a, m = FS.grids(V, seed)
    k = int(0.9 * (V - 1)) if V else 0
    p = FS.exact_percentile(V, k) if V else F32(0.9)
    tmin, tmax = -m, a
    t.set_extrema(tmin, tmax)
    t.both(tmin, tmax, True, p, _hip.UPDATE_NONE, 0, (-7.0, 7.0), probe=True, oracle=True, tag=("rows", B, T, pattern, H))
    return t


ROW_CASES = ([(B, pattern, (3072, 4096)[i % 2]) for i, (B, pattern) in enumerate(itertools.product(FS.ROW_B, FS.ROW_PATTERNS))] +
             [(B, "alternating", 768) for B in FS.ROW_B] +
             [(64, "alternating", 1024), (1024, "one_last", 1024), (1024, "leading", 1024), (63, "full", 1024)])


@pytest.mark.parametrize("B,pattern,H", ROW_CASES)
def test_row_mapping(B, pattern, H, dev):
    """Token -> row for held slots (bisection) and streamed ones (ballot counting; valid and padded variant) at B = 1, 63,
    64, 65, 1024 with runs of empty samples at either end: T is the smallest at which valid AND padded tokens are streamed
    (H >= 1024; NV = 3 keeps every token of a full grid), every row distinct, padded rows NaN / inf / 1e30, y pre-filled."""
    nwg = cus_of(dev) - 2
    nv = H // 256
    T = FS.row_mapping_T(B, pattern, nv, nwg) if nv >= 4 else 8
    t = run_rows(dev, nwg, B, T, pattern, H)
    if nv >= 4:
        assert t.total > FS.held_tokens(nv, nwg)
    finish(dev, (B, pattern, H))


@pytest.mark.parametrize("B,T", [(1025, 4), (12, 2731)])
def test_row_mapping_beyond_the_limits_falls_back(B, T, dev):
    """B = 1025 and B * T = 32772: the call runs as three launches (the probe sees no one-launch kernel) and is correct."""
    run_rows(dev, cus_of(dev) - 2, B, T, "alternating", 768, expect_fused=False)
    finish(dev, (B, T))


def test_parameter_forms(dev):
    """One small shape: zero-point buffer float32 / int32, Fixed / LSQ / LSQ+ with a grad factor, symmetric on / off, 2 / 4 / 8
    bits, rules NONE / RUNNING / AVERAGE; and V = 0: the parameters stay, y is quantised with the old ones."""
    from outlier_suppression_amd import _hip
    nwg = cus_of(dev) - 2
    B, T, H = 5, 12, 768
    for lengths in ([12, 0, 7, 1, 9], [0] * 5):
        rows, V = FS.enumeration_rows(lengths, T)
        xh = FS.base_rows(B * T, H, 5)
        if V == 0:
            xh[:, :] = FS.base_rows(B * T, H, 6) * F32(8.0)                 # finite everywhere: y of the old parameters says something
        else:
            FS.fill_padding(xh, rows, V)
        t = Tensor(dev, xh, lengths, T, nwg)
        a, m = FS.grids(V, 11)
        tmin, tmax = -m, a
        if V:
            t.set_extrema(tmin, tmax)
        n = 0
        for zp_dtype, mode, sym, bit, rule in itertools.product((torch.float32, torch.int32), MODES, (False, True), (2, 4, 8),
                                                                (_hip.UPDATE_NONE, _hip.UPDATE_RUNNING, _hip.UPDATE_AVERAGE)):
            state = (-2.5, 1.25) if n % 2 else (-3.5, 2.0)
            t.both(tmin, tmax, bool(n % 3), FS.exact_percentile(V, V // 2) if V else 0.5, rule, 2, state, bit=bit, sym=sym, mode=mode,
                   g=0.37 if mode != "fixed" else 1.0, zp_dtype=zp_dtype, old=(0.25, 2.0), probe=n in (0, 107), oracle=True,
                   tag=("forms", lengths, str(zp_dtype), mode, sym, bit, rule))
            n += 1
        assert n == 108 and t.fused
    finish(dev, "parameter forms")


# ----------------------------------------------------------------------------------- knobs (tunable build)

def _need_tunable():
    from outlier_suppression_amd import ops
    if not ops.tunable_build():
        pytest.skip("fused_grid, fused_gate and select_hint are compile-time constants in the release library; "
                    "tests/test_gpu_tunable_build.py runs this test against libosq_hip_dbg.so in a child process")
    return ops


KNOB_ROW_SHAPES = ((1, 192), (64, 3), (48, 4), (96, 2), (5, 36))


@pytest.mark.parametrize("nwg", FS.KNOB_NWG)
def test_knobs_chunk_geometry_small_grids(nwg, dev):
    """fused_grid = nwg + 2: all 21 (CH, lt) classes -- CH = 3 with tails up to 64 -- in tensors of at most 192 nwg tokens;
    nwg = 1, 2, 15, 16, 17, 33 and 130 (a wave with chunks of both groups, tails that share a register).  With one streaming
    workgroup tokens are streamed at every NV: the row-mapping patterns run there too.  192 nwg + 4 slots fall back."""
    ops = _need_tunable()
    record = []
    try:
        ops.set_tuning("fused_grid", nwg + 2)
        for V, B, T in FS.knob_cases(nwg):
            t = run_geometry(dev, nwg, V, B, T, record=record)
            assert t.fused, (nwg, V, B, T)
        if nwg == 1:
            for (B, T), pattern, H in itertools.product(KNOB_ROW_SHAPES, FS.ROW_PATTERNS, (768, 3072)):
                t = run_rows(dev, nwg, B, T, pattern, H)
                assert t.total > FS.held_tokens(H // 256, nwg)
        run_rows(dev, nwg, 4, 48 * nwg + 1, "trailing", 768, expect_fused=False)
        for r in record:
            print("geometry nwg %d total %d V %d CH %d tlen %d ntg %d launches %d" % r[:7])
    finally:
        ops.set_tuning("fused_grid", 0)
    finish(dev, ("small grid", nwg))


def test_knobs_gate_and_hint(dev):
    """fused_gate 0 / 1 / 2 x select_hint 0 / 1 on the full grid (set explicitly: the launcher keeps the last grid): the six
    results of three geometries with padded tokens -- selection-path cases that hit the window among them -- are the
    oracle's and word-equal to each other."""
    ops = _need_tunable()
    from outlier_suppression_amd import _hip
    cus = cus_of(dev)
    try:
        ops.set_tuning("fused_grid", cus)
        for name, side in (("hit", 0), ("eq_below", 1), ("crowded_listed", 0)):
            case = PATH_CASES[name]
            t, tmin, tmax, state, cnt = path_tensor(dev, case, side, cus - 2)
            assert t.fused and t.total > t.V
            first = None
            for gate, hint in itertools.product((0, 1, 2), (0, 1)):
                ops.set_tuning("fused_gate", gate)
                ops.set_tuning("select_hint", hint)
                o = t.both(tmin, tmax, True, case["p"], _hip.UPDATE_AVERAGE, cnt, state, probe=True, oracle=first is None, tag=(name, gate, hint))
                o = {k: o[k].clone() for k in ("cur", "mn", "mx", "scale", "zp", "y")}
                if first is None:
                    first = o
                for k in o:
                    assert same_words(o[k], first[k]), (name, gate, hint, k)
    finally:
        ops.set_tuning("fused_gate", 2)
        ops.set_tuning("select_hint", 1)
        ops.set_tuning("fused_grid", 0)
    finish(dev, "gate and hint")


def test_the_launch_state_is_clean(dev):
    """After everything above: no time-out flag on the workspace, nothing for check_persistent to report."""
    finish(dev, "end of file")

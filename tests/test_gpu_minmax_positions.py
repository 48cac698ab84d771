"""The min/max kernels of csrc/observer.hip with the extremum planted at every loop boundary (tests/_minmax_positions.py):
observe_flat_kernel, observe_rows_kernel, observe_channels_kernel, token_minmax_vec_kernel (single segment, head split),
token_minmax_generic_kernel and token_minmax_multi_kernel, for fp32, bf16 and fp16.  Expected values are known by
construction and equal the oracle's (tests/test_oracle_minmax_positions.py); every comparison is of words, no tolerance.
The test_knobs_* cases need the tunable build: tests/test_gpu_tunable_build.py runs them in a child process."""
import numpy as np
import pytest
import torch

import _minmax_positions as MP
from conftest import bits_equal

pytestmark = pytest.mark.gpu

DTYPES = {"fp32": (torch.float32, 4, None), "bf16": (torch.bfloat16, 2, "bf16"), "fp16": (torch.float16, 2, "fp16")}
INF = float("inf")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from outlier_suppression_amd import _hip
    _hip.load()
    return torch.device("cuda:0")


def on_device(a, dtype, dev, misalign=False):
    """A float32 host array as a device tensor of `dtype` (exact: every value is representable); misalign: one element
    past a 16-byte boundary."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not misalign:
        out = t.to(dev).to(dtype)
        assert out.data_ptr() % 16 == 0
        return out
    buf = torch.zeros(t.numel() + 8, dtype=dtype, device=dev)
    out = buf[1:1 + t.numel()].view(t.shape)
    out.copy_(t.to(dev))
    assert out.data_ptr() % 16 != 0 and out.is_contiguous()
    return out


# ----------------------------------------------------------------------------------- observe_flat_kernel

def run_flat(dev, dtype_name, n, aligned, seed, blocks=MP.OBS_BLOCKS, all_kinds=True):
    """Every representative pair of one size: one launch per (pair, kind), data on the device, two elements set and restored
    between launches; cur and the running statistic from a (+inf, -inf) state against the expected words."""
    from outlier_suppression_amd import ops, _hip
    dtype, isz, lowp = DTYPES[dtype_name]
    kinds = MP.kinds_for(isz, lowp)
    base = MP.flat_base(n, seed)
    pairs = MP.flat_pairs(MP.flat_representatives(n, isz, aligned, blocks))
    host = {s: MP.signed_base(base, s) for s in (0, 1, -1)}
    x = {s: on_device(host[s], dtype, dev, misalign=not aligned) for s in (0, 1, -1)}
    jobs = [(k, p) for k, p in enumerate(pairs)]
    runs = [(kind, imax, imin) for k, (imax, imin) in jobs for kind in (kinds if all_kinds else [kinds[k % len(kinds)]])]
    m = len(runs)
    mn = torch.full((m,), INF, device=dev)
    mx = torch.full((m,), -INF, device=dev)
    cur = torch.zeros(m, 2, device=dev)
    want = np.zeros((m, 2), np.float32)
    for r, (kind, imax, imin) in enumerate(runs):
        name, sign, vmax, vmin = kind
        t, h = x[sign], host[sign]
        two = imin is not None and vmin is not None
        t[imax] = float(vmax)
        if two:
            t[imin] = float(vmin)
        ops.observe_flat(t, _hip.UPDATE_RUNNING, 0, mn[r:r + 1], mx[r:r + 1], 0, 255, False, cur=cur[r])
        t[imax] = float(h[imax])
        if two:
            t[imin] = float(h[imin])
        if name == "nan":
            want[r] = np.nan
        elif two:
            want[r] = (vmin, vmax)
        else:
            want[r] = MP.plant_flat(base, kind, imax, imin)[1:]
    got_cur, got_mn, got_mx = cur.cpu().numpy(), mn.cpu().numpy(), mx.cpu().numpy()
    for s in (0, 1, -1):                                              # every element was put back
        assert bits_equal(x[s].float().cpu().numpy(), host[s]), "input not restored"
    for r, (kind, imax, imin) in enumerate(runs):
        tag = (dtype_name, n, blocks, kind[0], MP.flat_class_of(imax, n, isz, aligned, blocks),
               None if imin is None else MP.flat_class_of(imin, n, isz, aligned, blocks))
        assert bits_equal(got_cur[r], want[r]), (tag, "cur", got_cur[r].tolist(), want[r].tolist())
        assert bits_equal(np.array([got_mn[r], got_mx[r]]), want[r]), (tag, "running", got_mn[r], got_mx[r], want[r].tolist())
    return m


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_flat_small_sizes(dtype_name, dev):
    """n = 1, kPer - 1, kPer, kPer + 1, ng = 1023 .. 2048 and a misaligned pointer: every kind at every representative."""
    per = MP.GRANULE[DTYPES[dtype_name][1]]
    for name, size, aligned in MP.FLAT_SIZES:
        if name not in MP.FLAT_LARGE:
            run_flat(dev, dtype_name, size(per), aligned, MP.case_seed(name))


@pytest.mark.parametrize("name", sorted(MP.FLAT_LARGE))
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_flat_large_sizes(dtype_name, name, dev):
    """Grids of 257 / 259 workgroups (the finishing workgroup's raw[0] and raw[1]), the capped grid with a second unrolled
    trip, three remainder trips and a tail, and the scalar loop over 515 workgroups: every kind at every representative."""
    per = MP.GRANULE[DTYPES[dtype_name][1]]
    size, aligned = next((s, a) for nm, s, a in MP.FLAT_SIZES if nm == name)
    run_flat(dev, dtype_name, size(per), aligned, MP.case_seed(name))


# ----------------------------------------------------------------------------------- the per-row kernels

def sentinel_filled(n, dev):
    return torch.full((n,), int(MP.SENTINEL), dtype=torch.int32, device=dev).view(torch.float32)


def token_tensor(case, rows, dtype, dev):
    """The [R, F] row matrix of a token case in the layout its entry point is given, and the sequence axis."""
    B, T = len(case["lengths"]), case["T"]
    layout = case["layout"]
    if layout in ("single", "generic"):
        return on_device(rows.reshape(B, T, case["F"]), dtype, dev, misalign=layout == "generic"), 1
    r4 = rows.reshape(B, T, case["feat_outer"], case["feat_inner"])
    if layout == "head":
        return on_device(r4, dtype, dev), 1                           # [B, T, h, d]: segments of d, stride_outer = d
    return on_device(np.ascontiguousarray(r4.transpose(0, 2, 3, 1)), dtype, dev), 3     # [B, h, d, T]: stride_inner = T


def check_slots(got_min, got_max, emin, emax, valid, tag):
    gm, gx = got_min.cpu().numpy(), got_max.cpu().numpy()
    for got, want, what in ((gm, emin, "min"), (gx, emax, "max")):
        raw = got.view(np.uint32)
        assert (raw[~valid] == MP.SENTINEL).all(), (tag, what, "a padded slot was written", np.flatnonzero(raw[~valid] != MP.SENTINEL)[:8].tolist())
        assert not (raw[valid] == MP.SENTINEL).any(), (tag, what, "a valid slot was never written")
        if not bits_equal(got[valid], want[valid]):
            bad = np.flatnonzero(got[valid].view(np.uint32) != want[valid].view(np.uint32))
            rows = np.flatnonzero(valid)[bad]
            raise AssertionError((tag, what, "rows", rows[:8].tolist(), got[rows[:8]].tolist(), want[rows[:8]].tolist()))


def run_row_case(case, dtype_name, dev):
    from outlier_suppression_amd import ops, _hip
    dtype, isz, lowp = DTYPES[dtype_name]
    kinds = MP.kinds_for(isz, lowp)
    valid = case["valid"]
    for l, (x, emin, emax, cmax, cmin, kidx) in enumerate(MP.case_launches(case, kinds)):
        tag = (dtype_name, case["name"], l)
        if case["kernel"] == "rows":
            t = on_device(x, dtype, dev)
            mn, mx = torch.full((case["R"],), INF, device=dev), torch.full((case["R"],), -INF, device=dev)
            ops.observe_channels(t, 0, _hip.UPDATE_RUNNING, 0, mn, mx, 0, 255, False)
        elif case["kernel"] == "channels":
            C, outer, inner = case["R"], case["outer"], case["inner"]
            t = on_device(np.ascontiguousarray(x.reshape(C, outer, inner).transpose(1, 0, 2)), dtype, dev, misalign=case["misalign"])
            mn, mx = torch.full((C,), INF, device=dev), torch.full((C,), -INF, device=dev)
            ops.observe_channels(t, 1, _hip.UPDATE_RUNNING, 0, mn, mx, 0, 255, False)
        else:
            t, seq_pos = token_tensor(case, x, dtype, dev)
            L = torch.tensor(case["lengths"], dtype=torch.int64, device=dev)
            mn, mx = sentinel_filled(case["R"], dev), sentinel_filled(case["R"], dev)
            _, _, B, T, _ = ops.token_minmax(t, seq_pos, L, out=(mn, mx))
            assert (B, T) == (len(case["lengths"]), case["T"])
            check_slots(mn, mx, emin, emax, valid, tag)
            continue
        gm, gx = mn.cpu().numpy(), mx.cpu().numpy()
        for got, want, what in ((gm, emin, "min"), (gx, emax, "max")):
            if not bits_equal(got, want):
                bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
                raise AssertionError((tag, what, "rows", bad[:8].tolist(), "columns", (cmin if what == "min" else cmax)[bad[:8]].tolist(),
                                      got[bad[:8]].tolist(), want[bad[:8]].tolist()))


def cases_of(isz, kernels):
    return [c for c in MP.row_cases(isz) if c["kernel"] in kernels]


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_rows_kernel(dtype_name, dev):
    """observe_rows_kernel: inner_g either side of every trip of the kRowLoads-wide loop, 1 / 3 / 4 / 5 rows, and more rows
    than the capped grid has waves; the running statistic of every row from a (+inf, -inf) state."""
    for case in cases_of(DTYPES[dtype_name][1], ("rows",)):
        run_row_case(case, dtype_name, dev)


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_channels_kernel(dtype_name, dev):
    """observe_channels_kernel: inner 1 / 255 / 256 / 257 / 513 with outer 1 / 2 / 3 (outer 1 with a whole number of granules
    from a misaligned pointer, which the rows kernel refuses)."""
    for case in cases_of(DTYPES[dtype_name][1], ("channels",)):
        run_row_case(case, dtype_name, dev)


@pytest.mark.parametrize("kernel", ["single", "head", "generic"])
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_token_kernels(dtype_name, kernel, dev):
    """token_minmax_vec_kernel (one segment; head split at every lgG) and token_minmax_generic_kernel: sample lengths
    0, 1, 2, 3, 4, 5, 15, 16, 17 and T, padded tokens full of NaN / inf / 1e30, outputs sentinel-filled."""
    for case in cases_of(DTYPES[dtype_name][1], (kernel,)):
        run_row_case(case, dtype_name, dev)


# ----------------------------------------------------------------------------------- token_minmax_multi_kernel

def test_multi_site_table(dev):
    """The fp32 token cases as ONE table of sites (vector descriptors of both forms, scalar descriptors): expected words,
    and word-equal to the single-site calls, padded slots and the gaps between sites included.  Table launch l takes launch
    l % (its count) of every site, for as many launches as the site with the most column offsets has, so every site's
    extremum visits every column (tests/test_oracle_minmax_positions.py checks the loop parts those columns reach)."""
    from outlier_suppression_amd import ops, _hip
    lib = _hip.load()
    kinds = MP.kinds_for(4)
    cases = [c for c in cases_of(4, ("single", "head", "generic")) if "shifts" not in c]
    runs = [list(MP.case_launches(c, kinds)) for c in cases]
    gap = 3
    offs = np.cumsum([0] + [c["R"] + gap for c in cases])
    forms = set()
    for l in range(MP.multi_launch_count(runs)):                  # every launch of the site with the most column offsets
        tmin, tmax = sentinel_filled(int(offs[-1]), dev), sentinel_filled(int(offs[-1]), dev)
        one_min, one_max = sentinel_filled(int(offs[-1]), dev), sentinel_filled(int(offs[-1]), dev)
        descs = (_hip.SiteDesc * len(cases))()
        keep, ends, total = [], [], 0
        for d, c, launches, off in zip(descs, cases, runs, offs):
            x = launches[l % len(launches)][0]
            t, seq_pos = token_tensor(c, x, torch.float32, dev)
            L = torch.tensor(c["lengths"], dtype=torch.int64, device=dev)
            view = ops.token_view(t, seq_pos, L.numel())
            vec = int(view.stride_inner == 1 and view.feat_inner % 4 == 0 and t.data_ptr() % 16 == 0 and view.stride_batch % 4 == 0
                      and view.stride_token % 4 == 0 and (view.feat_outer == 1 or view.stride_outer % 4 == 0))      # as deferred.py
            assert vec == (c["kernel"] != "generic"), c["name"]
            forms.add(("scalar" if not vec else ("one" if view.feat_outer == 1 else "split")))
            sl = slice(int(off), int(off) + c["R"])
            d.x, d.lengths = t.data_ptr(), L.data_ptr()
            d.token_min, d.token_max = tmin[sl].data_ptr(), tmax[sl].data_ptr()
            d.view, d.vec = view, vec
            ops.token_minmax(t, seq_pos, L, out=(one_min[sl], one_max[sl]))
            keep += [t, L]
            total += c["R"]
            ends.append(total)
        table = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(dev)
        ends_d = torch.tensor(ends, dtype=torch.int64, device=dev)
        _hip.check(lib.osq_token_minmax_multi(table.data_ptr(), ends_d.data_ptr(), len(cases), total, _hip.stream_ptr(dev)), "token_minmax_multi")
        torch.cuda.synchronize()
        assert np.array_equal(tmin.cpu().numpy().view(np.uint32), one_min.cpu().numpy().view(np.uint32)), l
        assert np.array_equal(tmax.cpu().numpy().view(np.uint32), one_max.cpu().numpy().view(np.uint32)), l
        for c, launches, off in zip(cases, runs, offs):
            _, emin, emax, _, _, _ = launches[l % len(launches)]
            sl = slice(int(off), int(off) + c["R"])
            check_slots(tmin[sl], tmax[sl], emin, emax, c["valid"], ("multi", c["name"], l))
    assert forms == {"one", "split", "scalar"}


# ----------------------------------------------------------------------------------- knobs (tunable build)

def _need_tunable():
    from outlier_suppression_amd import ops
    if not ops.tunable_build():
        pytest.skip("obs_blocks and tok_nt are compile-time constants in the release library; "
                    "tests/test_gpu_tunable_build.py runs this test against libosq_hip_dbg.so in a child process")
    return ops


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_knobs_flat_obs_blocks(dtype_name, dev):
    """obs_blocks 1, 2, 3: second and third trips of the unrolled body, three remainder trips and the tail within a few
    thousand granules; obs_blocks 2048: all eight raw[j] of the finishing workgroup's read hold real partials."""
    ops = _need_tunable()
    per = MP.GRANULE[DTYPES[dtype_name][1]]
    try:
        for blocks in (1, 2, 3, MP.MAX_BLOCKS):
            ops.set_tuning("obs_blocks", blocks)
            for k, n in enumerate(MP.flat_knob_sizes(blocks, per)):
                run_flat(dev, dtype_name, n, True, 4000 + blocks + k, blocks=blocks, all_kinds=blocks != MP.MAX_BLOCKS)
    finally:
        ops.set_tuning("obs_blocks", MP.OBS_BLOCKS)


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_knobs_token_loads_without_the_streaming_hint(dtype_name, dev):
    """tok_nt = 0: the NT = false instantiations of token_minmax_vec_kernel on every vector case."""
    ops = _need_tunable()
    try:
        ops.set_tuning("tok_nt", 0)
        for case in cases_of(DTYPES[dtype_name][1], ("single", "head")):
            run_row_case(case, dtype_name, dev)
    finally:
        ops.set_tuning("tok_nt", 1)


# ----------------------------------------------------------------------------------- the one-launch step's load phase

FUSED_SHAPES = [(4, 16, 768), (4, 16, 1024), (3, 8, 3072), (2, 6, 4096)]
FUSED_KINDS = ("finite", "neg_zero_min", "pos_zero_max", "nan")          # (a), (c) both ways, (f)


def fused_columns(nv):
    """Feature columns of a token of 256 * nv floats read as (register slot u, lane, float4 component): every u, lanes 0 and 63,
    components 0 and 3.  fused_step.h: piece u of a row is the 1024 bytes at u * 1024, lane_off = lane * 16."""
    return [((u * 64 + lane) * 4 + comp, (u, lane, comp)) for u in range(nv) for lane in (0, 63) for comp in (0, 3)]


def fused_launch_seen(call):
    """Whether `call` ran a launch of the one-launch kernel family: the dispatch events armed for OSQ_TIME_FUSED_STEP are
    recorded only by that launch (as tests/test_gpu_fused_step.py does)."""
    import ctypes
    from outlier_suppression_amd import _hip
    lib = _hip.load()
    a, b = ctypes.c_void_p(), ctypes.c_void_p()
    _hip.check(lib.osq_timing_events_create(ctypes.byref(a), ctypes.byref(b)), "events")
    lib.osq_time_next_launch(_hip.TIME_FUSED_STEP, a, b)
    call()
    torch.cuda.synchronize()
    us = ctypes.c_float()
    seen = lib.osq_timing_elapsed_us(a, b, ctypes.byref(us)) == 0      # unrecorded events: error, nothing of that family ran
    lib.osq_time_next_launch(0, None, None)
    lib.osq_timing_events_destroy(a, b)
    return seen


def run_fused(dev, x_host, lengths, plants):
    """plants: [(kind name, (token, column) of the maximum, (token, column) of the minimum)] with token = (b, t).  Each is run
    in the one-launch form and with persistent=False; cur, min_val (running, from +-inf) and scale of both against the
    construction and the oracle's calculate_qparams.  The first and the last plant also check that the one-launch kernel was
    launched by the persistent call and not by the other."""
    from outlier_suppression_amd import ops, _hip
    from oracle import observer_oracle as OB
    kinds = {k[0]: k for k in MP.kinds_for(4)}
    B, T, H = x_host.shape
    L = torch.tensor(lengths, dtype=torch.int64, device=dev)
    up = torch.from_numpy(x_host).to(dev)
    pad = (torch.arange(T, device=dev)[None, :] >= L[:, None])[:, :, None]
    x = {0: up, 1: torch.where(pad, up, up.abs()), -1: torch.where(pad, up, -up.abs())}
    m = len(plants)
    out = {p: dict(mn=torch.full((m,), INF, device=dev), mx=torch.full((m,), -INF, device=dev), cur=torch.zeros(m, 2, device=dev),
                   scale=torch.ones(m, device=dev), zp=torch.zeros(m, dtype=torch.int32, device=dev)) for p in (True, False)}
    want = np.zeros((m, 2), np.float32)
    for r, (name, (tok_a, col_a), (tok_b, col_b)) in enumerate(plants):
        _, sign, vmax, vmin = kinds[name]
        t = x[sign]
        old_a, old_b = t[tok_a[0], tok_a[1], col_a].clone(), t[tok_b[0], tok_b[1], col_b].clone()
        t[tok_a[0], tok_a[1], col_a] = float(vmax)
        if vmin is not None:
            t[tok_b[0], tok_b[1], col_b] = float(vmin)
        for p, o in out.items():
            def call(p=p, o=o):
                ops.observe_tokens_fake_quant(t, 1, L, False, 1.0, _hip.UPDATE_RUNNING, 0, o["mn"][r:r + 1], o["mx"][r:r + 1], 0, 63, False,
                                              o["scale"][r:r + 1], o["zp"][r:r + 1], _hip.PARAM_FIXED, 1.0, cur=o["cur"][r], persistent=p)
            if r in (0, m - 1):                                  # the entry point falls back to three launches without a word: see that it did not
                assert fused_launch_seen(call) == p, (x_host.shape, "persistent" if p else "three launches", "one-launch kernel ran: %s" % (not p))
            else:
                call()
        t[tok_b[0], tok_b[1], col_b] = old_b
        t[tok_a[0], tok_a[1], col_a] = old_a
        want[r] = np.nan if name == "nan" else (vmin, vmax)
    ops.check_persistent("planted load-phase cases")
    scale_want = np.asarray(OB.calculate_qparams(want[:, 0], want[:, 1], 0, 63, False)[0], np.float32)
    for p, o in out.items():
        cur, mn, mx, sc = (o[k].cpu().numpy() for k in ("cur", "mn", "mx", "scale"))
        for r, plant in enumerate(plants):
            tag = (x_host.shape, "persistent" if p else "three launches", plant)
            assert bits_equal(cur[r], want[r]), (tag, "cur", cur[r].tolist(), want[r].tolist())
            assert bits_equal(np.array([mn[r], mx[r]]), want[r]), (tag, "min_val / max_val", mn[r], mx[r])
            assert bits_equal(sc[r:r + 1], scale_want[r:r + 1]), (tag, "scale", sc[r], scale_want[r])


def fused_input(shape, lengths, seed):
    x = MP.grid_values(np.random.default_rng(seed), shape)
    x[..., 0::97] *= np.float32(0.5)
    for b, ln in enumerate(lengths):                                       # padded tokens hold what would show if it were observed
        for t in range(ln, shape[1]):
            x[b, t] = MP.PAD_VALUES[(b + t) % len(MP.PAD_VALUES)]
    return x


@pytest.mark.parametrize("shape", FUSED_SHAPES)
def test_fused_step_load_phase(shape, dev):
    """prune = 0 at the four shapes test_gpu_fused_step.py runs in the one-launch form: the extremum at every register slot
    u = 0..NV-1 x lanes 0 / 63 x float4 components 0 / 3, in the first valid token, the last valid token and one between;
    kinds (a), (c) and (f) cycle so that each meets every u, lane, component and token choice (asserted below).  At these
    sizes every token is a wave's FIRST (register-held) one: none of the four shapes has an LDS-held or streamed token --
    test_fused_step_lds_and_streamed_tokens has small shapes that do."""
    B, T, H = shape
    lengths = [T] + [max(1, T - 3 - b) for b in range(1, B)]
    valid = [(b, t) for b in range(B) for t in range(lengths[b])]
    tokens = {"first": valid[0], "last": valid[-1], "middle": valid[len(valid) // 2]}
    cols = fused_columns(H // 256)
    plants, met = [], set()
    for i, (col, (u, lane, comp)) in enumerate(cols):
        k = u + 2 * (lane == 63) + (comp == 3)                       # two launches per column; the cycling is checked just below
        for kind in (FUSED_KINDS[k % 4], FUSED_KINDS[(k + 2) % 4]):
            which, other = ("first", "last", "middle")[i % 3], ("last", "middle", "first")[i % 3]
            col_b = cols[(i + len(cols) // 2 + 1) % len(cols)][0]
            plants.append((kind, (tokens[which], col), (tokens[other], col_b)))
            met |= {(kind, "u", u), (kind, "lane", lane), (kind, "comp", comp), (kind, "token", which)}
    full = {(k, "u", u) for k in FUSED_KINDS for u in range(H // 256)} | {(k, a, v) for k in FUSED_KINDS for a in ("lane", "comp") for v in ((0, 63) if a == "lane" else (0, 3))}
    assert full <= met, sorted(full - met, key=str)
    assert {(k, "token", w) for k in FUSED_KINDS for w in ("first", "last", "middle")} <= met
    run_fused(dev, fused_input(shape, lengths, sum(shape)), lengths, plants)


@pytest.mark.parametrize("share", ["lds", "streamed"])
def test_fused_step_lds_and_streamed_tokens(share, dev):
    """Small shapes with tokens outside the registers, on a grid of one workgroup per CU (G = CUs - 2 streaming
    workgroups, 16 G waves; wave w's k-th token is number k * 16 G + ... of the valid tokens): [B,128,1024] (NV = 4: 4
    register tokens, then 2 in LDS) with more than 4 * 16 G tokens, and [B,64,3072] (NV = 12: 1 register token, none in
    LDS, the rest streamed) with more than 16 G."""
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    nwv = (cus - 2) * MP.FUSED_WAVES
    if share == "lds":
        nv, T = 4, 128
        first = (MP.FUSED_HOLD_REGS // nv) * nwv
        assert MP.FUSED_HOLD_LDS // nv >= 1
    else:
        nv, T = 12, 64
        first = (MP.FUSED_HOLD_REGS // nv + MP.FUSED_HOLD_LDS // nv) * nwv
    B = (first + 64 + T - 1) // T + 1
    assert B * T <= 32768 and B <= 1024
    lengths = [T] * (B - 1) + [T - 5]
    V = sum(lengths)
    assert V > first + 40

    def tok(j):                                                            # every sample before the last is full
        return divmod(j, T)

    cols = fused_columns(nv)
    plants = []
    for i, kind in enumerate(FUSED_KINDS * 3):
        a = cols[(5 * i + 1) % len(cols)][0]
        b = cols[(5 * i + 2 * nv + 2) % len(cols)][0]
        ja, jb = (first + 3 + i, 7 + i) if i % 2 == 0 else (V - 1 - i, first + 20 + i)
        plants.append((kind, (tok(ja), a), (tok(jb), b)))
    run_fused(dev, fused_input((B, T, 256 * nv), lengths, 17 + nv), lengths, plants)

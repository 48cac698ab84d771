"""osq_token_range_finalize through ops.token_range_finalize at every selection path and size class of
tests/_token_finalize.py (tests/test_oracle_token_finalize.py asserts what those tables reach): the two-workgroup kernel
(select), the single-workgroup kernel (single) and the three-launch form (wide), each forced with the knobs "final_fast",
"select_shortcut" and set_wide_min_slots or reached through the layouts select rejects.  `cur` holds one NaN payload word
before every launch, the result is the oracle's word for word (NaN equal to NaN), every problem runs twice in a row (the
rendezvous word and the wide form's global scratch must be idle again), a problem of another implementation follows, the
input arrays are compared unchanged, and the timing hook of token_select_kernel says whether the predicted implementation ran.
All three kernels clamp a length beyond T to T; the "beyond_T" pattern holds them to it.
OSQ_TOKEN_FINALIZE_OUT=<path> makes the last test write what ran (profiles/token_finalize_paths.txt)."""
import contextlib
import ctypes
import os

import numpy as np
import pytest
import torch

import _token_finalize as TF
from _minmax_positions import case_seed
from conftest import bits_equal

pytestmark = pytest.mark.gpu
F32 = np.float32
IMPLS = ("select", "single", "wide")
CASES = TF.value_cases()
BY_NAME = {c["name"]: c for c in CASES}
RECORD = {impl: dict(classes={}, inst=set(), problems=0, launches=0) for impl in IMPLS}      # what test_z_report writes
OUTCOME = {}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from outlier_suppression_amd import _hip
    _hip.load()
    return torch.device("cuda:0")


@contextlib.contextmanager
def knobs(final_fast=1, wide_min=TF.WIDE_DEFAULT, shortcut=1, **_):
    from outlier_suppression_amd import ops
    try:
        ops.set_tuning("final_fast", final_fast)
        ops.set_tuning("select_shortcut", shortcut)
        ops.set_wide_min_slots(wide_min)
        yield
    finally:
        ops.set_tuning("final_fast", 1)
        ops.set_tuning("select_shortcut", 1)
        ops.set_wide_min_slots(TF.WIDE_DEFAULT)


def select_launch_seen(call):
    """Whether `call` launched token_select_kernel (the pattern of fused_launch_seen, tests/test_gpu_fused_select.py)."""
    from outlier_suppression_amd import _hip
    lib = _hip.load()
    a, b = ctypes.c_void_p(), ctypes.c_void_p()
    _hip.check(lib.osq_timing_events_create(ctypes.byref(a), ctypes.byref(b)), "events")
    lib.osq_time_next_launch(_hip.TIME_TOKEN_SELECT, a, b)
    call()
    torch.cuda.synchronize()
    us = ctypes.c_float()
    seen = lib.osq_timing_elapsed_us(a, b, ctypes.byref(us)) == 0
    lib.osq_time_next_launch(0, None, None)
    lib.osq_timing_events_destroy(a, b)
    return seen


class Problem:
    """One problem on the device: its arrays (at a chosen distance from a 16-byte boundary), lengths and expected words."""

    def __init__(self, dev, tmin, tmax, B, T, lengths, p, off_min=0, off_max=0):
        self.dev, self.B, self.T, self.p = dev, B, T, F32(p)
        S = B * T
        self.host = (tmin, tmax)
        self.arr = []
        for h, off in ((tmin, off_min), (tmax, off_max)):
            buf = torch.full((S + 8,), float("inf"), dtype=torch.float32, device=dev)
            view = buf[4 + off:4 + off + S]
            assert view.data_ptr() % 16 == 4 * off
            view.copy_(torch.from_numpy(h))
            self.arr.append((buf, view))
        self.L = None if lengths is None else torch.tensor(lengths, dtype=torch.int64, device=dev)
        ok = TF.valid_mask(B, T, lengths if lengths is not None else [T] * B)
        self.V = int(ok.sum())
        self.want = TF.expected_cur(tmin[ok], tmax[ok], p) if self.V else None
        self.cur = torch.empty(2, dtype=torch.float32, device=dev)

    def launch(self, rule=0, cnt=0, state=None, sink=None, bit=6, sym=False):
        from outlier_suppression_amd import ops
        from oracle import observer_oracle as OB
        qmin, qmax = OB.quant_range(bit, sym)
        self.cur.view(torch.int32).fill_(TF.SENTINEL)
        mn, mx = state if state is not None else (None, None)
        ops.token_range_finalize(self.arr[0][1], self.arr[1][1], self.B, self.T, self.L, True, float(self.p), rule, cnt, mn, mx,
                                 qmin, qmax, sym, sink, self.cur)

    def words(self):
        return self.cur.cpu().numpy()

    def check_inputs(self, tag):
        for (buf, view), h, what in zip(self.arr, self.host, ("token_min", "token_max")):
            assert bits_equal(view.cpu().numpy(), h), (tag, what, "the input array changed")
            rest = torch.cat([buf[:view.storage_offset()], buf[view.storage_offset() + view.numel():]])
            assert bool(torch.isinf(rest).all()), (tag, what, "a word beside the array changed")

    def run(self, impl, tag, times=2):
        """`times` launches in a row: the dispatch as predicted, the oracle's words every time, the inputs unchanged."""
        got = None
        for i in range(times):
            seen = select_launch_seen(self.launch)
            assert seen == (impl == "select"), (tag, "predicted", impl, "token_select_kernel launched" if seen else "no token_select_kernel launch")
            got = self.words()
            if self.V:
                assert bits_equal(got, self.want), (tag, impl, "launch", i, got.tolist(), self.want.tolist(), got.view(np.uint32).tolist(), self.want.view(np.uint32).tolist())
            else:
                assert got.view(np.uint32).tolist() == [TF.SENTINEL] * 2, (tag, "nothing observed, but cur was written", got)
            RECORD[impl]["launches"] += 1
        self.check_inputs(tag)
        return got


def note(impl, inst, classes, name):
    RECORD[impl]["inst"].add(inst)
    RECORD[impl]["problems"] += 1
    for c in classes:
        RECORD[impl]["classes"].setdefault(c, []).append(name)


def follower(dev, impl):
    """A small problem of the implementation after `impl`, with the knobs that reach it: run after a problem so that the scratch
    the first one left (rendezvous word, wide state, tickets) cannot leak into another kernel."""
    nxt = IMPLS[(IMPLS.index(impl) + 1) % 3]
    case = BY_NAME["off_first_batch"]
    B, T, L, kn = TF.value_geometry(nxt, case["vals"].size, 0)
    tmin, tmax, _ = TF.place(case["vals"], case["other"], 0, B, T, L, 5, "nan")
    return nxt, kn, Problem(dev, tmin, tmax, B, T, L, case["p"])


def sides_of(tmin, tmax, ok):
    return tmax[ok], -tmin[ok]


def classes_of(impl, tmin, tmax, ok, p, B, T, L):
    s0, s1 = sides_of(tmin, tmax, ok)
    if impl == "select":
        loader = TF.select_side_model(B, T, L)
        return set().union(*(TF.select_classes_of(TF.select_report(v, p), loader) for v in (s0, s1)))
    if impl == "single":
        return TF.single_classes_of(TF.single_path(s0, s1, p, B * T))
    geo = TF.wide_geometry(B, T, L)
    return set().union(*(TF.wide_classes_of(TF.wide_path(v, p), geo) for v in (s0, s1)))


def run_problem(dev, impl, kn, tmin, tmax, ok, B, T, L, p, name, off_min=0, off_max=0):
    pred, inst = TF.dispatch(B, T, kn["final_fast"], kn["wide_min"], off_min, off_max)
    assert pred == impl, (name, pred, impl)
    prob = Problem(dev, tmin, tmax, B, T, L, p, off_min, off_max)
    with knobs(**kn):
        got = prob.run(impl, name)
    if impl == "select":                                         # the register threshold pass instead of the shortcut: the same words
        with knobs(**dict(kn, shortcut=0)):
            full = prob.run(impl, (name, "select_shortcut 0"), times=1)
        assert bits_equal(got, full), (name, "shortcut on / off", got, full)
    note(impl, inst, classes_of(impl, tmin, tmax, ok, p, B, T, L) if prob.V > 0 and np.isfinite(prob.want).all() else (), name)
    return prob


# ----------------------------------------------------------------------------------- value cases

@pytest.mark.parametrize("impl", IMPLS)
def test_value_cases(impl, dev):
    """Every value case (tests/_token_finalize.py, value_cases) carried by token_max (side 0) and by -token_min (side 1), in
    two seeded permutations, padding NaN or huge in turn: the oracle's words, twice in a row; select with the shortcut on and
    off; after every case a problem of another implementation."""
    nxt, nkn, nprob = follower(dev, impl)
    for n, case in enumerate(CASES):
        B, T, L, kn = TF.value_geometry(impl, case["vals"].size, n)
        for side in (0, 1):
            tmin, tmax, ok = TF.place(case["vals"], case["other"], side, B, T, L, case_seed(case["name"]) + side, ("nan", "huge")[n % 2])
            run_problem(dev, impl, kn, tmin, tmax, ok, B, T, L, case["p"], "%s/side%d" % (case["name"], side))
        with knobs(**nkn):
            nprob.run(nxt, (case["name"], "followed by", nxt), times=1)
    OUTCOME["value cases, " + impl] = "passed"


# ----------------------------------------------------------------------------------- size classes

SIZES = ([("select", B, T, "layout") for B, T in TF.SELECT_SIZES] + [("single", B, T, how) for B, T, how in TF.SINGLE_SIZES] +
         [("wide", B, T, "wide_min_1024") for B, T in TF.WIDE_SIZES])


@pytest.mark.parametrize("impl,B,T,how", SIZES)
def test_size_classes(impl, B, T, how, dev):
    """Every size class x every length pattern (full -- without a lengths array on even B + T --, one token, zero and full
    alternating, T - 1, 1, lengths beyond T), filled with the scalable kinds in turn (rank r + 1 one ulp above rank r across a
    coarse bin, a first-level bin, inside one; duplicates; a spread), padding NaN or huge in turn.  single is reached the way
    `how` says: T < 4, a slot count that is no multiple of 4, final_fast = 0, token_min or token_max one element off a 16-byte
    boundary, or -- 32769 slots, the uncached body -- wide_min_slots raised."""
    kn = dict(final_fast=1, wide_min=TF.WIDE_DEFAULT, off_min=0, off_max=0)
    if impl == "single":
        kn = TF.single_knobs(how)
    elif impl == "wide":
        kn["wide_min"] = TF.WIDE_FLOOR
    nxt, nkn, nprob = follower(dev, impl)
    ran = 0
    for i, (pattern, L, kind, pad) in enumerate(TF.size_problems(impl, B, T)):
        V = sum(TF.clamp_lengths(L, T))
        vals, p = TF.scalable_values(kind, V, seed=B + T)
        side = (i + B) % 2
        tmin, tmax, ok = TF.place(vals, TF.default_other(V), side, B, T, L, B * 31 + T + i, pad)
        lengths = None if pattern == "full" and (B + T) % 2 == 0 else L
        run_problem(dev, impl, kn, tmin, tmax, ok, B, T, lengths, p, "size %dx%d/%s/%s/%s/side%d" % (B, T, how, pattern, kind, side),
                    kn["off_min"], kn["off_max"])
        ran += 1
    assert ran >= 3
    with knobs(**nkn):
        nprob.run(nxt, ((B, T), "followed by", nxt), times=1)
    OUTCOME["size %s %dx%d %s" % (impl, B, T, how)] = "passed"


def test_wide_threshold_floor():
    """osq_set_wide_min_slots refuses a threshold below 1024 slots, so the wide form cannot be reached at 513 slots: the
    smallest wide problems above have 1024 and 1025 slots (two and three workgroups)."""
    from outlier_suppression_amd import ops
    with pytest.raises(Exception):
        ops.set_wide_min_slots(513)
    ops.set_wide_min_slots(TF.WIDE_DEFAULT)


# ----------------------------------------------------------------------------------- finish step

FINISH_CASES = ("off_first_batch", "edge_same_first_level_bin", "dups_rank_last", "zeros_of_both_signs", "clip_rule_lo_above_up", "one_token")


@pytest.mark.parametrize("impl", IMPLS)
def test_finish_step(impl, dev):
    """The running statistic and the qparams behind each implementation, word for word against OB.ObserverState: UPDATE_AVERAGE
    at cnt 0 (state +-inf) and cnt 3, UPDATE_RUNNING with a state, UPDATE_NONE; a qparams sink symmetric and not, with an int32
    and an fp32 zero point; and no sink."""
    from outlier_suppression_amd import ops, _hip
    forms = [(_hip.UPDATE_AVERAGE, 0, (np.inf, -np.inf)), (_hip.UPDATE_AVERAGE, 3, (-2.5, 1.75)), (_hip.UPDATE_RUNNING, 2, (-0.75, 1.0)),
             (_hip.UPDATE_RUNNING, 2, (-9.0, 9.0)), (_hip.UPDATE_NONE, 0, None)]
    sinks = [(False, torch.int32, 6), (True, torch.float32, 8), (False, torch.float32, 4), (True, torch.int32, 2), None]
    for n, name in enumerate(FINISH_CASES):
        case = BY_NAME[name]
        B, T, L, kn = TF.value_geometry(impl, case["vals"].size, n)
        tmin, tmax, ok = TF.place(case["vals"], case["other"], n % 2, B, T, L, 17 + n, ("nan", "huge")[n % 2])
        prob = Problem(dev, tmin, tmax, B, T, L, case["p"])
        for f, (rule, cnt, state) in enumerate(forms):
            for s, sk in enumerate(sinks):
                sym, zdt, bit = sk if sk else (False, torch.int32, 6)
                st = None if state is None else (torch.tensor([state[0]], dtype=torch.float32, device=dev), torch.tensor([state[1]], dtype=torch.float32, device=dev))
                sink = ops.QParamSink(torch.tensor([0.125], device=dev), torch.tensor([3.0], device=dev).to(zdt)) if sk else None
                with knobs(**kn):
                    prob.launch(rule, cnt, st, sink, bit, sym)
                tag = (impl, name, "rule", rule, "cnt", cnt, state, sk)
                assert bits_equal(prob.words(), prob.want), (tag, prob.words(), prob.want)
                mn, mx, scale, zp = TF.expected_finish(prob.want, rule, cnt, state if state else (0.0, 0.0), bit, sym)
                if st is not None:
                    assert bits_equal(st[0].cpu().numpy(), np.array([mn], F32)) and bits_equal(st[1].cpu().numpy(), np.array([mx], F32)), \
                        (tag, "min_val / max_val", st[0].item(), st[1].item(), mn, mx)
                if sink is not None:
                    assert bits_equal(sink.scale.cpu().numpy(), np.array([scale], F32)), (tag, "scale", sink.scale.item(), scale)
                    if zdt == torch.int32:
                        assert sink.zero_point.item() == int(zp), (tag, "zero_point", sink.zero_point.item(), zp)
                    else:
                        assert bits_equal(sink.zero_point.cpu().numpy(), np.array([zp], F32)), (tag, "zero_point", sink.zero_point.item(), zp)
                RECORD[impl]["launches"] += 1
        prob.check_inputs((impl, name))
    OUTCOME["finish step, " + impl] = "passed"


# ----------------------------------------------------------------------------------- NaN and empty

NAN_SIZES = SIZES


@pytest.mark.parametrize("impl,B,T,how", NAN_SIZES)
def test_nan_and_empty(impl, B, T, how, dev):
    """A NaN at the first valid slot (of token_max) and at the last valid slot (of token_min): (NaN, NaN).  A NaN only in the
    padding: the result of the same problem with huge padding.  All lengths 0: cur, the running statistic and the qparams are
    untouched."""
    from outlier_suppression_amd import ops, _hip
    kn = dict(final_fast=1, wide_min=TF.WIDE_DEFAULT, off_min=0, off_max=0)
    if impl == "single":
        kn = TF.single_knobs(how)
    elif impl == "wide":
        kn["wide_min"] = TF.WIDE_FLOOR
    L = [max(T - 1 - b % 2, 1) for b in range(B)]
    V = sum(L)
    vals, p = TF.scalable_values("spread", V, seed=3)
    tmin, tmax, ok = TF.place(vals, TF.default_other(V), 0, B, T, L, 7, "huge")
    first, last = np.flatnonzero(ok)[[0, -1]]
    name = "nan %dx%d/%s" % (B, T, how)
    for what, arr_i, where in (("first valid slot", 1, first), ("last valid slot", 0, last)):
        a = [tmin.copy(), tmax.copy()]
        a[arr_i][where] = np.nan
        prob = run_problem(dev, impl, kn, a[0], a[1], ok, B, T, L, p, "%s/%s" % (name, what), kn["off_min"], kn["off_max"])
        assert np.isnan(prob.want).all() and np.isnan(prob.words()).all()
    if not ok.all():
        a = [tmin.copy(), tmax.copy()]
        pads = np.flatnonzero(~ok)
        a[1][pads[0]] = np.nan
        a[0][pads[-1]] = np.nan
        prob = run_problem(dev, impl, kn, a[0], a[1], ok, B, T, L, p, name + "/padding", kn["off_min"], kn["off_max"])
        assert np.isfinite(prob.want).all()
    empty = Problem(dev, tmin, tmax, B, T, [0] * B, p, kn["off_min"], kn["off_max"])
    st = (torch.tensor([-2.5], device=dev), torch.tensor([1.75], device=dev))
    sink = ops.QParamSink(torch.tensor([0.125], device=dev), torch.tensor([3.0], device=dev))
    with knobs(**kn):
        seen = select_launch_seen(lambda: empty.launch(_hip.UPDATE_AVERAGE, 3, st, sink))
    assert seen == (impl == "select")
    assert empty.words().view(np.uint32).tolist() == [TF.SENTINEL] * 2, (name, "all lengths 0: cur was written")
    assert (st[0].item(), st[1].item(), sink.scale.item(), sink.zero_point.item()) == (-2.5, 1.75, 0.125, 3.0), (name, "all lengths 0: the state moved")
    run_problem(dev, impl, kn, tmin, tmax, ok, B, T, L, p, name + "/after empty", kn["off_min"], kn["off_max"])    # the scratch is idle
    OUTCOME["nan and empty, %s %dx%d %s" % (impl, B, T, how)] = "passed"


# ----------------------------------------------------------------------------------- record

def test_z_report():
    """What this run executed, per implementation: the instantiations, every coverage class with the problems that reached
    it, and the tests that passed.  Every class of tests/_token_finalize.py must have been reached on the device too."""
    if not any(r["problems"] for r in RECORD.values()):          # run on its own: nothing to report
        return
    names = dict(select="token_select_kernel<R4>, R4 =", single="token_finalize_kernel<SLOTS>, SLOTS =",
                 wide="wide_hist_kernel / wide_collect_kernel / wide_select_kernel, workgroups =")
    lines = ["osq_token_range_finalize: what tests/test_gpu_token_finalize.py ran on the device.  Every result was compared with the",
             "oracle word for word.  The implementation of a problem is predicted by the restated dispatch (tests/_token_finalize.py,",
             "dispatch) and checked against the timing hook of token_select_kernel (seen where select is predicted, not seen elsewhere).", ""]
    wanted = dict(select=TF.SELECT_CLASSES, single=TF.SINGLE_CLASSES, wide=TF.WIDE_CLASSES)
    complete = len(OUTCOME) == 3 + len(SIZES) + 3 + len(NAN_SIZES)
    missing_all = []
    for impl in IMPLS:
        r = RECORD[impl]
        lines += ["== %s: %d problems, %d launches" % (impl, r["problems"], r["launches"]),
                  "   %s %s" % (names[impl], ", ".join(str(i) for i in sorted(r["inst"])))]
        for c in wanted[impl]:
            hit = r["classes"].get(c, [])
            lines.append("   %-52s %4d  %s" % (" ".join(str(x) for x in c), len(hit), ", ".join(hit[:2]) if hit else "NOT REACHED"))
            if not hit:
                missing_all.append((impl, c))
        lines.append("")
    lines += ["== tests"] + ["   %-60s %s" % kv for kv in sorted(OUTCOME.items())]
    lines += ["", "%d of %d test cases of this file passed before this report" % (len(OUTCOME), 3 + len(SIZES) + 3 + len(NAN_SIZES))]
    print("\n".join(lines))
    out = os.environ.get("OSQ_TOKEN_FINALIZE_OUT")
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
    if complete:                                                 # a partial run (-k) reaches what it reaches
        assert not missing_all, missing_all
        assert RECORD["select"]["inst"] == {1, 2, 4, 8} and RECORD["single"]["inst"] == {4, 8, 16, 32, 0}
        assert {2, 24} <= RECORD["wide"]["inst"]

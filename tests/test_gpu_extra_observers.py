"""The ten kernels of csrc/observers_extra.hip at every launch shape, against the float64 / torch.histc / oracle references
of tests/_extra_observers.py (whose promises tests/test_oracle_extra_observers.py checks on the CPU):

  1. moments (LSQPlusObserver): moments_flat_kernel and moments_channels_kernel within 4 ulp of the range computed from
     two-pass float64 moments -- every tail length, a misaligned base, the 1024-workgroup cap, |mean| up to 10^4 std;
  2. quantile (AvgQuantileObserver): abs_hist_kernel + quantile_finalize_kernel bit-equal to torch.histc + the oracle's clip
     and update over three batches, the table left zero -- the 256-workgroup cap, masked views, elements on bin edges, a
     target bin in every wave of the finaliser.  Every case observes fewer than 2^24 elements: above that the reference's
     fp32 running total stops counting single elements, which the kernel's integer prefix does not imitate -- not part of
     this suite;
  3. MSE grid (MSEObserver / AvgMSEObserver): the loss of EVERY candidate against the oracle's, the committed range against
     the device's own losses, the chosen candidate against the oracle's minimum -- through mse_grid_all_kernel (pieces,
     tokens, flat) and through the launch-per-32-candidates form; mse_grid_rows_kernel per channel."""
import ctypes

import numpy as np
import pytest
import torch

import _extra_observers as EO
from oracle import observer_oracle as OB

pytestmark = pytest.mark.gpu

F32 = np.float32


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from outlier_suppression_amd import _hip
    _hip.load()          # fail loudly if the HIP library is missing
    return torch.device("cuda:0")


def flat_on_device(x, offset, dev):
    """x as a dense 1-D device tensor whose base is `offset` floats past a 16-byte boundary."""
    x = np.ascontiguousarray(x, dtype=F32).reshape(-1)
    base = torch.empty(x.size + 4, dtype=torch.float32, device=dev)
    assert base.data_ptr() % 16 == 0
    t = base[offset:offset + x.size]
    t.copy_(torch.from_numpy(x))
    assert t.data_ptr() % 16 == 4 * offset
    return t


def site_on_device(site, dev):
    """-> (observed tensor, lengths tensor or None)."""
    if site.lengths is None:
        return flat_on_device(site.mem, site.offset, dev), None
    return site.view(torch.from_numpy(site.mem).to(dev)), torch.from_numpy(site.lengths).to(dev)


# ----------------------------------------------------------------------------------- 1. moments

def device_moments(x, ch_axis=-1, sink=None, quant=(-128, 127)):
    from outlier_suppression_amd import ops
    ch = 1 if ch_axis == -1 else x.shape[ch_axis]
    mn, mx = torch.zeros(ch, device=x.device), torch.zeros(ch, device=x.device)
    ops.observe_moments(x, ch_axis, mn, mx, quant[0], quant[1], True, sink)
    return mn.cpu().numpy(), mx.cpu().numpy()


def check_moments(got, want, tag, fails):
    """Bound and derivation: _extra_observers.moment_range."""
    (g_mn, g_mx), (mn, mx, bound) = got, want
    with np.errstate(invalid="ignore"):
        err = np.nanmax(np.abs(np.concatenate([np.ravel(g_mn - mn), np.ravel(g_mx - mx)]).astype(np.float64)) / np.max(bound)) \
            if not np.isnan(mn).all() else 0.0
    print(tag, "error / bound", float(err))
    if not (EO.moment_within(g_mn, mn, bound) and EO.moment_within(g_mx, mx, bound)):
        fails.append((tag, g_mn, mn, g_mx, mx, bound))


@pytest.mark.parametrize("mean,std", EO.MOMENT_PAIRS)
def test_moments_flat(mean, std, dev):
    """Every tail length, one and several workgroups, aligned and 4 bytes off: min / max within 4 ulp32(|mean| + 3 std) of
    mean32 -+ 3 std32 from two-pass float64 moments; NaN for one element, as torch.std."""
    k, fails = EO.MOMENT_PAIRS.index((mean, std)), []
    for n in EO.MOMENT_NS:
        x = EO.moment_data(n, mean, std, k)
        want = EO.moment_reference(x)
        assert np.isnan(want[0]) == (n == 1)
        for off in (0, 1):
            g = device_moments(flat_on_device(x, off, dev))
            check_moments((g[0][0], g[1][0]), want, (n, off), fails)
    assert not fails, fails


def test_moments_flat_at_the_block_cap(dev):
    """4 Mi + 3 elements: 1024 workgroups, a second grid-stride trip, a tail of 3."""
    fails = []
    for k, (mean, std) in enumerate(EO.MOMENT_PAIRS):
        x = EO.moment_data(EO.MOMENT_BIG_N, mean, std, k)
        want = EO.moment_reference(x)
        for off in (0, 1) if k == 4 else (0,):
            g = device_moments(flat_on_device(x, off, dev))
            check_moments((g[0][0], g[1][0]), want, (mean, std, off), fails)
    assert not fails, fails


def test_moments_constant_data(dev):
    """std is exactly 0: min == max == the value."""
    for c in EO.MOMENT_CONSTANTS:
        for n in EO.MOMENT_CONSTANT_NS:
            for off in (0, 1):
                mn, mx = device_moments(flat_on_device(np.full(n, c, dtype=F32), off, dev))
                want = EO.moment_reference(np.full(n, c, dtype=F32))
                assert want[0] == want[1] == F32(c)
                assert EO.moment_within(mn[0], want[0], want[2]) and EO.moment_within(mx[0], want[1], want[2]), (c, n, off, mn, mx)
    mn, mx = device_moments(torch.full((3, 5, 7), 2.5, device=dev), 1)
    assert (mn == 2.5).all() and (mx == 2.5).all()


@pytest.mark.parametrize("shape,axis", EO.MOMENT_CHANNEL_CASES)
def test_moments_channels(shape, axis, eq32, dev):
    """One workgroup per channel: inner > 256, inner == 1, outer > 1, one element per channel (NaN rows); the qparams a
    sink receives are the oracle's calculate_qparams of the range the launch wrote."""
    from outlier_suppression_amd import ops
    x = EO.moment_channel_data(shape, axis)
    want = EO.moment_reference(x, axis)
    ch = shape[axis]
    sink = ops.QParamSink(torch.zeros(ch, device=dev), torch.ones(ch, dtype=torch.int32, device=dev))
    fails = []
    got = device_moments(torch.from_numpy(x).to(dev), axis, sink, (-8, 7))
    check_moments(got, want, shape, fails)
    assert not fails, fails
    if not np.isnan(want[0]).any():
        scale, zp = OB.calculate_qparams(got[0], got[1], -8, 7, True)
        assert eq32(sink.scale.cpu().numpy(), scale) and np.array_equal(sink.zero_point.cpu().numpy(), zp)


def test_lsqplus_observer_on_bf16(eq32, dev):
    """LSQPlusObserver given bf16: the moments of the widened values, per tensor and per channel."""
    from outlier_suppression_amd.quantization.quantized_module import ObserverDict
    fails = []
    x = torch.from_numpy(EO.moment_data(20483, 10.0, 0.1, 3)).bfloat16()
    ob = ObserverDict["LSQPlusObserver"](bit=8, symmetric=True, ch_axis=-1).to(dev)
    ob(x.to(dev))
    check_moments((ob.min_val.cpu().numpy().reshape(()), ob.max_val.cpu().numpy().reshape(())), EO.moment_reference(x.float().numpy()),
                  "per tensor", fails)
    w = torch.from_numpy(EO.moment_channel_data((7, 300), 0)).bfloat16()
    ob = ObserverDict["LSQPlusObserver"](bit=4, symmetric=True, ch_axis=0).to(dev)
    ob(w.to(dev))
    check_moments((ob.min_val.cpu().numpy(), ob.max_val.cpu().numpy()), EO.moment_reference(w.float().numpy(), 0), "per channel", fails)
    assert not fails, fails


# ----------------------------------------------------------------------------------- 2. quantile

@pytest.mark.parametrize("name", EO.QUANTILE_CASES)
def test_quantile(name, eq32, dev):
    """AvgQuantileObserver over three batches at each threshold: min_val / max_val bit-equal to torch.histc (CPU) + the
    oracle's clip + the average rule after every batch; the histogram table is zero again after every call."""
    from outlier_suppression_amd.quantization.quantized_module import ObserverDict
    sites, thresholds = EO.quantile_case(name)
    on_dev = [site_on_device(s, dev) for s in sites]
    ref = EO.quantile_reference(name)
    for thr in thresholds:
        ob = ObserverDict["AvgQuantileObserver"](bit=6, threshold=thr).to(dev)
        for it, (s, (x, L)) in enumerate(zip(sites, on_dev)):
            ob(x, L, s.seq_pos)
            got = (ob.min_val.cpu().numpy(), ob.max_val.cpu().numpy())
            assert eq32(got[0], ref[thr][it][0]) and eq32(got[1], ref[thr][it][1]), (name, thr, it, got, ref[thr][it])
            assert int(ob._hist.count_nonzero().item()) == 0, (name, thr, it)
        assert ob.cnt == 3


# ----------------------------------------------------------------------------------- 3. MSE grid

GUARD = 32
SENTINEL = 12345.0


def device_grid(x, lengths, seq_pos, cur, quant, symmetric, side, rule, cnt, mn, mx, path):
    """One search -> the loss of every candidate (host array).  path "one_launch": ops.mse_grid_tensor (mse_grid_all_kernel);
    "per32": the C entry point with a scratch of exactly osq_mse_grid_candidates() floats -- smaller than
    osq_mse_grid_scratch_bytes(), so the library launches mse_grid_loss_kernel once per 32 candidates (include/osq_hip.h)."""
    from outlier_suppression_amd import _hip, ops
    two_d = side == "no" and not symmetric
    if path == "one_launch":
        losses = ops.mse_grid_tensor(x, lengths, seq_pos, cur, quant[0], quant[1], symmetric, side, two_d, rule, cnt, mn, mx)
        return losses.cpu().numpy()
    lib = _hip.load()
    xs, n, view, L = ops._source(x, lengths, seq_pos)
    n_cand = int(lib.osq_mse_grid_candidates(quant[0], quant[1], int(two_d)))
    assert 4 * n_cand < int(lib.osq_mse_grid_scratch_bytes(quant[0], quant[1], int(two_d)))
    scratch = torch.full((n_cand + GUARD,), SENTINEL, device=x.device)
    _hip.check(lib.osq_mse_grid_tensor(_hip.ptr(xs), n, ctypes.byref(view) if view is not None else None, _hip.ptr(L), _hip.ptr(cur),
                                       quant[0], quant[1], int(symmetric), ops.SIDE[side], int(two_d), _hip.ptr(scratch), 4 * n_cand,
                                       rule, int(cnt), _hip.ptr(mn), _hip.ptr(mx), None, None, _hip.ZP_INT32,
                                       _hip.ptr(_hip.workspace(x.device)), _hip.stream_ptr(x.device)), "mse_grid_tensor")
    out = scratch.cpu().numpy()
    assert (out[n_cand:] == F32(SENTINEL)).all(), "the launch wrote past the candidates' losses"
    return out[:n_cand]


@pytest.mark.parametrize("path", ["one_launch", "per32"])
@pytest.mark.parametrize("name,kind", EO.GRID_UNITS)
def test_mse_grid_tensor(name, kind, path, eq32, dev):
    """Two batches under the running and under the average rule.  After every batch:
      (a) every candidate's loss within 2^-19 (relative) of oracle.mse_grid_loss, a zero loss exactly zero (derivation:
          _extra_observers.grid_search_reference);
      (b) min_val / max_val bit-equal to the update rule applied to the ranges of the first strict minima of the DEVICE's
          own losses (mse_grid_commit_kernel, ties included);
      (c) the chosen candidate's oracle loss within a factor 1 + 2^-18 of the oracle's minimum; while every batch so far had
          a separated minimum, min_val / max_val bit-equal to oracle.observe_mse.
    per32 runs every search twice on the one workspace: the same losses both times (tickets reset by the last workgroup)."""
    from outlier_suppression_amd import ops
    bit, symmetric = EO.grid_scheme(kind)
    quant = OB.quant_range(bit, symmetric)
    sites, side = EO.grid_sites(name, kind)
    refs = EO.grid_reference(name, kind)
    on_dev = [site_on_device(s, dev) for s in sites]
    for average in (False, True):
        rule = ops.UPDATE_AVERAGE if average else ops.UPDATE_RUNNING
        mn, mx = torch.tensor(float("inf"), device=dev), torch.tensor(float("-inf"), device=dev)
        chosen, separated = [], True
        for it, (s, (x, L), ref) in enumerate(zip(sites, on_dev, refs)):
            tag = (name, kind, path, "average" if average else "running", it)
            cur = ops.batch_minmax(x, L, s.seq_pos)
            assert eq32(cur.cpu().numpy(), np.array([ref["x_min"], ref["x_max"]], dtype=F32)), tag
            if path == "per32":
                mn2, mx2 = mn.clone(), mx.clone()
                first = device_grid(x, L, s.seq_pos, cur, quant, symmetric, side, rule, it, mn2, mx2, path)
            got = device_grid(x, L, s.seq_pos, cur, quant, symmetric, side, rule, it, mn, mx, path)
            if path == "per32":
                assert eq32(first, got) and eq32(mn2.cpu().numpy(), mn.cpu().numpy()) and eq32(mx2.cpu().numpy(), mx.cpu().numpy()), tag
            want = ref["loss"].astype(np.float64)
            assert got.shape == want.shape and np.isfinite(got).all(), tag
            rel = np.abs(got.astype(np.float64) - want) / np.where(want > 0, want, 1.0)
            print(tag, "largest loss error / 2^-19:", float(rel.max() / EO.LOSS_RTOL), "separated:", ref["separated"])
            assert (rel <= EO.LOSS_RTOL).all() and (got[want == 0] == 0).all(), (tag, int(rel.argmax()), float(rel.max()))      # (a)
            k = int(np.argmin(got))
            assert got[k] < 1e10
            chosen.append((ref["lo"][k], ref["hi"][k]))
            mine = EO.update_chain(chosen, average)[it]
            state = (mn.cpu().numpy(), mx.cpu().numpy())
            assert eq32(state[0], mine[0]) and eq32(state[1], mine[1]), (tag, k, state, mine)                                 # (b)
            assert ref["near"][k], (tag, k, ref["best"], float(ref["loss"][k]), float(ref["loss"][ref["best"]]))             # (c)
            separated = separated and ref["separated"]
            if separated:
                theirs = EO.update_chain([r["best_range"] for r in refs[:it + 1]], average)[it]
                assert eq32(state[0], theirs[0]) and eq32(state[1], theirs[1]), (tag, k, ref["best"], state, theirs)


@pytest.mark.parametrize("kind", EO.GRID_KINDS)
@pytest.mark.parametrize("shape", EO.ROW_SHAPES)
def test_mse_grid_rows(shape, kind, eq32, dev):
    """One wave per row (1, 63, 65, 300 columns; rows all positive, all negative, mixed): the range bit-equal to
    oracle.observe_mse where the oracle's minimum is separated by 1 + 2^-18, else that of a candidate within that factor."""
    from outlier_suppression_amd import ops
    bit, symmetric = EO.grid_scheme(kind)
    quant = OB.quant_range(bit, symmetric)
    w, side, refs = EO.rows_reference(shape, kind)
    bmin, bmax = ops.mse_grid_rows(torch.from_numpy(w).to(dev), 0, quant[0], quant[1], symmetric, side, side == "no" and not symmetric)
    bmin, bmax = bmin.cpu().numpy(), bmax.cpu().numpy()
    for r, ref in enumerate(refs):
        if ref["separated"]:
            assert eq32(bmin[r], ref["best_range"][0]) and eq32(bmax[r], ref["best_range"][1]), (shape, kind, r, bmin[r], bmax[r], ref["best_range"])
        else:
            hit = (EO.OB_bits(ref["lo"]) == EO.OB_bits(bmin[r])) & (EO.OB_bits(ref["hi"]) == EO.OB_bits(bmax[r]))
            assert (hit & ref["near"]).any(), (shape, kind, r)

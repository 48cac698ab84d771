"""The table-driven multi-tensor kernels at every table shape, through the C ABI and through the host paths that build
their tables: osq_fake_quant_weights_multi, osq_token_minmax_multi, osq_token_range_finalize_batched.  Their difficulty
is indexing -- the bisection of the running counts in LDS or (long tables) in global memory, the row of a tensor,
row % channels, the unrolled row loop and its guarded tail, the grid-stride trip -- so every comparison is exact (words,
NaN equal to NaN) against the CPU references of tests/_multi_tables.py and against the single-tensor kernels, and every
word the launch must not write (guard words, padded slots, inputs) is checked.  The recipes' own properties are asserted
on the CPU in tests/test_oracle_multi_tables.py."""
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import _multi_tables as MT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from outlier_suppression_amd import _hip
    _hip.load()          # fail loudly if the HIP library is missing
    return torch.device("cuda:0")


def words(t):
    """uint32 words of a device fp32 tensor on the host, NaNs canonical."""
    return MT.bits(t.detach().cpu().numpy())


def sentinel_filled(n, dev):
    return torch.full((n,), int(MT.SENTINEL_BITS), dtype=torch.int32, device=dev).view(torch.float32)


def table_to_device(descs, dev):
    return torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(dev)


# ----------------------------------------------------------------------------------- 1. osq_fake_quant_weights_multi

@pytest.mark.parametrize("name", MT.WEIGHT_TABLES)
def test_weights_multi_table(name, dev):
    """One launch over the table: every entry bit-equal to oracle/fake_quant_oracle.py and to ops.fake_quant on that
    tensor alone; guard words and inputs unchanged."""
    from outlier_suppression_amd import _hip, ops
    lib = _hip.load()
    t = MT.weight_table(name)
    es = t["entries"]
    x = torch.from_numpy(t["x"]).to(dev)
    scale = torch.from_numpy(t["scale"]).to(dev)
    zp_i, zp_f = torch.from_numpy(t["zp_i32"]).to(dev), torch.from_numpy(t["zp_f32"]).to(dev)
    y = sentinel_filled(t["y_len"], dev)
    before = [a.clone() for a in (x, scale, zp_i, zp_f)]
    descs = (_hip.WeightDesc * len(es))()
    for d, e in zip(descs, es):
        zp = zp_i if e["zp_type"] == MT.ZP_INT32 else zp_f
        d.x, d.y = x.data_ptr() + 4 * e["x_off"], y.data_ptr() + 4 * e["y_off"]
        d.scale, d.zero_point = scale.data_ptr() + 4 * e["p_off"], zp.data_ptr() + 4 * e["p_off"]
        d.rows, d.channels, d.inner = e["rows"], e["channels"], e["inner"]
        d.zp_type, d.mode, d.grad_factor = e["zp_type"], e["mode"], e["grad_factor"]
        d.quant_min, d.quant_max = e["quant_min"], e["quant_max"]
    table = table_to_device(descs, dev)
    ends = torch.from_numpy(t["row_end"]).to(dev)
    _hip.check(lib.osq_fake_quant_weights_multi(table.data_ptr(), ends.data_ptr(), len(es), t["total_rows"], _hip.stream_ptr(dev)),
               "fake_quant_weights_multi")
    torch.cuda.synchronize()
    got = words(y)
    ref = MT.weight_reference(name)
    guard = MT.weight_guard_mask(t)
    assert (got[guard] == MT.SENTINEL_BITS).all(), ("guard words written", np.nonzero(guard & (got != MT.SENTINEL_BITS))[0][:8])
    for e in es:                       # entry by entry first: a failure names the entry
        sl = slice(e["y_off"], e["y_off"] + e["rows"] * e["inner"])
        if not np.array_equal(got[sl], ref[sl]):
            bad = np.nonzero(got[sl] != ref[sl])[0]
            raise AssertionError((name, "entry", e["index"], {k: e[k] for k in ("rows", "channels", "inner", "mode", "zp_type", "bit")},
                                  "first wrong row", int(bad[0]) // e["inner"], "wrong words", len(bad)))
    assert np.array_equal(got, ref)
    for a, b in zip((x, scale, zp_i, zp_f), before):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "an input was written"
    # the same tensors one by one through the single-tensor entry points
    single = sentinel_filled(t["y_len"], dev)
    for e in es:
        if e["rows"] == 0:
            continue
        ch, n = e["channels"], e["rows"] * e["inner"]
        xe = x[e["x_off"]:e["x_off"] + n].view(e["rows"] // ch, ch, e["inner"])
        zp = (zp_i if e["zp_type"] == MT.ZP_INT32 else zp_f)[e["p_off"]:e["p_off"] + ch]
        one = ops.fake_quant(xe, scale[e["p_off"]:e["p_off"] + ch], zp, -1 if ch == 1 else 1, e["quant_min"], e["quant_max"],
                             e["mode"], e["grad_factor"])
        single[e["y_off"]:e["y_off"] + n] = one.reshape(-1)
    assert np.array_equal(got, words(single))


# ----------------------------------------------------------------------------------- 2. osq_token_minmax_multi

@pytest.mark.parametrize("name", MT.SITE_TABLES)
def test_token_minmax_multi_table(name, dev):
    """One launch over the table: valid slots equal NumPy's min / max over the feature axes (a NaN poisons its own token,
    infinities come through, padded tokens change nothing), the whole output -- zero signs, padded slots, the gaps
    between sites -- equals ops.token_minmax site by site, word for word; inputs unchanged."""
    from outlier_suppression_amd import _hip, ops
    lib = _hip.load()
    t = MT.site_table(name)
    ss = t["sites"]
    x = torch.from_numpy(t["x"]).to(dev)
    lengths = torch.from_numpy(t["lengths"]).to(dev)
    before = x.clone()
    tmin, tmax = sentinel_filled(t["out_len"], dev), sentinel_filled(t["out_len"], dev)
    one_min, one_max = sentinel_filled(t["out_len"], dev), sentinel_filled(t["out_len"], dev)
    descs = (_hip.SiteDesc * len(ss))()
    for d, s in zip(descs, ss):
        xs = MT.site_view(x, s)
        L = None if s["len_off"] is None else lengths[s["len_off"]:s["len_off"] + s["B"]]
        view = ops.token_view(xs, s["seq_pos"], None if L is None else L.numel())
        assert (view.batch, view.tokens) == (s["B"], s["T"]) and view.feat_outer * view.feat_inner == MT.site_features(s)[0]
        vec = int(view.stride_inner == 1 and view.feat_inner % 4 == 0 and xs.data_ptr() % 16 == 0 and view.stride_batch % 4 == 0
                  and view.stride_token % 4 == 0 and (view.feat_outer == 1 or view.stride_outer % 4 == 0))      # as deferred.py
        assert vec == s["vec"], (s["index"], s["kind"])
        sl = slice(s["out_off"], s["out_off"] + s["B"] * s["T"])
        d.x, d.lengths = xs.data_ptr(), _hip.ptr(L)
        d.token_min, d.token_max = tmin[sl].data_ptr(), tmax[sl].data_ptr()
        d.view, d.vec = view, vec
        ops.token_minmax(xs, s["seq_pos"], L, out=(one_min[sl], one_max[sl]))
    table = table_to_device(descs, dev)
    ends = torch.from_numpy(t["tok_end"]).to(dev)
    _hip.check(lib.osq_token_minmax_multi(table.data_ptr(), ends.data_ptr(), len(ss), t["total_tokens"], _hip.stream_ptr(dev)),
               "token_minmax_multi")
    torch.cuda.synchronize()
    ref_min, ref_max, written = MT.site_reference(name)
    for got_t, ref, what in ((tmin, ref_min, "min"), (tmax, ref_max, "max")):
        got = got_t.cpu().numpy()
        assert (MT.bits(got[~written]) == MT.SENTINEL_BITS).all(), (what, "a padded slot or a gap was written")
        same = (got == ref) | (np.isnan(got) & np.isnan(ref))            # by value: the sign of a zero extremum is the device's
        if not same[written].all():
            k = int(np.nonzero(written & ~same)[0][0])
            site = max(s["index"] for s in ss if s["out_off"] <= k)
            raise AssertionError((name, what, "site", site, ss[site]["kind"], ss[site]["mem_shape"], "slot", k - ss[site]["out_off"],
                                  float(got[k]), float(ref[k]), "wrong slots", int((written & ~same).sum())))
    assert np.array_equal(words(tmin), words(one_min)) and np.array_equal(words(tmax), words(one_max))
    assert torch.equal(x.view(torch.int32), before.view(torch.int32))


# ----------------------------------------------------------------------------------- 3. osq_token_range_finalize_batched

@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
@pytest.mark.parametrize("n_q,n_b", MT.FINAL_SHAPES)
def test_finalize_batched_table(n_q, n_b, wide, dev):
    """Every row of cur_table bit-equal to ops.token_range_finalize on that problem alone (below the wide switch point
    and above it, where the single problem takes the three-launch form) and to the oracle's thresholds; the row of an
    all-padding problem and the slack behind every problem are left as they were."""
    from outlier_suppression_amd import ops
    t = MT.final_table(n_q, n_b, wide)
    B, T, S = t["B"], t["T"], t["B"] * t["T"]
    tmin, tmax = torch.from_numpy(t["tmin"]).to(dev), torch.from_numpy(t["tmax"]).to(dev)
    lengths, flags = torch.from_numpy(t["lengths"]).to(dev), torch.from_numpy(t["flags"]).to(dev)
    before = (tmin.clone(), tmax.clone())
    assert tmin.stride(1) == t["stride"] > S
    assert (S >= MT.FINAL_WIDE_MIN) == wide
    try:
        ops.set_wide_min_slots(MT.FINAL_WIDE_MIN if wide else 32769)
        for p in MT.FINAL_PERCENTILES:
            cur = sentinel_filled(n_b * n_q * 2, dev).view(n_b, n_q, 2)
            one = sentinel_filled(n_b * n_q * 2, dev).view(n_b, n_q, 2)
            ops.token_range_finalize_batched(tmin, tmax, n_q, n_b, B, T, lengths, flags, p, cur)
            for q in range(n_q):
                for b in range(n_b):
                    ops.token_range_finalize(tmin[q, b, :S], tmax[q, b, :S], B, T, lengths[q, b], bool(t["flags"][q]), p,
                                             ops.UPDATE_NONE, 0, None, None, 0, 63, False, None, one[b, q])
            torch.cuda.synchronize()
            got = words(cur)
            assert np.array_equal(got, words(one)), (p, np.argwhere(got != words(one))[:4])
            ref = MT.final_reference(n_q, n_b, p, wide)
            assert np.array_equal(got, ref), (p, np.argwhere(got != ref)[:4])
    finally:
        ops.set_wide_min_slots(32769)
    assert np.array_equal(words(tmin), words(before[0])) and np.array_equal(words(tmax), words(before[1]))


# ----------------------------------------------------------------------------------- 4. through the host paths

class _Operators(torch.nn.Module):
    def __init__(self, ops_list):
        super().__init__()
        self.ops = torch.nn.ModuleList(ops_list)


def test_prepare_weights_beyond_the_lds_table(dev):
    """weight_cache.prepare_weights over 1030 tiny quantized linear operators (a table the kernel bisects in global
    memory): ONE multi launch, every cached weight bit-equal to the operator's own launch."""
    from outlier_suppression_amd.quantization import Quantizer, weight_cache as WC
    gen = torch.Generator().manual_seed(11)
    n = 1030
    mods = []
    for i in range(n):
        per_channel = i % 3 != 0
        cfg = NS(quantizer="FixedFakeQuantize", observer="MinMaxObserver", bit=(4, 6, 8)[i % 3], symmetric=bool(i % 2),
                 ch_axis=0 if per_channel else -1)
        m = Quantizer(torch.nn.Linear(8, 4, bias=False), cfg)
        fq, ch = m.weight_fake_quant, 4 if per_channel else 1
        fq.scale = torch.rand(ch, generator=gen) * 0.05 + 0.01 * (1 + i % 7)
        fq.zero_point = torch.randint(fq.quant_min, fq.quant_max + 1, (ch,), generator=gen, dtype=torch.int32)
        fq.enable_fake_quant()
        mods.append(m)
    model = _Operators(mods).to(dev)
    saved = (WC.enabled, dict(WC.stats))
    try:
        with torch.no_grad():
            WC.enabled = False
            ref = torch.stack([m._quantized_weight() for m in model.ops])
            WC.enabled = True
            for k in WC.stats:
                WC.stats[k] = 0
            assert WC.prepare_weights(model) == n
            assert WC.stats["multi_launches"] == 1 and WC.stats["multi_tensors"] == n and WC.stats["module_launches"] == 0
            got = torch.stack([m._quantized_weight() for m in model.ops])
            assert WC.stats["hits"] == n and WC.stats["multi_launches"] == 1 and WC.stats["module_launches"] == 0
        assert len({int(w.data_ptr()) for w in got}) == n
        bad = (got.view(torch.int32) != ref.view(torch.int32)).flatten(1).any(dim=1).nonzero().flatten().tolist()
        assert not bad, ("operators whose cached weight differs", bad[:8], len(bad))
        assert not torch.equal(ref, torch.stack([m.weight for m in model.ops]))
    finally:
        WC.enabled = saved[0]
        WC.stats.update(saved[1])
        WC.invalidate(model)


def test_deferred_observation_beyond_the_lds_table(dev):
    """520 masked quantizers in one deferred flush (a site table the kernel bisects in global memory): statistics and
    parameters equal the site-by-site pass, as tests/test_gpu_deferred.py asserts for 7 sites."""
    from outlier_suppression_amd.quantization import Quantizer
    from outlier_suppression_amd.quantization.deferred import deferred_observation
    gen = torch.Generator().manual_seed(12)
    n, B, T = 520, 4, 6
    L = [torch.tensor([6, 0, 3, 1]).to(dev), torch.tensor([2, 6, 5, 0]).to(dev)]
    mem = torch.randn(B, T, 2, 8, generator=gen).to(dev)
    observers = ("AvgPruneMinMaxObserver", "AvgMinMaxObserver", "MinMaxObserver")

    def site(i, step):
        k = i % 4
        if k == 0:
            return torch.randn(B, T, (4, 20, 33, 68)[(i // 4) % 4], generator=gen).to(dev) * (1 + i % 5), L[i % 2], 1
        if k == 1:
            return mem.permute(0, 2, 1, 3) * float(1 + i % 9 + step), L[i % 2], 2         # [B,h,T,d] view
        if k == 2:
            return mem.permute(0, 2, 3, 1) * float(2 + i % 7 + step), L[(i + 1) % 2], 3   # [B,h,d,T] view
        return torch.rand(B, 2, T, T, generator=gen).to(dev), L[i % 2], 2

    inputs = [[site(i, step) for i in range(n)] for step in range(2)]
    results = []
    for deferred in (False, True):
        qs = []
        for i in range(n):
            cfg = NS(quantizer=("LSQPlusFakeQuantize", "FixedFakeQuantize")[i % 2], observer=observers[i % 3], bit=6,
                     symmetric=i % 5 == 0, ch_axis=-1)
            q = Quantizer(None, cfg).to(dev)
            q.observer.set_name(f"layer{i}.{'attention_probs' if i % 4 == 3 else 'x'}_post_act_fake_quantize.observer")
            if hasattr(q.observer, "set_percentile"):
                q.observer.set_percentile((0.9, 0.5)[i % 2])
            q.enable_observer()
            q.disable_fake_quant()
            qs.append(q)
        if deferred:
            with deferred_observation() as sites:
                for step in range(2):
                    for q, (x, m, sp) in zip(qs, inputs[step]):
                        assert q(x, m, sp) is x
                    assert sites.flush() == n
            assert sites.launches <= 2 * (1 + 2 * 8)
        else:
            for step in range(2):
                for q, (x, m, sp) in zip(qs, inputs[step]):
                    q(x, m, sp)
        torch.cuda.synchronize()
        results.append([(q.observer.min_val.clone(), q.observer.max_val.clone(), q.scale.detach().clone(),
                         q.zero_point.detach().clone(), getattr(q.observer, "cnt", None)) for q in qs])
    for i, (a, b) in enumerate(zip(*results)):
        assert all(torch.equal(u, v) for u, v in zip(a[:4], b[:4])) and a[4] == b[4], (i, a, b)
    assert sum(bool(torch.isfinite(a[1]).all()) for a in results[0]) == n

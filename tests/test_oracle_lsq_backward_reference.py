"""CPU proofs for tests/_lsq_backward_reference.py: every condition a recipe promises to the GPU tests of the LSQ / LSQ+
backward (tests/test_gpu_lsq_backward_accuracy.py), and lsq_backward_exact pinned to the reference project's stored runs."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _lsq_backward_reference as R  # noqa: E402
from conftest import same_f32  # noqa: E402

from oracle import fake_quant_oracle as FQ  # noqa: E402

F32 = np.float32


def _dyadic_case(seed, shape, ch_axis=-1, half=False):
    rng = np.random.default_rng([77, seed])
    qmin, qmax = R.DYADIC_RANGES[seed % len(R.DYADIC_RANGES)]
    nz = 1 if ch_axis == -1 else shape[ch_axis]
    zp = rng.integers(qmin, qmax + 1, nz).astype(F32) + (F32(0.5) if half else F32(0))
    x, gy = R.dyadic_xy(rng, shape, qmin, qmax, zp if ch_axis != -1 else zp[0], ch_axis)
    return x, gy, zp, qmin, qmax


def test_launch_geometry_is_read_from_the_sources():
    assert R.THREADS == 256 and R.MAX_BLOCKS == 2048 and 1 <= R.BWD_BLOCKS <= R.MAX_BLOCKS and R.ORDERED_MAX_INNER == 3072
    lengths = R.per_tensor_lengths()
    assert {0, 1, 3, 4, 5, 7, 1023, 1024, 1025, 1026, 1027, 3145728 + 13, (1 << 24) + 32 * 1024 + 37} <= set(lengths)
    for cap in (1, R.BWD_BLOCKS, R.MAX_BLOCKS):
        forms = np.array([R.lane_forms(n, cap) for n in lengths])
        assert forms.any(axis=0).all(), cap                      # one float4, two float4, several trips: each is run
        assert any(R.grid_of(n, cap) == cap for n in lengths)
        assert any(n % 4 == t and R.grid_of(n, cap) == cap and n > 4 for n in lengths for t in (1, 3))   # a tail with the grid at its cap
    assert {n % 4 for n in lengths} == {0, 1, 2, 3}
    # bwd_blocks = 2048: the last-block combine has all kPer = 8 partial loads of a lane live
    assert R.grid_of(lengths[-1], R.MAX_BLOCKS) == R.MAX_BLOCKS == 8 * R.THREADS
    assert any("second trip" in R.special_positions(n) for n in lengths)


@pytest.mark.parametrize("half", [False, True])
def test_dyadic_sums_do_not_depend_on_the_order(half):
    """math.fsum, NumPy's float64 sum and the reference-order fp32 cascades (8 and 16 lanes) agree bit for bit where the
    fp32 total stays below 2^24 eighth-units; fsum == float64 at every size; the effective parameters are exact."""
    for seed, n in enumerate([1, 3, 7, 1023, 1027, 5000, 40000, 300001]):
        x, gy, zp, qmin, qmax = _dyadic_case(seed, (n,), half=half)
        factors = R.dyadic_factors(n, qmax, zp)
        assert 2.0 ** -10 in factors
        for g in factors:
            for mode in (("lsqplus",) if half else FQ.MODES):
                assert R.effective_is_exact(R.DYADIC_SCALE, zp, g, mode)
                t = FQ.lsq_backward_terms(x, gy, R.DYADIC_SCALE, zp, qmin, qmax, g, mode)
                for k in ("ds_mul", "ds_div", "g_in", "ng_mul"):
                    assert np.array_equal(t[k] * 8, np.round(t[k] * 8)) and np.abs(t[k]).max() < 2 ** 15
                a = FQ.lsq_backward_exact(x, gy, R.DYADIC_SCALE, zp, qmin, qmax, g, mode, how="fsum")
                b = FQ.lsq_backward_exact(x, gy, R.DYADIC_SCALE, zp, qmin, qmax, g, mode, how="float64")
                assert a.S_s[0] == b.S_s[0] and a.S_z[0] == b.S_z[0]
                assert a.S_s[0] == math.fsum(t["ds_mul"].tolist() + t["ds_div"].tolist())
                fs, fz = FQ.lsq_grad_factors(F32(g), mode)
                assert a.dscale[0] == a.S_s[0] * fs and a.dzp[0] == a.S_z[0] * fz
                dx, ds, dz, A = R.dyadic_expected(x, gy, zp, qmin, qmax, g, mode)
                assert ds[0] == F32(a.S_s[0] * np.float64(F32(g) if mode != "fixed" else 1.0))
                if R.fp32_sums_exact(A)[0]:
                    for vec in (8, 16):
                        rdx, rds, rdz = FQ.lsq_backward_reference_order(x, gy, R.DYADIC_SCALE, zp, qmin, qmax, g, mode, vec=vec)
                        assert same_f32(rdx, dx) and rds == ds[0] and rdz == dz[0], (n, mode, vec)
    assert not R.fp32_sums_exact(A)[0]              # the largest size is beyond the fp32 claim: both branches are used


def test_dyadic_per_channel_equals_its_gathered_channels():
    for seed, (outer, C, inner) in enumerate([(1, 12, 20), (4, 6, 5), (3, 64, 130), (8, 12, 1)]):
        x, gy, zp, qmin, qmax = _dyadic_case(seed, (outer, C, inner), ch_axis=1)
        g = R.dyadic_factors(outer * C * inner, qmax, zp, C)[-1]
        dx, ds, dz, A = R.dyadic_expected(x, gy, zp, qmin, qmax, g, "lsqplus", 1)
        for c in range(C):
            cdx, cds, cdz, _ = R.dyadic_expected(x[:, c].reshape(-1), gy[:, c].reshape(-1), zp[c:c + 1], qmin, qmax, g, "lsqplus")
            assert same_f32(cdx.reshape(outer, inner), dx[:, c]) and cds[0] == ds[c] and cdz[0] == dz[c]
        if outer == 1:
            for vec in (8, 16):
                rdx, rds, rdz = FQ.lsq_backward_reference_order(x[0], gy[0], np.full(C, R.DYADIC_SCALE), zp, qmin, qmax, g, "lsqplus", 0, vec)
                ok = R.fp32_sums_exact(A)
                assert same_f32(rdx, dx[0]) and np.array_equal(rds[ok], ds[ok]) and np.array_equal(rdz[ok], dz[ok])


def _shares(x, s, z, g, qmin, qmax):
    se, ze = FQ.lsq_effective(s, z, g, "lsqplus")
    x_int = FQ.round_ste_value(x / se) + ze
    return float((x_int < qmin).mean()), float((x_int > qmax).mean())


def test_random_recipes_keep_their_conditions_and_the_floor_stands():
    """clipped: >= 40 % outside each side; one-sign: kappa = 1; cancelling: 1e3 <= kappa <= 1e5 (per-tensor, from 98309
    elements on).  And the yardstick itself, never measured before: e_ref (reference-order fp32 sums against the exact
    sums, in units of 2^-24 * g * A) over 32 seeds per recipe -- its median is below 4 units everywhere, so the bar's
    floor stays 4 (printed under -s; OSQ_LSQ_BACKWARD_EREF_OUT=<path> writes profiles/lsq_backward_eref_cpu.txt)."""
    n = 98304 + 5
    table = []
    for name in R.RECIPES:
        e_ref = []
        for seed in range(32):
            x, gy, s, z, qmin, qmax = R.recipe(name, seed, n, seed)
            g = FQ.lsqplus_grad_factor(n, qmax)
            e = FQ.lsq_backward_exact(x, gy, s, z, qmin, qmax, g, "lsqplus")
            _, rs, rz = FQ.lsq_backward_reference_order(x, gy, s, z, qmin, qmax, g, "lsqplus")
            e_ref += [float(R.units(rs, e.dscale[0], e.A_s[0], g)), float(R.units(rz, e.dzp[0], e.A_z[0], g))]
            ks, kz = R.kappa(e)
            if name == "clipped":
                lo, hi = _shares(x, s, z, g, qmin, qmax)
                assert lo >= 0.40 and hi >= 0.40, (seed, lo, hi)
            elif name == "one-sign":
                assert _shares(x, s, z, g, qmin, qmax)[1] == 1.0 and (gy > 0).all()
                assert abs(ks[0] - 1) < 1e-12 and abs(kz[0] - 1) < 1e-12
            elif name == "cancelling":
                assert 1e3 <= ks[0] <= 1e5 and 1e3 <= kz[0] <= 1e5, (seed, ks, kz)
        ds, dz = np.array(e_ref[0::2]), np.array(e_ref[1::2])
        table.append(f"{name:<12}{np.median(ds):>10.3f}{ds.max():>10.3f}{np.median(dz):>10.3f}{dz.max():>10.3f}")
        assert np.median(e_ref) < R.BAR_FLOOR and max(e_ref) < R.BAR_FLOOR, (name, np.median(e_ref), max(e_ref))
    text = ("# tests/test_oracle_lsq_backward_reference.py (CPU): e_ref = error of the reference's one-thread fp32 summation order\n"
            f"# against the exact sums, units of 2^-24 * g * A; LSQ+ per-tensor, n = {n}, 32 seeds per recipe.  Every median is below\n"
            "# 4 units, so the floor of the bar max(3 e_ref, 4) stays 4.\n"
            f"{'recipe':<12}{'ds median':>10}{'ds max':>10}{'dz median':>10}{'dz max':>10}\n" + "\n".join(table) + "\n")
    print(text)
    out = os.environ.get("OSQ_LSQ_BACKWARD_EREF_OUT")
    if out:
        with open(out, "w") as f:
            f.write(text)


def test_exact_oracle_against_the_reference_runs(golden):
    """lsq_backward_exact against tests/golden/lsqplus.npz (the reference's own fp32 autograd): dx as words; ds, dzp
    within the bar computed for the reference's result itself (e_ref <= max(3 e_ref, 4) + 1 ulp: ratio <= 1)."""
    g = golden("lsqplus")
    for k in range(int(g["n"])):
        scale, zp, qmin, qmax, gf = g[f"c{k}_meta"]
        e = FQ.lsq_backward_exact(g[f"c{k}_x"], g[f"c{k}_gy"], F32(scale), F32(zp), int(qmin), int(qmax), gf, "lsqplus")
        assert same_f32(e.dx, g[f"c{k}_dx"])
        for got, exact, A in ((g[f"c{k}_ds"][0], e.dscale[0], e.A_s[0]), (g[f"c{k}_dzp"][0], e.dzp[0], e.A_z[0])):
            e_ref = R.units(got, exact, A, gf)
            assert e_ref <= R.bar_units(e_ref, exact, A, gf) and e_ref < R.BAR_FLOOR + 2, (k, e_ref)
    qmin, qmax, gf = int(g["pc_meta"][1]), int(g["pc_meta"][2]), g["pc_meta"][3]
    e = FQ.lsq_backward_exact(g["pc_x"], g["pc_gy"], g["pc_scale"], g["pc_zp"], qmin, qmax, gf, "lsqplus", 0)
    assert same_f32(e.dx, g["pc_dx"])
    assert (R.units(g["pc_ds"], e.dscale, e.A_s, gf) < R.BAR_FLOOR).all() and (R.units(g["pc_dzp"], e.dzp, e.A_z, gf) < R.BAR_FLOOR).all()


def _widen(bits, kind):
    import torch
    t = torch.from_numpy(bits.astype(np.int16)).view(torch.bfloat16 if kind == "bf16" else torch.float16)
    return t.float().numpy()


@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_exact_oracle_against_the_low_precision_reference_rows(golden, kind):
    """The learnable rows of tests/golden/lowp.npz: x widened once, ds / dz of the reference's fp32 autograd."""
    import torch
    g = golden("lowp")
    x = _widen(g[f"lsq_{kind}_x"], kind)
    gy = g[f"lsq_{kind}_gy"]
    lowp = torch.bfloat16 if kind == "bf16" else torch.float16
    for tag, mode, ch_axis, dzkey in (("lsq", "lsq", -1, None), ("lsq", "lsq", 0, None), ("lsqp", "lsqplus", -1, "dz"), ("lsqp", "lsqplus", 0, "dz")):
        p = f"{tag}_{kind}_{'pt' if ch_axis == -1 else 'ch'}_"
        gf = float(g[p + "gf"])
        qmin, qmax = (-8, 7) if mode == "lsq" else (0, 31)          # make_golden_lowp.py: 4 bit symmetric / 5 bit asymmetric
        e = FQ.lsq_backward_exact(x, gy, g[p + "scale"], g[p + "zp"].astype(F32), qmin, qmax, gf, mode, ch_axis)
        want_dx = _widen(g[p + "dx"], kind)
        got_dx = torch.from_numpy(e.dx).to(lowp).float().numpy()
        assert same_f32(got_dx, want_dx), p
        assert (R.units(g[p + "ds"], e.dscale, e.A_s, gf) < R.BAR_FLOOR).all(), p
        if dzkey:
            assert (R.units(g[p + "dz"], e.dzp, e.A_z, gf) < R.BAR_FLOOR).all(), p


def test_specials_make_the_oracle_nan_only_where_they_sit():
    rng = np.random.default_rng(5)
    x, gy = R.dyadic_xy(rng, (3, 40), 0, 63, np.float32([5, 20, 40]), 0)
    for which, v in R.SPECIAL_VALUES:
        xs, gs = x.copy(), gy.copy()
        (xs if which == "x" else gs)[1, 7] = F32(v)
        e = FQ.lsq_backward_exact(xs, gs, np.full(3, R.DYADIC_SCALE), np.float32([5, 20, 40]), 0, 63, 2.0 ** -10, "lsqplus", 0)
        finite = np.isfinite(F32(v))
        assert np.isfinite(e.dscale[[0, 2]]).all() and np.isfinite(e.dzp[[0, 2]]).all()
        assert np.isfinite(e.dscale[1]) == finite, (which, v)

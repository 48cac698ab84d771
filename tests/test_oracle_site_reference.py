"""tests/_site_reference.py on the CPU: the float64 references the GPU accuracy tests judge the one-launch sites by
(tests/test_gpu_site_accuracy.py) are themselves pinned to the REFERENCE project's own runs, and every input recipe of
those tests is shown to meet its conditions with the references alone -- before either judges a kernel.

  * layernorm_site_f64 against the stored LayerNorm outputs of tests/golden/ln_site.npz (all three cases) and `ln_full` /
    `ln_split` of gamma.npz; softmax_site_f64 against the stored probabilities of attention_site.npz; gelu_f64 against
    torch's CPU F.gelu.  Bar: BASELINE.json's 1e-5 of the output's magnitude (the goldens are fp32 CPU results; the
    differences seen are a few 1e-7).
  * every LayerNorm / softmax recipe: float64 reference finite on every row, kappa finite; the edge rows give the NaN rows
    they are meant to give.
  * the GELU recipes: for every (input, scale) the tie neighbourhood |frac(gelu/s) - 1/2| * s <= delta covers at most 2e-3 of
    the entries, and torch's own CPU fp32 GELU meets the assertion the kernel is held to (integers at most one step from
    the float64 ones, and only inside the neighbourhood)."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _site_reference as R  # noqa: E402
from _attention_site import CASES as ATTN_CASES, PROBS_SLICE, attention_site_inputs, checksum as attn_checksum, scaling  # noqa: E402
from _ln_site import CASES as LN_CASES, FLOAT_SAMPLES, checksum, ln_site_inputs  # noqa: E402

from oracle import fake_quant_oracle as FQ, gamma_oracle as GM  # noqa: E402


def _within_baseline(ours, ref):
    return float(np.abs(ours - ref).max()) <= 1e-5 * max(1.0, float(np.abs(ref).max()))


def test_layernorm_reference_matches_tiny_wrappers(golden):
    g = golden("gamma")
    h = g["x"].shape[-1]
    full, _ = R.layernorm_site_f64(g["x"], None, None, g["gamma"], g["beta"], 1e-12)
    split, _ = R.layernorm_site_f64(g["x"], None, None, None, GM.split_bias(g["beta"], g["gamma"]), 1e-5)
    assert _within_baseline(full, g["ln_full"].reshape(-1, h))
    assert _within_baseline(split, g["ln_split"].reshape(-1, h))


@pytest.mark.parametrize("case", LN_CASES, ids=[c[0] for c in LN_CASES])
def test_layernorm_reference_matches_ln_site(golden, case):
    name, cls, eps, with_gamma, *_, seed = case
    g = golden("ln_site")
    x, hidden, gamma, beta, _ = ln_site_inputs(seed)
    assert [checksum(t) for t in (x, hidden, gamma, beta)] == list(g[name + "_sums"][:4]), "the seeded inputs drifted"
    x, hidden = x[:FLOAT_SAMPLES], hidden[:FLOAT_SAMPLES]
    hid = None if with_gamma is None else hidden
    gam = gamma if with_gamma else None
    if cls == "QuantizedSplitLayerNorm":          # quirk: the split wrapper's inner LayerNorm has torch's default eps
        y, kappa = R.layernorm_site_f64(x, hid, gam, None, GM.split_bias(beta.numpy(), gamma.numpy()), 1e-5)
    else:
        y, kappa = R.layernorm_site_f64(x, hid, gam, gamma, beta, eps)
    ref = g[name + "_ln"].reshape(y.shape)
    assert np.isfinite(kappa).all()
    d = float(np.abs(y - ref).max())
    print(f"{name}: max |f64 - reference| {d:.3e} on values up to {np.abs(ref).max():.4g}")
    assert _within_baseline(y, ref), (name, d)


@pytest.mark.parametrize("case", ATTN_CASES, ids=[c[0] for c in ATTN_CASES])
def test_softmax_reference_matches_attention_site(golden, case):
    name, kind, shape, d = case[:4]
    g = golden("attention_site")
    scores, mask, L = attention_site_inputs(case[-1], kind, shape, d)
    assert [attn_checksum(scores), attn_checksum(mask.contiguous()), int(L.sum())] == list(g[name + "_sums"]), "the seeded inputs drifted"
    root = scaling(kind, d)
    m = mask.expand(shape[0], 1, mask.shape[2], shape[3])[PROBS_SLICE[0]]
    _, p = R.softmax_site_f64(scores[PROBS_SLICE[:2]], m, divisor=root)
    ref = g[name + "_probs"]
    p = p[(slice(None), slice(None)) + PROBS_SLICE[2:]]
    dmax = float(np.abs(p - ref).max())
    print(f"{name}: max |f64 - reference| {dmax:.3e}")
    assert dmax <= 1e-5, (name, dmax)
    if root == 8.0:                               # the power-of-two head size: scores * (1/8) is the same fp32 value
        assert np.array_equal(R.pre_softmax_f32(scores[:1, :1], m, alpha=0.125), R.pre_softmax_f32(scores[:1, :1], m, divisor=8.0))


def test_gelu_reference_matches_torch_cpu():
    for name, x in R.gelu_inputs().items():
        g32 = F.gelu(torch.from_numpy(x)).numpy()
        g64 = R.gelu_f64(x)
        d = float(np.abs(g32 - g64).max())
        print(f"{name}: max |F.gelu fp32 - f64| {d:.3e}")
        assert d <= 1e-5 * max(1.0, float(np.abs(g64).max())), name
    # the closed form at points where it is known
    assert R.gelu_f64(np.array([0.0], np.float32))[0] == 0.0
    np.testing.assert_allclose(R.gelu_f64(np.array([1.0, -1.0], np.float32)), [0.8413447460685429, -0.15865525393145707], rtol=1e-15)


def test_layernorm_recipes_are_well_posed():
    """Every (width, class, operand form): float64 reference and kappa finite on every row, and torch's CPU LayerNorm --
    what sets the bar -- finite as well (so no class asks the kernel for more than the eager CPU sequence delivers)."""
    torch.set_num_threads(1)
    kmax = {}
    for cols in R.LN_WIDTHS:
        for cls in R.LN_CLASSES:
            for combo in R.LN_COMBOS:
                x, hidden, gamma, weight, bias = R.ln_inputs(cols, cls, combo)
                y64, kappa = R.layernorm_site_f64(x, hidden, gamma, weight, bias, 1e-12)
                assert np.isfinite(y64).all() and np.isfinite(kappa).all(), (cols, cls, combo[0])
                r = torch.from_numpy(R.residual_f32(x, hidden, gamma))
                assert torch.isfinite(R.eager_layernorm(r, weight, bias, 1e-12)).all(), (cols, cls, combo[0])
                kmax[cls] = max(kmax.get(cls, 0.0), float(kappa.max()))
    print({k: round(v, 1) for k, v in kmax.items()})
    assert kmax["offset1e3"] >= 1e3 and kmax["offset10"] >= 10 and kmax["randn"] < 10
    assert sorted({R.ln_template_r(c) for c in R.LN_WIDTHS}) == [1, 2, 3, 4, 8, 16]
    for r in (1, 2, 3, 4, 8, 16):                 # each instance with a full and with a ragged last lane group
        mine = [c for c in R.LN_WIDTHS if R.ln_template_r(c) == r]
        assert any(c % 256 == 0 for c in mine) and any(c % 256 != 0 for c in mine), r


def test_softmax_recipes_are_well_posed():
    for cols in R.SM_REGISTER_WIDTHS + R.SM_GENERIC_WIDTHS:
        for kind in R.SM_KINDS:
            for pre in R.SM_PRE:
                scores, mask = R.softmax_inputs(cols, kind, pre)
                for m in (mask, None):
                    v, p = R.softmax_site_f64(scores, m, **pre[1])
                    assert np.isfinite(p).all(), (cols, kind, pre[0])
                    assert np.abs(p.sum(-1) - 1.0).max() < 1e-12
                if kind == "peaked":
                    assert 1.0 < float(np.std(R.pre_softmax_f32(scores, None, **pre[1]))) < 4.0       # the recipe's spread survives the pre step
        s, m = R.softmax_edge_rows(cols, torch.Generator().manual_seed(cols))
        _, p = R.softmax_site_f64(s, m)
        nan_rows = np.isnan(p).all(-1)
        assert list(nan_rows) == [True, True, True, False, False] and not np.isnan(p[3:]).any(), cols
        assert np.allclose(p[3], 1.0 / cols, rtol=1e-12) and (p[4, cols // 2:] == 0).all()
        ref = torch.softmax(s + m, -1).numpy()                       # torch's CPU softmax has the same NaN rows
        assert np.array_equal(np.isnan(ref), np.isnan(p)), cols
    assert sorted({R.softmax_template_r(c) for c in R.SM_REGISTER_WIDTHS}) == [1, 2, 4, 8]
    assert all(c % 4 or c > 2048 for c in R.SM_GENERIC_WIDTHS)


@pytest.mark.parametrize("lsqplus", [False, True], ids=["fixed", "lsqplus"])
def test_gelu_recipes_meet_the_tie_condition(lsqplus):
    """The exclusion the GPU test grants the kernel is small (<= 2e-3 of the entries for every input and scale), and
    torch's own CPU fp32 GELU, pushed through the oracle's fake-quant, satisfies the assertion the kernel is held to."""
    torch.set_num_threads(1)
    for name, x in R.gelu_inputs().items():
        g64 = R.gelu_f64(x)
        delta = R.gelu_delta(x)
        g32 = F.gelu(torch.from_numpy(x)).numpy()
        for scale, zp, bits in R.GELU_QUANT:
            s, z, qmin, qmax, gf = R.effective_params(scale, zp, bits, lsqplus, x.size)
            q64, dist = R.gelu_q64(g64, s, z, qmin, qmax)
            near = dist <= delta
            share = float(near.mean())
            if lsqplus:
                xq, _ = FQ.fake_quantize_learnableplus_per_tensor(g32, np.float32(scale), np.float32(zp), qmin, qmax, gf)
            else:
                xq, _ = FQ.fake_quantize_per_tensor_affine(g32, scale, zp, qmin, qmax)
            diff = xq.astype(np.float64) - q64
            print(f"{name} s={scale}: delta {delta:.3e}, tie share {share:.3e}, torch-CPU integers differing {int((diff != 0).sum())} of {x.size}")
            assert share <= R.GELU_TIE_SHARE, (name, scale, share)
            assert np.abs(diff).max() <= 1 and not (diff != 0)[~near].any(), (name, scale)


def test_gelu_specials_cover_head_body_and_tail():
    cases = R.gelu_special_inputs()
    seen = set()
    for x, pos in cases:
        assert x.size % 4 == 3
        for p in pos:
            where = "tail" if p >= x.size - 3 else ("head" if p < 16 else "body")
            seen.add((where, np.float32(x[p]).tobytes()))
    for where in ("head", "body", "tail"):
        assert len([1 for w, _ in seen if w == where]) == len(R.GELU_SPECIALS), where

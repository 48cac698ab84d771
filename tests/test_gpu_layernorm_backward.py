"""Backward of the one-launch residual + LayerNorm + fake-quant site (csrc/layernorm_backward.hip) against float64.

The words the forward quantised are n = ops.residual_layernorm_fake_quant(.., quant=None); dn and the exact parameter sums are
the oracle's per-element rule on that n (oracle/fake_quant_oracle.py), dr / dx / dhidden float64 numpy from x, hidden, gamma,
w and dn.  scale.grad / zero_point.grad: the order-free tier's bar of tests/_lsq_backward_reference.py, as the softmax site.
dx / dhidden: test_gpu_site_backward._within -- error at most twice the eager chain's own largest error (torch's backward of
F.layer_norm(x * gamma + hidden, w, b) on the GPU, fed the same dn) plus one fp32 ulp at the largest reference magnitude.
Every figure is printed before it is asserted (pytest -s); profiles/layernorm_backward_accuracy.txt is that output."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _lsq_backward_reference as R  # noqa: E402
from conftest import bits_equal  # noqa: E402
from test_gpu_site_backward import VARIANTS, N, _quant, _within, dev  # noqa: E402,F401

from oracle import fake_quant_oracle as FQ  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
COLS = (4, 252, 256, 260, 512, 516, 768, 772, 1024, 1028, 2048)      # both sides of every R class (1 | 2 | 3 | 4 | 8)
FORMS = ("lone", "hidden", "hidden+gamma")
AFFINE = ("weight+bias", "bias", "none")
OUTPUTS = ("dx", "dhidden", "ds", "dz")


def _inputs(rng, rows, cols, form, affine):
    """Seeded normal data with a per-row offset and spread (mean and rstd differ by row); operands as the form asks."""
    def rowwise():
        return (rng.standard_normal((rows, cols)) * rng.uniform(0.5, 2.0, (rows, 1)) + rng.normal(0, 2.0, (rows, 1))).astype(F32)
    x = rowwise()
    hidden = rowwise() if form != "lone" else None
    gamma = rng.uniform(0.5, 1.5, cols).astype(F32) * np.where(rng.random(cols) < 0.2, -1, 1).astype(F32) if form == "hidden+gamma" else None
    w = rng.uniform(0.5, 1.5, cols).astype(F32) if affine == "weight+bias" else None
    b = (rng.standard_normal(cols) * 0.3).astype(F32) if affine != "none" else None
    return x, hidden, gamma, w, b


def _reference(x, hidden, gamma, w, eps, dn):
    """(dx, dhidden) in float64."""
    r = x.astype(np.float64) * (1.0 if gamma is None else gamma.astype(np.float64)) + (0.0 if hidden is None else hidden.astype(np.float64))
    mean = r.mean(-1, keepdims=True)
    rstd = 1.0 / np.sqrt(((r - mean) ** 2).mean(-1, keepdims=True) + eps)
    xhat = (r - mean) * rstd
    dxhat = dn.astype(np.float64) * (1.0 if w is None else w.astype(np.float64))
    dr = rstd * (dxhat - dxhat.mean(-1, keepdims=True) - xhat * (dxhat * xhat).mean(-1, keepdims=True))
    return dr * (1.0 if gamma is None else gamma.astype(np.float64)), dr


def clip_quant(exact):
    """(scale, zero point, qmax): 4 bits over about [-0.94, 0.94] of the normalised row, which cuts it off on both sides; else
    6 bits over [-3.9, 3.9].  Power-of-two scale: with integer gy and mode fixed every term of zero_point.grad is exact."""
    return (0.125, 7.0 if exact else 7.5, 15)


def _case(dev, cols, rows, form, affine, eps, variant, clip, off, exact=False):
    from outlier_suppression_amd import ops
    case = f"ln cols={cols} rows={rows} {form} {affine} eps={eps:g} {variant[0]} int_zp={variant[1]} clip={clip} off={off}"
    rng = np.random.default_rng([13, cols, rows, len(case)])
    x, hidden, gamma, w, b = _inputs(rng, rows, cols, form, affine)
    gy = rng.integers(-8, 9, (rows, cols)).astype(F32) if exact else rng.standard_normal((rows, cols)).astype(F32)
    T = lambda a: None if a is None else torch.from_numpy(a).to(dev)      # noqa: E731
    xd, hd, gd, wd, bd, gyd = (T(a) for a in (x, hidden, gamma, w, b, gy))
    mode, int_zp = variant
    scale, zp, qmax = clip_quant(exact) if clip else (0.125, 31.5, 63)
    s, z, code = _quant(dev, mode, int_zp, scale, zp)
    gf = FQ.lsqplus_grad_factor(x.size, qmax) if mode != "fixed" else 1.0
    quant = (s, z, 0, qmax, code, gf)
    n = N(ops.residual_layernorm_fake_quant(xd, hd, gd, wd, bd, eps, None))
    need = {name: name != off for name in OUTPUTS}
    run = lambda: ops.residual_layernorm_fake_quant_backward(xd, hd, gd, wd, bd, eps, gyd, quant, need["dx"], need["dhidden"],     # noqa: E731
                                                            need["ds"], need["dz"])
    dx, dh, ds, dz = run()
    assert [t is None for t in (dx, dh, ds, dz)] == [not need["dx"], not need["dhidden"] or hidden is None, not need["ds"], not need["dz"]]
    assert gamma is not None or dx is None or dh is None or dx.data_ptr() == dh.data_ptr(), "without gamma the two are one tensor"
    e = FQ.lsq_backward_exact(n, gy, N(s), N(z).astype(F32), 0, qmax, gf, mode)
    cut = float(np.mean(e.dx == 0))
    assert not clip or rows < 12 or 0.02 < cut < 0.98, (case, cut)       # a real share on either side of the clip decision
    _, ref_s, ref_z = FQ.lsq_backward_reference_order(n, gy, N(s), N(z).astype(F32), 0, qmax, gf, mode)
    for got, ex, A, ref, name in ((ds, e.dscale, e.A_s, ref_s, "ds"), (dz, e.dzp, e.A_z, ref_z, "dz")):
        if got is not None:
            fac = FQ.lsq_grad_factors(F32(gf), mode)[name == "dz"]
            e_k, bar = R.units(N(got), ex, A, fac), R.bar_units(R.units(ref, ex, A, fac), ex, A, fac)
            print(f"{case:<96} {name} {float(ex[0]):+.4e}  e_k {float(e_k.max()):.3f} units  bar {float(bar.max()):.3f}  clipped {cut:.2f}")
            assert (e_k <= bar).all(), (case, name, e_k, bar)
    if exact:       # the backward clipped exactly the elements the forward clipped: the sum of exact terms, rounded once
        assert bits_equal(N(dz), e.dzp.astype(F32)), (case, N(dz), e.dzp)
    # the eager chain: torch's backward of the same lines, fed the same dn
    xe, he = xd.clone().requires_grad_(True), None if hd is None else hd.clone().requires_grad_(True)
    r = xe if he is None else (xe if gd is None else xe * gd) + he
    ne = F.layer_norm(r, (cols,), wd, bd if wd is not None else None, eps)
    ne = ne + bd if (wd is None and bd is not None) else ne
    eager = torch.autograd.grad(ne, [xe] + ([] if he is None else [he]), T(e.dx.astype(F32)))
    ref_x, ref_h = _reference(x, hidden, gamma, w, eps, e.dx)
    if dx is not None:
        _within(case + " dx", N(dx), N(eager[0]), ref_x)
    if dh is not None:
        _within(case + " dhidden", N(dh), N(eager[1]), ref_h)
    assert all(a is None and b is None or bits_equal(N(a), N(b)) for a, b in zip(run(), (dx, dh, ds, dz))), "a second launch gives other words"


@pytest.mark.parametrize("cols", COLS)
def test_layernorm_site_backward(dev, cols):
    """Nine cases per width: rows 12 / 1 / 5 in turn, every operand form with three affine forms each, eps, the five quantizer
    variants, the clipping quantizer every other case, and each output switched off in turn (the fifth: none)."""
    for k in range(9):
        j = k + cols // 4
        _case(dev, cols, (12, 1, 5)[k % 3], FORMS[k // 3], AFFINE[(k + k // 3) % 3], (1e-5, 1e-12)[j % 2], VARIANTS[j % 5],
              clip=k % 2 == 1, off=(OUTPUTS + (None,))[j % 5])


@pytest.mark.parametrize("cols", (256, 512, 768, 1024, 2048))
def test_layernorm_site_backward_clips_what_the_forward_clipped(dev, cols):
    """One case per R class with integer gy, scale 2^-3 and mode fixed: zero_point.grad is word-equal to the exact sum."""
    _case(dev, cols, 12, "hidden+gamma", "weight+bias", 1e-5, ("fixed", True), clip=True, off=None, exact=True)


def test_layernorm_site_backward_grid_stride(dev):
    """Three rows past the first stride of the launcher's grid, at cols = 4."""
    from outlier_suppression_amd import ops
    _case(dev, 4, ops.LAYERNORM_BACKWARD_GRID_ROWS + 3, "hidden+gamma", "weight+bias", 1e-5, VARIANTS[0], clip=True, off=None)


def test_layernorm_site_backward_without_quantizer(dev):
    """quant=None (a site built with qoutput=False): dn = gy, no parameter gradients."""
    from outlier_suppression_amd import ops
    rng = np.random.default_rng(17)
    x, hidden, gamma, w, b = _inputs(rng, 5, 768, "hidden+gamma", "weight+bias")
    gy = rng.standard_normal(x.shape).astype(F32)
    xd, hd, gd, wd, bd, gyd = (torch.from_numpy(a).to(dev) for a in (x, hidden, gamma, w, b, gy))
    dx, dh, ds, dz = ops.residual_layernorm_fake_quant_backward(xd, hd, gd, wd, bd, 1e-5, gyd, None)
    assert ds is None and dz is None
    xe, he = xd.clone().requires_grad_(True), hd.clone().requires_grad_(True)
    eager = torch.autograd.grad(F.layer_norm(xe * gd + he, (768,), wd, bd, 1e-5), [xe, he], gyd)
    ref_x, ref_h = _reference(x, hidden, gamma, w, 1e-5, gy)
    _within("ln cols=768 rows=5 no quantizer dx", N(dx), N(eager[0]), ref_x)
    _within("ln cols=768 rows=5 no quantizer dhidden", N(dh), N(eager[1]), ref_h)


def test_layernorm_site_backward_refuses(dev):
    """2052 columns and a misaligned view raise from the launcher."""
    from outlier_suppression_amd import ops
    s, z, code = _quant(dev, "lsq", False, 0.125, 7.5)
    for x in (torch.randn(3, 2052, device=dev), torch.randn(3 * 256 + 4, device=dev)[1:-3].view(3, 256)):
        with pytest.raises(ValueError):
            ops.residual_layernorm_fake_quant_backward(x, None, None, None, None, 1e-5, torch.ones_like(x), (s, z, 0, 15, code, 1.0))

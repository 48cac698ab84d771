"""Backward of the head-split sites (csrc/heads_backward.hip) against ops.lsq_backward_per_tensor on the contiguous head-major
tensor and the oracle's exact float64 sums (oracle/fake_quant_oracle.py).

dx: WORD-EQUAL to ops.lsq_backward_per_tensor on the same elements, rearranged -- a per-element function, no tolerance.
scale.grad / zero_point.grad: the kernel walks another element order than the dense one, so they are held to the order-free
tier's bar of tests/test_gpu_lsq_backward_accuracy.py, max(3 e_ref, 4) U + 1 ulp (R.bar_units), against the exact sums; every
figure is printed before it is asserted (pytest -s; profiles/heads_backward_accuracy.txt is that output).  A second launch
gives the same words."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _lsq_backward_reference as R  # noqa: E402
from conftest import bits_equal  # noqa: E402
from test_gpu_site_backward import N, VARIANTS, _quant, dev  # noqa: E402,F401

from oracle import fake_quant_oracle as FQ  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
B, H = 2, 3
NEEDS = ((True, True, True), (False, True, True), (True, False, True), (True, True, False))     # (dx, scale.grad, zero_point.grad)
SENTINEL = -12345.0


def _grad(rng, dev, layout, shape):
    """A gradient of ``shape`` on the device in one of the layouts the launch meets, and its values."""
    g = rng.standard_normal(shape).astype(F32)
    if layout == "dense":
        return torch.from_numpy(g).to(dev), g
    if layout == "transposed":          # what matmul's backward returns for k^T: a view of the dense [B, h, d, T] tensor
        return torch.from_numpy(np.ascontiguousarray(np.swapaxes(g, -1, -2))).to(dev).transpose(-1, -2), g
    wide = torch.zeros(shape[:-1] + (2 * shape[-1],), device=dev)          # every other word of a wider tensor
    wide[..., ::2] = torch.from_numpy(g).to(dev)
    return wide[..., ::2], g


def _case(dev, direction, t, d, layouts, k=0, none_site=None):
    """One launch of len(layouts) sites with different parameters, variants and outputs per site."""
    from outlier_suppression_amd import ops
    split = direction == ops.HEADS_SPLIT
    n = len(layouts)
    rng = np.random.default_rng([23, direction, t, d, n, k])
    to_heads = lambda a: np.ascontiguousarray(a.reshape(B, t, H, d).transpose(0, 2, 1, 3))      # noqa: E731
    xs, grads, params, want, dx_out = [], [], [], [], []
    for i, layout in enumerate(layouts):
        mode, int_zp = VARIANTS[(i + k) % 5]
        qmin, qmax = ((0, 63), (-32, 31))[(i + k) % 2]
        x = (rng.standard_normal((B, t, H * d) if split else (B, H, t, d)) * 2.0).astype(F32)       # clips on both sides
        s, z, code = _quant(dev, mode, int_zp, 0.05 + 0.01 * i, (31.25, 0.75)[(i + k) % 2] + i)
        gf = FQ.lsqplus_grad_factor(x.size, qmax) if mode != "fixed" else 1.0
        g_dev, g = _grad(rng, dev, layout, (B, H, t, d) if split else (B, t, H * d))
        xs.append(torch.from_numpy(x).to(dev))
        grads.append(None if i == none_site else g_dev)
        params.append((s, z, qmin, qmax, code, gf))
        dx_out.append(torch.full_like(xs[-1], SENTINEL))
        want.append((to_heads(x) if split else x, g if split else to_heads(g), mode))
    needs = [NEEDS[(i + k) % 4] for i in range(n)]
    got = ops.fake_quant_heads_backward(xs, grads, params, H, direction, needs, dx_out=dx_out)
    again = ops.fake_quant_heads_backward(xs, grads, params, H, direction, needs)
    for i, ((dx, ds, dz), (xh, gh, mode), (s, z, qmin, qmax, code, gf)) in enumerate(zip(got, want, params)):
        case = f"{'split' if split else 'merge'} d={d} T={t} site {i + 1}/{n} {layouts[i]} {mode} zp={z.dtype} needs={needs[i]}"
        if i == none_site:
            assert (dx, ds, dz) == (None, None, None) and (N(dx_out[i]) == SENTINEL).all(), case
            continue
        assert [o is None for o in (dx, ds, dz)] == [not w for w in needs[i]], case
        assert all(a is None if b is None else bits_equal(N(a), N(b)) for a, b in zip(again[i], (dx, ds, dz))), "a second launch gives other words"
        if dx is None:
            assert (N(dx_out[i]) == SENTINEL).all(), case
        else:
            dxh = N(ops.lsq_backward_per_tensor(torch.from_numpy(xh).to(dev), torch.from_numpy(gh).to(dev), s, z, qmin, qmax, code, gf)[0])
            assert dx is dx_out[i] and bits_equal(N(dx), dxh.transpose(0, 2, 1, 3).reshape(B, t, H * d) if split else dxh), case
        zf = N(z).astype(F32)
        e = FQ.lsq_backward_exact(xh, gh, N(s), zf, qmin, qmax, gf, mode)
        cut = float(np.mean(e.dx == 0))
        assert xh.size < 100 or 0.1 < cut < 0.9, (case, cut)             # a real share on either side of the clip decision
        _, ref_s, ref_z = FQ.lsq_backward_reference_order(xh, gh, N(s), zf, qmin, qmax, gf, mode)
        for out, exact, A, ref, name in ((ds, e.dscale, e.A_s, ref_s, "ds"), (dz, e.dzp, e.A_z, ref_z, "dz")):
            if out is not None:
                fac = FQ.lsq_grad_factors(F32(gf), mode)[name == "dz"]
                e_k, bar = R.units(N(out), exact, A, fac), R.bar_units(R.units(ref, exact, A, fac), exact, A, fac)
                print(f"{case:<96} {name} {float(exact[0]):+.4e}  e_k {float(e_k.max()):.3f} units  bar {float(bar.max()):.3f}")
                assert (e_k <= bar).all(), (case, name, e_k, bar)


TILE = 64          # ops.HEADS_BACKWARD_TOKEN_TILE, asserted below: the parametrisation is made without the library
LAYOUTS = ("dense", "transposed", "strided")


# T: one token, no multiple of 4, a workgroup's sixteen tokens and one more, then either side of the transposed tile
@pytest.mark.parametrize("t", (1, 5, 16, 17, TILE - 1, TILE, TILE + 1))
@pytest.mark.parametrize("d", (4, 16, 64, 256))
def test_heads_backward(dev, d, t):
    from outlier_suppression_amd import ops
    assert ops.HEADS_BACKWARD_TOKEN_TILE == TILE
    k = (d.bit_length() + t) % 5
    n = (1, 3, 4)[k % 3]
    _case(dev, ops.HEADS_SPLIT, t, d, [LAYOUTS[(i + k) % 3] for i in range(n)], k, none_site=1 if k == 4 else None)
    _case(dev, ops.HEADS_SPLIT, t, d, ["transposed"], k + 1)
    _case(dev, ops.HEADS_MERGE, t, d, [("dense", "strided")[(i + k) % 2] for i in range((4, 1, 3)[k % 3])], k,
          none_site=0 if k == 3 else None)


def test_heads_backward_grid_stride(dev):
    """Four sites share the launch's workgroups: 448 each, two float4 per lane -- T = 600 at d = 256 is one float4 trip more."""
    from outlier_suppression_amd import ops
    _case(dev, ops.HEADS_SPLIT, 600, 256, ["dense", "transposed", "dense", "dense"])


@pytest.mark.parametrize("d", (12, 512))
def test_refused_geometry(dev, d):
    from outlier_suppression_amd import ops, util_layernorm as U
    from test_gpu_site_backward import _quantizer
    q = _quantizer(dev, "LSQPlusFakeQuantize", 0.05, 31.0)
    x = torch.zeros(B, 5, H * d, device=dev)
    saved = U.FUSE_HEADS_BACKWARD
    U.FUSE_HEADS_BACKWARD = True
    try:
        assert not ops.heads_fusable(B, 5, H, d)
        assert U.heads_backward_why_not((q,), (x,), H) == "the geometry is refused by heads_fusable"
        assert U.heads_backward_why_not((q,), (x.view(B, 5, H, d).transpose(1, 2).contiguous(),), H, ops.HEADS_MERGE) == \
            "the geometry is refused by heads_fusable"
    finally:
        U.FUSE_HEADS_BACKWARD = saved
    dx = torch.full_like(x, SENTINEL)
    with pytest.raises(ValueError, match="head_dim"):
        ops.fake_quant_heads_backward([x], [torch.zeros(B, H, 5, d, device=dev)], [(q.scale.data, q.zero_point.data, 0, 63, ops.PARAM_LSQPLUS, 1.0)],
                                      H, ops.HEADS_SPLIT, dx_out=[dx])
    assert (N(dx) == SENTINEL).all()

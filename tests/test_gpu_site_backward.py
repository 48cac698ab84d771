"""Backward of the one-launch GELU and attention-probabilities sites (csrc/site_backward.hip) against the oracle's per-element
rule (oracle/fake_quant_oracle.py, exact fp32) with the sums and the GELU / softmax derivative in float64.

scale.grad / zero_point.grad: the GELU site WORD-EQUAL to ops.lsq_backward_per_tensor(F.gelu(x), gy, ..); the softmax site under
the order-free tier's bar of tests/test_gpu_lsq_backward_accuracy.py (max(3 e_ref, 4) U + 1 ulp).  dx / dscores: error against
float64 at most twice the eager torch chain's own largest error on the same case plus one fp32 ulp at the largest reference
magnitude (the fused form recomputes one more rounding than eager).  Every figure is printed before it is asserted (pytest -s);
profiles/site_backward_accuracy.txt is that output."""
import math
import os
import sys
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _lsq_backward_reference as R  # noqa: E402
from conftest import bits_equal  # noqa: E402

from oracle import fake_quant_oracle as FQ  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
VARIANTS = (("lsqplus", False), ("lsq", True), ("lsq", False), ("fixed", True), ("fixed", False))     # (mode, int32 zero point)
NEEDS = ((True, True), (False, True), (True, False))                                                   # (scale.grad, zero_point.grad)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from outlier_suppression_amd import _hip
    _hip.load()
    return torch.device("cuda:0")


def N(t):
    return None if t is None else t.detach().cpu().numpy()


def _quant(dev, mode, int_zp, scale, zp):
    from outlier_suppression_amd import ops
    s = torch.tensor([scale], dtype=torch.float32, device=dev)
    z = torch.tensor([math.floor(zp) if int_zp else zp], dtype=torch.int32 if int_zp else torch.float32, device=dev)
    return s, z, {"fixed": ops.PARAM_FIXED, "lsq": ops.PARAM_LSQ, "lsqplus": ops.PARAM_LSQPLUS}[mode]


def _within(case, got, eager, ref):
    """The dx / dscores bar; prints the figures before it asserts."""
    e_k, e_e = (float(np.max(np.abs(a.astype(np.float64) - ref), initial=0.0)) for a in (got, eager))
    bar = 2.0 * e_e + float(np.spacing(F32(np.max(np.abs(ref), initial=0.0))))
    print(f"{case:<58} fused {e_k:.3e}  eager {e_e:.3e}  bar {bar:.3e}")
    assert np.isfinite(got).all() and e_k <= bar, (case, e_k, e_e, bar)


# one float4 either side of the two-load trip boundary of a one-block grid (256 lanes: 255 | 256 | 257 float4), several blocks
@pytest.mark.parametrize("n", (1, 3, 4, 1023, 1024 + 2, 4 * 255, 4 * 256, 4 * 257, 4 * 512 * 3 + 5))
def test_gelu_site_backward(dev, n):
    from outlier_suppression_amd import ops
    rng = np.random.default_rng([7, n])
    x = (rng.standard_normal(n) * 2.0).astype(F32)
    special = np.array([0.0, 0.5, -0.5, 6.0, -6.0, 40.0, -40.0], F32)[:n]
    x[rng.permutation(n)[:special.size]] = special
    gy = rng.standard_normal(n).astype(F32)
    xd, gd = torch.from_numpy(x).to(dev), torch.from_numpy(gy).to(dev)
    x64 = torch.from_numpy(x).double()
    dgelu = (0.5 * (1 + torch.special.erf(x64 / math.sqrt(2))) + x64 * torch.exp(-0.5 * x64 * x64) / math.sqrt(2 * math.pi)).numpy()
    g = N(F.gelu(xd))                        # the words the forward quantised (bit-identical to the kernel's: test_gpu_parity)
    for k, (mode, int_zp) in enumerate(VARIANTS):
        qmin, qmax = ((0, 63), (-32, 31))[k % 2]
        s, z, code = _quant(dev, mode, int_zp, 0.05, 2.5)
        gf = FQ.lsqplus_grad_factor(n, qmax) if mode != "fixed" else 1.0
        dx, ds, dz = ops.gelu_fake_quant_backward(xd, gd, s, z, qmin, qmax, code, gf)
        dg_t, ds_t, dz_t = ops.lsq_backward_per_tensor(F.gelu(xd), gd, s, z, qmin, qmax, code, gf)
        assert bits_equal(N(ds), N(ds_t)) and bits_equal(N(dz), N(dz_t)), (n, mode, int_zp)
        dg = FQ.lsq_backward_terms(g, gy, N(s), N(z).astype(F32), qmin, qmax, gf, mode)["dx"]
        assert bits_equal(N(dg_t), dg)
        _within(f"gelu n={n} {mode} int_zp={int_zp}", N(dx), N(torch.ops.aten.gelu_backward(dg_t, xd)), dg.astype(np.float64) * dgelu)
        for need_s, need_z in NEEDS:         # a second launch gives the same words; each output switched off in turn
            dx2, ds2, dz2 = ops.gelu_fake_quant_backward(xd, gd, s, z, qmin, qmax, code, gf, need_s, need_z)
            assert (ds2 is None) == (not need_s) and (dz2 is None) == (not need_z) and bits_equal(N(dx2), N(dx))
            assert (ds2 is None or bits_equal(N(ds2), N(ds))) and (dz2 is None or bits_equal(N(dz2), N(dz)))


def _mask(kind, b, t, s, rng, dev):
    """None, BERT's [B,1,1,S] with -inf keys, or BART's [B,1,T,S]."""
    if kind == "none":
        return None
    keep = rng.random((b, 1, 1 if kind == "bert" else t, s)) < 0.7
    keep[..., 0] = True                                        # no fully masked row ...
    keep[..., -1] = False                                      # ... and a masked key in every row
    return torch.from_numpy(np.where(keep, 0.0, -np.inf if kind == "bert" else -1e4).astype(F32)).to(dev)


def _softmax_case(dev, b, h, t, cols, pre, kind, variant, needs, clip):
    """``clip``: a 4-bit quantizer whose range [6, 21] / (8 cols) cuts the probabilities off on both sides (dp = 0 there, a
    term of zero_point.grad, and the zeros enter dot); else 6 bits over [0, 1], where nothing is clipped."""
    from outlier_suppression_amd import ops
    case = f"softmax cols={cols} [{b},{h},{t}] {pre} {kind} {variant[0]} int_zp={variant[1]} clip={clip}"
    rng = np.random.default_rng([11, b, h, t, cols, len(case)])
    scores = (rng.standard_normal((b, h, t, cols)) * 3.0).astype(F32)
    gy = rng.standard_normal((b, h, t, cols)).astype(F32)
    sd, gd = torch.from_numpy(scores).to(dev), torch.from_numpy(gy).to(dev)
    mask = _mask(kind, b, t, cols, rng, dev)
    kw = {"alpha": 0.125} if pre == "alpha" else {"divisor": 6.0} if pre == "divisor" else {}
    mode, int_zp = variant
    qmax = 15 if clip else 63
    s, z, code = _quant(dev, mode, int_zp, *((1.0 / (8 * cols), -5.75) if clip else (1.0 / 63, 0.25)))
    gf = FQ.lsqplus_grad_factor(scores.size, qmax) if mode != "fixed" else 1.0
    quant = (s, z, 0, qmax, code, gf)
    p_d = ops.attention_softmax_fake_quant(sd, mask, quant=None, **kw)
    p = N(p_d)
    dscores, ds, dz = ops.attention_softmax_fake_quant_backward(sd, mask, gd, quant, need_scale=needs[0], need_zp=needs[1], **kw)
    assert (ds is None) == (not needs[0]) and (dz is None) == (not needs[1])
    e = FQ.lsq_backward_exact(p, gy, N(s), N(z).astype(F32), 0, qmax, gf, mode)
    cut = float(np.mean(e.dx == 0))
    assert not clip or b * h * t < 12 or 0.02 < cut < 0.98, (case, cut)          # a real share on either side of the clip decision
    _, ref_s, ref_z = FQ.lsq_backward_reference_order(p, gy, N(s), N(z).astype(F32), 0, qmax, gf, mode)
    for got, exact, A, ref, name in ((ds, e.dscale, e.A_s, ref_s, "ds"), (dz, e.dzp, e.A_z, ref_z, "dz")):
        if got is not None:
            fac = FQ.lsq_grad_factors(F32(gf), mode)[name == "dz"]
            e_k, bar = R.units(N(got), exact, A, fac), R.bar_units(R.units(ref, exact, A, fac), exact, A, fac)
            print(f"{case:<58} {name} {float(exact[0]):+.4e}  e_k {float(e_k.max()):.3f} units  bar {float(bar.max()):.3f}  clipped {cut:.2f}")
            assert (e_k <= bar).all(), (case, name, e_k, bar)
    dp, p64 = e.dx.astype(np.float64), p.astype(np.float64)
    ref = p64 * (dp - (dp * p64).sum(-1, keepdims=True))
    ref = ref * 0.125 if pre == "alpha" else ref / 6.0 if pre == "divisor" else ref
    dv = torch._softmax_backward_data(ops.lsq_backward_per_tensor(p_d, gd, s, z, 0, qmax, code, gf)[0], p_d, -1, torch.float32)
    _within(case, N(dscores), N(dv * 0.125 if pre == "alpha" else dv / 6.0 if pre == "divisor" else dv), ref)
    if kind == "bert":
        dead = np.broadcast_to(np.isneginf(N(mask)), scores.shape)
        assert dead.any() and (N(dscores)[dead] == 0).all(), "a key masked with -inf got a gradient"
    again = ops.attention_softmax_fake_quant_backward(sd, mask, gd, quant, need_scale=needs[0], need_zp=needs[1], **kw)
    assert all(bits_equal(N(a), N(b)) for a, b in zip(again, (dscores, ds, dz))), "a second launch gives other words"


# both sides of every R class (R float4 per lane: 1 | 2 | 4 | 8 at 256 / 512 / 1024 columns)
@pytest.mark.parametrize("cols", (4, 252, 256, 260, 512, 516, 1024, 1028, 2048))
def test_softmax_site_backward(dev, cols):
    """12 rows: every (pre, mask) pair, the outputs asked for a latin square over them, the clipping quantizer every other
    case; 1 and 5 rows: every third combination each."""
    k = 0
    for b, h, t in ((1, 1, 1), (1, 5, 1), (2, 2, 3)):
        for j, pre in enumerate(("alpha", "divisor", "none")):
            for i, kind in enumerate(("none", "bert", "bart")):
                if (b, h, t) == (2, 2, 3) or k % 3 == (cols // 4) % 3:
                    _softmax_case(dev, b, h, t, cols, pre, kind, VARIANTS[k % 5], NEEDS[(i + j) % 3], clip=k % 2 == 1)
                k += 1


def test_softmax_site_backward_grid_stride(dev):
    """One row past the grid-stride start of the release grid: 2048 workgroups x 4 waves + 3 rows, at cols = 4."""
    _softmax_case(dev, 5, 1, 1639, 4, "alpha", "bart", VARIANTS[0], NEEDS[0], clip=True)      # a mask row per score row


def _quantizer(dev, kind, scale, zp):
    from outlier_suppression_amd.quantization import Quantizer
    q = Quantizer(None, NS(quantizer=kind, observer="MinMaxObserver", bit=6, symmetric=False, ch_axis=-1)).to(dev)
    q.disable_observer()
    q.enable_fake_quant()
    q.scale.data.fill_(scale)
    q.zero_point.data.fill_(zp if q.zero_point.dtype == torch.float32 else math.floor(zp))
    return q


@pytest.mark.parametrize("kind", ("LSQPlusFakeQuantize", "LSQFakeQuantize"))
def test_autograd_through_the_sites(dev, kind):
    """torch.autograd.grad through util_layernorm's two site functions returns the launchers' words with the switch on (the
    probabilities quantizer clips on both sides); with it off the eager lines run and the record says why."""
    from outlier_suppression_amd import ops, util_layernorm as U
    rng = np.random.default_rng(3)
    x = torch.from_numpy(rng.standard_normal((2, 5, 64)).astype(F32)).to(dev).requires_grad_(True)
    sc = torch.from_numpy((rng.standard_normal((2, 2, 5, 8)) * 8).astype(F32)).to(dev).requires_grad_(True)
    mask = torch.zeros(2, 1, 1, 8, device=dev)
    mask[1, ..., 6:] = -1e4
    saved = (U.FUSE_BACKWARD, U.FUSE_SOFTMAX)
    try:
        for fused in (True, False):
            U.FUSE_BACKWARD, U.FUSE_SOFTMAX = fused, True
            U.site_backward.reset()
            qg, qs = _quantizer(dev, kind, 0.05, 2.5), _quantizer(dev, kind, 1.0 / 256, -5.75)
            params = lambda q: [q.scale] + ([q.zero_point] if q.zero_point.requires_grad else [])    # noqa: E731
            y = U.activation_fake_quant(F.gelu, qg, x)
            gy = torch.from_numpy(rng.standard_normal(tuple(y.shape)).astype(F32)).to(dev)
            got = torch.autograd.grad(y, [x] + params(qg), gy)
            if kind == "LSQFakeQuantize":                      # BART's [B*h, T, S] view of the scores, the mask against [B, h, T, S]
                p = U.attention_probs_fake_quant(qs, sc.view(4, 5, 8), mask, alpha=0.125, heads=2)
            else:
                p = U.attention_probs_fake_quant(qs, sc, mask, alpha=0.125)
            gp = torch.from_numpy(rng.standard_normal(tuple(p.shape)).astype(F32)).to(dev)
            got_p = torch.autograd.grad(p, [sc] + params(qs), gp)
            counts = (U.site_backward.gelu, U.site_backward.softmax, U.site_backward.eager)
            if not fused:
                assert counts == (0, 0, 2) and U.site_backward.reason == "FUSE_BACKWARD is off"
                continue
            assert counts == (1, 1, 0)
            rec = lambda q, n: (q.scale.data, q.zero_point.data, q.quant_min, q.quant_max, q.param_mode, q._grad_factor(NS(numel=lambda: n)))    # noqa: E731
            want = ops.gelu_fake_quant_backward(x.detach(), gy, *rec(qg, x.numel()))
            want_p = ops.attention_softmax_fake_quant_backward(sc.detach(), mask, gp.view(sc.shape), rec(qs, sc.numel()), alpha=0.125)
            for g_, w_ in ((got, want), (got_p, want_p)):
                assert all(bits_equal(N(a), N(b).reshape(a.shape)) for a, b in zip(g_, w_))
    finally:
        U.FUSE_BACKWARD, U.FUSE_SOFTMAX = saved

"""One loss.backward() of the tiny W6A6 BERT of tests/test_gpu_site_backward_model.py in learn_scale's state with
FUSE_LAYERNORM_BACKWARD: all five LayerNorm sites take the one-launch pair, site_backward holds what it holds without the
switch, the logits are the no_grad forward's words.  The gradients' distance from the eager run is printed, not bounded: this
site's forward differs from torch's LayerNorm by a few ulp (README)."""
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch
from torch import nn

from conftest import bits_equal
from test_gpu_site_backward_model import _distance, _grads, model_and_batch  # noqa: F401

pytestmark = pytest.mark.gpu
N = lambda t: t.detach().cpu().numpy()      # noqa: E731


@pytest.fixture()
def switch():
    from outlier_suppression_amd import util_layernorm as U
    saved = U.FUSE_LAYERNORM_BACKWARD
    U.FUSE_LAYERNORM_BACKWARD = True
    U.layernorm_backward.reset()
    yield U
    U.FUSE_LAYERNORM_BACKWARD = saved


def test_one_backward_with_the_layernorm_sites_fused(model_and_batch, switch):
    from outlier_suppression_amd import token_wise_clipping as TWC
    U = switch
    U.FUSE_LAYERNORM_BACKWARD = False
    eager = _grads(model_and_batch)
    off = (U.site_backward.gelu, U.site_backward.softmax, U.site_backward.eager, U.site_backward.reason)
    assert (U.layernorm_backward.fused, U.layernorm_backward.reason) == (0, "FUSE_LAYERNORM_BACKWARD is off")
    U.FUSE_LAYERNORM_BACKWARD = True
    U.layernorm_backward.reset()
    fused = _grads(model_and_batch)
    assert (U.layernorm_backward.fused, U.layernorm_backward.eager) == (5, 0), U.layernorm_backward
    assert (U.site_backward.gelu, U.site_backward.softmax, U.site_backward.eager, U.site_backward.reason) == off
    assert all(torch.isfinite(g).all() for pair in fused.values() for g in pair)
    print(f"model     tiny BERT, LayerNorm sites fused: every quantizer's distance from eager {_distance(fused, eager, list(eager)):.3e} (recorded only: the forward differs by a few ulp)")

    model, batch, _, quantizers = model_and_batch
    with TWC._only_these_learn(model, [p for q in quantizers.values() for p in (q.scale, q.zero_point)]):
        logits = model(**batch)[0]
    with torch.no_grad():
        assert logits.requires_grad and bits_equal(N(logits), N(model(**batch)[0])), "both forwards take the same launch"

    U.layernorm_backward.reset()
    _grads(model_and_batch, strict=True)
    assert (U.layernorm_backward.fused, U.layernorm_backward.eager) == (0, 5), U.layernorm_backward
    assert U.layernorm_backward.reason == "the strict summation tier is defined on the eager tensors"


@pytest.mark.parametrize("split", (False, True))
def test_autograd_through_residual_layernorm(switch, split):
    """torch.autograd.grad through util_layernorm.residual_layernorm with a set gamma returns the launcher's words."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from outlier_suppression_amd import ops
    U, dev = switch, torch.device("cuda:0")
    rng = np.random.default_rng(9)
    T = lambda *shape: torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).to(dev)      # noqa: E731
    org = nn.LayerNorm(64).to(dev)
    org.weight.data, org.bias.data = T(64).abs() + 0.5, T(64) * 0.3
    a_q = NS(quantizer="LSQPlusFakeQuantize", observer="MinMaxObserver", bit=4, symmetric=False, ch_axis=-1)
    ln = (U.QuantizedSplitLayerNorm if split else U.QuantizedLayerNorm)(org, None, a_q).to(dev).requires_grad_(False)
    q = ln.layernorm_post_act_fake_quantize
    q.disable_observer()
    q.enable_fake_quant()
    q.scale.data.fill_(0.125)
    q.zero_point.data.fill_(7.5)
    q.scale.requires_grad_(True)
    q.zero_point.requires_grad_(True)
    res = U.GammaResidual()
    res.set_gamma(T(64).abs() + 0.5)
    res.requires_grad_(False)
    x, h = T(2, 5, 64).requires_grad_(True), T(2, 5, 64).requires_grad_(True)
    y = U.residual_layernorm(res, ln, x, h)
    assert (U.layernorm_backward.fused, U.layernorm_backward.eager) == (1, 0), U.layernorm_backward
    gy = T(2, 5, 64)
    got = torch.autograd.grad(y, [x, h, q.scale, q.zero_point], gy)
    weight, bias = (None, ln.bias) if split else (org.weight, org.bias)
    quant = (q.scale.data, q.zero_point.data, q.quant_min, q.quant_max, q.param_mode, q._grad_factor(NS(numel=lambda: x.numel())))
    want = ops.residual_layernorm_fake_quant_backward(x.detach(), h.detach(), res.gamma.data, weight, bias, ln.layernorm.eps, gy, quant)
    assert all(bits_equal(N(a), N(b).reshape(a.shape)) for a, b in zip(got, want))
    with torch.no_grad():
        assert bits_equal(N(y), N(U.residual_layernorm(res, ln, x, h)))

"""The FUSE_LAYERNORM_BACKWARD switch, its environment variable and every reason an autograd pass through a LayerNorm site keeps
the eager lines, on CPU tensors (no launch: the reasons are decided before any)."""
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import outlier_suppression_amd as osq
from outlier_suppression_amd import ops, util_layernorm as U
from test_site_backward_cpu import _q


@pytest.fixture()
def switches():
    saved = (U.FUSE_LAYERNORM_BACKWARD, U.FUSE_LAYERNORM, U.FUSE_BACKWARD, ops._tuning.get("bwd_sum_order", 0))
    yield
    U.FUSE_LAYERNORM_BACKWARD, U.FUSE_LAYERNORM, U.FUSE_BACKWARD = saved[:3]
    ops._tuning["bwd_sum_order"] = saved[3]
    U.layernorm_backward.reset()
    U.site_backward.reset()


def test_switch_and_environment(switches):
    assert U.FUSE_LAYERNORM_BACKWARD is False, "off when unset"
    osq.set_fast_layernorm_backward(True)
    assert U.FUSE_LAYERNORM_BACKWARD is True and U.FUSE_BACKWARD is False, "a switch of its own"
    osq.set_fast_layernorm_backward(False)
    assert U.FUSE_LAYERNORM_BACKWARD is False
    env = osq.fast_layernorm_backward_from_environment
    assert env({}) is False and env({"OSQ_FAST_LAYERNORM_BACKWARD": "0"}) is False and env({"OSQ_FAST_LAYERNORM_BACKWARD": "1"}) is True
    assert (osq.set_fast_layernorm_backward, "OSQ_FAST_LAYERNORM_BACKWARD") in osq._SWITCHES


LEARNS = nn.Parameter(torch.ones(8))
FROZEN = nn.Parameter(torch.ones(8), requires_grad=False)
WIDTH = "the row width is not a multiple of 4 up to 2048"
LAYOUT = "the operands are not dense, 16-byte aligned fp32 tensors of the site's shape"
REASONS = [          # (what differs from a call the kernel would take on a GPU, the reason)
    (dict(on=False), "FUSE_LAYERNORM_BACKWARD is off"),
    (dict(layernorm=False), "FUSE_LAYERNORM is off"),
    (dict(q=None), "the quantizer is missing"),
    (dict(q=_q(ch_axis=0)), "the quantizer is per-channel"),
    (dict(q=_q(observer_enabled=1)), "the quantizer is observing or disabled"),
    (dict(q=_q(fake_quant_enabled=0)), "the quantizer is observing or disabled"),
    (dict(weight=LEARNS), "a LayerNorm parameter requires a gradient"),
    (dict(bias=LEARNS), "a LayerNorm parameter requires a gradient"),
    (dict(hidden=torch.zeros(2, 3, 8), gamma=LEARNS), "a LayerNorm parameter requires a gradient"),
    (dict(strict=8), "the strict summation tier is defined on the eager tensors"),
    (dict(x=torch.zeros(2, 8, dtype=torch.float64)), "the input is not fp32"),
    (dict(x=torch.zeros(2, 6)), WIDTH),
    (dict(x=torch.zeros(1, 2052)), WIDTH),
    (dict(x=torch.zeros(8)), WIDTH),
    (dict(x=torch.zeros(3, 2, 8).transpose(0, 1)), LAYOUT),
    (dict(x=torch.zeros(2 * 3 * 8 + 4)[1:-3].view(2, 3, 8)), LAYOUT),
    (dict(hidden=torch.zeros(2, 1, 8)), LAYOUT),
    (dict(hidden=torch.zeros(2, 3, 8), gamma=FROZEN, weight=FROZEN, bias=FROZEN),
     "the input or the quantizer's parameters are not on a GPU"),       # frozen parameters are no reason
]


@pytest.mark.parametrize("case,reason", REASONS)
def test_reasons(switches, case, reason):
    U.FUSE_LAYERNORM_BACKWARD, U.FUSE_LAYERNORM = case.get("on", True), case.get("layernorm", True)
    ops._tuning["bwd_sum_order"] = case.get("strict", 0)
    why = U.layernorm_backward_why_not(case.get("q", _q()), case.get("x", torch.zeros(2, 3, 8)), case.get("hidden"),
                                       case.get("gamma"), case.get("weight"), case.get("bias"))
    assert why == reason


def test_a_refused_autograd_pass_takes_the_eager_lines(switches):
    """On CPU tensors the residual pair and both lone forms run their eager lines under autograd,
    whatever the switch says; the site's own record keeps the count and the reason, site_backward is left alone."""
    U.FUSE_LAYERNORM_BACKWARD = True
    U.layernorm_backward.reset()
    U.site_backward.reset()
    ln = U.QuantizedLayerNorm(nn.LayerNorm(8), None, None, qoutput=False)
    x, h = torch.randn(2, 3, 8, requires_grad=True), torch.randn(2, 3, 8)
    y = U.residual_layernorm(U.GammaResidual(), ln, x, h)
    assert torch.equal(y, ln.layernorm(x + h)) and y.requires_grad
    assert torch.equal(ln(x), F.layer_norm(x, (8,), ln.layernorm.weight, ln.layernorm.bias, ln.layernorm.eps))
    assert (U.layernorm_backward.fused, U.layernorm_backward.eager) == (0, 2), "the residual pair counts once"
    assert U.layernorm_backward.reason == "a LayerNorm parameter requires a gradient"
    for p in ln.layernorm.parameters():
        p.requires_grad_(False)
    ln(x)          # qoutput=False is no reason: such a site only normalises
    assert U.layernorm_backward.eager == 3 and U.layernorm_backward.reason == "the input or the quantizer's parameters are not on a GPU"
    with torch.no_grad():
        ln(x)
    assert U.layernorm_backward.eager == 3, "only autograd passes are counted"
    assert (U.site_backward.gelu, U.site_backward.softmax, U.site_backward.eager, U.site_backward.reason) == (0, 0, 0, None)

"""The FUSE_BACKWARD switch, its environment variable and every reason an autograd pass keeps the eager lines, on CPU tensors
(no launch: the reasons are decided before any)."""
from types import SimpleNamespace as NS

import pytest
import torch
import torch.nn.functional as F

import outlier_suppression_amd as osq
from outlier_suppression_amd import ops, util_layernorm as U


@pytest.fixture()
def switches():
    saved = (U.FUSE_BACKWARD, U.FUSE_SOFTMAX, U.FUSE_ACTIVATION, ops._tuning.get("bwd_sum_order", 0))
    yield
    U.FUSE_BACKWARD, U.FUSE_SOFTMAX, U.FUSE_ACTIVATION = saved[:3]
    ops._tuning["bwd_sum_order"] = saved[3]
    U.site_backward.reset()


def _q(**over):
    """A stand-in for a per-tensor quantizer in its plain quantising state with parameters on the CPU."""
    return NS(**{**dict(ch_axis=-1, fake_quant_enabled=1, observer_enabled=0, scale=torch.ones(1)), **over})


def test_switch_and_environment(switches):
    assert U.FUSE_BACKWARD is False, "off when unset"
    osq.set_fast_backward(True)
    assert U.FUSE_BACKWARD is True
    osq.set_fast_backward(False)
    assert U.FUSE_BACKWARD is False
    assert osq.fast_backward_from_environment({}) is False and osq.fast_backward_from_environment({"OSQ_FAST_BACKWARD": "0"}) is False
    assert osq.fast_backward_from_environment({"OSQ_FAST_BACKWARD": "1"}) is True
    assert (osq.set_fast_backward, "OSQ_FAST_BACKWARD") in osq._SWITCHES


REASONS = [          # (site, what differs from a call the kernels would take on a GPU, the reason)
    ("gelu", dict(on=False), "FUSE_BACKWARD is off"),
    ("gelu", dict(activation=False), "FUSE_ACTIVATION is off"),
    ("gelu", dict(q=None), "the quantizer is missing"),
    ("gelu", dict(q=_q(ch_axis=0)), "the quantizer is per-channel"),
    ("gelu", dict(q=_q(observer_enabled=1)), "the quantizer is observing or disabled"),
    ("gelu", dict(q=_q(fake_quant_enabled=0)), "the quantizer is observing or disabled"),
    ("gelu", dict(strict=8), "the strict summation tier is defined on the eager tensors"),
    ("gelu", dict(x=torch.zeros(2, 8, dtype=torch.float64)), "the input is not fp32"),
    ("gelu", dict(act=F.relu), "the activation is not the exact GELU"),
    ("gelu", dict(), "the input or the quantizer's parameters are not on a GPU"),
    ("softmax", dict(on=False), "FUSE_BACKWARD is off"),
    ("softmax", dict(softmax=False), "FUSE_SOFTMAX is off"),
    ("softmax", dict(dropout=(0.1, True)), "dropout is active"),
    ("softmax", dict(mask=torch.zeros(2, 1, 1, 8, requires_grad=True)), "the mask requires a gradient"),
    ("softmax", dict(x=torch.zeros(2, 2, 3, 6)), "the row width is not a multiple of 4 up to 2048"),
    ("softmax", dict(x=torch.zeros(1, 1, 1, 2052)), "the row width is not a multiple of 4 up to 2048"),
    ("softmax", dict(q=_q(ch_axis=1)), "the quantizer is per-channel"),
    ("softmax", dict(strict=16), "the strict summation tier is defined on the eager tensors"),
    ("softmax", dict(dropout=(0.1, False)), "the input or the quantizer's parameters are not on a GPU"),      # inactive dropout is no reason
]


@pytest.mark.parametrize("site,case,reason", REASONS)
def test_reasons(switches, site, case, reason):
    U.FUSE_BACKWARD, U.FUSE_ACTIVATION, U.FUSE_SOFTMAX = case.get("on", True), case.get("activation", True), case.get("softmax", True)
    ops._tuning["bwd_sum_order"] = case.get("strict", 0)
    q, x = case.get("q", _q()), case.get("x", torch.zeros(2, 2, 3, 8))
    why = U.gelu_backward_why_not(case.get("act", F.gelu), q, x) if site == "gelu" else \
        U.softmax_backward_why_not(q, x, case.get("mask"), case.get("dropout"))
    assert why == reason


def test_a_refused_autograd_pass_takes_the_eager_lines(switches):
    """On CPU tensors with no quantizer both sites run their eager lines under autograd, whatever the switch says, and
    the record keeps the count and the reason."""
    U.FUSE_BACKWARD, U.FUSE_SOFTMAX = True, True
    U.site_backward.reset()
    x = torch.randn(2, 3, 8, requires_grad=True)
    y = U.activation_fake_quant(F.gelu, None, x)
    p = U.attention_probs_fake_quant(None, torch.randn(2, 2, 3, 8, requires_grad=True), None, divisor=2.0)
    assert torch.equal(y, F.gelu(x)) and p.requires_grad
    assert (U.site_backward.gelu, U.site_backward.softmax, U.site_backward.eager) == (0, 0, 2)
    assert U.site_backward.reason == "the quantizer is missing"
    with torch.no_grad():
        U.activation_fake_quant(F.gelu, None, x)
    assert U.site_backward.eager == 2, "only autograd passes are counted"

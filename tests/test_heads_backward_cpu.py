"""The FUSE_HEADS_BACKWARD switch, its environment variable and every reason an autograd pass through the query / key / value
head-split sites or the context site keeps the eager lines, on CPU tensors (no launch: the reasons are decided before any)."""
import pytest
import torch

import outlier_suppression_amd as osq
from outlier_suppression_amd import ops, util_layernorm as U
from test_site_backward_cpu import _q


@pytest.fixture()
def switches():
    saved = (U.FUSE_HEADS_BACKWARD, U.FUSE_QKV, U.FUSE_BACKWARD, ops._tuning.get("bwd_sum_order", 0))
    yield
    U.FUSE_HEADS_BACKWARD, U.FUSE_QKV, U.FUSE_BACKWARD = saved[:3]
    ops._tuning["bwd_sum_order"] = saved[3]
    U.heads_backward.reset()


def test_switch_and_environment(switches):
    assert U.FUSE_HEADS_BACKWARD is False, "off when unset"
    osq.set_fast_heads_backward(True)
    assert U.FUSE_HEADS_BACKWARD is True and U.FUSE_BACKWARD is False, "a switch of its own"
    osq.set_fast_heads_backward(False)
    assert U.FUSE_HEADS_BACKWARD is False
    env = osq.fast_heads_backward_from_environment
    assert env({}) is False and env({"OSQ_FAST_HEADS_BACKWARD": "0"}) is False and env({"OSQ_FAST_HEADS_BACKWARD": "1"}) is True
    assert (osq.set_fast_heads_backward, "OSQ_FAST_HEADS_BACKWARD") in osq._SWITCHES
    assert ops.HEADS_BACKWARD_TOKEN_TILE == 64
    assert ops.heads_fusable(2, 5, 3, 16) and ops.heads_fusable(1, 1, 1, 256)
    assert not any(ops.heads_fusable(2, 5, 3, d) for d in (0, 2, 6, 12, 512)) and not ops.heads_fusable(0, 5, 3, 16)


GEOMETRY = "the geometry is refused by heads_fusable"
LAYOUT = "the input is not a dense, 16-byte aligned tensor"
REASONS = [          # (what differs from a call the kernel would take on a GPU, the reason); x: [2, 5, 3 heads * 16]
    (dict(on=False), "FUSE_HEADS_BACKWARD is off"),
    (dict(qkv=False), "FUSE_QKV is off"),
    (dict(q=None), "the quantizer is missing"),
    (dict(q=_q(ch_axis=0)), "the quantizer is per-channel"),
    (dict(q=_q(observer_enabled=1)), "the quantizer is observing or disabled"),
    (dict(q=_q(fake_quant_enabled=0)), "the quantizer is observing or disabled"),
    (dict(strict=8), "the strict summation tier is defined on the eager tensors"),
    (dict(x=torch.zeros(2, 5, 48, dtype=torch.float64)), "the input is not fp32"),
    (dict(x=torch.zeros(2, 5, 36)), GEOMETRY),                    # d = 12: d / 4 is no power of two
    (dict(x=torch.zeros(2, 5, 3 * 512)), GEOMETRY),               # d = 512: beyond 64 float4s
    (dict(x=torch.zeros(2, 5, 50)), GEOMETRY),                    # the width is no multiple of the heads
    (dict(x=torch.zeros(5, 48)), GEOMETRY),
    (dict(x=torch.zeros(5, 2, 48).transpose(0, 1)), LAYOUT),
    (dict(x=torch.zeros(2 * 5 * 48 + 4)[1:-3].view(2, 5, 48)), LAYOUT),
    (dict(), "the input or the quantizer's parameters are not on a GPU"),
    (dict(merge=True, x=torch.zeros(2, 3, 5, 12)), GEOMETRY),
    (dict(merge=True, x=torch.zeros(2, 4, 5, 16)), GEOMETRY),     # another number of heads
    (dict(merge=True, x=torch.zeros(2, 5, 3, 16).transpose(1, 2)), LAYOUT),
    (dict(merge=True, x=torch.zeros(2, 3, 5, 16)), "the input or the quantizer's parameters are not on a GPU"),
]


@pytest.mark.parametrize("case,reason", REASONS)
def test_reasons(switches, case, reason):
    U.FUSE_HEADS_BACKWARD, U.FUSE_QKV = case.get("on", True), case.get("qkv", True)
    ops._tuning["bwd_sum_order"] = case.get("strict", 0)
    x = case.get("x", torch.zeros(2, 5, 48))
    direction = ops.HEADS_MERGE if case.get("merge") else ops.HEADS_SPLIT
    assert U.heads_backward_why_not((_q(), case.get("q", _q())), (torch.zeros_like(x), x), 3, direction) == reason


class _Scale(torch.nn.Module):
    """A quantizer's call signature on CPU tensors: x * 0.5, whatever the view."""
    ch_axis, fake_quant_enabled, observer_enabled = -1, 1, 0

    def __init__(self):
        super().__init__()
        self.scale = torch.nn.Parameter(torch.ones(1))

    def forward(self, x, observation_mask=None, seq_pos=-1):
        return x * 0.5


@pytest.mark.parametrize("on", (False, True))
def test_a_refused_autograd_pass_takes_the_eager_lines(switches, on):
    """Switch off, or on with CPU tensors: the three functions return what they return today, and the record says why."""
    U.FUSE_HEADS_BACKWARD = on
    U.heads_backward.reset()
    q = _Scale()
    x = torch.randn(2, 5, 48, requires_grad=True)
    ctx = torch.randn(2, 3, 5, 16, requires_grad=True)
    assert U.qkv_heads_fake_quant((q, q, q), (x, x, x), 3) is None
    y = U.split_heads_fake_quant(q, x, 3)
    assert torch.equal(y, (x * 0.5).view(2, 5, 3, 16).transpose(1, 2)) and y.is_contiguous() and y.requires_grad
    m = U.merge_heads_fake_quant(q, ctx)
    assert torch.equal(m, (ctx * 0.5).permute(0, 2, 1, 3).reshape(2, 5, 48)) and m.requires_grad
    assert torch.equal(U.merge_heads_fake_quant(None, ctx), ctx.permute(0, 2, 1, 3).reshape(2, 5, 48))
    r = U.heads_backward
    assert (r.split, r.merge, r.eager) == (0, 0, 4)
    assert r.reason == ("the quantizer is missing" if on else "FUSE_HEADS_BACKWARD is off")
    with torch.no_grad():
        U.split_heads_fake_quant(q, x, 3)
        U.merge_heads_fake_quant(q, ctx)
    assert r.eager == 4, "only autograd passes are counted"

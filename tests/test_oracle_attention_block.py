"""The cases of tests/_attention_block.py against the reference's own arithmetic on the CPU: torch's eager fp32 sequence of
an attention block -- matmul, scaling, + mask, softmax, fake-quant (oracle/fake_quant_oracle.py), matmul, merge heads,
fake-quant -- in two summation orders (the matrix products as torch.matmul adds them, and as explicit loops over the summed
index) must keep to the helper's rule: entries the helper calls sure are word-equal to the float64 restatement, the others at
most one quantization step off, and no output of any case has more than 10 % of its entries unsure.  This is what entitles
tests/test_gpu_attention_block.py to hold the kernel to the same rule: the bound is verified here, not on the kernel."""
import numpy as np
import pytest
import torch

import _attention_block as AB
from oracle import fake_quant_oracle as FQ


def _fake_quant(x, g):
    if g is None:
        return x
    s, z = FQ.lsq_effective(g.scale_after, g.zp_after, g.grad_factor, g.mode)
    xq = FQ.quantize_affine(x, np.float32(s), np.float32(z), g.qmin, g.qmax)
    return FQ.dequantize_affine(xq, np.float32(s), np.float32(z))


def _eager(ref, loops):
    """(probabilities [B, h, T, S], merged output [B, T, h*d]) of the eager sequence; ``loops``: both products as explicit
    loops over the summed index, one fp32 multiply and one fp32 add per step."""
    q, k, v = (torch.from_numpy(ref[n]) for n in "qkv")
    mask = None if ref["mask"] is None else torch.from_numpy(ref["mask"])
    if loops:
        w = torch.zeros(q.shape[:3] + (k.shape[2],))
        for i in range(q.shape[3]):
            w = w + q[..., i:i + 1] * k[..., i].unsqueeze(2)
    else:
        w = torch.matmul(q, k.transpose(-1, -2))
    if ref["alpha"] is not None:
        w = torch.add(mask, w, alpha=ref["alpha"]) if mask is not None else w * ref["alpha"]
    else:
        if ref["divisor"] is not None:
            w = w / ref["divisor"]
        if mask is not None:
            w = w + mask
    probs = _fake_quant(torch.softmax(w, dim=-1).numpy(), ref["probs_q"])
    p = torch.from_numpy(probs)
    if loops:
        ctx = torch.zeros(q.shape)
        for j in range(k.shape[2]):
            ctx = ctx + p[..., j:j + 1] * v[:, :, j].unsqueeze(2)
    else:
        ctx = torch.matmul(p, v)
    b, h, t, d = ctx.shape
    out = _fake_quant(ctx.permute(0, 2, 1, 3).contiguous().view(b, t, h * d).numpy(), ref["ctx_q"])
    return probs, out


@pytest.mark.parametrize("head_dim", AB.HEAD_DIMS)
def test_eager_sequence_keeps_to_the_rule(head_dim):
    worst = [0.0, 0.0]
    with torch.no_grad():
        for case in AB.table(head_dim):
            ref = AB.reference(case)           # raises where no instance keeps to the cap: nothing is skipped
            for loops in (False, True):
                probs, out = _eager(ref, loops)
                ctx = AB.expect_context(ref, probs)
                for name, expect, got in (("probs", ref["probs"], probs), ("ctx", ctx, out)):
                    assert expect.mismatch(got) is None, (case, ref["seed"], loops, name, expect.mismatch(got))
                worst = [max(worst[0], ref["probs"].share), max(worst[1], ctx.share)]
    print(f"head_dim {head_dim}: {len(AB.table(head_dim))} cases, largest unsure share probs {worst[0]:.4f} ctx {worst[1]:.4f}")


def test_table_covers_what_it_claims():
    for head_dim in AB.HEAD_DIMS:
        t = AB.table(head_dim)
        assert {(c.tokens, c.kv_len) for c in t} == {(a, b) for a in AB.TOKENS for b in AB.KV_LENS}
        assert {(c.bits, c.mode) for c in t} == set(AB.QUANTS) and any(c.bad_params for c in t)
        assert {c.mask for c in t} == set(AB.MASKS) and {c.pre for c in t} == set(AB.PRES) and {c.sites for c in t} == set(AB.SITES)
        assert {(c.batch, c.heads) for c in t} == set(AB.GEOMETRIES)
        for s in AB.KV_LENS:                   # every length with each geometry, a mask, a pre-scaling and both quantizers
            row = [c for c in t if c.kv_len == s]
            assert {(c.batch, c.heads) for c in row} == set(AB.GEOMETRIES)
            assert any(c.mask != "none" for c in row) and any(c.pre != "none" for c in row) and any(c.sites == "both" for c in row)
    assert AB.TOKENS == (1, 31, 32, 33, 67) and AB.KV_LENS == (1, 3, 31, 32, 33, 69, 1024)


def test_a_fully_masked_row_is_uniform():
    """finfo.min on every position of a row: the scores are finfo.min, their differences 0, every probability 1 / S."""
    rng = np.random.default_rng(5)
    q, k = (rng.standard_normal((1, 1, 2, 16)).astype(np.float32) for _ in range(2))
    mask = np.zeros((1, 1, 2, 2), np.float32)
    mask[0, 0, 1] = AB.FMIN
    p, _ = AB.probabilities64(q, k, mask, None, None)
    assert (p[0, 0, 1] == 0.5).all() and p[0, 0, 0, 0] != 0.5
    with torch.no_grad():
        w = torch.matmul(torch.from_numpy(q), torch.from_numpy(k).transpose(-1, -2)) + torch.from_numpy(mask)
        assert (torch.softmax(w, -1)[0, 0, 1] == 0.5).all()

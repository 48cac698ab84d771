"""The tie-free cases of tests/_decode_attention.py against the reference's own arithmetic on the CPU: the eager torch fp32
sequence of quant_bart.py:232-268 for one query token -- bmm, + mask, softmax, fake-quant (oracle/fake_quant_oracle.py),
bmm, fake-quant -- must give the helper's float64 integer codes EXACTLY ("0 entries differ"), in two summation orders: as
written, and with the cache positions reversed.  This is what entitles tests/test_gpu_decode_attention.py to compare the
kernel's words with the helper's: the bound behind "tie-free" is verified here, not on the kernel under test."""
import numpy as np
import pytest
import torch

import _decode_attention as DA
from conftest import same_f32
from oracle import fake_quant_oracle as FQ


def _fake_quant(x, g):
    s, z = FQ.lsq_effective(g.scale_after, g.zp_after, g.grad_factor, g.mode)
    xq = FQ.quantize_affine(x, np.float32(s), np.float32(z), g.qmin, g.qmax)
    return xq, FQ.dequantize_affine(xq, np.float32(s), np.float32(z))


def _eager(ref, reverse):
    """(probabilities codes [B, h, 1, S], context codes [B, h, d], output [B, 1, h*d]) of the eager sequence."""
    case = ref["case"]
    b, h, d, s = case.batch, case.heads, case.head_dim, case.kv_len
    q, k, v = (torch.from_numpy(ref[n]) for n in "qkv")
    mask = None if ref["mask"] is None else torch.from_numpy(ref["mask"])
    if reverse:
        k, v = k.flip(2).contiguous(), v.flip(2).contiguous()
        mask = None if mask is None else mask.flip(3).contiguous()
    w = torch.bmm(q.view(b * h, 1, d), k.view(b * h, s, d).transpose(1, 2))
    if mask is not None:
        w = (w.view(b, h, 1, s) + mask).view(b * h, 1, s)
    probs = torch.softmax(w, dim=-1)
    p_codes, p_fq = _fake_quant(probs.numpy(), ref["probs_q"])
    ctx = torch.bmm(torch.from_numpy(p_fq), v.view(b * h, s, d)).view(b, h, 1, d)
    ctx = ctx.permute(0, 2, 1, 3).contiguous().view(b, 1, h * d)
    c_codes, out = _fake_quant(ctx.numpy(), ref["ctx_q"])
    p_codes = p_codes.reshape(b, h, 1, s)
    return (p_codes[..., ::-1] if reverse else p_codes), c_codes.reshape(b, h, d), out


def _check(case):
    ref = DA.reference(case)
    for reverse in (False, True):
        p_codes, c_codes, out = _eager(ref, reverse)
        bad_p, bad_c = int((p_codes != ref["probs_codes"]).sum()), int((c_codes != ref["ctx_codes"]).sum())
        assert bad_p == 0 and bad_c == 0, (case, ref["seed"], reverse, bad_p, bad_c, ref["margin"], ref["worst_g"])
        assert same_f32(out, ref["out"]), (case, reverse)


@pytest.mark.parametrize("head_dim", DA.HEAD_DIMS)
def test_eager_sequence_gives_the_float64_codes(head_dim):
    with torch.no_grad():
        for case in DA.table(head_dim):
            _check(case)


def test_eager_sequence_at_the_kv_limit():
    with torch.no_grad():
        _check(DA.LIMIT_CASE)


def test_table_covers_what_it_claims():
    """Every head size meets every quantizer variant with every mask and cap variant, bad raw parameters included, and a
    fully masked row gives the uniform row of the eager formula."""
    for head_dim in DA.HEAD_DIMS:
        t = DA.table(head_dim)
        assert {(c.bits, c.mode, c.mask) for c in t} == {(b, m, k) for b, m in DA.QUANTS for k in DA.MASKS}
        assert {(c.mask, c.cap) for c in t} == {(m, c) for m in DA.MASKS for c in DA.CAPS}
        assert any(c.bad_params for c in t) and {c.kv_len for c in t} == set(DA.kv_lens(head_dim))
    case = next(c for c in DA.table(64) if c.mask == "full" and c.kv_len == 17 and c.batch == 2 and c.bits == "sym8")
    ref = DA.reference(case)
    g = ref["probs_q"]
    uniform = g.quantize(np.float64(np.float32(1.0) / np.float32(case.kv_len)) / float(g.scale_eff) * np.ones(1))[1][0]
    assert (ref["probs"][-1] == uniform).all()

"""Whole-sequence attention on integer codes, the CPU side: the numpy restatement of the rule (tests/_attention_int.py)
against torch's eager float64 sequence, the condition on the cases of the GPU table (the unsure share of the float64
reference alone), the exactness lemma the kernel rests on, and the gate of util_layernorm.attention_int_block_fake_quant."""
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import _attention_int as AI
from _attention_int import F32, U


def _t64(x):
    return torch.from_numpy(np.ascontiguousarray(x)).double()


def _fq64(x, g):
    """torch's eager fake-quant (util_quant.py:12-14) in float64 with the effective parameters of ``g``."""
    if g is None:
        return x
    s, zp = float(g.scale_eff), float(g.zp_eff)
    return (torch.clamp(torch.round(x / s) + zp, g.qmin, g.qmax) - zp) * s


def _eager64(ref):
    """q / k / v fake-quant, matmul, pre, mask, softmax, probabilities fake-quant, matmul, merge, context fake-quant."""
    qg, kg, vg, pq, cq = ref["groups"]
    q, k, v = _fq64(_t64(ref["q"]), qg), _fq64(_t64(ref["k"]), kg), _fq64(_t64(ref["v"]), vg)
    x = torch.matmul(q, k.transpose(-1, -2))
    if ref["alpha"] is not None:
        x = x * ref["alpha"]
    elif ref["divisor"] is not None:
        x = x / ref["divisor"]
    if ref["mask"] is not None:
        x = x + _t64(ref["mask"])
    probs = _fq64(torch.softmax(x, -1), pq)
    return probs, v


def _cpu_cases():
    return [c for d in (16, 64) for c in AI.table(d)[::7] if c.kv_len <= 257]


@pytest.mark.parametrize("case", _cpu_cases(), ids=lambda c: f"{c.head_dim}-{c.tokens}-{c.kv_len}")
def test_restatement_against_the_eager_float64_sequence(case):
    ref = AI.reference(case)
    qg, kg, vg, pq, cq = ref["groups"]
    for x, g in zip((ref["q"], ref["k"], ref["v"]), (qg, kg, vg)):           # on the grid: the quantizer changes no word
        assert np.array_equal(AI.fake_quant(x, g), x)
    out, probs = AI.rule_f32(ref)
    eager_probs, v64 = _eager64(ref)
    expect = ref["probs"]
    assert np.array_equal(eager_probs.numpy().astype(F32)[expect.sure], expect.words[expect.sure])
    assert expect.mismatch(probs) is None, (case, expect.mismatch(probs))
    # the context of the restatement's own probability words, eager in float64: the rule rounds C once, s_p * s_v once and
    # their product once; the eager operands are the WORDS fl(n_p * s_p) and fl(n_v * s_v), one rounding each per term
    c64 = torch.matmul(_t64(probs), v64)
    abs64 = torch.matmul(_t64(probs).abs(), v64.abs())
    merged, terms = (x.permute(0, 2, 1, 3).reshape(out.shape).numpy() for x in (c64, abs64))
    ctx = AI.Expect(merged, 3 * U * np.abs(merged) + 2 * U * terms + 2.0 ** -148, cq)
    eager_out = _fq64(torch.from_numpy(merged), cq).numpy().astype(F32)
    assert np.array_equal(eager_out[ctx.sure], ctx.words[ctx.sure])
    # (no cap on the unsure share here: values on a coarse grid land on exact ties of the context quantizer, S = 1 at 4 bits)
    assert not np.isnan(out).any() and np.array_equal(out[ctx.sure], ctx.words[ctx.sure]), case
    assert (np.abs(out.astype(np.float64) - ctx.words.astype(np.float64)) <= ctx.slack).all(), case


@pytest.mark.parametrize("head_dim", AI.HEAD_DIMS)
def test_unsure_share_of_every_gpu_case(head_dim):
    """A condition on the cases, not a measurement: the float64 reference alone stays within UNSURE_CAP."""
    worst = (0.0, 0.0, None)
    for case in AI.table(head_dim):
        ref = AI.reference(case)
        assert ref["probs"].share <= AI.UNSURE_CAP and ref["probs"].worst < 0.5, case
        worst = max(worst, (ref["probs"].share, ref["probs"].worst, case), key=lambda w: w[0])
    print(f"\nhead_dim {head_dim}: {len(AI.table(head_dim))} cases, largest unsure share {worst[0]:.5f} "
          f"(largest 4 g there {worst[1]:.4f}) at {worst[2]}")


def test_table_meets_every_tile_and_chunk_edge():
    lens = {c.kv_len for c in AI.table(16)}
    for m in range(AI.TK, 2 * AI.CHUNK + 1, AI.TK):
        assert {m - 1, m, m + 1} <= lens, m
    assert {1, 3, 1023, 1024, 1025, 2049} <= lens and {c.tokens for c in AI.table(16)} == set(AI.TOKENS)
    assert {(c.batch, c.heads) for c in AI.table(16)} == set(AI.GEOMETRIES)
    assert {c.quant for c in AI.table(16)} == set(AI.QUANTS) and {c.ctx for c in AI.table(16)} == {True, False}


def _sums(terms):
    fwd = rev = F32(0)
    for a, b in zip(terms, terms[::-1]):
        fwd, rev = F32(fwd + a), F32(rev + b)
    pair = terms.copy()
    while len(pair) > 1:
        pair = (pair[0::2] + pair[1::2]).astype(F32)
    return fwd, rev, pair[0]


@pytest.mark.parametrize("signs", ("plus", "minus", "mixed"))
def test_exactness_lemma(signs):
    """head_dim 128 with every |n| = 255, and a 128-key context chunk of 255 x 255 products: fp32 accumulation forward, in
    reverse and pairwise equals the int64 sum (255 is exact in bf16: 8 significant bits)."""
    rng = np.random.default_rng(5)
    sign = dict(plus=np.ones(128), minus=-np.ones(128), mixed=rng.choice([-1.0, 1.0], 128))[signs]
    terms = (F32(255) * F32(255) * sign).astype(F32)
    exact = int((255 * 255 * sign.astype(np.int64)).sum())
    assert abs(exact) < 2 ** 24 and 128 * 255 * 255 < 2 ** 24
    for total in _sums(terms):
        assert int(total) == exact and float(total) == exact
    b = np.array([255.0], F32).view(np.uint32)
    assert b & 0xFFFF == 0                                   # the bf16 word of 255 is its fp32 word's upper half


def _quantizer(kind="FixedFakeQuantize", bit=8, ch_axis=-1):
    from outlier_suppression_amd.quantization import Quantizer
    q = Quantizer(None, NS(quantizer=kind, observer="AvgMinMaxObserver", bit=bit, symmetric=False, ch_axis=ch_axis))
    q.disable_observer()
    q.enable_fake_quant()
    return q


def test_gate_names_its_reason():
    from outlier_suppression_amd import util_layernorm as UL
    qs = [_quantizer() for _ in range(5)]
    q, k, v = torch.zeros(1, 2, 4, 16), torch.zeros(1, 2, 5, 16), torch.zeros(1, 2, 5, 16)
    old = UL.FUSE_ATTENTION_INT
    UL.FUSE_ATTENTION_INT = True
    try:
        def gate(quantizers=qs, **kw):
            reason = UL.attention_int_refusal(*quantizers, q, k, v, **kw)
            assert UL.attention_int_block_fake_quant(*quantizers, q, k, v, **kw) is None
            return reason
        with torch.no_grad():
            assert "GPU" in gate()                                                   # CPU tensors
            assert "dropout" in gate(dropout=(0.1, True))
            assert gate(dropout=(0.1, False)) == gate()
            assert "per-channel" in gate(qs[:2] + [_quantizer(ch_axis=3)] + qs[3:])
            observing = _quantizer()
            observing.enable_observer()
            assert "observing" in gate(qs[:3] + [observing] + qs[4:])
            for i, name in enumerate("qkv"):
                assert f"the {name} quantizer is missing" == gate(qs[:i] + [None] + qs[i + 1:])
            assert "GPU" in gate(qs[:4] + [None])                                    # the context quantizer is optional
            assert "256 codes" in gate([_quantizer(bit=9)] + qs[1:])
        with torch.enable_grad():
            assert "autograd" in gate()
        UL.FUSE_ATTENTION_INT = False
        with torch.no_grad():
            assert "off" in gate()
    finally:
        UL.FUSE_ATTENTION_INT = old


def test_switch():
    import outlier_suppression_amd as osq
    from outlier_suppression_amd import util_layernorm as UL
    assert UL.FUSE_ATTENTION_INT is False
    osq.set_fast_attention_int(True)
    try:
        assert UL.FUSE_ATTENTION_INT is True
    finally:
        osq.set_fast_attention_int(False)


@pytest.mark.parametrize("value,want", ((None, False), ("", False), ("0", False), ("1", True), ("yes", True)))
def test_environment_switch_through_reset_tier(monkeypatch, value, want):
    """OSQ_FAST_ATTENTION_INT as reset_tier applies it (what the first load of the library does), whatever the flag held
    before; the fp32 form's switch has a variable of its own and does not move with it."""
    import outlier_suppression_amd as osq
    from outlier_suppression_amd import util_layernorm as UL
    for name in ("FUSE_ATTENTION_INT", "FUSE_ATTENTION"):
        monkeypatch.setattr(UL, name, getattr(UL, name))               # put back after the test
    monkeypatch.delenv("OSQ_FAST_ATTENTION", raising=False)
    if value is None:
        monkeypatch.delenv("OSQ_FAST_ATTENTION_INT", raising=False)
    else:
        monkeypatch.setenv("OSQ_FAST_ATTENTION_INT", value)
    UL.FUSE_ATTENTION_INT = not want
    osq.reset_tier()
    assert UL.FUSE_ATTENTION_INT is want and UL.FUSE_ATTENTION is False

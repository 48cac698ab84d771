"""The edge table of tests/_attention_block.py against the reference's own arithmetic on the CPU: what entitles
tests/test_gpu_attention_block_edges.py to hold the kernel to the helper's rule at lengths chosen from the kernel's constants,
with masks of every stride pattern, finite mask values, -inf and a scaling factor that is no power of two.  Torch's eager fp32
sequence (``_eager`` of tests/test_oracle_attention_block.py, in both summation orders) must keep to ``Expect.mismatch`` on
every case, the context restated from its own probability words: the bound is verified here, not on the kernel.

The table's claim to meet the kernel's loop boundaries is asserted from the tile sizes ops exports: if the kernel's tiling
changes, the assertion fails and the table cannot quietly stop covering it."""
import numpy as np
import pytest
import torch

import _attention_block as AB
from test_oracle_attention_block import _eager


@pytest.mark.parametrize("head_dim", AB.HEAD_DIMS)
def test_eager_sequence_keeps_to_the_rule_at_the_edges(head_dim):
    worst = [0.0, 0.0]
    with torch.no_grad():
        for case in AB.edge_table(head_dim):
            ref = AB.reference(case)           # raises where no instance keeps to the cap: nothing is skipped
            for loops in (False, True):
                probs, out = _eager(ref, loops)
                ctx = AB.expect_context(ref, probs)
                for name, expect, got in (("probs", ref["probs"], probs), ("ctx", ctx, out)):
                    assert expect.mismatch(got) is None, (case, ref["seed"], loops, name, expect.mismatch(got))
                worst = [max(worst[0], ref["probs"].share), max(worst[1], ctx.share)]
    print(f"head_dim {head_dim}: {len(AB.edge_table(head_dim))} edge cases, largest unsure share probs {worst[0]:.4f} ctx {worst[1]:.4f}")


def test_edge_table_meets_the_kernels_boundaries():
    """per (steps of a wave's segment of the context) on both sides of one and of two batches of IN_FLIGHT steps at every
    segment count; key tiles on both sides of one and of two rounds of the waves; every class of S; the ragged split."""
    from outlier_suppression_amd import ops
    assert (ops.ATTENTION_TQ, ops.ATTENTION_TK, ops.ATTENTION_MAX_KV) == (AB.TQ, AB.TK, AB.S_CLASSES[-1])
    assert ops.ATTENTION_HEAD_DIMS == AB.HEAD_DIMS
    assert [AB.segments(d) for d in AB.HEAD_DIMS] == [4, 4, 2, 1]
    n = AB.IN_FLIGHT
    for d in AB.HEAD_DIMS:
        t = AB.edge_table(d)
        assert len(t) == 28 and {(c.tokens, c.kv_len) for c in t} == {(a, b) for a in AB.EDGE_TOKENS for b in AB.EDGE_KV_LENS}
        per = {AB.steps_per_segment(d, c.kv_len) for c in t}
        # one segment (head_dim 128) has S = 2 per: the edge table meets two batches and one step more, table() one batch
        assert {2 * n, 2 * n + 1} <= per and ({n, n + 1} <= per or AB.segments(d) == 1), (d, sorted(per))
        assert {n, n + 1} <= per | {AB.steps_per_segment(d, c.kv_len) for c in AB.table(d)}, d
        assert {AB.WAVES, AB.WAVES + 1, 2 * AB.WAVES, 2 * AB.WAVES + 1} <= {AB.key_tiles(c.kv_len, ops.ATTENTION_TK) for c in t}
        for cls in AB.S_CLASSES:               # each class at its top, its odd top and (but the first) one past the class below
            assert {cls - 1 if cls == 1024 else cls, cls - 1} <= {c.kv_len for c in t if AB.s_class(c.kv_len) == cls}
            assert cls == 128 or cls // 2 + 1 in {c.kv_len for c in t}
        # five steps: 2, 2, 1 and none for four segments, 3 and 2 for two
        assert 9 in AB.EDGE_KV_LENS and -(-9 // 2) == 5
        assert {(c.bits, c.mode) for c in t} == set(AB.QUANTS) and any(c.bad_params for c in t)
        assert {c.mask for c in t} == set(AB.EDGE_MASKS) and {c.sites for c in t} == set(AB.SITES)
        assert {(c.mask, c.pre) for c in t} == {(m, p) for m in AB.EDGE_MASKS for p in AB.EDGE_PRES}
        for m in AB.EDGE_MASKS:                # every mask with both geometries and with both token counts
            assert {(c.batch, c.heads) for c in t if c.mask == m} == set(AB.GEOMETRIES), (d, m)
            assert {c.tokens for c in t if c.mask == m} == set(AB.EDGE_TOKENS), (d, m)
        for s in AB.EDGE_KV_LENS:
            assert {(c.batch, c.heads) for c in t if c.kv_len == s} == set(AB.GEOMETRIES)
    assert AB.EDGE_KV_LENS == (9, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023) and AB.EDGE_TOKENS == (1, 33)
    # alpha_d is a power of two at head_dim 16 and 64 and rounds at 32 and 128
    assert [np.frexp(AB.pre_args(AB.Case(d, 1, 9, 1, 1, "sym8", "fixed", False, "none", "alpha_d", "both"))[0])[0] == 0.5
            for d in AB.HEAD_DIMS] == [True, False, True, False]


def test_mask_kinds_have_the_strides_they_are_for():
    """What the ops wrapper hands the kernel is ``mask.expand(B, h, T, S).stride()``: head leaves the batch stride 0 with a
    head stride, bias has all three, neginf a token stride alone."""
    rng = np.random.default_rng(0)
    for kind, expect in (("head", (False, True, True)), ("bias", (True, True, True)), ("neginf", (False, False, True))):
        for d in AB.HEAD_DIMS[:2]:             # the masks start at the head size's index: both parities of the rotation
            assert any(c.mask == kind and (c.batch, c.heads) == (2, 3) for c in AB.edge_table(d)), (kind, d)
        case = next(c for d in AB.HEAD_DIMS for c in AB.edge_table(d)
                    if c.mask == kind and (c.batch, c.heads) == (2, 3) and c.tokens > 1)
        m = AB.build_mask(case, rng)
        assert m.dtype == np.float32
        strides = torch.from_numpy(m).expand(case.batch, case.heads, case.tokens, case.kv_len).stride()
        assert tuple(x > 0 for x in strides[:3]) == expect and strides[3] == 1, (kind, strides)
        closed = np.broadcast_to(m <= np.float32(AB.FMIN), (case.batch, case.heads, case.tokens, case.kv_len))
        assert closed.any() == (kind != "bias") and not closed.all(-1).any(), kind      # every row keeps an open position
        if kind == "head":
            assert set(np.unique(m)) == {np.float32(AB.FMIN), np.float32(0.0)} and (m[..., 0] == 0).all()
            assert 0.2 < (m != 0).mean() < 0.4 and (m[0, 0] != m[0, 1]).any()
        if kind == "bias":
            finite = m[m != -10000.0]
            assert (m == -10000.0).any() and (finite != 0).all() and np.abs(finite).max() < 4.0
            assert (m[0, 0] != m[0, 1]).any() and (m[0] != m[1]).any()
        if kind == "neginf":
            assert set(np.unique(m)) == {np.float32(-np.inf), np.float32(0.0)}
            assert (m[0, 0, 0, 1:] == -np.inf).sum() == min(case.tokens, case.kv_len) - 1


def test_masks_of_zero_and_finfo_min_are_restated_as_before():
    """A finite mask entry is added in float64 and widens the bound by one rounding; 0 and finfo.min give the numbers they
    gave when they were the only values: -inf is finfo.min, and an entry below half an ulp of the score changes no bound
    but its own."""
    rng = np.random.default_rng(2)
    q, k = (rng.standard_normal((2, 3, 5, 16)).astype(np.float32) for _ in range(2))
    m = np.zeros((2, 1, 5, 9), np.float32)
    k = np.concatenate([k, k], 2)[:, :, :9]
    m[:, :, :, 6:] = AB.FMIN
    m[0, 0, 2, 1] = AB.FMIN
    p, err = AB.probabilities64(q, k, m, 0.25, None)
    assert (p[:, :, :, 6:] == 0).all() and (p[0, :, 2, 1] == 0).all() and (p[1, :, 2, 1] > 0).all()
    inf = np.where(m != 0, np.float32(-np.inf), m)
    p2, err2 = AB.probabilities64(q, k, inf, 0.25, None)
    assert (p2 == p).all() and (err2 == err).all()
    # a finite entry: the float64 softmax of dot + m, and a wider bound at that entry's row only
    b = m.copy()
    b[1, 0, 3, 2] = 0.75
    p3, err3 = AB.probabilities64(q, k, b, 0.25, None)
    dot = np.einsum("bhtd,bhsd->bhts", q.astype(np.float64), k.astype(np.float64)) * 0.25 + np.where(b == np.float32(AB.FMIN), -np.inf, b)
    e = np.exp(dot - dot.max(-1, keepdims=True))
    assert np.allclose(p3, e / e.sum(-1, keepdims=True), rtol=1e-13, atol=0)
    other = np.ones(p.shape, bool)
    other[1, :, 3] = False
    assert (p3[other] == p[other]).all() and (err3[other] == err[other]).all()
    assert (err3[1, :, 3, 2] / p3[1, :, 3, 2] > err[1, :, 3, 2] / p[1, :, 3, 2]).all()
    # a factor that is no power of two rounds once more than one that is
    _, err4 = AB.probabilities64(q, k, m, float(np.float32(0.3)), None)
    _, err5 = AB.probabilities64(q * np.float32(1.2), k, m, 0.25, None)
    assert np.frexp(0.25)[0] == 0.5 and np.frexp(float(np.float32(0.3)))[0] != 0.5
    open_ = p > 0
    assert (err4[open_] / np.maximum(err5[open_], 1e-300)).min() > 1.0


def test_minus_infinity_in_torch_softmax():
    """A row of only -inf is NaN; -inf beyond an open position is an exact zero, as finfo.min is."""
    w = torch.tensor([[0.5, -1.0, 2.0, 0.25], [0.5, -1.0, 2.0, 0.25], [0.5, -1.0, 2.0, 0.25]])
    ninf = float("-inf")
    mask = torch.tensor([[0.0, ninf, 0.0, ninf], [ninf, ninf, ninf, ninf], [ninf, ninf, 0.0, ninf]])
    p = torch.softmax(w + mask, -1)
    assert torch.isnan(p[1]).all() and not torch.isnan(p[0]).any() and not torch.isnan(p[2]).any()
    assert (p[0, 1::2] == 0).all() and (p[0, 0::2] > 0).all()
    assert p[2].tolist() == [0.0, 0.0, 1.0, 0.0]
    twin = torch.softmax(w + torch.where(mask == ninf, torch.tensor(AB.FMIN), mask), -1)
    assert torch.equal(twin[0], p[0]) and torch.equal(twin[2], p[2]) and (twin[1] == 0.25).all()

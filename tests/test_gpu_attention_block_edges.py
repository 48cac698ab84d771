"""ops.attention_fake_quant (csrc/attention_block.hip) where tests/test_gpu_attention_block.py does not reach: the edge table
of tests/_attention_block.py -- every class of S at its top, its odd top and one past the class below; a wave's segment of
the context on both sides of one and of two batches of loads; key tiles on both sides of one and of two rounds of the waves;
the ragged split of five steps -- under masks with a head stride and no batch stride, finite mask values, -inf and a scaling
factor that is no power of two, against the float64 restatement under the rule tests/test_oracle_attention_block_edges.py
holds the eager CPU sequence to.  Then the forms no table case takes: no ``probs_out`` (the only form the models launch),
zero strides on K and V, a mask that is an offset view with rows further apart than S, NaN and -inf at the rows a ragged
tile repeats, and the refusals for empty tensors and a token stride that is no multiple of four."""
import numpy as np
import pytest
import torch

import _attention_block as AB
from conftest import same_f32
from test_gpu_attention_block import SENTINEL, dev, launch, quant, tensors  # noqa: F401  (dev is the module's fixture)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("head_dim", AB.HEAD_DIMS)
def test_edge_table_against_float64(dev, head_dim):
    worst = [0.0, 0.0]
    for case in AB.edge_table(head_dim):
        ref = AB.reference(case)
        got = launch(ref, dev, *tensors(ref, dev))
        assert got is not None, case
        out, probs = got
        assert not (probs == SENTINEL).any() and not (out == SENTINEL).any(), case
        ctx = AB.expect_context(ref, probs)
        for name, expect, words in (("probs", ref["probs"], probs), ("ctx", ctx, out)):
            assert expect.mismatch(words) is None, (case, ref["seed"], name, expect.mismatch(words))
        worst = [max(worst[0], ref["probs"].share), max(worst[1], ctx.share)]
    print(f"head_dim {head_dim}: {len(AB.edge_table(head_dim))} edge cases, largest unsure share probs {worst[0]:.4f} ctx {worst[1]:.4f}")


def _class_cases():
    """One length per class of S, one past the class below (and past one batch of loads at two segments), one per head size."""
    return [AB.Case(d, AB.TQ + 1, s, 2, 3, bits, mode, False, mask, pre, "both")
            for (d, s, mask, pre), (bits, mode) in zip(((16, 513, "pad", "alpha"), (32, 257, "bias", "alpha_d"),
                                                        (64, 65, "head", "divisor"), (128, 129, "neginf", "none")), AB.QUANTS)]


@pytest.mark.parametrize("case", _class_cases(), ids=lambda c: f"{c.head_dim}-{c.kv_len}")
def test_without_probs_out_the_context_has_the_same_words(dev, case):
    """The launch the models make: ``probs_out`` a null pointer.  The tensor alone comes back, word for word the context of
    the launch that also wrote the probabilities; with ``want_probs`` and no buffer the pair comes back."""
    from outlier_suppression_amd import ops
    assert AB.s_class(case.kv_len) == {16: 1024, 32: 512, 64: 128, 128: 256}[case.head_dim]
    ref = AB.evaluate(case, AB.first_seed(case))
    q, k, v, mask = tensors(ref, dev)
    full_out, full_probs = launch(ref, dev, q, k, v, mask)
    out = torch.full((case.batch, case.tokens, case.heads * case.head_dim), SENTINEL, dtype=torch.float32, device=dev)
    got = ops.attention_fake_quant(q, k, v, mask, quant(ref["probs_q"], dev), quant(ref["ctx_q"], dev), alpha=ref["alpha"],
                                   divisor=ref["divisor"], want_probs=False, out=out)
    torch.cuda.synchronize()
    assert got is out and same_f32(out.cpu().numpy(), full_out)
    pair = ops.attention_fake_quant(q, k, v, mask, quant(ref["probs_q"], dev), quant(ref["ctx_q"], dev), alpha=ref["alpha"],
                                    divisor=ref["divisor"], want_probs=True)
    torch.cuda.synchronize()
    assert isinstance(pair, tuple) and len(pair) == 2 and pair[1].shape == (case.batch, case.heads, case.tokens, case.kv_len)
    assert same_f32(pair[0].cpu().numpy(), full_out) and same_f32(pair[1].cpu().numpy(), full_probs)


def test_broadcast_and_offset_views(dev):
    """K and V shared by the batch rows (``expand``: batch stride 0, beam search's cross-attention), and a mask that is a
    ``[..., 1:S + 1]`` view of a wider buffer full of NaN: the words of the materialised copies.  A mask expanded along S is
    refused."""
    case = AB.Case(32, AB.TQ + 1, 129, 2, 3, "sym8", "fixed", False, "causal", "alpha", "both")
    ref = AB.evaluate(case, AB.first_seed(case))
    q, k, v, mask = tensors(ref, dev)
    b, h, t, s, d = case.batch, case.heads, case.tokens, case.kv_len, case.head_dim
    k1, v1 = k[:1].contiguous(), v[:1].contiguous()
    ke, ve = k1.expand(b, h, s, d), v1.expand(b, h, s, d)
    assert ke.stride(0) == 0 and ve.stride(0) == 0 and ke.data_ptr() == k1.data_ptr()
    dense = launch(ref, dev, q, ke.contiguous(), ve.contiguous(), mask)
    got = launch(ref, dev, q, ke, ve, mask)
    assert got is not None and same_f32(got[0], dense[0]) and same_f32(got[1], dense[1])
    assert not same_f32(dense[0][1], launch(ref, dev, q, k, v, mask)[0][1])      # batch row 1 did read the shared K and V
    qe = q[:1].contiguous().expand(b, h, t, d)                                   # and one query for every batch row
    got = launch(ref, dev, qe, k, v, mask)
    assert qe.stride(0) == 0 and got is not None
    dense = launch(ref, dev, qe.contiguous(), k, v, mask)
    assert same_f32(got[0], dense[0]) and same_f32(got[1], dense[1])

    buf = torch.full((b, 1, t, s + 3), float("nan"), dtype=torch.float32, device=dev)
    view = buf[..., 1:s + 1]
    view.copy_(mask)
    assert view.data_ptr() % 16 == 4 and view.stride() == (t * (s + 3), t * (s + 3), s + 3, 1)
    dense = launch(ref, dev, q, k, v, mask)
    got = launch(ref, dev, q, k, v, view)
    assert got is not None and same_f32(got[0], dense[0]) and same_f32(got[1], dense[1])

    column = torch.zeros((b, 1, t, 1), dtype=torch.float32, device=dev).expand(b, 1, t, s)
    assert column.stride(3) == 0 and launch(ref, dev, q, k, v, column) is None


def test_special_rows_at_the_edges(dev):
    """T = TQ + 5: the second tile has five rows, and its 27 padded rows repeat row T - 1.  S = 65: odd, one position past
    two key tiles and past one batch of loads of each of the two segments."""
    case = AB.Case(64, AB.TQ + 5, 2 * AB.TK + 1, 2, 3, "sym8", "lsqplus", False, "causal", "divisor", "both")
    ref = AB.evaluate(case, AB.first_seed(case))
    q, k, v, mask = tensors(ref, dev)
    b, h, t, s, d = case.batch, case.heads, case.tokens, case.kv_len, case.head_dim
    clean_out, clean_probs = launch(ref, dev, q, k, v, mask)
    assert not np.isnan(clean_out).any() and not np.isnan(clean_probs).any()
    b0, h0, t0 = 1, 2, t - 1

    def only(rows_p, rows_o, out, probs, what):
        """NaN at exactly these entries; every other word is the clean launch's."""
        assert (np.isnan(probs) == rows_p).all() and (np.isnan(out) == rows_o).all(), what
        assert same_f32(probs[~rows_p], clean_probs[~rows_p]) and same_f32(out[~rows_o], clean_out[~rows_o]), what

    # ---- a NaN in the row the padded rows repeat
    q2 = q.clone()
    q2[b0, h0, t0, 5] = float("nan")
    out, probs = launch(ref, dev, q2, k, v, mask)
    nan_p, nan_o = np.zeros(probs.shape, bool), np.zeros(out.shape, bool)
    nan_p[b0, h0, t0] = True
    nan_o[b0, t0, h0 * d:(h0 + 1) * d] = True
    only(nan_p, nan_o, out, probs, "NaN in q")

    # ---- a mask row of only -inf: NaN in that row of every head the mask row covers
    for row in (t0, AB.TQ - 1):
        m = mask.clone()
        m[b0, 0, row] = float("-inf")
        out, probs = launch(ref, dev, q, k, v, m)
        nan_p, nan_o = np.zeros(probs.shape, bool), np.zeros(out.shape, bool)
        nan_p[b0, :, row] = True
        nan_o[b0, row] = True
        only(nan_p, nan_o, out, probs, ("-inf row", row))

    # ---- -inf on every position but one: the probabilities are fq(1) there and fq(0) elsewhere, whatever q and k are; the
    # context is ONE product, fq(1) * V[j] rounded once, plus zeros (fq(0) is +0 for an integer zero point)
    pq, cq = ref["probs_q"], ref["ctx_q"]
    for row, j in ((t0, s - 1), (0, 0), (AB.TQ, AB.TK)):           # s - 1: the position whose partner in the last step is S
        m = mask.clone()
        m[b0, 0, row] = float("-inf")
        m[b0, 0, row, j] = 0.0
        out, probs = launch(ref, dev, q, k, v, m)
        p64 = np.zeros((h, s))
        p64[:, j] = 1.0
        expect_p = AB.Expect(p64, np.zeros((h, s)), pq)
        assert expect_p.sure.all() and expect_p.mismatch(probs[b0, :, row]) is None, (row, j, expect_p.mismatch(probs[b0, :, row]))
        assert (probs[b0, :, row, :j] == 0).all() and (probs[b0, :, row, j + 1:] == 0).all() and (probs[b0, :, row, j] > 0).all()
        one = probs[b0, :, row, j].astype(np.float64)[:, None] * ref["v"][b0, :, j].astype(np.float64)         # [h, d]
        expect_c = AB.Expect(one.reshape(h * d), AB.U * np.abs(one).reshape(h * d), cq)
        assert expect_c.mismatch(out[b0, row]) is None, (row, j, expect_c.mismatch(out[b0, row]))
        assert expect_c.sure.mean() > 0.9
        other_p, other_o = np.ones(probs.shape, bool), np.ones(out.shape, bool)
        other_p[b0, :, row] = False
        other_o[b0, row] = False
        assert same_f32(probs[other_p], clean_probs[other_p]) and same_f32(out[other_o], clean_out[other_o]), (row, j)


def test_empty_tensors_and_a_token_stride_of_two_mod_four_launch_nothing(dev):
    ref = dict(alpha=None, divisor=None, probs_q=None, ctx_q=None)

    def randn(*shape):
        return torch.randn(*shape, device=dev)
    k, v = randn(1, 2, 7, 32), randn(1, 2, 7, 32)
    got = launch(ref, dev, randn(1, 2, 0, 32), k, v, None)          # T = 0: None, or the empty output
    assert got is None or (got[0].size == 0 and got[1].size == 0)
    assert launch(ref, dev, randn(1, 2, 5, 32), randn(1, 2, 0, 32), randn(1, 2, 0, 32), None) is None          # S = 0
    # [B, T, h * d] values in rows of h * d + 2 floats: head_dim contiguous, 16-byte aligned, token stride 66
    wide = randn(1, 5, 2 * 32 + 2)
    q = wide[..., :64].view(1, 5, 2, 32).permute(0, 2, 1, 3)
    assert q.stride() == (5 * 66, 32, 66, 1) and q.data_ptr() % 16 == 0
    assert launch(ref, dev, q, k, v, None) is None
    assert launch(ref, dev, q.contiguous(), k, v, None) is not None

"""ops.attention_fake_quant (osq_attention_fake_quant, csrc/attention_block.hip): an attention block over a whole sequence in
one launch, against the float64 restatement of tests/_attention_block.py under the rule the eager CPU sequence is held to in
tests/test_oracle_attention_block.py: entries the helper calls sure are word-equal to ``(code - zp) * scale``, the others at
most one quantization step off, at most 10 % of an output unsure; the context is restated from the kernel's own
``probs_out`` words.  ``out`` and ``probs_out`` hold a sentinel before the launch and none after.

The shapes are tiny: what can go wrong sits at the tile edges.  A workgroup serves TQ = 32 query rows, a score tile has
TK = 32 key columns, and the kernel comes in four classes of S (128 / 256 / 512 / 1024 floats per score row): T runs over 1,
TQ - 1, TQ, TQ + 1, 2 TQ + 3 and S over 1, 3, TK - 1, TK, TK + 1, 2 TK + 5, 1024 at every head size; the classes in between
are met by the row-independence and stride checks."""
import numpy as np
import pytest
import torch

import _attention_block as AB
from conftest import same_f32

pytestmark = pytest.mark.gpu

SENTINEL = -777.25


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def quant(g, dev):
    """(scale, zero_point, quant_min, quant_max, mode, grad_factor) of a QuantGroup with its RAW parameters, or None."""
    from outlier_suppression_amd import ops
    if g is None:
        return None
    scale = torch.tensor([g.scale_raw], dtype=torch.float32, device=dev)
    if g.mode == "lsqplus":
        return (scale, torch.tensor([g.zp_raw], dtype=torch.float32, device=dev), g.qmin, g.qmax,
                ops.PARAM_LSQPLUS | ops.PARAM_SANITIZE, g.grad_factor)
    return (scale, torch.tensor([int(g.zp_raw)], dtype=torch.int32, device=dev), g.qmin, g.qmax, ops.PARAM_FIXED, 1.0)


def check_repaired(g, qt):
    """OSQ_PARAM_SANITIZE leaves the repaired values in the parameters (fake_quant.py:188-191)."""
    if g is not None:
        assert np.float32(qt[0].item()) == g.scale_after and np.float32(qt[1].item()) == g.zp_after


def tensors(ref, dev):
    q, k, v = (torch.from_numpy(ref[n]).to(dev) for n in "qkv")
    return q, k, v, None if ref["mask"] is None else torch.from_numpy(ref["mask"]).to(dev)


def launch(ref, dev, q, k, v, mask, quants=None):
    """One call on sentinel-filled outputs.  Returns (out, probs) as numpy, or None when the op refused."""
    from outlier_suppression_amd import ops
    b, h, t, d = q.shape
    s = k.shape[2]
    out = torch.full((b, t, h * d), SENTINEL, dtype=torch.float32, device=dev)
    probs = torch.full((b, h, t, s), SENTINEL, dtype=torch.float32, device=dev)
    pq, cq = quants if quants is not None else (quant(ref["probs_q"], dev), quant(ref["ctx_q"], dev))
    got = ops.attention_fake_quant(q, k, v, mask, pq, cq, alpha=ref["alpha"], divisor=ref["divisor"], out=out, probs_out=probs)
    torch.cuda.synchronize()
    if got is None:
        assert (out == SENTINEL).all() and (probs == SENTINEL).all()
        return None
    assert got[0] is out and got[1] is probs
    if quants is None:
        check_repaired(ref["probs_q"], pq)
        check_repaired(ref["ctx_q"], cq)
    return out.cpu().numpy(), probs.cpu().numpy()


def test_tiles_are_the_kernels(dev):
    from outlier_suppression_amd import ops
    assert (ops.ATTENTION_TQ, ops.ATTENTION_TK, ops.ATTENTION_MAX_KV) == (AB.TQ, AB.TK, max(AB.KV_LENS))
    assert ops.ATTENTION_HEAD_DIMS == AB.HEAD_DIMS


@pytest.mark.parametrize("head_dim", AB.HEAD_DIMS)
def test_table_against_float64(dev, head_dim):
    worst = [0.0, 0.0]
    for case in AB.table(head_dim):
        ref = AB.reference(case)
        got = launch(ref, dev, *tensors(ref, dev))
        assert got is not None, case
        out, probs = got
        assert not (probs == SENTINEL).any() and not (out == SENTINEL).any(), case
        ctx = AB.expect_context(ref, probs)
        for name, expect, words in (("probs", ref["probs"], probs), ("ctx", ctx, out)):
            assert expect.mismatch(words) is None, (case, ref["seed"], name, expect.mismatch(words))
        worst = [max(worst[0], ref["probs"].share), max(worst[1], ctx.share)]
    print(f"head_dim {head_dim}: {len(AB.table(head_dim))} cases, largest unsure share probs {worst[0]:.4f} ctx {worst[1]:.4f}")


def _row_cases():
    """Two query tiles and a ragged third, S in three of the kernel's four classes, every head size, all three masks."""
    return [AB.Case(d, 2 * AB.TQ + 3, s, 2, 3, bits, mode, False, mask, pre, "both")
            for (d, s, mask, pre), (bits, mode) in zip(((16, 69, "causal", "alpha"), (32, 200, "pad", "divisor"),
                                                        (64, 300, "causal", "none"), (128, 33, "none", "alpha")), AB.QUANTS)]


@pytest.mark.parametrize("case", _row_cases(), ids=lambda c: f"{c.head_dim}-{c.kv_len}")
def test_every_row_is_the_row_launched_alone(dev, case):
    """out and probs_out of the full launch are word-equal, row by row, to launches on q[:, :, t:t+1] with that row of the
    mask and the same explicit parameters: the first and the last row of every tile included."""
    ref = AB.evaluate(case, AB.first_seed(case))
    q, k, v, mask = tensors(ref, dev)
    pg, cg = ref["probs_q"], ref["ctx_q"]

    def repaired():          # explicit effective parameters: grad factors are those of the full launch
        return quant(pg, dev), quant(cg, dev)
    out, probs = launch(ref, dev, q, k, v, mask, repaired())
    for t in range(case.tokens):
        m = None if mask is None else (mask if mask.shape[2] == 1 else mask[:, :, t:t + 1])
        o1, p1 = launch(ref, dev, q[:, :, t:t + 1], k, v, m, repaired())
        assert same_f32(p1[:, :, 0], probs[:, :, t]) and same_f32(o1[:, 0], out[:, t]), (case, t)


def test_strided_inputs_give_the_words_of_the_dense_copies(dev):
    """BERT's permuted views of [B, T, H] tensors, and [:, :, :S] views of cap buffers whose tail beyond S is NaN."""
    case = AB.Case(64, AB.TQ + 1, 2 * AB.TK + 5, 2, 3, "sym8", "lsqplus", False, "pad", "alpha", "both")
    ref = AB.evaluate(case, 11)
    q, k, v, mask = tensors(ref, dev)
    b, h, t, d = q.shape
    s = k.shape[2]
    dense = launch(ref, dev, q, k, v, mask)

    def bert(x):            # the values of x [B, h, n, d] held as [B, n, h * d], handed over as the permuted view
        n = x.shape[2]
        return x.permute(0, 2, 1, 3).contiguous().view(b, n, h * d).view(b, n, h, d).permute(0, 2, 1, 3)
    got = launch(ref, dev, bert(q), bert(k), bert(v), mask)
    assert not bert(q).is_contiguous() and same_f32(got[0], dense[0]) and same_f32(got[1], dense[1])

    def cap(x, extra):
        buf = torch.full((b, h, s + extra, d), float("nan"), dtype=torch.float32, device=dev)
        buf[:, :, :s] = x
        return buf[:, :, :s]
    got = launch(ref, dev, q, cap(k, 7), cap(v, 3), mask)
    assert same_f32(got[0], dense[0]) and same_f32(got[1], dense[1])


def test_special_rows(dev):
    """A fully masked row is uniform; a NaN or a +inf planted in one row makes that row NaN and leaves every other word."""
    case = AB.Case(32, AB.TQ + 1, AB.TK + 1, 2, 3, "asym6", "fixed", False, "causal", "none", "both")
    ref = AB.evaluate(case, 3)
    q, k, v, mask = tensors(ref, dev)
    clean_out, clean_probs = launch(ref, dev, q, k, v, mask)
    b0, h0, t0 = 1, 2, AB.TQ - 1                 # the last row of the first tile
    d = case.head_dim
    # fully masked: finfo.min everywhere in row t0 of batch row b0 (every head of it)
    m = mask.clone()
    m[b0, 0, t0] = AB.FMIN
    out, probs = launch(ref, dev, q, k, v, m)
    g = ref["probs_q"]
    uniform = g.quantize(np.float64(np.float32(1.0) / np.float32(case.kv_len)) / float(g.scale_eff) * np.ones(1))[1][0]
    assert (probs[b0, :, t0] == uniform).all() and uniform != 0
    other = np.ones(probs.shape[:3], bool)
    other[b0, :, t0] = False
    assert same_f32(probs[other], clean_probs[other])
    rows = np.ones(out.shape[:2], bool)
    rows[b0, t0] = False
    assert same_f32(out[rows], clean_out[rows]) and not np.isnan(out).any()
    for poison in (float("nan"), float("inf")):
        q2 = q.clone()
        col = int(torch.argmax(k[b0, h0, 0]))    # a positive element of key 0 (open in every row): +inf * it is +inf
        assert k[b0, h0, 0, col] > 0
        q2[b0, h0, t0, col] = poison
        out, probs = launch(ref, dev, q2, k, v, mask)
        nan_p = np.zeros(probs.shape, bool)
        nan_p[b0, h0, t0] = True
        nan_o = np.zeros(out.shape, bool)
        nan_o[b0, t0, h0 * d:(h0 + 1) * d] = True
        assert (np.isnan(probs) == nan_p).all() and (np.isnan(out) == nan_o).all(), poison
        assert same_f32(probs[~nan_p], clean_probs[~nan_p]) and same_f32(out[~nan_o], clean_out[~nan_o]), poison


def test_refusals_launch_nothing(dev):
    """head_dim 8 / 256, S = 1025, a misaligned view and a non-contiguous last axis: None, outputs untouched."""
    ref = dict(alpha=None, divisor=None, probs_q=None, ctx_q=None)

    def randn(*shape):
        return torch.randn(*shape, device=dev)
    for d in (8, 256):
        assert launch(ref, dev, randn(1, 2, 5, d), randn(1, 2, 7, d), randn(1, 2, 7, d), None) is None
    assert launch(ref, dev, randn(1, 1, 3, 16), randn(1, 1, 1025, 16), randn(1, 1, 1025, 16), None) is None
    q, k, v = randn(1, 2, 5, 32), randn(1, 2, 7, 32), randn(1, 2, 7, 32)
    assert launch(ref, dev, q, k, v, None) is not None
    off = torch.randn(2 * 7 * 32 + 1, device=dev)[1:].view(1, 2, 7, 32)              # four bytes past a 16-byte boundary
    assert off.data_ptr() % 16 == 4 and launch(ref, dev, q, off, v, None) is None
    odd = torch.randn(1, 2, 7, 34, device=dev)[..., :32]                              # rows 34 floats apart
    assert launch(ref, dev, q, k, odd, None) is None
    wide = torch.randn(1, 2, 7, 64, device=dev)[..., ::2]                             # last axis not contiguous
    assert wide.shape[-1] == 32 and launch(ref, dev, q, wide, v, None) is None
    from outlier_suppression_amd import ops
    with pytest.raises(ValueError):
        ops.attention_fake_quant(q, k, v, None, None, None, alpha=0.5, divisor=2.0)


def test_capture_and_replay(dev):
    """One torch.cuda.graph capture of the launch, replayed twice: the words of the direct call."""
    from outlier_suppression_amd import ops
    case = AB.Case(64, AB.TQ + 1, 2 * AB.TK + 5, 2, 3, "asym6", "lsqplus", True, "causal", "none", "both")
    ref = AB.evaluate(case, 5)
    q, k, v, mask = tensors(ref, dev)
    direct = launch(ref, dev, q, k, v, mask)
    pq, cq = quant(ref["probs_q"], dev), quant(ref["ctx_q"], dev)
    out = torch.full((case.batch, case.tokens, case.heads * case.head_dim), SENTINEL, dtype=torch.float32, device=dev)
    probs = torch.full((case.batch, case.heads, case.tokens, case.kv_len), SENTINEL, dtype=torch.float32, device=dev)
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            assert ops.attention_fake_quant(q, k, v, mask, pq, cq, out=out, probs_out=probs) is not None
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        out.fill_(SENTINEL)
        probs.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        assert same_f32(out.cpu().numpy(), direct[0]) and same_f32(probs.cpu().numpy(), direct[1])

"""ops.attention_int_fake_quant (osq_attention_fake_quant_int, csrc/attention_int.hip): whole-sequence attention on the
quantizers' integer codes, both products on the bf16 matrix instruction.

(a) the probabilities against float64 under the rule of tests/_attention_int.py -- word-equal where sure, one step
elsewhere, the bound that of the rule; (b) the context WORD-EQUAL, no tolerance, to the int64 restatement applied to the
kernel's own probs_out and v; (c) the launch without probs_out; (d) every quantizer variant; (e) the saturated cases, which
are the measurement that the matrix instruction returns the exact integer; (f) masks and pre-scaling; (g) non-finite
inputs; (h) strided views; (i) row independence; (j) determinism; (k) a bad zero point; (l) refusals; (m) capture.

Every launch of the table reads q / k / v from buffers that hold NaN beyond T / S and writes into sentinel-filled outputs
with canaries behind them."""
import numpy as np
import pytest
import torch

import _attention_int as AI
from _attention_int import F32
from conftest import same_f32

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
CANARY = 12345.5
TAIL = 64


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


def padded(x, dev, extra=3):
    """x [B, h, n, d] as the [:, :, :n] view of a buffer whose rows beyond n are NaN."""
    x = torch.as_tensor(x)
    b, h, n, d = x.shape
    buf = torch.full((b, h, n + extra, d), float("nan"), dtype=torch.float32, device=dev)
    buf[:, :, :n] = x.to(dev)
    return buf[:, :, :n]


def tensors(ref, dev):
    q, k, v = (padded(ref[n], dev) for n in "qkv")
    return q, k, v, None if ref["mask"] is None else torch.from_numpy(ref["mask"]).to(dev)


def _with_canary(shape, dev):
    n = int(np.prod(shape))
    buf = torch.full((n + TAIL,), SENTINEL, dtype=torch.float32, device=dev)
    buf[n:] = CANARY
    return buf, buf[:n].view(shape)


def launch(ref, dev, q, k, v, mask, quants=None, want_probs=True):
    """One call on sentinel-filled outputs with canaries behind them.  (out, probs) as numpy -- probs None without
    ``want_probs`` -- or None when the op refused (the sentinels are then untouched)."""
    from outlier_suppression_amd import ops
    b, h, t, d = q.shape
    s = k.shape[2]
    obuf, out = _with_canary((b, t, h * d), dev)
    pbuf, probs = _with_canary((b, h, t, s), dev)
    groups = ref["groups"]
    qs = quants if quants is not None else [quant(g, dev) for g in groups]
    got = ops.attention_int_fake_quant(q, k, v, mask, *qs, alpha=ref["alpha"], divisor=ref["divisor"], out=out,
                                       probs_out=probs if want_probs else None)
    torch.cuda.synchronize()
    assert (obuf[out.numel():] == CANARY).all() and (pbuf[probs.numel():] == CANARY).all()
    if got is None:
        assert (out == SENTINEL).all() and (probs == SENTINEL).all()
        return None
    if want_probs:
        assert got[0] is out and got[1] is probs
    else:
        assert got is out and (probs == SENTINEL).all()
    if quants is None:
        for g, qt in zip(groups, qs):              # OSQ_PARAM_SANITIZE leaves the repaired values in the parameters
            if g is not None:
                assert F32(qt[0].item()) == g.scale_after and F32(qt[1].item()) == g.zp_after
    return out.cpu().numpy(), probs.cpu().numpy() if want_probs else None


def restated(ref, probs, v=None):
    qg, kg, vg, pq, cq = ref["groups"]
    return AI.context_words(probs, ref["v"] if v is None else v, pq, vg, cq)


def check(ref, out, probs):
    """(a) and (b) for one launch."""
    case = ref["case"]
    assert not (probs == SENTINEL).any() and not (out == SENTINEL).any(), case
    bad = ref["probs"].mismatch(probs)
    assert bad is None, (case, ref["seed"], bad)
    want = restated(ref, probs)
    assert same_f32(out, want), (case, ref["seed"], int((out.view(np.uint32) != want.view(np.uint32)).sum()))


def test_constants_are_the_kernels(dev):
    from outlier_suppression_amd import ops
    assert (ops.ATTENTION_INT_TQ, ops.ATTENTION_INT_TK, ops.ATTENTION_INT_CHUNK, ops.ATTENTION_INT_MAX_KV) == \
        (AI.TQ, AI.TK, AI.CHUNK, AI.MAX_KV)
    assert ops.ATTENTION_HEAD_DIMS == AI.HEAD_DIMS and ops.ATTENTION_INT_MAX_RANGE == 255


@pytest.mark.parametrize("head_dim", AI.HEAD_DIMS)
def test_table(dev, head_dim):
    """(a), (b), (c), (d), (f) over the table; (j) on every fifth case."""
    worst = [0.0, 0.0]
    cases = AI.table(head_dim)
    for i, case in enumerate(cases):
        ref = AI.reference(case)
        args = tensors(ref, dev)
        got = launch(ref, dev, *args)
        assert got is not None, case
        out, probs = got
        check(ref, out, probs)
        alone = launch(ref, dev, *args, want_probs=False)
        assert alone is not None and same_f32(alone[0], out), case
        if i % 5 == 0:
            again = launch(ref, dev, *args)
            assert same_f32(again[0], out) and same_f32(again[1], probs), case
        worst = [max(worst[0], ref["probs"].share), max(worst[1], ref["probs"].worst)]
    print(f"\nhead_dim {head_dim}: {len(cases)} cases, probabilities: largest unsure share {worst[0]:.5f}, largest 4 g among "
          f"the unsure {worst[1]:.4f}; context word-equal everywhere")


def _asym8(scale, zp, numel):
    return AI.group("asym8", "fixed", scale, zp, numel)


SAT_N = 128 * 255 * 255            # 8 323 200: head_dim 128, every product at its largest


def _saturated_scores(s):
    """q all at code 255 and four kinds of key row, scales 1, head_dim 128, with a mask bias that makes every EXACT score
    the same number: all 255 (N = SAT_N, bias 0); one element 254 (SAT_N - 255, bias 255); one element 253 (SAT_N - 510,
    bias 510); all 0 (N = 0, bias SAT_N -- a score that owes nothing to the instruction, so an error common to all the large
    sums shows as well).  Every term is an integer below 2**24: x = float(N) * 1 + bias = SAT_N exactly, e = 1, the sum is S,
    p = 1 * (1 / S).  If the instruction returned any N off by one, that score would differ by 1 and its e by a factor e."""
    k = np.full((1, 2, s, 128), 255.0, F32)
    bias = np.zeros((1, 1, 1, s), F32)
    for kind, (code, add) in enumerate(((255.0, 0.0), (254.0, 255.0), (253.0, 510.0))):
        k[:, :, kind::4, (kind * 37) % 128] = code
        bias[..., kind::4] = add
    k[:, :, 3::4] = 0.0
    bias[..., 3::4] = float(SAT_N)
    return k, bias


@pytest.mark.parametrize("which", ("scores", "context"))
def test_e_saturated(dev, which):
    """The measurement that the bf16 matrix instruction returns the exact integer; NO context quantizer, so that ``out`` is
    ``float(C) * (s_p * s_v)`` and is compared word for word with the int64 value.

    scores: _saturated_scores -- the probabilities are uniform only if every N the kernel got is the exact integer (the
    test first shows in numpy that N off by one in a single entry moves that entry's code).
    context: a probabilities scale so small that every code is 255, v at 255 and 254 steps in a pattern that differs from
    element to element, S = 1025: every C is above 2**24 and most are odd, so float(C) rounds; a lost low bit, a dropped
    chunk or a chunk summed in fp32 beyond 2**24 changes the word."""
    d, t, b, h = 128, 33, 1, 2
    s = 1025 if which == "context" else 257
    one = F32(1.0)
    p = one * (one / F32(s))
    if which == "scores":
        q = np.full((b, h, t, d), 255.0, F32)
        k, mask = _saturated_scores(s)
        v = (np.arange(b * h * s * d).reshape(b, h, s, d) * 7 % 256).astype(F32)
        sq = sk = sv = one
        sp = F32(p / 100.3)
    else:
        q = np.zeros((b, h, t, d), F32)
        sq, sk, sv, sp = F32(0.004), F32(0.003), F32(0.01), F32(1e-6)
        k = np.full((b, h, s, d), F32(255) * sk, F32)
        codes = 255.0 - ((np.arange(s)[:, None] * 7 + np.arange(d)[None, :]) % 3 == 0)
        v = np.broadcast_to((codes.astype(F32) * sv).astype(F32), (b, h, s, d)).copy()
        mask = None
    groups = (_asym8(sq, 0, q.size), _asym8(sk, 0, k.size), _asym8(sv, 0, v.size), _asym8(sp, 0, b * h * t * s), None)
    ref = dict(q=q, k=k, v=v, mask=mask, alpha=None, divisor=None, groups=groups)
    n_p = float(AI.codes(np.full(1, p, F32), groups[3])[0])
    assert n_p == (255 if which == "context" else 100)
    if which == "scores":
        n = AI.scores_int(q, k, groups[0], groups[1])[0]
        assert sorted(set(n.ravel().tolist())) == [0, SAT_N - 510, SAT_N - 255, SAT_N]
        assert ((n.astype(F32) + mask).astype(F32) == F32(SAT_N)).all()
        for off in (-1.0, 1.0):                # what the test could see: one N off by one moves that entry's code
            x = np.full(s, F32(SAT_N), F32)
            x[5] += F32(off)
            e = np.exp((x - x.max()).astype(F32).astype(np.float64))
            assert AI.codes((e / e.sum()).astype(F32), groups[3])[5] != n_p
    out, probs = launch(ref, dev, *tensors(ref, dev))
    assert (probs == F32(F32(n_p) * sp)).all(), np.unique(probs)[:8]
    c_int = np.matmul(np.full((b, h, t, s), n_p), AI.codes(v, groups[2]).astype(np.float64)).astype(np.int64)
    if which == "context":
        assert c_int.min() > 2 ** 24 and (c_int % 2 == 1).any() and len(np.unique(c_int)) > 1
    want = AI.merged((c_int.astype(F32) * F32(sp * sv)).astype(F32))
    assert same_f32(out, want) and same_f32(out, restated(ref, probs)), int((out != want).sum())


def _small(dev, seed=3, **kw):
    case = AI.Case(32, 33, 67, 2, 3, AI.QUANTS[0], "causal", "none", True)._replace(**kw)
    return AI.evaluate(case, seed)


def test_f_closed_and_nan_mask_rows(dev):
    ref = _small(dev)
    q, k, v, mask = tensors(ref, dev)
    clean_out, clean_probs = launch(ref, dev, q, k, v, mask)
    b0, t0, d = 1, 31, 32
    for poison, where in ((float("-inf"), slice(None)), (float("nan"), slice(5, 6))):
        m = mask.clone()
        m[b0, 0, t0, where] = poison
        out, probs = launch(ref, dev, q, k, v, m)
        nan_p = np.zeros(probs.shape, bool)
        nan_p[b0, :, t0] = True
        nan_o = np.zeros(out.shape, bool)
        nan_o[b0, t0] = True
        assert (np.isnan(probs) == nan_p).all() and (np.isnan(out) == nan_o).all(), poison
        assert same_f32(probs[~nan_p], clean_probs[~nan_p]) and same_f32(out[~nan_o], clean_out[~nan_o]), poison


@pytest.mark.parametrize("poison", (float("nan"), float("inf"), float("-inf")))
def test_g_nonfinite_inputs(dev, poison):
    """In q: that query row of that head.  In k: every row of that (batch row, head).  In v: that element of that head, in
    every row (0 * NaN is NaN in the eager sequence as well); the probabilities keep their words."""
    ref = _small(dev, mask="pad")
    q, k, v, mask = tensors(ref, dev)
    clean_out, clean_probs = launch(ref, dev, q, k, v, mask)
    b0, h0, t0, j0, i0, d = 1, 2, 32, 40, 7, 32
    for name in "qkv":
        x = dict(q=q, k=k, v=v)
        x[name] = x[name].clone()
        x[name][b0, h0, t0 if name == "q" else j0, i0] = poison
        out, probs = launch(ref, dev, x["q"], x["k"], x["v"], mask)
        nan_p, nan_o = np.zeros(probs.shape, bool), np.zeros(out.shape, bool)
        if name == "q":
            nan_p[b0, h0, t0] = True
            nan_o[b0, t0, h0 * d:(h0 + 1) * d] = True
        elif name == "k":
            nan_p[b0, h0] = True
            nan_o[b0, :, h0 * d:(h0 + 1) * d] = True
        else:
            nan_o[b0, :, h0 * d + i0] = True
        assert (np.isnan(probs) == nan_p).all() and (np.isnan(out) == nan_o).all(), (name, poison)
        assert same_f32(probs[~nan_p], clean_probs[~nan_p]) and same_f32(out[~nan_o], clean_out[~nan_o]), (name, poison)


def test_h_strided_views(dev):
    """BERT's permuted views of [B, T, H] memory, and [:, :, :S] views of a [B, h, cap, d] buffer."""
    ref = _small(dev, head_dim=64, kv_len=161, mask="pad", pre="alpha")
    b, h, d = 2, 3, 64
    q, k, v = (torch.from_numpy(ref[n]).to(dev) for n in "qkv")
    mask = torch.from_numpy(ref["mask"]).to(dev)
    dense = launch(ref, dev, q, k, v, mask)
    check(ref, *dense)

    def bert(x):
        n = x.shape[2]
        return x.permute(0, 2, 1, 3).contiguous().view(b, n, h * d).view(b, n, h, d).permute(0, 2, 1, 3)
    got = launch(ref, dev, bert(q), bert(k), bert(v), mask)
    assert not bert(q).is_contiguous() and same_f32(got[0], dense[0]) and same_f32(got[1], dense[1])
    got = launch(ref, dev, q, padded(k, dev, 7), padded(v, dev, 40), mask)
    assert same_f32(got[0], dense[0]) and same_f32(got[1], dense[1])


@pytest.mark.parametrize("head_dim,kv_len", ((16, 129), (128, 300)))
def test_i_every_row_is_the_row_launched_alone(dev, head_dim, kv_len):
    ref = AI.evaluate(AI.Case(head_dim, 67, kv_len, 2, 3, AI.QUANTS[5], "causal", "divisor", True), 9)
    q, k, v, mask = tensors(ref, dev)

    def fresh():             # explicit raw parameters with the grad factors of the full launch
        return [quant(g, dev) for g in ref["groups"]]
    out, probs = launch(ref, dev, q, k, v, mask, fresh())
    for t in range(67):
        o1, p1 = launch(ref, dev, q[:, :, t:t + 1], k, v, mask[:, :, t:t + 1], fresh())
        assert same_f32(p1[:, :, 0], probs[:, :, t]) and same_f32(o1[:, 0], out[:, t]), t


def test_k_bad_zero_point_is_nan_everywhere(dev):
    """A zero point outside the range in FIXED mode is not repaired: |n| could exceed 255, the whole output is NaN."""
    from outlier_suppression_amd import ops
    ref = _small(dev)
    args = tensors(ref, dev)
    for site in range(4):
        qs = [quant(g, dev) for g in ref["groups"]]
        assert qs[site][4] == ops.PARAM_FIXED
        qs[site][1].fill_(ref["groups"][site].qmax + 1)
        out, probs = launch(ref, dev, *args, quants=qs)
        assert np.isnan(out).all() and np.isnan(probs).all(), site
        out, _ = launch(ref, dev, *args, quants=qs, want_probs=False)
        assert np.isnan(out).all(), site


def test_l_refusals_launch_nothing(dev):
    from outlier_suppression_amd import ops
    ref = _small(dev)
    q, k, v, mask = tensors(ref, dev)

    def qs():
        return [quant(g, dev) for g in ref["groups"]]
    assert launch(ref, dev, q, k, v, mask, qs()) is not None
    for site in range(4):                                                    # 257 codes
        wide = qs()
        wide[site] = wide[site][:2] + (0, 256) + wide[site][4:]
        assert launch(ref, dev, q, k, v, mask, wide) is None, site
        missing = qs()
        missing[site] = None
        assert launch(ref, dev, q, k, v, mask, missing) is None, site
        channels = qs()                                                      # per-channel parameters
        channels[site] = (channels[site][0].repeat(32), channels[site][1].repeat(32)) + channels[site][2:]
        assert launch(ref, dev, q, k, v, mask, channels) is None, site

    def randn(*shape):
        return torch.randn(*shape, device=dev)
    plain = dict(ref, alpha=None, divisor=None)
    assert launch(plain, dev, randn(1, 2, 5, 24), randn(1, 2, 7, 24), randn(1, 2, 7, 24), None, qs()) is None
    assert launch(plain, dev, randn(1, 1, 2, 16), randn(1, 1, 16385, 16), randn(1, 1, 16385, 16), None, qs()) is None
    assert launch(plain, dev, randn(1, 1, 2, 16), randn(1, 1, 16384, 16), randn(1, 1, 16384, 16), None, qs()) is not None
    off = torch.randn(2 * 3 * 67 * 32 + 1, device=dev)[1:].view(2, 3, 67, 32)        # four bytes past a 16-byte boundary
    assert launch(ref, dev, q, off, v, mask, qs()) is None
    with pytest.raises(ValueError):
        ops.attention_int_fake_quant(q, k, v, None, *qs(), alpha=0.5, divisor=2.0)


def test_m_capture_and_replay(dev):
    from outlier_suppression_amd import ops
    ref = _small(dev, quant=AI.QUANTS[7], head_dim=64, kv_len=129)
    q, k, v, mask = tensors(ref, dev)
    direct = launch(ref, dev, q, k, v, mask)
    check(ref, *direct)
    qs = [quant(g, dev) for g in ref["groups"]]
    out = torch.full((2, 33, 3 * 64), SENTINEL, dtype=torch.float32, device=dev)
    probs = torch.full((2, 3, 33, 129), SENTINEL, dtype=torch.float32, device=dev)
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            assert ops.attention_int_fake_quant(q, k, v, mask, *qs, out=out, probs_out=probs) is not None
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        out.fill_(SENTINEL)
        probs.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        assert same_f32(out.cpu().numpy(), direct[0]) and same_f32(probs.cpu().numpy(), direct[1])

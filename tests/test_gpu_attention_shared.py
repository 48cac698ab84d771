"""ops.attention_fake_quant / ops.attention_int_fake_quant with ``group`` = G (osq_attention_fake_quant_shared,
osq_attention_fake_quant_int_shared; the row map of csrc/attention_seq.h): q [B * G, h, T, d] whose rows b * G .. b * G + G - 1
share row b of k / v [B, h, S, d] and of the mask.

THE COMPARATOR is the unshared op -- which tests/test_gpu_attention_block*.py and tests/test_gpu_attention_int.py hold to
float64 -- on k, v and mask ``repeat_interleave``d G times: out and probs_out are compared as WORDS (same_f32: NaN equals
NaN, -0.0 differs from +0.0), no tolerance.  Batch 2 and heads 3 so that the arithmetic of b, of the decoder row b * G + j
and of the head all matter.  The (G, T) pairs, with a tile of 128 rows in waves of 32 (integer kernel) and of 32 rows (fp32):

    (1, 33)     must equal the unshared op            (2, 1)
    (3, 31)     candidate edges at rows 31 and 62, inside a wave
    (5, 33)     candidate 3 = rows 99 .. 131 straddles the 128 edge
    (6, 62)     edges straddle both tile seams; the last tile has 116 rows
    (2, 129)    T above a tile; the last tile has 2 rows
    (129, 1)    every row another decoder row; the last tile has 1 row

each at kv_len 1, 33, 129 and head sizes 16 and 64; (5, 33, 33) at all four.  Masks: none; [B, 1, 1, S] and [B, 1, T, S] of
finite values with EVERY row different (in b, and in t) plus a closed tail -- a kernel that takes the mask's row by the decoder
row or by the virtual row reads another row's values.  Quantizers: fixed, and LSQ+ with raw parameters that need the repair.
Every output of the grouped launch is sentinel-filled with canaries behind it; every case is launched twice."""
import functools

import numpy as np
import pytest
import torch

import _attention_block as AB
import _attention_int as AI
from _attention_int import F32
from _decode_attention import FMIN
from conftest import same_f32

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
CANARY = 12345.5
TAIL = 64
B, HEADS = 2, 3
PAIRS = ((1, 33), (2, 1), (3, 31), (5, 33), (6, 62), (2, 129), (129, 1))
KV_LENS = (1, 33, 129)
KERNELS = ("int", "fp32")
MASKS = ("none", "pad", "rows")
INT_QUANTS = (AI.QUANTS[0], AI.QUANTS[6], AI.QUANTS[2], AI.QUANTS[7])          # fixed / LSQ+ with bad raw parameters, <= 256 codes
PRES = ("none", "alpha", "divisor")


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


def shapes(head_dim):
    """(G, T, S) of one head size."""
    if head_dim in (16, 64):
        return [(g, t, s) for g, t in PAIRS for s in KV_LENS]
    return [(5, 33, 33)]


def build_mask(kind, rng, t, s):
    if kind == "none":
        return None
    m = (0.5 * rng.standard_normal((B, 1, 1 if kind == "pad" else t, s))).astype(F32)
    for b in range(B):
        keep = s if s < 2 else int(rng.integers(1, s))              # a closed tail per batch row; position 0 stays open
        m[b, ..., keep:] = FMIN
    return m


@functools.lru_cache(maxsize=None)
def instance(kernel, head_dim, g, t, s, i):
    """q [B * G, h, T, d], k / v [B, h, S, d], the mask and the quantizers of case number i, from the seeded generators of
    tests/_attention_int.py / tests/_attention_block.py at batch B * G (k and v: their first B rows).  Computed once per
    process; callers must not modify it."""
    mask, pre = MASKS[i % 3], PRES[(i // 3) % 3]
    seed = 7000 + 13 * i + head_dim
    if kernel == "int":
        case = AI.Case(head_dim, t, s, B * g, HEADS, INT_QUANTS[i % 4], "none", pre, i % 3 != 2)
        ref = AI.evaluate(case, seed)
        groups = list(ref["groups"])
    else:
        bits, mode = AB.QUANTS[i % 4]
        case = AB.Case(head_dim, t, s, B * g, HEADS, bits, mode, mode == "lsqplus" and (i // 4) % 2 == 0, "none", pre,
                       AB.SITES[i % 5])
        ref = AB.evaluate(case, seed)
        groups = [ref["probs_q"], ref["ctx_q"]]
    rng = np.random.default_rng(seed + 1)
    return dict(kernel=kernel, group=g, q=ref["q"], k=np.ascontiguousarray(ref["k"][:B]), v=np.ascontiguousarray(ref["v"][:B]),
                mask=build_mask(mask, rng, t, s), alpha=ref["alpha"], divisor=ref["divisor"], groups=groups,
                what=(kernel, head_dim, g, t, s, mask, pre))


def tensors(inst, dev):
    q, k, v = (torch.from_numpy(inst[n]).to(dev) for n in "qkv")
    return q, k, v, None if inst["mask"] is None else torch.from_numpy(inst["mask"]).to(dev)


def op(inst):
    from outlier_suppression_amd import ops
    return ops.attention_int_fake_quant if inst["kernel"] == "int" else ops.attention_fake_quant


def quants(inst, dev):
    """Fresh RAW parameters: a launch with OSQ_PARAM_SANITIZE repairs them in place."""
    return [quant(g, dev) for g in inst["groups"]]


def _with_canary(shape, dev):
    n = int(np.prod(shape))
    buf = torch.full((n + TAIL,), SENTINEL, dtype=torch.float32, device=dev)
    buf[n:] = CANARY
    return buf, buf[:n].view(shape)


def grouped(inst, dev, q, k, v, mask, qs=None, want_probs=True, group=None):
    """One grouped launch on sentinel-filled outputs with canaries behind them: (out, probs) as numpy -- probs None without
    ``want_probs`` -- or None when the op refused (the sentinels are then untouched)."""
    bq, h, t, d = q.shape
    s = k.shape[2]
    obuf, out = _with_canary((bq, t, h * d), dev)
    pbuf, probs = _with_canary((bq, h, t, s), dev)
    got = op(inst)(q, k, v, mask, *(quants(inst, dev) if qs is None else qs), alpha=inst["alpha"], divisor=inst["divisor"],
                   out=out, probs_out=probs if want_probs else None, group=inst["group"] if group is None else group)
    torch.cuda.synchronize()
    assert (obuf[out.numel():] == CANARY).all() and (pbuf[probs.numel():] == CANARY).all(), inst["what"]
    if got is None:
        assert (out == SENTINEL).all() and (probs == SENTINEL).all()
        return None
    if want_probs:
        assert got[0] is out and got[1] is probs
    else:
        assert got is out and (probs == SENTINEL).all()
    return out.cpu().numpy(), probs.cpu().numpy() if want_probs else None


def unshared(inst, dev, q, k, v, mask, qs=None):
    """THE COMPARATOR: the op without a group on k, v and mask repeated G times along the batch."""
    g = inst["group"]
    k, v = k.repeat_interleave(g, dim=0), v.repeat_interleave(g, dim=0)
    mask = None if mask is None else mask.repeat_interleave(g, dim=0)
    out, probs = op(inst)(q, k, v, mask, *(quants(inst, dev) if qs is None else qs), alpha=inst["alpha"],
                          divisor=inst["divisor"], want_probs=True)
    torch.cuda.synchronize()
    return out.cpu().numpy(), probs.cpu().numpy()


def differing(a, b):
    return int((np.asarray(a).view(np.uint32) != np.asarray(b).view(np.uint32)).sum())


@pytest.mark.parametrize("head_dim", AI.HEAD_DIMS)
@pytest.mark.parametrize("kernel", KERNELS)
def test_words_are_those_of_the_unshared_op_on_repeated_rows(dev, kernel, head_dim):
    for i, (g, t, s) in enumerate(shapes(head_dim)):
        inst = instance(kernel, head_dim, g, t, s, i)
        args = tensors(inst, dev)
        got = grouped(inst, dev, *args)
        assert got is not None, inst["what"]
        out, probs = got
        assert not (out == SENTINEL).any() and not (probs == SENTINEL).any(), inst["what"]
        want_out, want_probs = unshared(inst, dev, *args)
        assert same_f32(probs, want_probs), (inst["what"], differing(probs, want_probs))
        assert same_f32(out, want_out), (inst["what"], differing(out, want_out))
        again = grouped(inst, dev, *args)
        assert same_f32(again[0], out) and same_f32(again[1], probs), inst["what"]
    print(f"\n{kernel} head_dim {head_dim}: {len(shapes(head_dim))} shapes word-equal to the unshared op, twice")


def _seams(kernel, head_dim=64, s=33, i=5):
    """(6, 62): decoder rows cross both tile seams of the integer kernel and most of the fp32 kernel's; a [B, 1, T, S] mask."""
    inst = instance(kernel, head_dim, 6, 62, s, i)
    assert inst["mask"] is not None and inst["mask"].shape[2] == 62
    return inst


@pytest.mark.parametrize("kernel", KERNELS)
def test_group_one_is_the_unshared_op(dev, kernel):
    inst = instance(kernel, 16, 1, 33, 33, 4)
    args = tensors(inst, dev)
    got = grouped(inst, dev, *args)
    plain = op(inst)(*args, *quants(inst, dev), alpha=inst["alpha"], divisor=inst["divisor"], want_probs=True)
    assert same_f32(got[0], plain[0].cpu().numpy()) and same_f32(got[1], plain[1].cpu().numpy())


@pytest.mark.parametrize("kernel", KERNELS)
def test_launch_without_probs_out(dev, kernel):
    inst = _seams(kernel)
    args = tensors(inst, dev)
    out, _ = grouped(inst, dev, *args)
    alone = grouped(inst, dev, *args, want_probs=False)
    assert alone is not None and alone[1] is None and same_f32(alone[0], out)


@pytest.mark.parametrize("kernel", KERNELS)
def test_q_as_a_permuted_strided_view(dev, kernel):
    """q as the [B * G, h, T, d] view of [B * G, T, h, d] memory, inside a wider buffer: strides that are not the dense ones."""
    inst = _seams(kernel)
    q, k, v, mask = tensors(inst, dev)
    dense = grouped(inst, dev, q, k, v, mask)
    bq, h, t, d = q.shape
    buf = torch.full((bq, t + 3, h, d), float("nan"), dtype=torch.float32, device=dev)
    buf[:, :t] = q.permute(0, 2, 1, 3)
    view = buf[:, :t].permute(0, 2, 1, 3)
    assert not view.is_contiguous() and torch.equal(view, q)
    got = grouped(inst, dev, view, k, v, mask)
    assert got is not None and same_f32(got[0], dense[0]) and same_f32(got[1], dense[1])


@pytest.mark.parametrize("kernel", KERNELS)
def test_a_nan_in_one_decoder_row_of_q_stays_in_that_row(dev, kernel):
    inst = _seams(kernel)
    q, k, v, mask = tensors(inst, dev)
    clean_out, clean_probs = grouped(inst, dev, q, k, v, mask)
    g, d = inst["group"], q.shape[3]
    for bd, h0, t0 in ((1 * g + 3, 2, 61), (0 * g + 2, 0, 4)):          # virtual rows 247 (second tile) and 128 (first of a tile)
        x = q.clone()
        x[bd, h0, t0, 7] = float("nan")
        out, probs = grouped(inst, dev, x, k, v, mask)
        nan_p, nan_o = np.zeros(probs.shape, bool), np.zeros(out.shape, bool)
        nan_p[bd, h0, t0] = True
        nan_o[bd, t0, h0 * d:(h0 + 1) * d] = True
        assert (np.isnan(probs) == nan_p).all() and (np.isnan(out) == nan_o).all(), (bd, h0, t0)
        assert same_f32(probs[~nan_p], clean_probs[~nan_p]) and same_f32(out[~nan_o], clean_out[~nan_o]), (bd, h0, t0)
        want = unshared(inst, dev, x, k, v, mask)
        assert same_f32(out, want[0]) and same_f32(probs, want[1])


@pytest.mark.parametrize("g,t,s", ((6, 62, 33), (129, 1, 129), (2, 129, 1)))
def test_int_bad_zero_point_fills_all_of_both_outputs_and_nothing_else(dev, g, t, s):
    """A zero point outside the range in FIXED mode is not repaired: every workgroup writes NaN to ITS rows of both outputs
    through the row map -- all of them, and (the canaries of ``grouped``) nothing beyond."""
    from outlier_suppression_amd import ops
    inst = instance("int", 16, g, t, s, 0)
    args = tensors(inst, dev)
    for site in range(4):
        qs = quants(inst, dev)
        assert qs[site][4] == ops.PARAM_FIXED
        qs[site][1].fill_(inst["groups"][site].qmax + 1)
        out, probs = grouped(inst, dev, *args, qs=qs)
        assert np.isnan(out).all() and np.isnan(probs).all(), site
        out, _ = grouped(inst, dev, *args, qs=qs, want_probs=False)
        assert np.isnan(out).all(), site


@pytest.mark.parametrize("kernel", KERNELS)
def test_capture_and_replay(dev, kernel):
    inst = _seams(kernel, s=129, i=11)
    q, k, v, mask = tensors(inst, dev)
    direct = grouped(inst, dev, q, k, v, mask)
    qs = quants(inst, dev)
    bq, h, t, d = q.shape
    out = torch.full((bq, t, h * d), SENTINEL, dtype=torch.float32, device=dev)
    probs = torch.full((bq, h, t, 129), SENTINEL, dtype=torch.float32, device=dev)
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            assert op(inst)(q, k, v, mask, *qs, alpha=inst["alpha"], divisor=inst["divisor"], out=out, probs_out=probs,
                            group=inst["group"]) is not None
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        out.fill_(SENTINEL)
        probs.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        assert same_f32(out.cpu().numpy(), direct[0]) and same_f32(probs.cpu().numpy(), direct[1])


@pytest.mark.parametrize("kernel", KERNELS)
def test_q_rows_that_are_not_batch_times_group_are_refused(dev, kernel):
    from outlier_suppression_amd import ops
    inst = instance(kernel, 16, 3, 31, 33, 2)
    q, k, v, mask = tensors(inst, dev)
    assert grouped(inst, dev, q, k, v, mask) is not None
    assert grouped(inst, dev, q[:-1], k, v, mask) is None                   # 5 rows for 2 rows of k: no multiple of 3
    assert grouped(inst, dev, q, k, v, mask, group=2) is None               # 6 rows in groups of 2 are 3 rows of k, not 2
    assert grouped(inst, dev, q, k, v, mask, group=6) is None
    assert grouped(inst, dev, q, k[:1], v[:1], None if mask is None else mask[:1]) is None
    assert not ops.attention_fusable(q, k, v, mask, 2) and ops.attention_fusable(q, k, v, mask, 3)
    with pytest.raises(ValueError):
        grouped(inst, dev, q, k, v, mask, group=0)

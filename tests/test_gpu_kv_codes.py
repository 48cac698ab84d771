"""The KV cache as integer codes, through ``ops`` (csrc/kv_codes.hip, csrc/decode_attention.hip).

Append (ops.fake_quant_kv_append_codes): the bytes written equal ``ops.quantize_codes`` of the head-split view, and
dequantised with the record they equal the buffer of the fp32 append (ops.fake_quant_kv_append) word for word; the kept
prefix is copied as bytes, with and without a row index, in place and into a partner buffer; bytes past ``offset + t`` keep a
sentinel; ``rejected`` stays 0.  The copy loop is a plain grid-stride loop (not unrolled) with two widths, so the offsets
are chosen at its own edges: 0 and 1; 4 and 5 (at head size 4 a prefix of whole 16-byte units, and one that is not: the
4-byte path); 67 and 257 (at head size 4 and batch * heads 1, one unit either side of the 256 units of a workgroup); and,
once, a prefix of more units than the largest grid holds (the loop's second trip).

Uncodable input: a NaN, an infinite value and a fractional zero point move ``rejected`` by the exact number of elements
they affect, as do a record mismatch (by 1) and a row index out of range (by the elements of the prefix it stands for), and
attention over such a cache returns NaN only.

Attention (ops.decode_attention_codes): ``out`` and ``probs_out`` word-equal to ops.decode_attention_fake_quant on the
dequantised fp32 K / V -- both kernels see the same on-grid values and add in the same order, so there is no tie filter and
no tolerance.  (The fp32 kernel is itself pinned to float64 by tests/test_gpu_decode_attention.py at every head size, and so is
the coded form, on code bytes whose values numpy forms from the record; this comparison stays as the one that runs on what an
append leaves behind, asym8 records included.)"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

RANGES = {"asym6": (0, 63, 31), "sym8": (-128, 127, 0), "asym8": (0, 255, 128)}
QUANTS = [(bits, mode) for bits in RANGES for mode in ("fixed", "lsqplus")]
HEAD_DIMS = (4, 8, 16, 32, 64, 128, 256)           # attention: every head size the kernel is instantiated for
# append: any multiple of 4.  8 and 12 (two and three words per row) are the sizes at which the 16-byte copy decision --
# (offset * dv) % 4, (cap * dv) % 4 -- depends on the offset and the cap in a way one word and whole units of four do not show
APPEND_HEAD_DIMS = (4, 8, 12, 16, 64, 128)
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


class Params:
    """The raw parameters of one quantizer as a launch takes them; ``fresh()`` a copy (a launch with OSQ_PARAM_SANITIZE
    repairs them in place).  ``bad``: LSQ+ with a negative raw scale and a raw zero point above the range."""

    def __init__(self, bits, mode, scale, numel, dev, bad=False, zero_point=None):
        from outlier_suppression_amd import ops
        self.qmin, self.qmax, zp = RANGES[bits]
        zp = zp if zero_point is None else zero_point
        if mode == "fixed":
            self.scale = torch.tensor([scale], dtype=torch.float32, device=dev)
            self.zp = torch.tensor([zp], dtype=torch.float32 if isinstance(zp, float) else torch.int32, device=dev)
            self.mode, self.base, self.gf = ops.PARAM_FIXED, ops.PARAM_FIXED, 1.0
        else:
            self.scale = torch.tensor([-scale if bad else scale], dtype=torch.float32, device=dev)
            self.zp = torch.tensor([float(self.qmax + 7 if bad else zp)], dtype=torch.float32, device=dev)
            self.mode, self.base = ops.PARAM_LSQPLUS | ops.PARAM_SANITIZE, ops.PARAM_LSQPLUS
            self.gf = 1.0 / math.sqrt(numel * self.qmax)

    def fresh(self):
        return (self.scale.clone(), self.zp.clone(), self.qmin, self.qmax, self.mode, self.gf)


def headsplit(x, heads):
    b, t, w = x.shape
    return x.view(b, t, heads, w // heads).transpose(1, 2).contiguous()


def words(t):
    return t.contiguous().view(torch.int32)


def new_record(dev):
    return (torch.full((1,), float("nan"), device=dev), torch.full((1,), float("nan"), device=dev))


def caps_for(kind, length):
    """(k_cap, v_cap): equal to the length; the length plus 7; different for K and V, K's a multiple of 4."""
    if kind == "eq":
        return length, length
    if kind == "plus7":
        return length + 7, length + 7
    return (length + 4) // 4 * 4, length + 7


# ------------------------------------------------------------------------------------------------ append

def check_append(dev, g, bits, mode, d, b, h, t, offset, cap_kind, src_kind, bad):
    """One launch of a query site and two coded sites against quantize_codes and the fp32 append."""
    from outlier_suppression_amd import ops
    qmin, qmax, _ = RANGES[bits]
    span = qmax - qmin
    caps = caps_for(cap_kind, offset + t)
    xs = [torch.randn(b, t, h * d, generator=g, device=dev) * 2 for _ in range(3)]
    quants = [Params(bits, mode, 0.11, xs[0].numel(), dev), Params(bits, mode, 0.07, xs[1].numel(), dev, bad),
              Params(bits, mode, 0.05, xs[2].numel(), dev, bad)]
    rejected = torch.zeros(1, dtype=torch.int32, device=dev)
    records = [new_record(dev), new_record(dev)]
    rows = None
    ys, srcs, fulls = [], [], []
    for cap in caps:
        y = torch.full((b, h, cap, d), SENTINEL, dtype=torch.uint8, device=dev)
        src = full = None
        if offset and src_kind == "inplace":
            y[:, :, :offset] = torch.randint(0, span + 1, (b, h, offset, d), generator=g, device=dev).to(torch.uint8)
            src = y[:, :, :offset]
        elif offset and src_kind in ("partner", "rows"):
            src_b = b + 1 if src_kind == "rows" else b
            src_cap = offset + (0, 3, 4 - offset % 4)[(offset + t) % 3]
            full = torch.randint(0, span + 1, (src_b, h, src_cap, d), generator=g, device=dev).to(torch.uint8)
            src = full[:, :, :offset]
        ys.append(y)
        srcs.append(src)
        fulls.append(full)
    if offset and src_kind == "rows":
        rows = torch.randint(0, b + 1, (b,), generator=g, device=dev)
    before = [y.clone() for y in ys]
    live = [q.fresh() for q in quants]
    yq = torch.empty(b, h, t, d, device=dev)
    out = ops.fake_quant_kv_append_codes(
        [(xs[0], yq, 0, live[0], None, None, None, False),
         (xs[1], ys[0], offset, live[1], srcs[0], rows, records[0], True),
         (xs[2], ys[1], offset, live[2], srcs[1], rows, records[1], True)], h, rejected)
    assert out is not None and out[1] is ys[0] and out[2] is ys[1]
    # the fp32 append of the same step, its prefix the dequantised source
    ref_live = [q.fresh() for q in quants]
    ref_q = torch.empty(b, h, t, d, device=dev)
    ref_ys, ref_srcs = [], []
    for j, cap in enumerate(caps):
        rec = records[j] + (qmin,)
        y32 = torch.full((b, h, cap, d), float("nan"), device=dev)
        s32 = None
        if srcs[j] is not None:
            if src_kind == "inplace":
                y32[:, :, :offset] = ops.dequantize_kv_codes(before[j], rec)[:, :, :offset]
                s32 = y32[:, :, :offset]
            else:
                s32 = ops.dequantize_kv_codes(fulls[j], rec)[:, :, :offset]
        ref_ys.append(y32)
        ref_srcs.append(s32)
    ref = ops.fake_quant_kv_append([(xs[0], ref_q, 0, ref_live[0], None, None),
                                    (xs[1], ref_ys[0], offset, ref_live[1], ref_srcs[0], rows),
                                    (xs[2], ref_ys[1], offset, ref_live[2], ref_srcs[1], rows)], h)
    assert ref is not None
    assert torch.equal(words(yq), words(ref_q))
    for j in range(2):
        y, cap, quant, rec = ys[j], caps[j], quants[j + 1], records[j]
        what = (bits, mode, d, b, h, t, offset, cap_kind, src_kind, "kv"[j])
        # the step's bytes: quantize_codes of the head-split view with the (now repaired) parameters
        want = ops.quantize_codes(headsplit(xs[j + 1], h), live[j + 1][0], live[j + 1][1], -1, qmin, qmax, quant.base, quant.gf,
                                  code_bits=8)
        assert torch.equal(y[:, :, offset:offset + t].reshape(-1), want.codes), what
        assert torch.equal(words(rec[0]), words(want.scale)) and torch.equal(words(rec[1]), words(want.zero_point)), what
        # the kept prefix, byte for byte
        if offset:
            if srcs[j] is None:
                assert bool((y[:, :, :offset] == SENTINEL).all()), what
            elif src_kind == "inplace":
                assert torch.equal(y[:, :, :offset], before[j][:, :, :offset]), what
            else:
                kept = srcs[j] if rows is None else srcs[j].index_select(0, rows)
                assert torch.equal(y[:, :, :offset], kept), what
        assert bool((y[:, :, offset + t:] == SENTINEL).all()), what
        # dequantised with the record: the fp32 append's buffer, word for word
        if offset == 0 or srcs[j] is not None:
            got = ops.dequantize_kv_codes(y, rec + (qmin,))
            assert got.shape == (b, h, cap, d) and got.is_contiguous()
            assert torch.equal(words(got[:, :, :offset + t]), words(ref_ys[j][:, :, :offset + t])), what
    # the repaired parameters were written back as by the fp32 launch
    for a, r in zip(live, ref_live):
        assert torch.equal(a[0], r[0]) and torch.equal(a[1], r[1])
    assert int(rejected.item()) == 0


@pytest.mark.parametrize("d", APPEND_HEAD_DIMS)
@pytest.mark.parametrize("bits, mode", QUANTS)
def test_append(dev, bits, mode, d):
    g = torch.Generator(device=dev).manual_seed(1000 + d)
    i = 0
    for b, h in ((1, 1), (2, 3)):
        for t in (1, 3):
            for offset in (0, 1, 4, 5, 67, 257):
                for src_kind in ("partner", "rows", "inplace", "none"):
                    if offset == 0 and src_kind != "none":
                        continue
                    cap_kind = ("eq", "plus7", "differ")[i % 3]
                    check_append(dev, g, bits, mode, d, b, h, t, offset, cap_kind, src_kind, bad=(mode == "lsqplus" and i % 2 == 1))
                    i += 1


def test_append_prefix_longer_than_the_grid(dev):
    """2 x 3 heads x 11000 positions x 128: 528000 copy units of 16 bytes, more than 2048 workgroups of 256 hold."""
    g = torch.Generator(device=dev).manual_seed(5)
    check_append(dev, g, "asym6", "lsqplus", 128, 2, 3, 1, 11000, "plus7", "rows", bad=True)


def test_append_layouts_not_taken(dev):
    from outlier_suppression_amd import ops
    p = Params("asym6", "fixed", 0.1, 1, dev)
    rejected = torch.zeros(1, dtype=torch.int32, device=dev)
    x = torch.randn(2, 1, 3 * 6, device=dev)
    y = torch.zeros(2, 3, 4, 6, dtype=torch.uint8, device=dev)
    assert ops.fake_quant_kv_append_codes([(x, y, 0, p.fresh(), None, None, new_record(dev), True)], 3, rejected) is None  # d % 4
    x = torch.randn(2, 1, 3 * 8, device=dev)
    y = torch.zeros(2, 3, 4, 8, dtype=torch.uint8, device=dev)
    rows = torch.tensor([1, 0], device=dev)
    site = (x, y, 2, p.fresh(), y[:, :, :2], rows, new_record(dev), True)          # src == y with a row index
    assert ops.fake_quant_kv_append_codes([site], 3, rejected) is None
    assert int(y.sum().item()) == 0 and int(rejected.item()) == 0
    with pytest.raises(TypeError):
        ops.fake_quant_kv_append_codes([(x, y.float(), 0, p.fresh(), None, None, new_record(dev), True)], 3, rejected)
    wide = Params("asym8", "fixed", 0.1, 1, dev)
    wide.qmax = 256
    with pytest.raises(ValueError):
        ops.fake_quant_kv_append_codes([(x, y, 0, wide.fresh(), None, None, new_record(dev), True)], 3, rejected)


# ------------------------------------------------------------------------------------------------ uncodable input

def attention_over(dev, yk, yv, rk, rv, qmin, rejected, s):
    from outlier_suppression_amd import ops
    b, h, _, d = yk.shape
    q = torch.randn(b, h, 1, d, device=dev)
    probs_q = Params("asym6", "fixed", 1 / 63, 1, dev, zero_point=0)
    return ops.decode_attention_codes(q, yk[:, :, :s], yv[:, :, :s], None, probs_q.fresh(), None, rk + (qmin,), rv + (qmin,),
                                      rejected, want_probs=True)


def coded_step(dev, x, p_k, p_v, h, cap, rejected, records, write=True, offset=0, ys=None, src=None, rows=None):
    from outlier_suppression_amd import ops
    b, t, w = x.shape
    d = w // h
    ys = ys or [torch.zeros(b, h, cap, d, dtype=torch.uint8, device=dev) for _ in range(2)]
    srcs = src or [None, None]
    out = ops.fake_quant_kv_append_codes([(x, ys[0], offset, p_k, srcs[0], rows, records[0], write),
                                          (x, ys[1], offset, p_v, srcs[1], rows, records[1], write)], h, rejected)
    assert out is not None
    return ys


@pytest.mark.parametrize("kind", ["nan", "inf", "fractional_zero_point", "record_mismatch", "bad_row"])
def test_uncodable_input_moves_rejected_and_attention_returns_nan(dev, kind):
    b, h, d, t = 2, 3, 16, 5
    g = torch.Generator(device=dev).manual_seed(11)
    x = torch.randn(b, t, h * d, generator=g, device=dev)
    good = Params("asym6", "fixed", 0.1, 1, dev)
    rejected = torch.zeros(1, dtype=torch.int32, device=dev)
    records = [new_record(dev), new_record(dev)]
    s = t
    if kind in ("nan", "inf"):
        x[1, 2, 7] = float(kind)
        x[0, 4, 40] = float(kind)
        ys = coded_step(dev, x, good.fresh(), good.fresh(), h, t + 3, rejected, records)
        expect = 2 * 2                                           # two elements, in K and in V
        assert int(ys[0][1, 0, 2, 7]) == 0 and int(ys[0][0, 2, 4, 8]) == 0      # code 0 is written for them
    elif kind == "fractional_zero_point":
        frac = Params("asym6", "fixed", 0.1, 1, dev, zero_point=2.5)
        ys = coded_step(dev, x, frac.fresh(), good.fresh(), h, t + 3, rejected, records)
        u = (x / frac.scale).cpu()
        x_quant = torch.clamp(torch.round(u) + 2.5, 0, 63)       # an element the clamp moves onto a bound has a code
        expect = int((x_quant != torch.round(x_quant)).sum())
        assert 0 < expect < x.numel()
    elif kind == "record_mismatch":
        ys = coded_step(dev, x[:, :3].contiguous(), good.fresh(), good.fresh(), h, t + 3, rejected, records)
        assert int(rejected.item()) == 0
        assert not bool(torch.isnan(attention_over(dev, ys[0], ys[1], records[0], records[1], 0, rejected, 3)[0]).any())
        other = Params("asym6", "fixed", 0.2, 1, dev)            # the parameters were rewritten behind the cache's back
        coded_step(dev, x[:, 3:].contiguous(), other.fresh(), good.fresh(), h, t + 3, rejected, records, write=False, offset=3,
                   ys=ys)
        expect = 1
    else:
        ys0 = coded_step(dev, x[:, :3].contiguous(), good.fresh(), good.fresh(), h, 3, rejected, records)
        rows = torch.tensor([0, 2], device=dev)                  # row 2 of a source of two rows
        ys = coded_step(dev, x[:, 3:].contiguous(), good.fresh(), good.fresh(), h, t + 3, rejected, records, write=False,
                        offset=3, src=ys0, rows=rows)
        expect = 2 * h * 3 * d                                   # the prefix of one batch row, in K and in V
        assert int(ys[0][1, :, :3].sum()) == 0 and torch.equal(ys[0][0, :, :3], ys0[0][0])
    assert int(rejected.item()) == expect
    out, probs = attention_over(dev, ys[0], ys[1], records[0], records[1], 0, rejected, s)
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(probs).all())
    assert out.shape == (b, 1, h * d) and probs.shape == (b, h, 1, s)


# ------------------------------------------------------------------------------------------------ attention

def kv_lens(d):
    """1; 3; both sides of one trip of the four waves (4 R positions, R = 64 / (d / 4) rows per wave load); a second trip
    with a ragged tail; one position more than the sixteen trips of loads the coded form keeps in flight plus one wave's
    rows (where that fits below the limit of 4096)."""
    r = 64 // (d // 4)
    return (1, 3, 4 * r - 1, 4 * r, 4 * r + 1, 2 * 4 * r + 5, min(16 * 4 * r + r + 1, 4096))


def build_mask(kind, b, s, g, dev):
    if kind == "none":
        return None
    fmin = torch.finfo(torch.float32).min
    m = torch.zeros(b, 1, 1, s, device=dev)
    for i in range(b):
        keep = s if s < 2 else int(torch.randint(1, s, (1,), generator=g, device=dev))
        m[i, 0, 0, keep:] = fmin
    if kind == "full":
        m[b - 1] = fmin
    return m


def site_quantizer(i, numel, dev):
    """The probabilities / context quantizer of case i: none, fixed 6-bit, LSQ+ 8-bit with a negative raw scale (repaired in
    the launch)."""
    if i % 3 == 0:
        return None
    if i % 3 == 1:
        return Params("asym6", "fixed", 0.02, numel, dev, zero_point=3)
    return Params("sym8", "lsqplus", -0.01, numel, dev)


def check_attention(dev, g, i, bits, mode, d, b, h, s, mask_kind, cap_kind):
    from outlier_suppression_amd import ops
    qmin = RANGES[bits][0]
    caps = caps_for(cap_kind, s)
    rejected = torch.zeros(1, dtype=torch.int32, device=dev)
    records = [new_record(dev), new_record(dev)]
    bufs = []
    for j, cap in enumerate(caps):          # the cache as an append leaves it, garbage behind the length
        x = torch.randn(b, s, h * d, generator=g, device=dev)
        y = torch.randint(0, 256, (b, h, cap, d), generator=g, device=dev).to(torch.uint8)
        p = Params(bits, mode, (0.06, 0.045)[j], x.numel(), dev, bad=(mode == "lsqplus" and i % 2 == 1))
        assert ops.fake_quant_kv_append_codes([(x, y, 0, p.fresh(), None, None, records[j], True)], h, rejected) is not None
        bufs.append(y)
    q = torch.randn(b, h, 1, d, generator=g, device=dev) * (d ** -0.5 * 2)
    mask = build_mask(mask_kind, b, s, g, dev)
    pq, cq = site_quantizer(i, b * h * s, dev), site_quantizer(i + 1, b * h * d, dev)
    fresh = lambda p: None if p is None else p.fresh()  # noqa: E731
    recs = [records[0] + (qmin,), records[1] + (qmin,)]
    k32 = ops.dequantize_kv_codes(bufs[0], recs[0])[:, :, :s]
    v32 = ops.dequantize_kv_codes(bufs[1], recs[1])[:, :, :s]
    want = ops.decode_attention_fake_quant(q, k32, v32, mask, fresh(pq), fresh(cq), want_probs=True)
    assert want is not None
    what = (bits, mode, d, b, h, s, mask_kind, cap_kind)
    for _ in range(2):                       # twice: the same words
        got = ops.decode_attention_codes(q, bufs[0][:, :, :s], bufs[1][:, :, :s], mask, fresh(pq), fresh(cq), recs[0], recs[1],
                                         rejected, want_probs=True)
        assert got is not None, what
        assert torch.equal(words(got[0]), words(want[0])), what
        assert torch.equal(words(got[1]), words(want[1])), what
    assert int(rejected.item()) == 0
    assert not bool(torch.isnan(got[0]).any()) and not bool(torch.isnan(got[1]).any())


@pytest.mark.parametrize("d", HEAD_DIMS)
def test_attention_equals_the_fp32_form_on_dequantised_codes(dev, d):
    g = torch.Generator(device=dev).manual_seed(77 + d)
    i = 0
    for s in kv_lens(d):
        for b, h in ((1, 1), (2, 3)):
            for bits, mode in QUANTS:
                check_attention(dev, g, i, bits, mode, d, b, h, s, ("none", "pad", "full")[i % 3], ("eq", "plus7", "differ")[(i // 3) % 3])
                i += 1


def test_attention_at_the_limit(dev):
    g = torch.Generator(device=dev).manual_seed(3)
    check_attention(dev, g, 1, "asym6", "lsqplus", 16, 1, 1, 4096, "pad", "plus7")


def test_attention_layouts_not_taken(dev):
    from outlier_suppression_amd import ops
    b, h, d = 1, 2, 16
    rejected = torch.zeros(1, dtype=torch.int32, device=dev)
    rec = (torch.tensor([0.1], device=dev), torch.tensor([31.0], device=dev), 0)
    q = torch.randn(b, h, 1, d, device=dev)
    long = torch.zeros(b, h, 4097, d, dtype=torch.uint8, device=dev)
    assert ops.decode_attention_codes(q, long, long, None, None, None, rec, rec, rejected) is None
    assert ops.decode_attention_codes(q, long[:, :, :4096], long[:, :, :4096], None, None, None, rec, rec, rejected) is not None
    flat = torch.zeros(b * h * 8 * d + 1, dtype=torch.uint8, device=dev)
    off = flat[1:].view(b, h, 8, d)                      # one byte off a word
    ok = flat[:-1].view(b, h, 8, d)
    assert ops.decode_attention_codes(q, off, ok, None, None, None, rec, rec, rejected) is None
    assert ops.decode_attention_codes(q, ok, off, None, None, None, rec, rec, rejected) is None
    assert ops.decode_attention_codes(q, ok, ok, None, None, None, rec, rec, rejected) is not None
    assert ops.decode_attention_codes(q, ok.float(), ok, None, None, None, rec, rec, rejected) is None

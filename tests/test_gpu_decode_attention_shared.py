"""osq_decode_attention_shared / osq_decode_attention_shared_codes (csrc/decode_attention.hip): one decoding step's
attention for `group` query rows per batch row that share that row's keys, values and mask -- beam search's cross-attention.

The comparator is the one-query-per-workgroup launch (osq_decode_attention_fake_quant / osq_decode_attention_codes, pinned to
float64 by tests/test_gpu_decode_attention.py) on k, v and mask repeated `group` times along the batch.  The shared kernel
forms and adds every score, denominator and context element in that kernel's order, so ``out`` and ``probs_out`` are compared
as WORDS (torch.equal on the int32 view; NaN-aware where NaN is expected), for fp32 and coded K / V alike.

K and V of batch row b come from the seeded cases of tests/_decode_attention.py; every beam gets a
query of its own.  Masks are built so that batch rows differ: a kernel that indexed the mask by query row would read another
row.  Shapes are tiny; what can go wrong sits in the trip counts (kv_lens of the helper, plus the limit 1024), the chunking of
the group (8 queries per workgroup: 9 leaves a chunk of one, 17 three chunks) and the row arithmetic (batch 2, heads 3).

All seven head sizes the kernel is instantiated for are launched.  At head_dim 256 (LPR 64) the final loop over the
chunk's gn * LPR output words takes a second trip from five queries on: groups 5 and 8 run it, the chunks of one that 9 and
17 leave do not; with kv_len 1024 and a chunk of eight the score rows and the partial vectors that reuse them both fill
the LDS to its limit."""
import functools

import numpy as np
import pytest
import torch

import _decode_attention as DA
from conftest import same_f32

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
GROUPS = (1, 2, 3, 5, 6, 8, 9, 17)
assert {1, 5, 8} <= {g % 8 or 8 for g in GROUPS} and any(g > 8 for g in GROUPS)      # ragged last chunks of 1 and 5, a full one
KINDS = (None, "fixed", "lsqplus_bad")
FMIN = torch.finfo(torch.float32).min


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def words(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _kv(d, s, b, h):
    """K and V of the helper's seeded case of this shape (computed once; not modified)."""
    r = DA.evaluate(DA.Case(d, s, b, h, "asym6", "fixed", False, "none", "eq"), 11 * d + s)
    return r["k"], r["v"]


def _caps(variant, s):
    return {"eq": (s, s), "plus7": (s + 7, s + 7), "differ": (s + 7, s + 3)}[variant]


def _mask(kind, b, s, dev):
    """Rows that differ between batch rows: row i keeps s - 1 - i positions (at least one); "full" masks the last row whole."""
    if kind == "none":
        return None
    m = torch.zeros(b, 1, 1, s, device=dev)
    for i in range(b):
        m[i, 0, 0, max(1, s - 1 - i):] = FMIN
    if kind == "full":
        m[b - 1] = FMIN
    return m


class Quant:
    """One quantizer of the site with fresh device parameters: absent, fixed asymmetric 6-bit, or LSQ+ symmetric 8-bit whose raw
    parameters are bad (negative scale, zero point below the range) and are repaired by the launch (OSQ_PARAM_SANITIZE)."""

    def __init__(self, kind, scale, numel, dev, zero_point=3):
        from outlier_suppression_amd import _hip
        self.kind = kind
        if kind is None:
            self.args = [None, None, _hip.ZP_INT32, _hip.PARAM_FIXED, 1.0, 0, 1]
        elif kind == "fixed":
            self.scale = torch.tensor([scale], dtype=torch.float32, device=dev)
            self.zp = torch.tensor([zero_point], dtype=torch.int32, device=dev)
            self.args = [self.scale.data_ptr(), self.zp.data_ptr(), _hip.ZP_INT32, _hip.PARAM_FIXED, 1.0, 0, 63]
        else:
            self.scale = torch.tensor([-scale], dtype=torch.float32, device=dev)
            self.zp = torch.tensor([-300.0], dtype=torch.float32, device=dev)
            gf = float(np.float32(1.0 / (numel * 127) ** 0.5))
            self.args = [self.scale.data_ptr(), self.zp.data_ptr(), _hip.ZP_FLOAT32, _hip.PARAM_LSQPLUS | _hip.PARAM_SANITIZE,
                         gf, -128, 127]

    def same_params(self, other):
        if self.kind is None:
            return True
        return torch.equal(words(self.scale), words(other.scale)) and torch.equal(self.zp, other.zp)


def _inputs(dev, d, s, b, h, group, mask_kind, cap_kind, codes, seed=0):
    ref = dict(zip("kv", _kv(d, s, b, h)))
    g = torch.Generator(device=dev).manual_seed(1000 * d + 10 * s + group + seed)
    k_cap, v_cap = _caps(cap_kind, s)
    q = torch.randn(b * group, h, 1, d, generator=g, device=dev) * (d ** -0.5 * (1 + 0.3 * np.log2(s)))
    x = dict(q=q, mask=_mask(mask_kind, b, s, dev), group=group, shape=(b, h, d, s), caps=(k_cap, v_cap), records=None)
    if codes:       # 6-bit codes 0..63 in the first s positions, bytes without a code behind them; one record per tensor
        x["k"] = torch.randint(64, 256, (b, h, k_cap, d), generator=g, device=dev).to(torch.uint8)
        x["v"] = torch.randint(64, 256, (b, h, v_cap, d), generator=g, device=dev).to(torch.uint8)
        x["k"][:, :, :s] = torch.randint(0, 64, (b, h, s, d), generator=g, device=dev).to(torch.uint8)
        x["v"][:, :, :s] = torch.randint(0, 64, (b, h, s, d), generator=g, device=dev).to(torch.uint8)
        x["records"] = [(torch.tensor([sc], device=dev), torch.tensor([zp], device=dev), 0) for sc, zp in ((0.06, 31.25), (0.045, 29.5))]
        x["rejected"] = torch.zeros(1, dtype=torch.int32, device=dev)
    else:           # the case's K / V as the first s positions of larger buffers whose tail is NaN
        for name, cap in (("k", k_cap), ("v", v_cap)):
            buf = torch.full((b, h, cap, d), float("nan"), device=dev)
            buf[:, :, :s] = torch.from_numpy(ref[name]).to(dev)
            x[name] = buf
    return x


def _launch(x, dev, shared, pq_kind, cq_kind, want_probs=True, head_dim=None, kv_len=None, group=None, k_offset=0):
    """One call through the C ABI on sentinel-filled outputs: the shared entry point, or the existing one on the repeated
    tensors.  Returns (status, out, probs_out or None, Quant, Quant)."""
    from outlier_suppression_amd import _hip
    lib = _hip.load()
    b, h, d, s = x["shape"]
    grp = x["group"]
    rows = b * grp
    k, v, mask = x["k"], x["v"], x["mask"]
    if not shared:
        k, v = k.repeat_interleave(grp, 0), v.repeat_interleave(grp, 0)
        mask = None if mask is None else mask.repeat_interleave(grp, 0).contiguous()
    out = torch.full((rows, 1, h * d), SENTINEL, dtype=torch.float32, device=dev)
    probs = torch.full((rows, h, 1, s), SENTINEL, dtype=torch.float32, device=dev) if want_probs else None
    pq, cq = Quant(pq_kind, 0.004, rows * h * s, dev), Quant(cq_kind, 0.02, rows * h * d, dev, zero_point=31)
    d_arg, s_arg = d if head_dim is None else head_dim, s if kv_len is None else kv_len
    head = [x["q"].data_ptr(), k.data_ptr() + k_offset, v.data_ptr(), _hip.ptr(mask), out.data_ptr(), _hip.ptr(probs)]
    shape = [b, grp if group is None else group, h, d_arg, s_arg] if shared else [rows, h, d_arg, s_arg]
    recs = []
    if x["records"] is not None:
        for r in x["records"]:
            recs += [r[0].data_ptr(), r[1].data_ptr(), r[2]]
        recs.append(x["rejected"].data_ptr())
        fn = lib.osq_decode_attention_shared_codes if shared else lib.osq_decode_attention_codes
    else:
        fn = lib.osq_decode_attention_shared if shared else lib.osq_decode_attention_fake_quant
    rc = fn(*head, *shape, *x["caps"], *recs, *pq.args, *cq.args, _hip.raw_stream(dev))
    torch.cuda.synchronize()
    return rc, out, probs, pq, cq


def _check(dev, d, s, b, h, group, mask_kind="pad", cap_kind="eq", pq_kind="fixed", cq_kind="fixed", codes=False):
    x = _inputs(dev, d, s, b, h, group, mask_kind, cap_kind, codes)
    what = (d, s, b, h, group, mask_kind, cap_kind, pq_kind, cq_kind, codes)
    rc, want, want_probs, wp, wc = _launch(x, dev, False, pq_kind, cq_kind)
    assert rc == 0, what
    rc, got, got_probs, gp, gc = _launch(x, dev, True, pq_kind, cq_kind)
    assert rc == 0, what
    assert torch.equal(words(got), words(want)), (what, int((words(got) != words(want)).sum()))
    assert torch.equal(words(got_probs), words(want_probs)), (what, int((words(got_probs) != words(want_probs)).sum()))
    assert not bool((got == SENTINEL).any()) and not bool((got_probs == SENTINEL).any()), what
    assert not bool(torch.isnan(got).any()) and not bool(torch.isnan(got_probs).any()), what
    assert gp.same_params(wp) and gc.same_params(wc), what          # the repaired parameters are the comparator's
    if pq_kind == "lsqplus_bad":
        assert float(gp.scale) > 0 and float(gp.zp) == -128.0, what
    return x, got, got_probs


@pytest.mark.parametrize("codes", [False, True], ids=["fp32", "codes"])
@pytest.mark.parametrize("head_dim", DA.HEAD_DIMS)
def test_words_of_the_unshared_launch(dev, head_dim, codes):
    """Every kv_len of the helper's table and 1024, batch x heads (1, 1) and (2, 3), every group; masks, caps and the two
    quantizers (absent, fixed, LSQ+ with bad raw parameters) rotate at different periods."""
    i = 0
    for s in tuple(n for n in DA.kv_lens(head_dim) if n <= 1024) + (1024,):     # head_dim 4: 17 R + 1 = 1089 is past this kernel's limit
        for b, h in ((1, 1), (2, 3)):
            for group in GROUPS:
                _check(dev, head_dim, s, b, h, group, DA.MASKS[i % 3], DA.CAPS[(i // 3) % 3], KINDS[(i // 9) % 3],
                       KINDS[(i // 2) % 3], codes)
                i += 1


@pytest.mark.parametrize("codes", [False, True], ids=["fp32", "codes"])
@pytest.mark.parametrize("mask", DA.MASKS)
@pytest.mark.parametrize("cap", DA.CAPS)
def test_masks_and_caps(dev, mask, cap, codes):
    """The mask belongs to the batch row, not to the query row; cap == kv_len, cap + 7, k_cap != v_cap.  A row masked whole
    gives the uniform probabilities of the eager formula for every beam of that row."""
    _, _, probs = _check(dev, 64, 37, 2, 3, 3, mask, cap, codes=codes)
    if mask == "full":
        last = probs[3:]
        assert bool((last == last.flatten()[0]).all()) and float(last.flatten()[0]) != 0


@pytest.mark.parametrize("codes", [False, True], ids=["fp32", "codes"])
@pytest.mark.parametrize("pq_kind", KINDS, ids=str)
@pytest.mark.parametrize("cq_kind", KINDS, ids=str)
def test_quantizers_present_or_absent(dev, pq_kind, cq_kind, codes):
    _check(dev, 64, 37, 2, 3, 9, "pad", "plus7", pq_kind, cq_kind, codes)


@pytest.mark.parametrize("codes", [False, True], ids=["fp32", "codes"])
def test_probs_out_null(dev, codes):
    x = _inputs(dev, 64, 37, 2, 3, 9, "pad", "differ", codes)
    rc, want, _, _, _ = _launch(x, dev, False, "fixed", "lsqplus_bad", want_probs=False)
    assert rc == 0
    rc, got, probs, _, _ = _launch(x, dev, True, "fixed", "lsqplus_bad", want_probs=False)
    assert rc == 0 and probs is None and torch.equal(words(got), words(want))


def test_rejected_counter_gives_nan(dev):
    """A coded cache that holds an element without a code never yields numbers: every word of out and probs_out is NaN, as
    in the comparator."""
    x = _inputs(dev, 64, 37, 2, 3, 9, "pad", "eq", True)
    x["rejected"].fill_(2)
    rc, want, want_probs, _, _ = _launch(x, dev, False, "fixed", "fixed")
    assert rc == 0
    rc, got, got_probs, _, _ = _launch(x, dev, True, "fixed", "fixed")
    assert rc == 0
    assert bool(torch.isnan(got).all()) and bool(torch.isnan(got_probs).all())
    assert same_f32(got.cpu().numpy(), want.cpu().numpy()) and same_f32(got_probs.cpu().numpy(), want_probs.cpu().numpy())


@pytest.mark.parametrize("codes", [False, True], ids=["fp32", "codes"])
def test_two_runs_are_bit_equal(dev, codes):
    """Without quantizers every last bit of the sums shows."""
    x = _inputs(dev, 64, 85, 2, 3, 17, "pad", "eq", codes)
    runs = [_launch(x, dev, True, None, None) for _ in range(2)]
    assert runs[0][0] == 0 and runs[1][0] == 0
    assert torch.equal(words(runs[0][1]), words(runs[1][1])) and torch.equal(words(runs[0][2]), words(runs[1][2]))


@pytest.mark.parametrize("what", ["kv_len 1025", "kv_len 0", "group 65", "head_dim 12", "misaligned k"])
@pytest.mark.parametrize("codes", [False, True], ids=["fp32", "codes"])
def test_unsupported(dev, what, codes):
    """OSQ_ERR_UNSUPPORTED, nothing launched: the outputs keep their sentinel."""
    from outlier_suppression_amd import _hip
    x = _inputs(dev, 16, 64, 1, 1, 2, "none", "plus7", codes)
    kw = {"kv_len 1025": dict(kv_len=1025), "kv_len 0": dict(kv_len=0), "group 65": dict(group=65), "head_dim 12": dict(head_dim=12),
          "misaligned k": dict(k_offset=1 if codes else 4)}[what]
    rc, out, probs, _, _ = _launch(x, dev, True, "fixed", "fixed", **kw)
    assert rc == _hip.ERR_UNSUPPORTED
    assert bool((out == SENTINEL).all()) and bool((probs == SENTINEL).all())


def _op_inputs(dev, codes, group=6, s=37):
    x = _inputs(dev, 64, s, 2, 3, group, "pad", "plus7", codes)
    pq, cq = Quant("fixed", 0.004, 1, dev), Quant("fixed", 0.02, 1, dev, zero_point=31)
    quant = lambda p: (p.scale, p.zp, p.args[5], p.args[6], p.args[3], p.args[4])  # noqa: E731
    k, v = x["k"][:, :, :s], x["v"][:, :, :s]
    cd = None if not codes else (x["records"][0], x["records"][1], x["rejected"])
    return x, k, v, quant(pq), quant(cq), cd


def _unshared_op(x, k, v, pq, cq, cd, group):
    from outlier_suppression_amd import ops
    kr, vr = k.repeat_interleave(group, 0), v.repeat_interleave(group, 0)
    mr = x["mask"].repeat_interleave(group, 0).contiguous()
    if cd is None:
        return ops.decode_attention_fake_quant(x["q"], kr, vr, mr, pq, cq, want_probs=True)
    return ops.decode_attention_codes(x["q"], kr, vr, mr, pq, cq, cd[0], cd[1], cd[2], want_probs=True)


@pytest.mark.parametrize("codes", [False, True], ids=["fp32", "codes"])
def test_python_op_on_cache_views(dev, codes):
    """ops.decode_attention_shared on ``[:, :, :S]`` views of larger buffers: the comparator's words, nothing copied; None where
    the launch refuses."""
    from outlier_suppression_amd import ops
    x, k, v, pq, cq, cd = _op_inputs(dev, codes)
    want = _unshared_op(x, k, v, pq, cq, cd, 6)
    got = ops.decode_attention_shared(x["q"], k, v, x["mask"], pq, cq, 6, codes=cd, want_probs=True)
    assert torch.equal(words(got[0]), words(want[0])) and torch.equal(words(got[1]), words(want[1]))
    out = ops.decode_attention_shared(x["q"], k, v, x["mask"], pq, cq, 6, codes=cd)
    assert torch.equal(words(out), words(want[0]))
    assert ops.decode_attention_shared(x["q"], k, v, x["mask"], pq, cq, 4, codes=cd) is None          # 12 rows are no 4 x 2
    assert ops.decode_attention_shared(x["q"], k, v, x["mask"].repeat_interleave(6, 0), pq, cq, 6, codes=cd) is None
    big = 1025
    kk = torch.zeros(1, 3, big, 64, dtype=k.dtype, device=dev)
    assert ops.decode_attention_shared(x["q"][:2], kk, kk, None, pq, cq, 2, codes=cd) is None
    assert ops.decode_attention_shared(x["q"][:2], kk[:, :, :1024], kk[:, :, :1024], None, pq, cq, 2, codes=cd) is not None
    q65 = torch.zeros(65, 3, 1, 64, device=dev)
    assert ops.decode_attention_shared(q65, kk[:, :, :8], kk[:, :, :8], None, pq, cq, 65, codes=cd) is None


@pytest.mark.parametrize("codes", [False, True], ids=["fp32", "codes"])
def test_group_of_one_is_the_existing_op(dev, codes):
    from outlier_suppression_amd import ops
    x, k, v, pq, cq, cd = _op_inputs(dev, codes, group=1, s=85)
    want = _unshared_op(x, k, v, pq, cq, cd, 1)
    got = ops.decode_attention_shared(x["q"], k, v, x["mask"], pq, cq, 1, codes=cd, want_probs=True)
    assert torch.equal(words(got[0]), words(want[0])) and torch.equal(words(got[1]), words(want[1]))


@pytest.mark.parametrize("codes", [False, True], ids=["fp32", "codes"])
def test_captured_launch_replays(dev, codes):
    """One launch captured on a single stream: the replay gives the comparator's words, also after the queries changed."""
    from outlier_suppression_amd import ops
    x, k, v, pq, cq, cd = _op_inputs(dev, codes, group=9)
    q = x["q"]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert ops.decode_attention_shared(q, k, v, x["mask"], pq, cq, 9, codes=cd, want_probs=True) is not None     # warm
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, probs = ops.decode_attention_shared(q, k, v, x["mask"], pq, cq, 9, codes=cd, want_probs=True)
    for step in range(2):
        if step:
            q.copy_(torch.randn(q.shape, generator=torch.Generator(device=dev).manual_seed(5), device=dev) * 0.3)
        out.fill_(SENTINEL)
        probs.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        want = _unshared_op(x, k, v, pq, cq, cd, 9)
        assert torch.equal(words(out), words(want[0])) and torch.equal(words(probs), words(want[1])), step


@pytest.mark.parametrize("where", ["q", "k"])
@pytest.mark.parametrize("head_dim", [4, 64, 256])
def test_nan_as_data(dev, head_dim, where):
    """The shared twin of test_gpu_decode_attention.py::test_nan_and_infinity_as_data, batch x heads 2 x 3, nine beams (a chunk
    of eight and a chunk of one), kv_len 3 and one position beyond a trip.  A NaN in ONE beam's query makes that beam's
    probabilities and head_dim columns of that head NaN and nothing else: the seven beams that share its workgroup keep the
    clean run's words.  A NaN in the shared K makes them NaN for every beam of that batch row and head, in both chunks.
    Either way the words are the unshared launch's on the repeated tensors."""
    b, h, group, b0, h0, beam = 2, 3, 9, 1, 1, 3
    for s in (3, DA.kv_lens(head_dim)[4]):
        x = _inputs(dev, head_dim, s, b, h, group, "pad", "plus7", False)
        rc, clean, clean_probs, _, _ = _launch(x, dev, True, "fixed", "fixed")
        assert rc == 0 and not bool(torch.isnan(clean).any()) and not bool(torch.isnan(clean_probs).any())
        x = dict(x, q=x["q"].clone(), k=x["k"].clone())
        nan_rows = torch.zeros(b * group, h, dtype=torch.bool, device=dev)
        if where == "q":
            x["q"][b0 * group + beam, h0, 0, head_dim - 1] = float("nan")
            nan_rows[b0 * group + beam, h0] = True
        else:
            x["k"][b0, h0, 0, 0] = float("nan")
            nan_rows[b0 * group:(b0 + 1) * group, h0] = True
        rc, want, want_probs, _, _ = _launch(x, dev, False, "fixed", "fixed")
        assert rc == 0
        rc, got, got_probs, _, _ = _launch(x, dev, True, "fixed", "fixed")
        assert rc == 0
        what = (head_dim, s, where)
        assert same_f32(got.cpu().numpy(), want.cpu().numpy()) and same_f32(got_probs.cpu().numpy(), want_probs.cpu().numpy()), what
        nan_probs = nan_rows[:, :, None, None].expand(b * group, h, 1, s)
        nan_out = nan_rows[:, None, :, None].expand(b * group, 1, h, head_dim).reshape(b * group, 1, h * head_dim)
        assert torch.equal(torch.isnan(got_probs), nan_probs) and torch.equal(torch.isnan(got), nan_out), what
        assert torch.equal(words(got_probs)[~nan_probs], words(clean_probs)[~nan_probs]), what
        assert torch.equal(words(got)[~nan_out], words(clean)[~nan_out]), what

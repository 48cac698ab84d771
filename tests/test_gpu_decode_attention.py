"""osq_decode_attention_fake_quant (csrc/decode_attention.hip) through the C ABI: the attention of one decoding step --
scores, mask, softmax, probabilities quantizer, context, context quantizer -- in one launch, against the float64
restatement of tests/_decode_attention.py on its tie-free cases.  On those any correct fp32 evaluation has the float64
integer codes (tests/test_oracle_decode_attention.py shows it for the eager CPU sequence in two summation orders), so
``out`` and ``probs_out`` are compared as WORDS with ``(code - zp) * scale``.

All shapes are tiny: what can go wrong sits in the trip counts.  A wave covers R = 64 / (head_dim / 4) rows per load, the
four waves 4 R positions per trip, four trips of loads are in flight; the seven head sizes the kernel is instantiated for
(4 .. 256: LPR 1 .. 64, R 64 .. 1) give 256 .. 4 positions per trip and kv_len runs over 1, 3, 4R - 1, 4R, 4R + 1, 8R + 5,
17R + 1, plus the limit once per head size (4096; at head_dim 256 also 1024).

osq_decode_attention_codes is held to the same float64 restatement on the helper's CODED cases: the values of the code bytes
are formed in numpy from the record, so a misreading of the record that the library's own dequantize_kv_codes shared would
show here.  NaN and infinity as data are compared with the patterns the eager sequence gives them.

Measured on MI355X: profiles/decode_attention_head_sizes.txt (written when OSQ_DECODE_ATTENTION_HEAD_SIZES_OUT=<path> is set)."""
import os

import numpy as np
import pytest
import torch

import _decode_attention as DA
from conftest import same_f32

pytestmark = pytest.mark.gpu

SENTINEL = -777.25


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _cap_buffer(x, cap, dev):
    """x [B, h, S, d] as the first S positions of a [B, h, cap, d] buffer whose tail is NaN: a read past kv_len poisons the output."""
    b, h, s, d = x.shape
    buf = torch.full((b, h, cap, d), float("nan"), dtype=torch.float32, device=dev)
    buf[:, :, :s] = torch.from_numpy(x).to(dev)
    return buf


def _caps(variant, s):
    return {"eq": (s, s), "plus7": (s + 7, s + 7), "differ": (s + 7, s + 3)}[variant]


class Params:
    """Device tensors and the ABI's argument group of one quantizer (None: absent)."""

    def __init__(self, g, dev):
        from outlier_suppression_amd import _hip
        self.g = g
        if g is None:
            self.args = [None, None, _hip.ZP_INT32, _hip.PARAM_FIXED, 1.0, 0, 1]
            return
        self.scale = torch.tensor([g.scale_raw], dtype=torch.float32, device=dev)
        if g.mode == "lsqplus":
            self.zp = torch.tensor([g.zp_raw], dtype=torch.float32, device=dev)
            zp_type, mode = _hip.ZP_FLOAT32, _hip.PARAM_LSQPLUS | _hip.PARAM_SANITIZE
        else:
            self.zp = torch.tensor([int(g.zp_raw)], dtype=torch.int32, device=dev)
            zp_type, mode = _hip.ZP_INT32, _hip.PARAM_FIXED
        self.args = [self.scale.data_ptr(), self.zp.data_ptr(), zp_type, mode, g.grad_factor, g.qmin, g.qmax]

    def check_repaired(self):
        """OSQ_PARAM_SANITIZE leaves the repaired values in the parameters (fake_quant.py:188-191)."""
        if self.g is not None:
            assert np.float32(self.scale.item()) == self.g.scale_after and np.float32(self.zp.item()) == self.g.zp_after


def _code_buffer(codes, cap, record, seed, dev):
    """codes [B, h, S, d] as the first S positions of a [B, h, cap, d] byte buffer.  Under a 6-bit record the tail holds bytes
    that are no code (64..255): a read past kv_len shows as a value no code has."""
    b, h, s, d = codes.shape
    g = torch.Generator().manual_seed(seed)
    buf = torch.randint(64 if record[2] == 0 else 0, 256, (b, h, cap, d), generator=g).to(torch.uint8)
    buf[:, :, :s] = torch.from_numpy(codes)
    return buf.to(dev)


def launch(ref, dev, cap="eq", probs_q=True, ctx_q=True, want_probs=True, head_dim=None, kv_len=None, k_offset=0):
    """One call of the entry point on the case's tensors: osq_decode_attention_fake_quant, or osq_decode_attention_codes on
    the code bytes and records of a coded case (``rejected`` must stay 0).  Returns (status, out, probs_out or None, Params,
    Params)."""
    from outlier_suppression_amd import _hip
    lib = _hip.load()
    case = ref["case"]
    b, h, d, s = case.batch, case.heads, case.head_dim, case.kv_len
    k_cap, v_cap = _caps(cap, s)
    q = torch.from_numpy(ref["q"]).to(dev)
    mask = None if ref["mask"] is None else torch.from_numpy(ref["mask"]).to(dev)
    out = torch.full((b, 1, h * d), SENTINEL, dtype=torch.float32, device=dev)
    probs = torch.full((b, h, 1, s), SENTINEL, dtype=torch.float32, device=dev) if want_probs else None
    pp, cp = Params(ref["probs_q"] if probs_q else None, dev), Params(ref["ctx_q"] if ctx_q else None, dev)
    shape = [b, h, d if head_dim is None else head_dim, s if kv_len is None else kv_len, k_cap, v_cap]
    if case.coded:
        k = _code_buffer(ref["k_codes"], k_cap, ref["k_record"], ref["seed"], dev)
        v = _code_buffer(ref["v_codes"], v_cap, ref["v_record"], ref["seed"] + 1, dev)
        rejected = torch.zeros(1, dtype=torch.int32, device=dev)
        recs, keep = [], []
        for scale_eff, zp_eff, quant_min in (ref["k_record"], ref["v_record"]):
            keep += [torch.tensor([scale_eff], dtype=torch.float32, device=dev), torch.tensor([zp_eff], dtype=torch.float32, device=dev)]
            recs += [keep[-2].data_ptr(), keep[-1].data_ptr(), quant_min]
        rc = lib.osq_decode_attention_codes(q.data_ptr(), k.data_ptr() + k_offset, v.data_ptr(), _hip.ptr(mask), out.data_ptr(),
                                            _hip.ptr(probs), *shape, *recs, rejected.data_ptr(), *pp.args, *cp.args,
                                            _hip.raw_stream(dev))
        torch.cuda.synchronize()
        assert int(rejected.item()) == 0
    else:
        k, v = _cap_buffer(ref["k"], k_cap, dev), _cap_buffer(ref["v"], v_cap, dev)
        rc = lib.osq_decode_attention_fake_quant(q.data_ptr(), k.data_ptr() + k_offset, v.data_ptr(), _hip.ptr(mask), out.data_ptr(),
                                                 _hip.ptr(probs), *shape, *pp.args, *cp.args, _hip.raw_stream(dev))
        torch.cuda.synchronize()
    return rc, out.cpu().numpy(), None if probs is None else probs.cpu().numpy(), pp, cp


REPORT = {}        # case -> line of profiles/decode_attention_head_sizes.txt, filled as the cases pass


def _report(ref, extra=""):
    c = ref["case"]
    REPORT[c] = (f"{c.head_dim:4d} {c.kv_len:5d} {'codes' if c.coded else 'fp32':5s} {c.batch}x{c.heads} {c.bits:5s} {c.mode:7s} {c.mask:4s} "
                 f"{ref['seed']:7d} {ref['margin']:10.3e} {ref['worst_g']:9.3e}{extra}")


def _check_case(case, dev, cap=None):
    ref = DA.reference(case)
    rc, out, probs, pp, cp = launch(ref, dev, case.cap if cap is None else cap)
    assert rc == 0, case
    bad_p = int((probs.view(np.uint32) != ref["probs"].view(np.uint32)).sum())
    bad_c = int((out.view(np.uint32) != ref["out"].view(np.uint32)).sum())
    assert same_f32(probs, ref["probs"]) and same_f32(out, ref["out"]), (case, cap, ref["seed"], bad_p, bad_c)
    pp.check_repaired()
    cp.check_repaired()
    _report(ref)


@pytest.mark.parametrize("head_dim", DA.HEAD_DIMS)
def test_cases_through_the_c_abi(dev, head_dim):
    """Asymmetric 6-bit and symmetric 8-bit, Fixed and LSQ+ (OSQ_PARAM_SANITIZE, on a negative scale and an out-of-range zero
    point in half of them), every kv_len of the table, batch * heads 1 and 6 (2 and 2 at head_dim 256), the mask and cap
    variants rotating."""
    for case in DA.table(head_dim):
        _check_case(case, dev)


@pytest.mark.parametrize("head_dim", DA.HEAD_DIMS)
def test_coded_cases_through_the_c_abi(dev, head_dim):
    """osq_decode_attention_codes against the CODED float64 reference: K and V as 6-bit and 8-bit code bytes whose values
    numpy forms as ((u + quant_min) as fp32 - zp_eff) * scale_eff, with fractional zp_eff -- not another kernel's reading of
    the record.  The coded kv_lens (sixteen trips of loads in flight), bytes that are no code behind kv_len, rejected 0."""
    for case in DA.table(head_dim, coded=True):
        _check_case(case, dev)


def test_kv_limit(dev):
    _check_case(DA.LIMIT_CASE, dev)


@pytest.mark.parametrize("case", DA.LIMIT_CASES[1:], ids=lambda c: f"{c.head_dim}-{c.kv_len}")
def test_kv_limit_at_the_other_head_sizes(dev, case):
    """kv_len 4096 at head_dim 4, 8 and 32 (16 to 128 trips); head_dim 256 at 1024 (256 trips of four positions)."""
    _check_case(case, dev)


def test_kv_limit_at_head_dim_256(dev):
    """1024 trips of four positions.  The one case without a tie-free instance (DA.RELAXED_CASE): its probabilities are
    tie-free and compared as words; the context as words wherever the float64 u is further than 4 g from a tie, and at most
    one quantization step off elsewhere.  The share of sure entries (at least 0.9) is asserted on the reference alone in
    tests/test_oracle_decode_attention.py.  No other case is compared this way."""
    ref = DA.reference(DA.RELAXED_CASE)
    sure, _ = DA.sure_entries(ref)
    assert sure.mean() >= 0.9
    rc, out, probs, pp, cp = launch(ref, dev, DA.RELAXED_CASE.cap)
    assert rc == 0 and same_f32(probs, ref["probs"])
    assert same_f32(out[sure], ref["out"][sure])
    assert (np.abs(out - ref["out"]) <= float(ref["ctx_q"].scale_eff) * (1 + 1e-6)).all()
    pp.check_repaired()
    cp.check_repaired()
    off = int((out.view(np.uint32) != ref["out"].view(np.uint32)).sum())
    _report(ref, f"   sure share {sure.mean():.4f}, {off} of {out.size} entries one step off")


@pytest.mark.parametrize("head_dim", DA.HEAD_DIMS)
@pytest.mark.parametrize("cap", DA.CAPS)
def test_cap(dev, head_dim, cap):
    """cap == kv_len; cap = kv_len + 7 with a NaN tail behind both K and V; k_cap != v_cap."""
    case = next(c for c in DA.table(head_dim) if c.kv_len == DA.kv_lens(head_dim)[5] and c.batch == 2 and c.mode == "lsqplus")
    _check_case(case, dev, cap)


@pytest.mark.parametrize("mask", DA.MASKS)
def test_mask(dev, mask):
    """No mask; a padding tail of finfo.min; one row masked altogether, which gives the uniform row of the eager formula."""
    case = next(c for c in DA.table(64) if c.mask == mask and c.kv_len == 37 and c.batch == 2)
    _check_case(case, dev)
    if mask == "full":
        _, _, probs, _, _ = launch(DA.reference(case), dev)
        assert (probs[-1] == probs[-1].flat[0]).all() and probs[-1].flat[0] != 0


def _plain_case(head_dim=64):
    return next(c for c in DA.table(head_dim) if c.kv_len == DA.kv_lens(head_dim)[5] and c.batch == 2 and c.mask == "pad")


def test_probs_out_null(dev):
    ref = DA.reference(_plain_case())
    rc, out, probs, _, _ = launch(ref, dev, want_probs=False)
    assert rc == 0 and probs is None and same_f32(out, ref["out"])


def test_ctx_quantizer_absent(dev):
    """Probabilities as with the quantizer (words); the context passes through: the float64 sum of p' * v within the bound of
    an fp32 sum in any order, four times over as in the helper."""
    ref = DA.reference(_plain_case())
    rc, out, probs, _, _ = launch(ref, dev, ctx_q=False)
    assert rc == 0 and same_f32(probs, ref["probs"])
    c = ref["ctx64"].reshape(out.shape)
    tol = 4 * (ref["err_ctx"].reshape(out.shape) + np.abs(c) * DA.U)
    assert (np.abs(out.astype(np.float64) - c) <= tol).all(), float((np.abs(out - c) / tol).max())


def test_probs_quantizer_absent(dev):
    """The probabilities pass through: float64 softmax within four times the helper's bound.  The context is then a sum
    over unquantised probabilities; with no context quantizer either it is the float64 sum within the propagated bound,
    with one it is a dequantised code at most one step from the float64 code, and the same code wherever the float64 u is
    further than 4 g from a tie."""
    ref = DA.reference(_plain_case())
    case = ref["case"]
    p, err_p, v = ref["p64"], ref["err_p"], ref["v"].astype(np.float64)
    c = (p[..., None] * v).sum(2)
    err_c = (err_p[..., None] * np.abs(v)).sum(2) + DA.gamma(case.kv_len) * (p[..., None] * np.abs(v)).sum(2) + np.abs(c) * DA.U
    rc, out, probs, _, _ = launch(ref, dev, probs_q=False, ctx_q=False)
    assert rc == 0
    assert (np.abs(probs[:, :, 0].astype(np.float64) - p) <= 4 * err_p).all()
    assert (np.abs(out.astype(np.float64) - c.reshape(out.shape)) <= 4 * err_c.reshape(out.shape)).all()
    rc, out2, probs2, _, cp = launch(ref, dev, probs_q=False)
    assert rc == 0 and same_f32(probs2, probs)
    g = ref["ctx_q"]
    u = c / float(g.scale_eff)
    gu = err_c / float(g.scale_eff) + np.abs(u) * DA.U
    codes, want = g.quantize(u)
    want = want.reshape(out2.shape)
    sure = (np.abs(u - (np.floor(u) + 0.5)) > 4 * gu).reshape(out2.shape)
    assert sure.mean() > 0.9
    assert same_f32(out2[sure], want[sure])
    assert (np.abs(out2 - want) <= float(g.scale_eff) * (1 + 1e-6)).all()
    cp.check_repaired()


@pytest.mark.parametrize("what", ["head_dim 12", "kv_len 0", "kv_len 4097", "misaligned k", "head_dim 260", "head_dim 24"])
def test_unsupported(dev, what):
    """OSQ_ERR_UNSUPPORTED, nothing launched: out keeps its sentinel.  head_dim 260 is LPR 65, more lanes than a wave has;
    24 is LPR 6, no power of two."""
    from outlier_suppression_amd import _hip
    ref = DA.reference(_plain_case(16))
    kw = {"head_dim 12": dict(head_dim=12), "kv_len 0": dict(kv_len=0), "kv_len 4097": dict(kv_len=4097),
          "misaligned k": dict(k_offset=4), "head_dim 260": dict(head_dim=260), "head_dim 24": dict(head_dim=24)}[what]
    rc, out, probs, _, _ = launch(ref, dev, cap="plus7", **kw)
    assert rc == _hip.ERR_UNSUPPORTED
    assert (out == np.float32(SENTINEL)).all() and (probs == np.float32(SENTINEL)).all()


@pytest.mark.parametrize("quantized", [True, False])
def test_determinism(dev, quantized):
    """The same case twice, and once more with another cap: identical words -- also without quantizers, where every last
    bit of the two sums shows."""
    ref = DA.reference(_plain_case(64))
    runs = [launch(ref, dev, cap, probs_q=quantized, ctx_q=quantized) for cap in ("eq", "eq", "differ")]
    for rc, out, probs, _, _ in runs[1:]:
        assert rc == 0 and same_f32(out, runs[0][1]) and same_f32(probs, runs[0][2])


def test_host_wrapper_on_cache_views(dev):
    """ops.decode_attention_fake_quant on ``[:, :, :S]`` views of larger buffers with different caps (what the cached path
    hands over): the expected words, nothing copied; None for a geometry the library does not take."""
    from outlier_suppression_amd import ops
    ref = DA.reference(_plain_case(64))
    case = ref["case"]
    s = case.kv_len

    def quant(g):
        p = Params(g, dev)
        return p, (p.scale, p.zp, g.qmin, g.qmax, p.args[3], g.grad_factor)
    (pp, pq), (cp, cq) = quant(ref["probs_q"]), quant(ref["ctx_q"])
    q = torch.from_numpy(ref["q"]).to(dev)
    k, v = _cap_buffer(ref["k"], s + 9, dev)[:, :, :s], _cap_buffer(ref["v"], s + 2, dev)[:, :, :s]
    mask = torch.from_numpy(ref["mask"]).to(dev)
    out, probs = ops.decode_attention_fake_quant(q, k, v, mask, pq, cq, want_probs=True)
    assert same_f32(out.cpu().numpy(), ref["out"]) and same_f32(probs.cpu().numpy(), ref["probs"])
    out = ops.decode_attention_fake_quant(q, k, v, None, None, None)
    assert out.shape == (case.batch, 1, case.heads * case.head_dim) and bool(torch.isfinite(out).all())
    assert ops.decode_attention_fake_quant(q[..., :12].contiguous(), k[..., :12].contiguous(), v[..., :12].contiguous(),
                                           None, None, None) is None
    assert ops.decode_attention_fake_quant(q, k.transpose(1, 2).contiguous().transpose(1, 2), v, None, None, None) is None


@pytest.mark.parametrize("kind", DA.NONFINITE_KINDS)
def test_nan_and_infinity_as_data(dev, kind):
    """NaN and infinity in q, K, V and the mask, at head_dim 4, 64 and 256 (LPR 1, 16, 64), batch x heads 2 x 3, kv_len 3 and
    one position beyond a trip.  The patterns are DA.nonfinite()'s, which tests/test_oracle_decode_attention.py derives from
    the eager sequence: exactly the stated words are NaN -- all probabilities and all head_dim columns of the touched
    (b, h) for a NaN in K or q and a +inf in K, every head of a batch row whose mask is -inf throughout, one column for a NaN
    in V under a zero probability -- and every other word is the clean run's, which is the float64 reference's.  -inf in part
    of a mask row gives the words of finfo.min there."""
    for case in DA.nonfinite_cases():
        ref = DA.reference(case)
        rc, clean_out, clean_probs, _, _ = launch(ref, dev, case.cap)
        assert rc == 0 and same_f32(clean_out, ref["out"]) and same_f32(clean_probs, ref["probs"]), case
        x = DA.nonfinite(ref, kind)
        rc, out, probs, _, _ = launch(dict(ref, q=x["q"], k=x["k"], v=x["v"], mask=x["mask"]), dev, case.cap)
        assert rc == 0, case
        if x["twin_mask"] is not None:
            rc, clean_out, clean_probs, _, _ = launch(dict(ref, mask=x["twin_mask"]), dev, case.cap)
            assert rc == 0, case
            assert (probs[0][..., np.isneginf(x["mask"][0, 0, 0])] == 0).all(), case
        assert (np.isnan(probs) == x["nan_probs"]).all(), (case, kind, int(np.isnan(probs).sum()), int(x["nan_probs"].sum()))
        assert (np.isnan(out) == x["nan_out"]).all(), (case, kind, int(np.isnan(out).sum()), int(x["nan_out"].sum()))
        assert same_f32(probs[~x["nan_probs"]], clean_probs[~x["nan_probs"]]), (case, kind)
        assert same_f32(out[~x["nan_out"]], clean_out[~x["nan_out"]]), (case, kind)


def test_z_report():
    """What this run compared, per case: profiles/decode_attention_head_sizes.txt (written when
    OSQ_DECODE_ATTENTION_HEAD_SIZES_OUT=<path> is set)."""
    if not REPORT:           # run on its own: nothing to report
        return
    lines = ["osq_decode_attention_fake_quant / osq_decode_attention_codes against the float64 restatement (tests/_decode_attention.py):",
             "every case below gave the reference's words in out and probs_out (tests/test_gpu_decode_attention.py).",
             "margin: min |u - nearest tie| - 4 g over both quantizers (positive: tie-free); worst g: the largest forward bound on a u.",
             "",
             "head kv_len form  BxH bits  mode    mask    seed     margin   worst g"]
    lines += [REPORT[c] for c in sorted(REPORT, key=lambda c: (c.head_dim, c.coded, c.kv_len, c.batch, c.bits, c.mode, c.mask))]
    lines += ["", f"{len(REPORT)} cases"]
    out = os.environ.get("OSQ_DECODE_ATTENTION_HEAD_SIZES_OUT")
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")

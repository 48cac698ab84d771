"""osq_decode_attention_fake_quant (csrc/decode_attention.hip) through the C ABI: the attention of one decoding step --
scores, mask, softmax, probabilities quantizer, context, context quantizer -- in one launch, against the float64
restatement of tests/_decode_attention.py on its tie-free cases.  On those any correct fp32 evaluation has the float64
integer codes (tests/test_oracle_decode_attention.py shows it for the eager CPU sequence in two summation orders), so
``out`` and ``probs_out`` are compared as WORDS with ``(code - zp) * scale``.

All shapes are tiny: what can go wrong sits in the trip counts.  A wave covers R = 64 / (head_dim / 4) rows per load, the
four waves 4 R positions per trip, four trips of loads are in flight; head_dim 16 / 64 / 128 give 64 / 16 / 8 positions per
trip and kv_len runs over 1, 3, 4R - 1, 4R, 4R + 1, 8R + 5, 17R + 1, plus 4096 once."""
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


def launch(ref, dev, cap="eq", probs_q=True, ctx_q=True, want_probs=True, head_dim=None, kv_len=None, k_offset=0):
    """One call of the entry point on the case's tensors.  Returns (status, out, probs_out or None, Params, Params)."""
    from outlier_suppression_amd import _hip
    lib = _hip.load()
    case = ref["case"]
    b, h, d, s = case.batch, case.heads, case.head_dim, case.kv_len
    k_cap, v_cap = _caps(cap, s)
    q = torch.from_numpy(ref["q"]).to(dev)
    k, v = _cap_buffer(ref["k"], k_cap, dev), _cap_buffer(ref["v"], v_cap, dev)
    mask = None if ref["mask"] is None else torch.from_numpy(ref["mask"]).to(dev)
    out = torch.full((b, 1, h * d), SENTINEL, dtype=torch.float32, device=dev)
    probs = torch.full((b, h, 1, s), SENTINEL, dtype=torch.float32, device=dev) if want_probs else None
    pp, cp = Params(ref["probs_q"] if probs_q else None, dev), Params(ref["ctx_q"] if ctx_q else None, dev)
    rc = lib.osq_decode_attention_fake_quant(q.data_ptr(), k.data_ptr() + k_offset, v.data_ptr(), _hip.ptr(mask), out.data_ptr(),
                                             _hip.ptr(probs), b, h, d if head_dim is None else head_dim,
                                             s if kv_len is None else kv_len, k_cap, v_cap, *pp.args, *cp.args,
                                             _hip.raw_stream(dev))
    torch.cuda.synchronize()
    return rc, out.cpu().numpy(), None if probs is None else probs.cpu().numpy(), pp, cp


def _check_case(case, dev, cap=None):
    ref = DA.reference(case)
    rc, out, probs, pp, cp = launch(ref, dev, case.cap if cap is None else cap)
    assert rc == 0, case
    bad_p = int((probs.view(np.uint32) != ref["probs"].view(np.uint32)).sum())
    bad_c = int((out.view(np.uint32) != ref["out"].view(np.uint32)).sum())
    assert same_f32(probs, ref["probs"]) and same_f32(out, ref["out"]), (case, cap, ref["seed"], bad_p, bad_c)
    pp.check_repaired()
    cp.check_repaired()


@pytest.mark.parametrize("head_dim", DA.HEAD_DIMS)
def test_cases_through_the_c_abi(dev, head_dim):
    """Asymmetric 6-bit and symmetric 8-bit, Fixed and LSQ+ (OSQ_PARAM_SANITIZE, on a negative scale and an out-of-range zero
    point in half of them), every kv_len of the table, batch * heads 1 and 6, the mask and cap variants rotating."""
    for case in DA.table(head_dim):
        _check_case(case, dev)


def test_kv_limit(dev):
    _check_case(DA.LIMIT_CASE, dev)


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


@pytest.mark.parametrize("what", ["head_dim 12", "kv_len 0", "kv_len 4097", "misaligned k"])
def test_unsupported(dev, what):
    """OSQ_ERR_UNSUPPORTED, nothing launched: out keeps its sentinel."""
    from outlier_suppression_amd import _hip
    ref = DA.reference(_plain_case(16))
    kw = {"head_dim 12": dict(head_dim=12), "kv_len 0": dict(kv_len=0), "kv_len 4097": dict(kv_len=4097),
          "misaligned k": dict(k_offset=4)}[what]
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

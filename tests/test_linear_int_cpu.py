"""Integer linear layers (util_layernorm.FUSE_LINEAR_INT, csrc/linear_int.hip) without a GPU: the numpy restatement of the
rule against float64, the refusals of ops.linear_int, the routing reasons of QLinear and the binding of producers."""
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import _linear_int as LI

W_Q = NS(quantizer="FixedFakeQuantize", observer="MinMaxObserver", bit=8, symmetric=True, ch_axis=0)
A_Q = NS(quantizer="FixedFakeQuantize", observer="MinMaxObserver", bit=8, symmetric=False, ch_axis=-1)


@pytest.mark.parametrize("quant", LI.QUANTS, ids=lambda q: "-".join(map(str, q)))
@pytest.mark.parametrize("with_bias", (False, True))
def test_restatement_against_float64(quant, with_bias):
    """The operands in float64 are n * s exactly (9 + 24 bits), so F.linear in float64 is N * s_x * s_w + bias up to 2**-53
    terms.  The rule rounds three times: s = fl(s_x * s_w), p = fl(N * s) (N < 2**24 here: float(N) is exact) and fl(p + bias),
    each by a factor within 1 +- u, u = 2**-24.  With P = N s_x s_w: |p - P| <= (2u + u**2) |P| and |out - (p + bias)| <= u |out|,
    so |out - ref| <= u |out| + (2u + u**2) |P| <= 3.1 u |out| + 2.1 u |bias| (|P| <= (|out| + |bias|) / (1 - 3u))
    < 2**-22 (|out| + |bias|)."""
    from outlier_suppression_amd import ops
    x, xq, w, wq, bias = LI.make_case(11, 33, 20, (k := 80), quant, with_bias)
    record = (torch.from_numpy(xq.scale), torch.from_numpy(xq.zero_point), xq.qmin, xq.qmax)
    assert "GPU" in ops.linear_int_refusal(k, record) and 255 * 255 * k < 2 ** 24      # a case the launches take, but for where it lives
    out = LI.rule(x, xq, w, wq, bias)[0]
    xf, wf = ((LI.units(t, q) + q.qmin - q.zero_point.astype(np.float64)[:, None]) * q.scale.astype(np.float64)[:, None]
              for t, q in ((x, xq), (w, wq)))
    ref = torch.nn.functional.linear(torch.from_numpy(xf), torch.from_numpy(wf), None if bias is None else torch.from_numpy(bias).double()).numpy()
    bound = 2.0 ** -22 * (np.abs(out.astype(np.float64)) + (0 if bias is None else np.abs(bias.astype(np.float64))[None, :]))
    assert np.all(np.abs(out - ref) <= bound), float(np.max(np.abs(out - ref) - bound))


@pytest.mark.parametrize("reason, change", [
    ("per-channel", dict(channels=4)), ("more than 256 codes", dict(span=256)), ("not a multiple of 16", dict(k=24)),
    ("exceeds 16384", dict(k=16400)), ("not fp32", dict(bias=torch.zeros(8, dtype=torch.float64))),
    ("not contiguous", dict(transpose=True)), ("not on a GPU", {})])
def test_linear_int_refuses_with_its_reason(reason, change):
    from outlier_suppression_amd import ops
    k, n, channels, span = change.get("k", 32), 8, change.get("channels", 1), change.get("span", 255)
    record = (torch.ones(channels), torch.zeros(channels, dtype=torch.int32), 0, span, ops.PARAM_FIXED, 1.0)
    entry = ops.WeightCodes(torch.zeros(n, k, dtype=torch.uint8), torch.zeros(n, dtype=torch.int32), torch.ones(n),
                            torch.zeros(n, dtype=torch.int32), torch.zeros(1, dtype=torch.int32))
    codes = torch.zeros(k, 3, dtype=torch.uint8).t() if change.get("transpose") else torch.zeros(3, k, dtype=torch.uint8)
    with pytest.raises(ValueError, match=reason):
        ops.linear_int(codes, torch.zeros(3, dtype=torch.int32), record, entry, change.get("bias"))


@pytest.fixture(scope="module")
def tiny():
    from transformers import BertConfig, BertForSequenceClassification
    from outlier_suppression_amd.quant_model import quantize_model
    from outlier_suppression_amd.quantization import enable_quantization
    torch.manual_seed(0)
    cfg = BertConfig(vocab_size=60, hidden_size=32, num_hidden_layers=2, num_attention_heads=2, intermediate_size=64,
                     max_position_embeddings=20, num_labels=2)
    model = quantize_model(BertForSequenceClassification(cfg).eval(), W_Q, A_Q)
    enable_quantization(model)
    return model


def _route(op, x):
    from outlier_suppression_amd import util_layernorm as UL
    from outlier_suppression_amd.quantization import linear_int
    UL.linear_int.reset()
    assert linear_int.forward(op, x) is None and (UL.linear_int.fused, UL.linear_int.eager) == (0, 1)
    return UL.linear_int.reason


def test_routing_falls_back_with_a_reason_and_binding_adds_no_state(tiny):
    import outlier_suppression_amd as osq
    from outlier_suppression_amd import util_layernorm as UL
    from outlier_suppression_amd.quantization import Quantizer, linear_int
    from outlier_suppression_amd.quantization.quantized_module import QLinear
    op, x = tiny.bert.encoder.layer[1].attention.self.query, torch.zeros(2, 5, 32)
    producer = linear_int.producer_of(op)
    assert producer is tiny.bert.encoder.layer[0].output.LayerNorm.layernorm_post_act_fake_quantize
    with torch.no_grad():
        assert "not on a GPU" in _route(op, x)
        producer.enable_observer()
        assert _route(op, x) == "the producer is observing or disabled"
        producer.disable_observer()
        owner = tiny.bert.encoder.layer[0].output.LayerNorm
        owner.layernorm_post_act_fake_quantize = Quantizer(None, NS(**{**vars(A_Q), "ch_axis": 2}))
        assert _route(op, x) == "the producer is per-channel"           # the quantizer found is the one on the owner NOW
        owner.layernorm_post_act_fake_quantize = producer
        assert _route(Quantizer(torch.nn.Linear(32, 32), W_Q), x) == "no producer"
        op.train()
        assert _route(op, x) == "the module is in training mode"
        op.eval()
    with torch.enable_grad():
        assert _route(op, x) == "autograd is on"
    # the switch is off unless asked for, and binding adds nothing to what a model saves or lists
    assert UL.FUSE_LINEAR_INT is False and (osq.set_fast_linear_int, "OSQ_FAST_LINEAR_INT") in osq._SWITCHES

    def names():
        return list(tiny.state_dict()), [n for n, _ in tiny.named_modules()], [n for n, _ in tiny.named_parameters()]
    linears = [m for m in tiny.modules() if isinstance(m, QLinear)]
    bound = names()
    for m in linears:
        m.__dict__.pop("_linear_producer")
    assert names() == bound and len(linears) == 2 * 6 + 2
    linear_int.bind_linear_producers(tiny)
    assert names() == bound and all(linear_int.producer_of(m) is not None for m in linears)


# ---- the helpers and cases of tests/test_gpu_linear_int_edges.py, without a GPU ---------------------------------------------

@pytest.mark.parametrize("g_kind", LI.GRAD_FACTORS, ids=str)
@pytest.mark.parametrize("what", ("good",) + LI.REPAIRS + ("NaN scale",))
@pytest.mark.parametrize("mode", ("lsq", "lsqplus"))
def test_helpers_against_the_modules_torch_arithmetic(mode, what, g_kind):
    """LI.repaired and LI.effective against the arithmetic of LSQFakeQuantize / LSQPlusFakeQuantize.forward with the observer
    off, in torch on the CPU: the in-place repair (fake_quant.py:152-153 / 188-191: scale.abs_(), scale.clamp_(min=eps),
    zero_point.clamp_(qmin, qmax) for LSQ+), then util_quant.py:29-34 / 48-55 with this package's round_ste and grad_scale.
    The modules themselves take GPU tensors only; tests/test_gpu_linear_int_edges.py runs them.  Compared word for word: the
    parameters left behind and the fake-quantised output."""
    from outlier_suppression_amd.quantization.util_quant import grad_scale, round_ste
    m = 2
    (x, xq, *_), g, zp_int = LI.repair_case(m, mode, what if what in LI.REPAIRS else LI.REPAIRS[0])
    if what not in LI.REPAIRS:
        xq = xq._replace(scale=np.abs(xq.scale) if what == "good" else np.full(1, np.nan, np.float32))
    g = LI.grad_factor(g_kind, m, x.shape[1], xq.qmax)
    scale, zp = torch.from_numpy(xq.scale.copy()), torch.from_numpy(xq.zero_point.copy()).to(torch.int32 if zp_int else torch.float32)
    scale.abs_()
    scale.clamp_(min=torch.tensor([torch.finfo(torch.float32).eps]))
    if mode == "lsqplus":
        zp.clamp_(xq.qmin, xq.qmax)
    left = LI.repaired(xq.scale, xq.zero_point, mode, not zp_int, xq.qmin, xq.qmax)
    assert LI.words(scale.numpy()) == LI.words(left[0]) or (what == "NaN scale" and np.isnan(left[0]).all() and scale.isnan().all())
    assert LI.words(zp.float().numpy()) == LI.words(left[1])
    s, z = grad_scale(scale, g), (grad_scale(round_ste(zp), g) if mode == "lsqplus" else zp)
    xt = torch.from_numpy(x)
    x_quant = torch.clamp(round_ste(xt / s) + z, xq.qmin, xq.qmax)
    y = ((x_quant - z) * s).numpy()
    es, ez = LI.effective(*left, mode, g)
    if what == "NaN scale":
        assert np.isnan(es).all() and np.isnan(y).all()
        return
    assert LI.words(s.numpy()) == LI.words(es) and LI.words(z.float().numpy()) == LI.words(ez)
    u = LI.units(x, xq._replace(scale=es, zero_point=ez))
    assert not np.isnan(u).any() and y.dtype == np.float32
    assert LI.words(y) == LI.words(((u.astype(np.float32) + np.float32(xq.qmin) - ez) * es).astype(np.float32))
    assert LI.words(x_quant.numpy() - np.float32(xq.qmin)) == LI.words(u.astype(np.float32))


@pytest.mark.parametrize("g_kind", LI.GRAD_FACTORS, ids=str)
@pytest.mark.parametrize("x_mode", LI.MODES)
@pytest.mark.parametrize("m", (2, 33))
def test_mode_cases_have_teeth(m, x_mode, g_kind):
    """The conditions the GPU test of the parameter modes states before it asks the GPU, here where a bad seed costs nothing:
    the launch is good, the effective input scale is not the raw word, and the rule on the raw words of either quantizer
    gives other words of out -- all NaN for the weight's fractional zero points."""
    for w_mode in LI.W_MODES:
        raw, g, want = LI.mode_reference(m, x_mode, g_kind, w_mode)
        assert g == (0.3 if g_kind == 0.3 else 1.0 / (m * 144 * 255) ** 0.5) and want[0].shape == (m, LI.EDGE_N)
        assert (x_mode == "lsqplus") == bool(raw[1].zero_point[0] % 1) and (w_mode == "lsqplus") == bool((raw[3].zero_point % 1).all())


@pytest.mark.parametrize("mode", ("fixed", "lsq", "lsqplus"))
@pytest.mark.parametrize("m", (2, 33))
def test_repair_cases_are_what_they_say(m, mode):
    """With the repair only an int32 zero point stays outside its range (all of out NaN); without it every zero point does,
    and a negative or tiny scale alone leaves a good launch."""
    for what in LI.REPAIRS:
        for sanitize in (True, False):
            raw, g, zp_int, left, want = LI.repair_reference(m, mode, what, sanitize and mode != "fixed")
            outside = "zero point" in what and (zp_int or not sanitize or mode == "fixed")
            assert np.isnan(want[0]).all() == outside and np.isfinite(want[0]).all() == (not outside)
            assert zp_int == (mode != "lsqplus") and (want[2] != -2 ** 31).all()


@pytest.mark.parametrize("k", LI.EDGE_KS)
def test_edge_cases_stay_inside_the_rule(k):
    """Every K of the GPU file's section A: |N| <= 255 * 255 * K (the rule's own assertion), no row without codes."""
    for m in LI.EDGE_MS:
        out, codes, rowsum = LI.rule(*LI.edge_case(m, k))
        assert np.isfinite(out).all() and (rowsum != -2 ** 31).all() and codes.shape == (m, k)

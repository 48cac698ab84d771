"""Packed 4-bit weights of the integer linear layers (csrc/linear_int.hip) against the int64 restatement of tests/_linear_int.py
and the 8-bit entry of the same weight, WORD FOR WORD.  K: 16 (a lone half granule), 48 (the 8-byte tail load), 112 / 128 / 144
(a wave's chunk and its edges), 512 / 528 (a round of the four waves and one past it), 1040 (two whole chunks in a wave); the
tile kernel's K steps of 64 from both sides.  N 36 (scalar epilogue, a ragged channel tile), 132 (a second tile)."""
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import _linear_int as LI

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]

dev = torch.device("cuda:0")
# (qmin, qmax, where the zero points lie, what is added to the weight so that its values lie on the range's side)
W_RANGES = ((0, 15, "inside", 0.0), (0, 15, "qmin", 0.25), (0, 15, "qmax", -0.25), (-8, 7, "inside", 0.0), (0, 7, "inside", 0.0))
ROWS = [(m, n, k) for m in (1, 32) for n in (36, 132) for k in (16, 32, 48, 112, 128, 144, 512, 528, 1040)]
TILE = [(m, n, k) for m in (33, 129) for n in (36, 132) for k in (16, 48, 64, 80, 144)]


def gpu(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev).to(dtype)


def w4_case(i, m, n, k):
    """Seeded normal operands; the weight ranges rotate, per-channel on every other pair of cases, bias on every other case."""
    x, xq, w, _, bias = LI.make_case(7000 + i, m, n, k, LI.QUANTS[0], i % 2 == 0)
    rng = np.random.default_rng(i)
    qmin, qmax, where, shift = W_RANGES[i % len(W_RANGES)]
    channels = n if (i // 2) % 2 == 0 else 1
    zp = {"qmin": qmin, "qmax": qmax, "inside": (qmin + qmax + 1) // 2 + rng.integers(-2, 3, channels)}[where] + np.zeros(channels)
    wq = LI.Quant((0.6 / (qmax - qmin) * rng.uniform(0.8, 1.0, channels)).astype(LI.F32), zp.astype(LI.F32), qmin, qmax)
    return x, xq, (w + LI.F32(shift)).astype(LI.F32), wq, bias


def launch(case, bits):
    """(out, entry) of ops.linear_int under a ``bits`` entry of the case's weight."""
    from outlier_suppression_amd import ops
    x, xq, w, wq, bias = case
    record = (gpu(xq.scale), gpu(xq.zero_point, torch.int32), xq.qmin, xq.qmax, ops.PARAM_FIXED, 1.0)
    entry = ops.weight_codes(gpu(w), gpu(wq.scale), gpu(wq.zero_point, torch.int32), 0 if wq.scale.size > 1 else -1, wq.qmin, wq.qmax, bits=bits)
    codes, rowsum = ops.activation_codes(gpu(x), record)
    return ops.linear_int(codes, rowsum, record, entry, None if bias is None else gpu(bias)).cpu().numpy(), entry


@pytest.mark.parametrize("i, shape", list(enumerate(ROWS + TILE)), ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_packed_words_are_the_rule_s_and_the_8_bit_entry_s(i, shape):
    case = w4_case(i, *shape)
    want = LI.rule(*case)[0]
    (packed, entry), (bytewise, _) = launch(case, 4), launch(case, 8)
    assert tuple(entry.codes.shape) == (shape[1], shape[2] // 2) and np.isfinite(want).all()
    assert LI.words(packed) == LI.words(want) and LI.words(bytewise) == LI.words(want)


@pytest.mark.parametrize("i, shape", ((3, (1, 36, 48)), (4, (1, 132, 1040))))
def test_packed_bytes_are_quantize_codes_and_the_sums_are_numpy_s(i, shape):
    from outlier_suppression_amd import ops
    case = w4_case(i, *shape)
    _, _, w, wq, _ = case
    entry = launch(case, 4)[1]
    rec = ops.quantize_codes(gpu(w), gpu(wq.scale), gpu(wq.zero_point, torch.int32), 0 if wq.scale.size > 1 else -1, wq.qmin, wq.qmax, code_bits=4)
    assert torch.equal(entry.codes.flatten(), rec.codes) and int(entry.bad) == 0
    u = LI.units(w, wq).astype(np.int64)
    assert np.array_equal(entry.colsum.cpu().numpy(), u.sum(1)) and entry.colsum.dtype == torch.int32
    assert np.array_equal(entry.zw.cpu().numpy(), np.broadcast_to(wq.zero_point.astype(np.int64) - wq.qmin, shape[1:2]))


@pytest.mark.parametrize("m", (2, 34))
def test_saturation_at_the_longest_k(m):
    """K = 16384, every uw = 15, x rows of all-127 and all-(-128) bytes in turn, the input's zero point at 255."""
    k, n = 16384, 8
    x = np.tile(np.where(np.arange(m) % 2 == 0, 1e6, -1e6).astype(LI.F32)[:, None], (1, k))
    case = (x, LI.Quant(np.full(1, 0.5, LI.F32), np.full(1, 255, LI.F32), 0, 255), np.full((n, k), 1e6, LI.F32),
            LI.Quant(np.full(n, 0.25, LI.F32), np.zeros(n, LI.F32), 0, 15), None)
    want = LI.rule(*case)[0]
    assert want[1, 0] == LI.F32(-255 * 15 * k) * LI.F32(0.125) and want[0, 0] == 0
    assert LI.words(launch(case, 4)[0]) == LI.words(want)


@pytest.mark.parametrize("m", (2, 33))
def test_a_nan_weight_element_and_a_nan_activation_row(m):
    x, xq, w, wq, bias = w4_case(0, m, 36, 144)
    x[m - 2, 129] = np.nan
    out = launch((x, xq, w, wq, bias), 4)[0]
    assert np.isnan(out[m - 2]).all() and LI.words(out) == LI.words(LI.rule(x, xq, w, wq, bias)[0])
    assert not np.isnan(np.delete(out, m - 2, 0)).any()
    w[35, 143] = np.nan
    out, entry = launch((x, xq, w, wq, bias), 4)
    assert int(entry.bad) == 1 and np.isnan(out).all()


def test_a_w4_bert_packs_every_weight_and_keeps_its_logits():
    """tests/test_linear_int_cpu.py's tiny BERT with 4-bit weights, frozen: the same words with PACK_W4 on and off."""
    import outlier_suppression_amd as osq
    from transformers import BertConfig, BertForSequenceClassification
    from outlier_suppression_amd import util_layernorm as UL
    from outlier_suppression_amd.quant_model import quantize_model
    from outlier_suppression_amd.quantization import disable_all, enable_calibration_woquantization, enable_quantization, linear_int, weight_cache
    from outlier_suppression_amd.quantization.quantized_module import QLinear
    w_q = NS(quantizer="FixedFakeQuantize", observer="MinMaxObserver", bit=4, symmetric=True, ch_axis=0)
    a_q = NS(quantizer="FixedFakeQuantize", observer="MinMaxObserver", bit=8, symmetric=False, ch_axis=-1)
    torch.manual_seed(0)
    cfg = BertConfig(vocab_size=60, hidden_size=32, num_hidden_layers=2, num_attention_heads=2, intermediate_size=64,
                     max_position_embeddings=20, num_labels=2)
    q = quantize_model(BertForSequenceClassification(cfg).eval().to(dev), w_q, a_q).to(dev)
    ids = torch.randint(3, 60, (4, 17), generator=torch.Generator().manual_seed(1)).to(dev)
    batch = dict(input_ids=ids, attention_mask=torch.ones_like(ids), token_type_ids=torch.zeros_like(ids))
    enable_calibration_woquantization(q)
    with torch.no_grad():
        q(**batch)
    disable_all(q)
    enable_quantization(q)
    linears = [m for m in q.modules() if isinstance(m, QLinear)]      # with PACK_W4 on each one's cached entry is packed, none runs F.linear
    old, logits = (UL.FUSE_LINEAR_INT, linear_int.PACK_W4), {}
    try:
        osq.set_fast_linear_int(True)
        for on in (True, False, True):                   # back on: the 8-bit entries of the second pass are not served
            linear_int.PACK_W4 = on
            UL.linear_int.reset()
            with torch.no_grad():
                logits[on] = q(**batch)[0].cpu().numpy()
            assert (UL.linear_int.fused, UL.linear_int.eager) == (len(linears), 0), UL.linear_int
            shapes = [(tuple(weight_cache._CODES[m][1].codes.shape), tuple(m.weight.shape)) for m in linears]
            assert all(got == (n, k // 2 if on else k) for got, (n, k) in shapes), shapes
    finally:
        osq.set_fast_linear_int(old[0])
        linear_int.PACK_W4 = old[1]
    assert np.isfinite(logits[True]).all() and LI.words(logits[True]) == LI.words(logits[False])

"""The KV-cache append of incremental decoding (ops.fake_quant_kv_append, util_layernorm.kv_append_fake_quant): one launch
writes each site's head-split fake-quant at [offset, offset + t) of a [B, h, cap, d] buffer, after copying the first
offset positions from a source buffer through a row index.  The cache contents must be word-equal to the reference's
eager form ``torch.cat([past.index_select(0, idx), split_heads(quantizer(x))], 2)``."""
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from conftest import bits_equal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


QUANTIZERS = ("FixedFakeQuantize", "LSQFakeQuantize", "LSQPlusFakeQuantize")


def _quantizer(dev, kind, bit, symmetric, scale, zp):
    from outlier_suppression_amd.quantization import Quantizer
    q = Quantizer(None, NS(quantizer=kind, observer="AvgMinMaxObserver", bit=bit, symmetric=symmetric, ch_axis=-1)).to(dev)
    q.enable_fake_quant()
    q.scale.data.fill_(scale)
    q.zero_point.data.fill_(zp)
    return q


def _special(x, scale):
    """NaN, +-inf, +-0 and exact ties of the rounding in the first rows."""
    flat = x.view(-1)
    vals = torch.tensor([float("nan"), float("inf"), float("-inf"), 0.0, -0.0, 0.5 * scale, -1.5 * scale, 2.5 * scale],
                        device=x.device)
    n = min(flat.numel(), vals.numel())
    flat[:n] = vals[:n]
    return x


def _eager(q, x, past, rows, heads):
    b, t, w = x.shape
    new = q(x).view(b, t, heads, w // heads).transpose(1, 2).contiguous()
    if past is None:
        return new
    if rows is not None:
        past = past.index_select(0, rows)
    return torch.cat([past, new], dim=2)


def _run(dev, kind, bit, symmetric, d, t, offset, row_kind, n_sites, gen):
    from outlier_suppression_amd import util_layernorm as UL
    B, h = 5, 3
    sites, saved = [], []
    for i in range(n_sites):
        ti = t + i                                 # every site its own token count
        scale = 0.07 * (i + 1) * (-1.0 if kind != "FixedFakeQuantize" and i == 1 else 1.0)    # LSQ: the repair must run
        zp = 0 if symmetric else (i + 1) % (2 ** (bit - 1))
        q = _quantizer(dev, kind, bit, symmetric, scale, zp)
        x = _special((torch.randn(B, ti, h * d, generator=gen) * (1.0 + i)).to(dev), abs(scale))
        if offset:
            src = torch.randn(B, h, offset + 3, d, generator=gen).to(dev)[:, :, :offset]      # a view of a larger buffer
        else:
            src = None
        rows = {"none": None, "perm": torch.randperm(B, generator=gen), "repeat": torch.tensor([4, 4, 0, 2, 0])}[row_kind]
        rows = rows.to(dev) if rows is not None else None
        y = torch.full((B, h, offset + ti + 2, d), 7.0, device=dev)
        sites.append((q, x, y, offset, src, rows))
        saved.append((q.scale.data.clone(), q.zero_point.data.clone()))
    with torch.no_grad():
        got = UL.kv_append_fake_quant(sites, h)
        assert got is not None, (kind, d, t, offset, row_kind)
        after = [(s[0].scale.data.clone(), s[0].zero_point.data.clone()) for s in sites]
        for (q, x, y, off, src, rows), (s0, z0), (s1, z1) in zip(sites, saved, after):
            q.scale.data.copy_(s0)
            q.zero_point.data.copy_(z0)
            ref = _eager(q, x, src, rows, h)
            n = ref.shape[2]
            assert bits_equal(y[:, :, :n].cpu().numpy(), ref.cpu().numpy()), (kind, bit, symmetric, d, t, offset, row_kind)
            assert bool((y[:, :, n:] == 7.0).all())                      # nothing written past offset + t
            assert torch.equal(q.scale.data, s1) and torch.equal(q.zero_point.data, z1)


@pytest.mark.parametrize("d", [4, 8, 12, 16, 32, 64, 128, 256])      # any multiple of 4; 12: three float4s per row, no power of two
@pytest.mark.parametrize("t", [1, 3])
@pytest.mark.parametrize("offset", [0, 1, 61])
@pytest.mark.parametrize("row_kind", ["none", "perm", "repeat"])
def test_geometry_word_equal_to_cat(dev, d, t, offset, row_kind):
    gen = torch.Generator().manual_seed(d * 1000 + t * 100 + offset)
    for n_sites in (1, 4):
        _run(dev, "LSQPlusFakeQuantize", 6, False, d, t, offset, row_kind, n_sites, gen)


@pytest.mark.parametrize("kind", QUANTIZERS)
@pytest.mark.parametrize("bit", [2, 4, 6, 8])
@pytest.mark.parametrize("symmetric", [True, False])
def test_quantizer_settings_word_equal_to_cat(dev, kind, bit, symmetric):
    gen = torch.Generator().manual_seed(bit * 10 + symmetric)
    for n_sites in (1, 3):
        _run(dev, kind, bit, symmetric, 16, 2, 5, "perm", n_sites, gen)


def test_zero_point_types(dev):
    """int32 zero points (Fixed) and float32 ones (LSQ / LSQ+) in one launch."""
    from outlier_suppression_amd import util_layernorm as UL
    gen = torch.Generator().manual_seed(3)
    qs = [_quantizer(dev, k, 8, False, 0.05, 10) for k in QUANTIZERS]
    assert {q.zero_point.dtype for q in qs} == {torch.int32, torch.float32}
    xs = [torch.randn(2, 1, 64, generator=gen).to(dev) for _ in qs]
    past = torch.randn(2, 4, 3, 16, generator=gen).to(dev)
    ys = [torch.empty(2, 4, 4, 16, device=dev) for _ in qs]
    with torch.no_grad():
        assert UL.kv_append_fake_quant([(q, x, y, 3, past, None) for q, x, y in zip(qs, xs, ys)], 4) is not None
        for q, x, y in zip(qs, xs, ys):
            assert bits_equal(y.cpu().numpy(), _eager(q, x, past, None, 4).cpu().numpy())


def test_refused_launches_nothing(dev):
    from outlier_suppression_amd import ops
    from outlier_suppression_amd import util_layernorm as UL
    q = _quantizer(dev, "FixedFakeQuantize", 8, True, 0.05, 0)
    params = (q.scale.data, q.zero_point.data, q.quant_min, q.quant_max, ops.PARAM_FIXED, 1.0)
    with torch.no_grad():
        x = torch.randn(2, 1, 3 * 6, device=dev)                               # d = 6: not a multiple of 4
        y = torch.full((2, 3, 4, 6), 7.0, device=dev)
        assert ops.fake_quant_kv_append([(x, y, 2, params, None, None)], 3) is None
        assert bool((y == 7.0).all())
        x = torch.randn(2, 1, 64, device=dev)
        y = torch.full((2, 4, 5, 16), 7.0, device=dev)
        rows = torch.tensor([1, 0], device=dev)
        assert ops.fake_quant_kv_append([(x, y, 3, params, y[:, :, :3], rows)], 4) is None          # src aliases y
        assert bool((y == 7.0).all())
        base = torch.empty(2 * 4 * 5 * 16 + 1, device=dev)
        ymis = base[1:].view(2, 4, 5, 16)                                                            # not 16-byte aligned
        ymis.fill_(7.0)
        assert ops.fake_quant_kv_append([(x, ymis, 0, params, None, None)], 4) is None
        assert bool((ymis == 7.0).all())
        # the same buffer without a row index: an in-place append, the prefix kept
        y.copy_(torch.randn_like(y))
        keep = y[:, :, :3].clone()
        assert ops.fake_quant_kv_append([(x, y, 3, params, y[:, :, :3], None)], 4) is not None
        assert torch.equal(y[:, :, :3], keep)
        assert bits_equal(y[:, :, 3:4].cpu().numpy(), _eager(q, x, None, None, 4).cpu().numpy())
        UL.FUSE_KV_APPEND = False
        try:
            assert UL.kv_append_fake_quant([(q, x, y, 3, None, None)], 4) is None
        finally:
            UL.FUSE_KV_APPEND = True
        q.enable_observer()
        assert UL.kv_append_fake_quant([(q, x, y, 3, None, None)], 4) is None
        q.disable_observer()
    assert UL.kv_append_fake_quant([(q, x, y, 3, None, None)], 4) is None                  # autograd on


def test_side_stream(dev):
    gen = torch.Generator().manual_seed(9)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _run(dev, "LSQPlusFakeQuantize", 6, False, 64, 1, 7, "perm", 3, gen)
    torch.cuda.synchronize()


def test_model_eager_fallback_on_refused_geometry(dev):
    """A head size the kernel refuses (d = 6) in the quantising state: the attention takes the eager cat form, the same
    logits and cache as with the one-launch path switched off."""
    from transformers import BartConfig, BartForConditionalGeneration
    from outlier_suppression_amd import util_layernorm as UL
    from outlier_suppression_amd.quant_model import quantize_model
    from outlier_suppression_amd.quantization import disable_all, enable_calibration_woquantization, enable_quantization
    torch.manual_seed(0)
    cfg = BartConfig(vocab_size=50, d_model=12, encoder_layers=1, decoder_layers=1, encoder_attention_heads=2,
                     decoder_attention_heads=2, encoder_ffn_dim=16, decoder_ffn_dim=16, max_position_embeddings=32,
                     dropout=0.0, attention_dropout=0.0, activation_dropout=0.0)
    fp = BartForConditionalGeneration(cfg).eval()
    w = NS(quantizer="FixedFakeQuantize", observer="MinMaxObserver", bit=8, symmetric=True, ch_axis=0)
    a = NS(quantizer="FixedFakeQuantize", observer="AvgMinMaxObserver", bit=8, symmetric=False, ch_axis=-1)
    q = quantize_model(fp, w, a).to(dev).eval()
    ids = torch.randint(3, 50, (2, 6), device=dev)
    dec = torch.randint(3, 50, (2, 4), device=dev)
    mask = torch.ones_like(ids)
    enable_calibration_woquantization(q)
    with torch.no_grad():
        q(ids, mask, decoder_input_ids=dec)
    disable_all(q)
    enable_quantization(q)

    def decode():
        with torch.no_grad():
            out, cache, enc = q(ids, mask, decoder_input_ids=dec[:, :1], use_cache=True)
            logits = [out]
            for t in range(1, 4):
                logits.append(q(attention_mask=mask, decoder_input_ids=dec[:, t:t + 1], encoder_outputs=(enc,),
                                past_key_values=cache, use_cache=True)[0])
        return torch.cat(logits, 1), cache[0][0].clone()
    a_logits, a_cache = decode()
    UL.FUSE_KV_APPEND = False
    try:
        b_logits, b_cache = decode()
    finally:
        UL.FUSE_KV_APPEND = True
    assert torch.equal(a_logits, b_logits) and torch.equal(a_cache, b_cache)
    assert np.isfinite(a_logits.cpu().numpy()).all()

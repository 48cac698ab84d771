"""ops.linear_int_codes (csrc/linear_int.hip, the kCodes epilogue) against the three-launch chain it replaces WORD FOR WORD and
against float64: rows kernels (M <= 32) and the tile kernel, one and several channel tiles, a ragged last tile of 16 channels,
two row tiles (two tickets), a K of one partial step, the packed K % 32 == 16 tail.  Bound (b): a value in code units is below
256 and the fp32 steps between out32 and the code (erff, three multiplies, the division, the add) are under 16 ulp, so under
256 * 16 * 2**-24 = 2**-12 code units; the margin over the half step is four times that."""
import functools

import numpy as np
import pytest
import torch

import _linear_int as LI
from test_gpu_linear_int_w4 import gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]

dev = torch.device("cuda:0")
SHAPES = ((1, 48, 144), (32, 48, 1040), (32, 272, 16), (33, 48, 144), (130, 144, 1040), (130, 272, 176))
OUT_RANGES = ((0, 255), (-32, 31))
NO_ROW, PAD, MARGIN = -2 ** 31, 64, 0.5 + 2.0 ** -10


@functools.lru_cache(maxsize=None)
def reference(i, shape, bits, activation):
    """(case, out quantizer, g float64) of one case, computed once and not to be modified.  The quantizer sets rotate; a packed
    case swaps in a 16-code weight range; the out scale comes from the span of the reference's own out, a little short of it:
    most codes are interior, some clamp at both ends (under GELU, whose values stop at -0.17, at the upper end)."""
    m, n, k = shape
    x, xq, w, wq, bias = LI.make_case(9000 + i, m, n, k, LI.QUANTS[i % len(LI.QUANTS)], i % 2 == 0)
    if bits == 4:
        rng, channels = np.random.default_rng(i), wq.scale.size
        wq = LI.Quant((0.6 / 15 * rng.uniform(0.8, 1.0, channels)).astype(LI.F32), (8 + rng.integers(-2, 3, channels)).astype(LI.F32), 0, 15)
    out32 = LI.rule(x, xq, w, wq, bias)[0]
    g = torch.from_numpy(out32.astype(np.float64))
    g = (g * 0.5 * (1.0 + torch.special.erf(g * 2.0 ** -0.5)) if activation else g).numpy()
    qmin, qmax = OUT_RANGES[i % 2]
    lo, hi = float(out32.min()), float(out32.max())
    if qmin == 0:
        scale = LI.F32(0.9 * (hi - lo) / 255)
        zp = float(np.clip(np.rint(-(lo + 0.05 * (hi - lo)) / scale), 0, 255))
    else:
        scale, zp = LI.F32(0.9 * max(-lo, hi) / 31), 0.0
    return (x, xq, w, wq, bias), LI.Quant(np.full(1, scale, LI.F32), np.full(1, zp, LI.F32), qmin, qmax), g


def operands(case, oq, bits, out_zp=torch.int32):
    from outlier_suppression_amd import ops
    x, xq, w, wq, bias = case
    record = (gpu(xq.scale), gpu(xq.zero_point, torch.int32), xq.qmin, xq.qmax, ops.PARAM_FIXED, 1.0)
    out_record = (gpu(oq.scale), gpu(oq.zero_point, out_zp), oq.qmin, oq.qmax, ops.PARAM_FIXED, 1.0)
    entry = ops.weight_codes(gpu(w), gpu(wq.scale), gpu(wq.zero_point, torch.int32), 0 if wq.scale.size > 1 else -1, wq.qmin, wq.qmax, bits=bits)
    return ops.activation_codes(gpu(x), record) + (record, entry, None if bias is None else gpu(bias), out_record)


def chain(xc, xr, record, entry, bias, out_record, activation):
    """The three launches linear_int_codes replaces."""
    from outlier_suppression_amd import ops
    site = ops.gelu_fake_quant_per_tensor if activation else ops.fake_quant_per_tensor
    return ops.activation_codes(site(ops.linear_int(xc, xr, record, entry, bias), *out_record), out_record)


def words(*tensors):
    return [LI.words(t.cpu().numpy()) for t in tensors]


@pytest.mark.parametrize("activation", ("gelu", None))
@pytest.mark.parametrize("bits", (8, 4))
@pytest.mark.parametrize("i, shape", list(enumerate(SHAPES)), ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_words_are_the_chain_s_and_float64_holds_them(i, shape, bits, activation):
    from outlier_suppression_amd import ops
    case, oq, g = reference(i, shape, bits, activation)
    args = operands(case, oq, bits)
    codes, rowsum = ops.linear_int_codes(*args, activation)
    assert words(codes, rowsum) == words(*chain(*args, activation))                               # (a)
    u = (codes.cpu().numpy().view(np.int8).astype(np.int64) + 128).astype(np.float64)
    t = np.clip(g / np.float64(oq.scale[0]) + np.float64(oq.zero_point[0]), oq.qmin, oq.qmax) - oq.qmin
    err = np.abs(u - t)
    print(f"\nmax |u - t| {err.max():.6f} of {MARGIN:.6f}")
    assert (err <= MARGIN).all()                                                                  # (b)
    assert np.array_equal(rowsum.cpu().numpy(), codes.cpu().numpy().view(np.int8).astype(np.int64).sum(1))   # (c)


@pytest.mark.parametrize("m", (2, 33))
def test_rows_and_launches_without_codes(m):
    from outlier_suppression_amd import ops
    (x, xq, w, wq, bias), oq, _ = reference(0, (m, 48, 144), 8, "gelu")
    x, w, bias = x.copy(), w.copy(), bias.copy()
    x[m - 2, 5] = np.nan
    args = operands((x, xq, w, wq, bias), oq, 8)
    (codes, rowsum), (c_codes, c_rowsum) = ops.linear_int_codes(*args), chain(*args, "gelu")
    keep = [r for r in range(m) if r != m - 2]
    assert int(rowsum[m - 2]) == NO_ROW and words(rowsum, codes[keep]) == words(c_rowsum, c_codes[keep])
    x[m - 2, 5] = 0.0
    bad_w, bad_bias = w.copy(), bias.copy()
    bad_w[47, 143], bad_bias[3] = np.nan, np.nan
    for case, zp, dt in (((x, xq, bad_w, wq, bias), 0.0, torch.int32), ((x, xq, w, wq, bad_bias), 0.0, torch.int32),
                         ((x, xq, w, wq, bias), 0.5, torch.float32)):
        rowsum = ops.linear_int_codes(*operands(case, oq._replace(zero_point=oq.zero_point + LI.F32(zp)), 8, dt))[1]
        assert (rowsum == NO_ROW).all(), (zp, rowsum)


def test_stream_capture_replays_a_fresh_call_s_words():
    """The capture holds the zeroing and the kernel: a sum or a ticket that survived a replay would show in the next one."""
    from outlier_suppression_amd import ops
    case, oq, _ = reference(0, (130, 144, 176), 8, "gelu")
    xc, xr, *rest = operands(case, oq, 8)
    ops.linear_int_codes(xc, xr, *rest)                   # the library is loaded and warm before the capture
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        codes, rowsum = ops.linear_int_codes(xc, xr, *rest)
    for seed in (1, 2, 3):
        x = np.random.default_rng(seed).standard_normal(case[0].shape).astype(LI.F32)
        new = ops.activation_codes(gpu(x), rest[0])
        xc.copy_(new[0])
        xr.copy_(new[1])
        graph.replay()
        assert words(codes, rowsum) == words(*ops.linear_int_codes(*new, *rest))


@pytest.mark.parametrize("shape", ((33, 48, 144), (32, 48, 1040)))
def test_canaries(shape):
    """Through the C ABI on this test's buffers: nothing either side of codes and of rowsum is written."""
    from outlier_suppression_amd import _hip, ops
    m, n, k = shape
    case, oq, _ = reference(1, shape, 8, "gelu")
    xc, xr, (xs, xz, xlo, xhi, xmode, xg), e, bias, (os_, oz, olo, ohi, omode, og) = args = operands(case, oq, 8)
    codes = torch.full((2 * PAD + m * n,), 0x5A, dtype=torch.uint8, device=dev)
    rowsum = torch.full((2 * PAD + m,), 77, dtype=torch.int32, device=dev)
    rowsum[PAD:-PAD] = 0
    scratch = torch.zeros(m + (m + 127) // 128, dtype=torch.int32, device=dev)
    _hip.check(_hip.load().osq_linear_int_codes(
        xc.data_ptr(), xr.data_ptr(), e.codes.data_ptr(), e.colsum.data_ptr(), e.scale.data_ptr(), e.zw.data_ptr(), e.bad.data_ptr(),
        _hip.ptr(bias), codes[PAD:].data_ptr(), rowsum[PAD:].data_ptr(), scratch.data_ptr(), m, n, k,
        xs.data_ptr(), xz.data_ptr(), ops._zp_type(xz), xmode, xg, xlo, xhi,
        os_.data_ptr(), oz.data_ptr(), ops._zp_type(oz), omode, og, olo, ohi, 1, 8, _hip.stream_ptr(dev)))
    want = ops.linear_int_codes(*args)
    for buf, fill, body in ((codes, 0x5A, want[0]), (rowsum, 77, want[1])):
        assert (buf[:PAD] == fill).all() and (buf[-PAD:] == fill).all() and torch.equal(buf[PAD:-PAD], body.flatten())

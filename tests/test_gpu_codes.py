"""osq_quantize_codes / osq_dequantize_codes on the device against tests/_codes.py: the code bytes, the effective
parameters (words) and the dequantised y (words equal to the oracle's fake-quant y), on every path of csrc/codes.hip --
rows with 4-, 8- and 16-byte code stores for fp32 / bf16 / fp16, the generic kernel, misaligned buffers, the nibble
tail -- plus the rejected counter and the argument checks.  The same inputs' recipe properties: tests/test_oracle_codes.py."""
import numpy as np
import pytest
import torch
from conftest import bits_equal

import _codes as C

pytestmark = pytest.mark.gpu

TORCH_DTYPE = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
GUARD = 32


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from outlier_suppression_amd import _hip
    _hip.load()
    return torch.device("cuda:0")


def _split(shape, ch_axis):
    from outlier_suppression_amd import ops
    return ops._codes_split(shape, ch_axis)


def run_quantize(dev, x, scale, zp, shape, ch_axis, qmin, qmax, mode, g, bits, dtype="f32", x_off=0, codes_off=0, counter=None,
                 want_eff=True):
    """One osq_quantize_codes call through the C ABI.  x_off: elements the x pointer is moved off its 16-byte aligned
    allocation; codes_off: bytes likewise.  The codes buffer is pre-filled with 0xFF and longer than needed: returns
    (codes, bytes after the buffer, bytes before it, scale_eff, zp_eff, status)."""
    from outlier_suppression_amd import _hip, ops
    lib = _hip.load()
    n = int(np.prod(shape))
    outer, channels, inner = _split(shape, ch_axis)
    xb = torch.zeros(n + x_off + 8, dtype=TORCH_DTYPE[dtype], device=dev)
    xs = xb[x_off:x_off + n]
    xs.copy_(torch.from_numpy(np.ascontiguousarray(x).reshape(-1)).to(dev))
    nbytes = C.code_bytes(n, bits)
    cb = torch.full((codes_off + nbytes + GUARD,), 0xFF, dtype=torch.uint8, device=dev)
    s_t = torch.from_numpy(np.asarray(scale, np.float32)).to(dev)
    z_t = torch.from_numpy(np.asarray(zp)).to(dev)
    s_eff = torch.full((channels,), float("nan"), device=dev)
    z_eff = torch.full((channels,), float("nan"), device=dev)
    rc = lib.osq_quantize_codes(ops._elem_code(xs), xs.data_ptr(), cb.data_ptr() + codes_off, outer, channels, inner, s_t.data_ptr(),
                                z_t.data_ptr(), ops._zp_type(z_t), C.MODE_CODE[mode], float(g), qmin, qmax, bits,
                                s_eff.data_ptr() if want_eff else None, z_eff.data_ptr() if want_eff else None,
                                None if counter is None else counter.data_ptr(), _hip.stream_ptr(dev))
    torch.cuda.synchronize()
    host = cb.cpu().numpy()
    return (host[codes_off:codes_off + nbytes], host[codes_off + nbytes:], host[:codes_off], s_eff.cpu().numpy(), z_eff.cpu().numpy(), rc)


def run_dequantize(dev, codes, s_eff, z_eff, shape, ch_axis, qmin, bits, codes_off=0, y_off=0):
    from outlier_suppression_amd import _hip
    lib = _hip.load()
    n = int(np.prod(shape))
    outer, channels, inner = _split(shape, ch_axis)
    cb = torch.zeros(codes_off + codes.size + 8, dtype=torch.uint8, device=dev)
    cb[codes_off:codes_off + codes.size] = torch.from_numpy(np.ascontiguousarray(codes)).to(dev)
    yb = torch.full((y_off + n + 8,), float("nan"), device=dev)
    s_t, z_t = torch.from_numpy(s_eff).to(dev), torch.from_numpy(z_eff).to(dev)
    rc = lib.osq_dequantize_codes(cb.data_ptr() + codes_off, yb.data_ptr() + 4 * y_off, outer, channels, inner, s_t.data_ptr(), z_t.data_ptr(),
                                  qmin, bits, _hip.stream_ptr(dev))
    torch.cuda.synchronize()
    assert rc == 0
    host = yb.cpu().numpy()
    assert np.isnan(host[:y_off]).all() and np.isnan(host[y_off + n:]).all(), "dequantize wrote outside y"
    return host[y_off:y_off + n].reshape(shape)


def check_case(dev, c, x_off=0, codes_off=0):
    built = C.build(c)
    x, scale, zp, qmin, qmax = built
    e = C.expected_of(c, built)
    assert e.rejected == 0
    counter = torch.zeros(1, dtype=torch.int32, device=dev)
    codes, after, before, s_eff, z_eff, rc = run_quantize(dev, x, scale, zp, c.shape, c.ch_axis, qmin, qmax, c.mode, c.g, e.bits, c.dtype,
                                                          x_off, codes_off, counter)
    assert rc == 0, c.name
    assert (after == 0xFF).all() and (before == 0xFF).all(), (c.name, "bytes outside the codes buffer were written")
    if not np.array_equal(codes, e.codes):
        bad = np.nonzero(codes != e.codes)[0]
        raise AssertionError((c.name, "code bytes differ", len(bad), "first", int(bad[0]), int(codes[bad[0]]), int(e.codes[bad[0]])))
    assert bits_equal(s_eff, e.scale_eff) and bits_equal(z_eff, e.zp_eff), (c.name, "effective parameters")
    assert int(counter.item()) == 0, c.name
    if c.mode == "lsqplus":
        assert np.array_equal(e.zp_eff, np.rint(e.zp_eff)), (c.name, "the case needs an integer effective zero point")
    y = run_dequantize(dev, codes, s_eff, z_eff, c.shape, c.ch_axis, qmin, e.bits, codes_off, x_off)
    assert bits_equal(y, e.y), (c.name, "dequantised y differs from the oracle's fake-quant y")
    return codes, s_eff, z_eff, y


@pytest.mark.parametrize("group", list(C.GROUPS))
def test_codes_equal_the_oracle(group, dev):
    """Aligned buffers: every case of the group (tests/_codes.py says which path each shape takes)."""
    for c in C.GROUPS[group]:
        check_case(dev, c)


@pytest.mark.parametrize("group", ["generic", "modes", "row-f32-1028", "row-bf16-1032", "row-f32-1040"])
def test_misaligned_buffers_give_the_aligned_results(group, dev):
    """x four bytes (two for a 16-bit x: one element) off its 16-byte alignment, the codes buffer one byte off: the generic
    kernel, the same bytes, parameters and y as the aligned call."""
    for c in C.GROUPS[group]:
        a = check_case(dev, c)
        for x_off, codes_off in ((1, 0), (0, 1), (1, 1)):
            b = check_case(dev, c, x_off, codes_off)
            assert np.array_equal(a[0], b[0]) and bits_equal(a[3], b[3]), (c.name, x_off, codes_off)


@pytest.mark.parametrize("n", [7, 1025])
def test_nibble_tail(n, dev):
    """Odd n at four code bits: ceil(n / 2) bytes, the last high nibble 0, the byte after the buffer untouched (the buffer is
    pre-filled with 0xFF and one byte -- and more -- longer)."""
    c = C.case(f"tail-{n}", (n,), -1, "a4", seed=31 + n)
    x, scale, zp, qmin, qmax = C.build(c)
    e = C.expected_of(c)
    codes, after, _, _, _, rc = run_quantize(dev, x, scale, zp, c.shape, -1, qmin, qmax, "fixed", 1.0, 4)
    assert rc == 0 and codes.size == (n + 1) // 2
    assert codes[-1] >> 4 == 0 and (codes[-1] & 15) == e.u[-1]
    assert after[0] == 0xFF and (after == 0xFF).all()
    assert np.array_equal(codes, e.codes)


def test_code_bits_4_on_a_6_bit_range_is_refused(dev):
    x = np.zeros(8, np.float32)
    r = run_quantize(dev, x, [0.5], np.int32([0]), (8,), -1, 0, 63, "fixed", 1.0, 4)
    assert r[5] == -1 and (r[0] == 0xFF).all()
    r = run_quantize(dev, x, [0.5], np.int32([0]), (8,), -1, 0, 15, "fixed", 1.0, 8)           # 8 bits forced on a 4-bit range: fine
    assert r[5] == 0 and (r[0] == 0).all()


def _rejected_case(dev, x, scale, zp, shape, ch_axis, qmin, qmax, mode, g):
    from outlier_suppression_amd import ops
    e = C.expected(x, scale, zp, ch_axis, qmin, qmax, mode, g)
    assert e.rejected > 0
    counter = torch.zeros(1, dtype=torch.int32, device=dev)
    codes, after, _, s_eff, z_eff, rc = run_quantize(dev, x, scale, zp, shape, ch_axis, qmin, qmax, mode, g, e.bits, counter=counter)
    assert rc == 0 and int(counter.item()) == e.rejected, (int(counter.item()), e.rejected)
    assert np.array_equal(codes, e.codes), "codes: 0 at the rejected positions, the oracle's everywhere else"
    assert (C.unpack(codes, x.size, e.bits)[e.bad.reshape(-1)] == 0).all()
    assert bits_equal(s_eff, e.scale_eff) and bits_equal(z_eff, e.zp_eff)
    run_quantize(dev, x, scale, zp, shape, ch_axis, qmin, qmax, mode, g, e.bits, counter=counter)
    assert int(counter.item()) == 2 * e.rejected, "the counter is added to, not overwritten"
    y = run_dequantize(dev, codes, s_eff, z_eff, shape, ch_axis, qmin, e.bits)
    good = ~e.bad
    assert bits_equal(y[good], e.y[good])
    xs = torch.from_numpy(x).to(dev)
    z_t = torch.from_numpy(np.asarray(zp)).to(dev)
    with pytest.raises(ValueError, match=f"{e.rejected} of {x.size} elements have no integer code"):
        ops.quantize_codes(xs, torch.from_numpy(np.asarray(scale, np.float32)).to(dev), z_t, ch_axis, qmin, qmax, C.MODE_CODE[mode], g)


@pytest.mark.parametrize("shape,ch_axis", [((3, 1028), 0), ((2, 3, 5), 1), ((2, 1024), -1)])
def test_rejected_nan_and_infinities(shape, ch_axis, dev):
    c = C.case("rej", shape, ch_axis, "a4", seed=77)
    x, scale, zp, qmin, qmax = C.build(c)
    flat = x.reshape(-1)
    flat[[1, 4, flat.size // 2, flat.size - 2]] = [np.nan, np.inf, -np.inf, np.nan]
    for k in range(70, min(flat.size, 140)):               # a whole wave's worth of lanes and more
        flat[k] = np.nan
    _rejected_case(dev, x, scale, zp, shape, ch_axis, qmin, qmax, "fixed", 1.0)


def test_rejected_fractional_zero_point(dev):
    """FIXED with a float zero point k + 0.37: x_quant is fractional wherever the clamp does not catch it."""
    c = C.case("rej-zp", (3, 1028), 0, "a6", seed=78)
    x, scale, zp, qmin, qmax = C.build(c)
    zp = zp.astype(np.float32) + np.float32(0.37)
    zp[1] = np.float32(7.0)                                # one channel keeps an integer zero point: its codes stay right
    _rejected_case(dev, x, scale, zp, c.shape, 0, qmin, qmax, "fixed", 1.0)


def test_rejected_lsqplus_effective_zero_point(dev):
    """LSQ+ whose EFFECTIVE zero point -- grad_scale's forward value (zp - zp * g) + zp * g of an integer zp -- is not an
    integer, if _codes.lsqplus_fractional_zero_point's search of 400 (zp, g) pairs (integer zp in the range, g = 1 /
    sqrt(numel * quant_max) as the quantizers compute it; the oracle's arithmetic) finds one.  IT FINDS NONE: for g < 1 the
    rounding error of zp - zp * g is at most half an ulp of a number smaller than zp, so adding zp * g back rounds to the
    integer zp (also none among all zp <= 255 x numel < 20000 tried when this was written).  There is then no such rejected
    case to run, and the test runs the device on pairs of the same search as ACCEPTED cases instead: effective zero point
    an integer word for word, no element rejected, codes and y equal to the oracle's."""
    found = C.lsqplus_fractional_zero_point(0, 63)
    if found is not None:
        zp, g = found
        c = C.case("rej-lsqplus", (2, 1024), -1, "a6", seed=79)
        x, scale, _, qmin, qmax = C.build(c)
        _rejected_case(dev, x, scale, np.float32([zp]), c.shape, -1, qmin, qmax, "lsqplus", g)
        return
    for k, numel in enumerate((24, 2048, 3 * 1028)):
        check_case(dev, C.case(f"lsqplus-g-{numel}", (3, 1028), 0, "a6", mode="lsqplus", g=1.0 / (numel * 63) ** 0.5, zp_kind="f32", seed=80 + k))


def test_argument_checks_launch_nothing(dev):
    from outlier_suppression_amd import _hip
    lib = _hip.load()
    x = torch.zeros(16, device=dev)
    codes = torch.full((16,), 0xFF, dtype=torch.uint8, device=dev)
    s, z = torch.ones(1, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    y = torch.full((16,), 7.0, device=dev)
    st = _hip.stream_ptr(dev)

    def q(dtype=0, xp=x.data_ptr(), cp=codes.data_ptr(), outer=1, channels=1, inner=16, sp=s.data_ptr(), zp=z.data_ptr(), zt=0, mode=0,
          qmin=0, qmax=255, bits=8):
        return lib.osq_quantize_codes(dtype, xp, cp, outer, channels, inner, sp, zp, zt, mode, 1.0, qmin, qmax, bits, None, None, None, st)

    assert q() == 0
    torch.cuda.synchronize()
    assert (codes.cpu() == 0).all()
    codes.fill_(0xFF)
    for kw in (dict(dtype=3), dict(dtype=-1), dict(bits=6), dict(bits=0), dict(bits=16), dict(channels=0), dict(xp=None), dict(cp=None),
               dict(sp=None), dict(zp=None), dict(zt=2), dict(mode=3), dict(mode=16), dict(qmin=0, qmax=256), dict(qmin=5, qmax=4),
               dict(outer=-1), dict(inner=-1), dict(qmax=63, bits=4)):
        assert q(**kw) == -1, kw
    d = lambda cp=codes.data_ptr(), yp=y.data_ptr(), channels=1, sp=s.data_ptr(), zp=s.data_ptr(), bits=8: lib.osq_dequantize_codes(  # noqa: E731
        cp, yp, 1, channels, 16, sp, zp, 0, bits, st)
    for kw in (dict(cp=None), dict(yp=None), dict(channels=0), dict(sp=None), dict(zp=None), dict(bits=2), dict(bits=6)):
        assert d(**kw) == -1, kw
    assert lib.osq_dequantize_codes_multi(None, None, 1, 1, st) == -1 and lib.osq_dequantize_codes_multi(None, None, -1, 0, st) == -1
    assert lib.osq_dequantize_codes_multi(None, None, 0, 0, st) == 0
    torch.cuda.synchronize()
    assert (codes.cpu() == 0xFF).all() and (y.cpu() == 7.0).all(), "a refused call launched something"


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_ops_and_quantizer_surface(dtype, dev):
    """ops.quantize_codes / dequantize_codes and QuantizeBase.to_codes / from_codes: the record's fields, code_bits None
    picking 4 where the range allows, 16-bit x accepted, y word-equal to ops.fake_quant_per_channel of the same tensor."""
    from types import SimpleNamespace as NS
    from outlier_suppression_amd import ops
    from outlier_suppression_amd.quantization import Quantizer
    for rn, want_bits in (("s4", 4), ("a6", 8)):
        c = C.case("ops", (5, 24), 0, rn, dtype=dtype, seed=91)
        x, scale, zp, qmin, qmax = C.build(c)
        e = C.expected_of(c)
        xt = torch.from_numpy(x).to(dev).to(TORCH_DTYPE[dtype])
        st, zt = torch.from_numpy(scale).to(dev), torch.from_numpy(zp).to(dev)
        rec = ops.quantize_codes(xt, st, zt, 0, qmin, qmax)
        assert (rec.code_bits, rec.quant_min, rec.quant_max, rec.shape, rec.ch_axis) == (want_bits, qmin, qmax, (5, 24), 0)
        assert rec.codes.dtype == torch.uint8 and np.array_equal(rec.codes.cpu().numpy(), e.codes)
        assert bits_equal(rec.scale.cpu().numpy(), e.scale_eff) and bits_equal(rec.zero_point.cpu().numpy(), e.zp_eff)
        y = ops.dequantize_codes(rec)
        assert y.dtype == torch.float32 and bits_equal(y.cpu().numpy(), e.y)
        assert bits_equal(y.cpu().numpy(), ops.fake_quant_per_channel(xt, st, zt, 0, qmin, qmax).cpu().numpy())
        out = torch.empty(5, 24, device=dev)
        assert ops.dequantize_codes(rec, out=out) is out and torch.equal(out, y)
        forced = ops.quantize_codes(xt, st, zt, 0, qmin, qmax, code_bits=8)
        assert forced.code_bits == 8 and forced.codes.numel() == 120 and torch.equal(ops.dequantize_codes(forced), y)
    q = Quantizer(None, NS(quantizer="FixedFakeQuantize", observer="MinMaxObserver", bit=4, symmetric=True, ch_axis=0)).to(dev)
    w = torch.randn(6, 20, device=dev).to(TORCH_DTYPE[dtype])
    q.enable_observer()
    q(w)
    q.disable_observer()
    q.enable_fake_quant()
    rec = q.to_codes(w)
    assert rec.code_bits == 4 and rec.codes.numel() == 60
    assert torch.equal(q.from_codes(rec).view(torch.int32), q(w).float().view(torch.int32))

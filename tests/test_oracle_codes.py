"""CPU: the properties of the integer-code recipe (tests/_codes.py, include/osq_hip.h "integer codes") that the device
tests and export.load_codes rely on, over the very inputs tests/test_gpu_codes.py sends to the device."""
import numpy as np
import pytest
from conftest import bits_equal

import _codes as C
from oracle import fake_quant_oracle as FQ


def test_pack_unpack_is_the_identity():
    rng = np.random.default_rng(0)
    for n in (0, 1, 2, 7, 8, 1025):
        for bits, top in ((8, 256), (4, 16)):
            u = rng.integers(0, top, n).astype(np.uint8)
            codes = C.pack(u, bits)
            assert codes.dtype == np.uint8 and codes.size == C.code_bytes(n, bits)
            assert np.array_equal(C.unpack(codes, n, bits), u)
            if bits == 4 and n % 2:
                assert codes[-1] >> 4 == 0                      # the nibble of the element that does not exist
    assert np.array_equal(C.pack(np.array([1, 2, 3], np.uint8), 4), np.array([0x21, 0x03], np.uint8))   # element 2k: low nibble


@pytest.mark.parametrize("group", list(C.GROUPS))
def test_codes_carry_the_integer_tensor_word_for_word(group):
    for c in C.GROUPS[group]:
        built = C.build(c)
        x, scale, zp, qmin, qmax = built
        e = C.expected_of(c, built)
        assert e.rejected == 0, (c.name, "an input of the accepted cases has no integer code")
        xq = e.x_quant
        assert np.array_equal(xq, np.rint(xq)) and xq.min() >= qmin and xq.max() <= qmax, c.name
        assert not (np.signbit(xq) & (xq == 0)).any(), (c.name, "x_quant holds -0.0")
        assert bits_equal(e.x_quant_from_codes, xq), (c.name, "u + quant_min differs from x_quant as words")
        assert bits_equal(e.y_from_codes, e.y), (c.name, "the dequantisation from codes differs from the fake-quant y")
        assert e.codes.size == C.code_bytes(x.size, e.bits)
        if c.mode == "lsqplus":
            assert np.array_equal(e.zp_eff, np.rint(e.zp_eff)), (c.name, "the case must have an integer effective zero point")
        # fake-quantising y again returns y: what load_codes followed by an enabled weight quantizer relies on
        s, z = C._broadcast(e.scale_eff, x.shape, c.ch_axis), C._broadcast(e.zp_eff, x.shape, c.ch_axis)
        again = FQ.dequantize_affine(FQ.quantize_affine(e.y, s, z, qmin, qmax), s, z)
        assert bits_equal(again, e.y), (c.name, "fake-quant of y is not y", int((again.view(np.uint32) != e.y.view(np.uint32)).sum()))


def test_the_inputs_cover_what_they_claim():
    """Both clamp ends (u = 0 and u = quant_max - quant_min: the top bit of an 8-bit byte), signed zeros, subnormals, a -0.0
    float zero point, an LSQ scale that moves, and more rows than the rows launch has waves."""
    c = next(c for c in C.GROUPS["row-f32-1028"] if c.range == "a8" and c.shape[0] == 3)
    x, scale, zp, qmin, qmax = C.build(c)
    e = C.expected_of(c)
    assert e.u.max() == 255 and e.u.min() == 0 and (e.codes & 0x80).any()
    assert (np.signbit(x) & (x == 0)).any() and ((x == 0) & ~np.signbit(x)).any()
    assert ((x != 0) & (np.abs(x) < np.finfo(np.float32).tiny)).any()
    assert scale.min() <= 1e-3 * 1.001 and scale.max() >= 30 * 0.999
    nz = next(c for c in C.GROUPS["modes"] if c.zp_kind == "f32-negzero")
    assert np.signbit(C.build(nz)[2][0])
    lsq = [c for c in C.GROUPS["modes"] if c.mode == "lsq"]
    assert any(not bits_equal(C.expected_of(c).scale_eff, C.build(c)[1]) for c in lsq), "no LSQ case moves its scale by an ulp"
    assert C.GROUPS["rows-beyond-the-grid"][0].shape[0] > C.ROWS_WAVE_CAP
    u4 = C.expected_of(next(c for c in C.GROUPS["generic"] if c.range == "a2")).u
    assert u4.max() == 3


def test_rejected_inputs_have_no_code():
    x = np.array([1.0, np.nan, np.inf, -np.inf, 2.0, -1.0, 0.25], np.float32)
    e = C.expected(x, np.float32([0.5]), np.int32([3]), -1, 0, 15)
    assert e.rejected == 3 and list(np.nonzero(e.bad)[0]) == [1, 2, 3] and (e.u[e.bad] == 0).all()
    e = C.expected(x[[0, 4, 5, 6]], np.float32([0.5]), np.float32([3.37]), -1, 0, 63)       # a fractional zero point
    assert e.rejected >= 1


def test_lsqplus_effective_zero_point_of_an_integer_stays_an_integer():
    """What tests/test_gpu_codes.py::test_rejected_lsqplus_effective_zero_point states: the search for an integer LSQ+ zero
    point whose grad_scale value is fractional finds none."""
    assert all(C.lsqplus_fractional_zero_point(qmin, qmax, 400, seed) is None for seed in range(3) for qmin, qmax in ((0, 63), (0, 15), (0, 255)))

"""NumPy helper of the integer-code tests (not a test): the expected codes of a tensor from the oracle's x_quant
(oracle/fake_quant_oracle.py: quantize_affine, lsq_effective for the modes), the nibble packing of include/osq_hip.h
("integer codes"), the expected dequantisation -- and the inputs that tests/test_gpu_codes.py runs on the device and
tests/test_oracle_codes.py checks the recipe's own properties on."""
from types import SimpleNamespace as NS

import numpy as np

from oracle import fake_quant_oracle as FQ

F32 = np.float32
MODE_CODE = {"fixed": 0, "lsq": 1, "lsqplus": 2}
RANGES = {"a8": (0, 255), "s8": (-128, 127), "a6": (0, 63), "s6": (-32, 31), "a4": (0, 15), "s4": (-8, 7), "a2": (0, 3)}


def default_bits(qmin, qmax):
    return 4 if qmax - qmin <= 15 else 8


def code_bytes(n, bits):
    return (n * bits + 7) // 8


def pack(u, bits):
    """uint8 codes of the flattened u: one per byte, or element 2k in the low and 2k + 1 in the high nibble of byte k
    (an odd n leaves the last high nibble 0)."""
    u = np.asarray(u, dtype=np.uint8).reshape(-1)
    if bits == 8:
        return u.copy()
    assert bits == 4 and (u <= 15).all()
    if u.size % 2:
        u = np.concatenate([u, np.zeros(1, np.uint8)])
    return (u[0::2] | (u[1::2] << 4)).astype(np.uint8)


def unpack(codes, n, bits):
    codes = np.asarray(codes, dtype=np.uint8).reshape(-1)
    if bits == 8:
        return codes[:n].copy()
    out = np.empty(2 * codes.size, np.uint8)
    out[0::2], out[1::2] = codes & 15, codes >> 4
    return out[:n]


def _broadcast(p, shape, ch_axis):
    p = np.asarray(p)
    if ch_axis == -1:
        return p.reshape(())
    shp = [1] * len(shape)
    shp[ch_axis] = shape[ch_axis]
    return p.reshape(shp)


def expected(x, scale, zero_point, ch_axis, qmin, qmax, mode="fixed", g=1.0, bits=None):
    """What the device must produce for fp32 x (a 16-bit x widened): the effective parameters, x_quant and y of the
    oracle, the mask of elements without an integer code (x_quant NaN or fractional; their code is 0), the packed codes
    and the dequantisation from the codes."""
    x = np.asarray(x, dtype=F32)
    bits = default_bits(qmin, qmax) if bits is None else bits
    s_eff, z_eff = FQ.lsq_effective(np.asarray(scale, F32), np.asarray(zero_point).astype(F32), F32(g), mode)
    s_eff, z_eff = np.asarray(s_eff, F32).reshape(-1), np.asarray(z_eff, F32).reshape(-1)
    s, z = _broadcast(s_eff, x.shape, ch_axis), _broadcast(z_eff, x.shape, ch_axis)
    xq = FQ.quantize_affine(x, s, z, qmin, qmax)
    y = FQ.dequantize_affine(xq, s, z)
    with np.errstate(invalid="ignore"):
        bad = np.isnan(xq) | (xq != np.rint(xq))
        u = np.where(bad, F32(0), xq - F32(qmin)).astype(np.int64)
    assert u.min(initial=0) >= 0 and u.max(initial=0) <= qmax - qmin
    u = u.astype(np.uint8)
    codes = pack(u, bits)
    q_back = (unpack(codes, x.size, bits).astype(np.int32) + qmin).astype(F32).reshape(x.shape)
    return NS(bits=bits, scale_eff=s_eff, zp_eff=z_eff, x_quant=xq, y=y, bad=bad, rejected=int(bad.sum()), u=u, codes=codes,
              x_quant_from_codes=q_back, y_from_codes=FQ.dequantize_affine(q_back, s, z))


# ------------------------------------------------------------------------------------------------ inputs

def to_bf16(x):
    """fp32 values rounded to bfloat16 (nearest even), still fp32 storage."""
    b = np.ascontiguousarray(x, dtype=F32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return b.astype(np.uint32).view(F32).reshape(np.shape(x))


def round_to(x, dtype):
    if dtype == "bf16":
        return to_bf16(x)
    if dtype == "f16":
        return np.asarray(x, F32).astype(np.float16).astype(F32)
    return np.asarray(x, F32)


def make_params(channels, qmin, qmax, seed, zp_kind="i32"):
    """Per-channel scales spanning 1e-3 ... 30 (one channel: 0.05) and integer zero points: 0 for a symmetric range, anywhere
    in the range otherwise.  zp_kind: "i32", "f32" (integer-valued floats) or "f32-negzero" (channel 0 holds -0.0)."""
    rng = np.random.default_rng(seed)
    scale = (np.geomspace(1e-3, 30.0, channels) if channels > 1 else np.array([0.05])).astype(F32)
    rng.shuffle(scale)
    zp = np.zeros(channels, np.int32) if qmin < 0 else rng.integers(qmin, qmax + 1, channels).astype(np.int32)
    if zp_kind == "i32":
        return scale, zp
    zp = zp.astype(F32)
    if zp_kind == "f32-negzero":
        zp[0] = F32(-0.0)
    return scale, zp


def make_data(shape, ch_axis, scale, zero_point, qmin, qmax, seed, dtype="f32"):
    """Values over the whole range and three steps beyond both clamp ends, with, at random places: exact ties
    (k + 0.5) * s for even and odd k, +0.0, -0.0, subnormals of both signs and values far beyond both ends."""
    rng = np.random.default_rng(seed)
    s = np.broadcast_to(_broadcast(np.asarray(scale, F32), shape, ch_axis), shape)
    z = np.broadcast_to(_broadcast(np.asarray(zero_point).astype(F32), shape, ch_axis), shape)
    t = (rng.uniform(qmin - 3.0, qmax + 3.0, shape).astype(F32) - z).astype(F32)
    n = int(np.prod(shape))
    kinds = rng.integers(0, 40, shape)               # 0..13: a special value, the rest: the uniform draw
    ties = np.array([-3.5, -2.5, -1.5, -0.5, 0.5, 1.5, 2.5, 3.5], F32)
    for k, tie in enumerate(ties):
        t = np.where(kinds == k, tie, t)
    t = np.where(kinds == 8, F32(1000.0), t)
    t = np.where(kinds == 9, F32(-1000.0), t)
    x = (t * s).astype(F32)
    for k, v in ((10, F32(0.0)), (11, F32(-0.0)), (12, F32(1e-45)), (13, F32(-1e-40))):
        x = np.where(kinds == k, v, x)
    if n >= 2:                                        # both clamp ends and a signed zero, whatever the draw
        flat = x.reshape(-1).copy()
        sf, zf = s.reshape(-1), z.reshape(-1)
        flat[0] = F32(qmax + 5 - zf[0]) * sf[0]
        flat[-1] = F32(qmin - 5 - zf[-1]) * sf[-1]
        if n >= 3:
            flat[n // 2] = F32(-0.0)
        x = flat.reshape(shape)
    return round_to(x, dtype)


def case(name, shape, ch_axis, rng_name, mode="fixed", g=1.0, bits=None, dtype="f32", zp_kind="i32", seed=0):
    return NS(name=name, shape=tuple(shape), ch_axis=ch_axis, range=rng_name, mode=mode, g=g, bits=bits, dtype=dtype,
              zp_kind=zp_kind, seed=seed)


def build(c):
    """(x [fp32 storage, values exact in c.dtype], scale, zero_point, qmin, qmax) of a case."""
    qmin, qmax = RANGES[c.range]
    channels = 1 if c.ch_axis == -1 else c.shape[c.ch_axis]
    scale, zp = make_params(channels, qmin, qmax, c.seed + 17, c.zp_kind)
    x = make_data(c.shape, c.ch_axis, scale, zp, qmin, qmax, c.seed, c.dtype)
    return x, scale, zp, qmin, qmax


def expected_of(c, built=None):
    x, scale, zp, qmin, qmax = built if built is not None else build(c)
    return expected(x, scale, zp, c.ch_axis, qmin, qmax, c.mode, c.g, c.bits)


# The launch geometry the shapes below are chosen from (csrc/codes.hip, csrc/osq_device.h):
#   a wave walks a row; fp32: 4 elements per 16-byte granule, Granule<float>::kRowLoads = 4 granules in flight, so ONE
#   unrolled trip of one wave is 4 * 64 * 4 = 1024 elements; bf16 / fp16: 8 per granule, kRowLoads = 2: 1024 as well.
#   A lane stores 16 bytes of codes where a row's code bytes are a multiple of 16 (16 elements at 8 bits, 32 at 4),
#   otherwise 4 (8 for a 16-bit x at 8 bits).  The rows launch has at most kMaxBlocks * 2 = 4096 workgroups of 4 waves.
ROW_INNER = {"f32": (4, 16, 1020, 1024, 1028, 1040, 2052), "bf16": (8, 32, 1016, 1024, 1032, 2056), "f16": (8, 32, 1016, 1024, 1032, 2056)}
ROWS_WAVE_CAP = 2048 * 2 * 4
ALL_RANGES = (("a8", None), ("s8", None), ("a6", None), ("s6", None), ("a4", None), ("s4", None), ("a2", None), ("a4", 8))
FEW_RANGES = (("a8", None), ("s6", None), ("a4", None), ("a2", None))


def _groups():
    groups = {}
    for dtype, inners in ROW_INNER.items():
        for inner in inners:
            cs = []
            for rows in (1, 3):
                for k, (rn, bits) in enumerate(ALL_RANGES if dtype == "f32" else FEW_RANGES):
                    cs.append(case(f"{rows}x{inner}-{rn}-{bits}", (rows, inner), 0, rn, bits=bits, dtype=dtype, seed=100 * rows + k))
            groups[f"row-{dtype}-{inner}"] = cs
    groups["rows-beyond-the-grid"] = [          # more rows than the launch has waves: a wave takes a second row
        case("many-rows-a4", (ROWS_WAVE_CAP + 3, 4), 0, "a4", seed=1),
        case("many-rows-s8-per-tensor", (ROWS_WAVE_CAP + 3, 4), -1, "s8", seed=2)]
    groups["outer-and-per-tensor"] = [
        case("2x3x1024-ch1", (2, 3, 1024), 1, "a8", seed=3), case("2x3x8-ch1-a4", (2, 3, 8), 1, "a4", seed=4),
        case("2x3x8-ch1-bf16", (2, 3, 8), 1, "a4", dtype="bf16", seed=5), case("3x1028-per-tensor", (3, 1028), -1, "a6", seed=6),
        case("1x2052-per-tensor-a4", (1, 2052), -1, "s4", seed=7), case("3x1024-per-tensor-f16", (3, 1024), -1, "a8", dtype="f16", seed=8)]
    generic = []
    for k, (shape, ax) in enumerate((((2, 3, 5), 1), ((7,), -1), ((3, 1), 0), ((5, 3), 0), ((1025,), -1), ((3, 1022), 0))):
        for j, (rn, bits) in enumerate((("a8", None), ("s6", None), ("a4", None), ("s4", None), ("a2", None), ("a4", 8))):
            generic.append(case(f"{shape}-{rn}-{bits}", shape, ax, rn, bits=bits, seed=1000 + 10 * k + j))
        generic.append(case(f"{shape}-bf16", shape, ax, "a4", dtype="bf16", seed=1500 + k))
        generic.append(case(f"{shape}-f16", shape, ax, "a8", dtype="f16", seed=1600 + k))
    groups["generic"] = generic
    modes = []
    for k, (shape, ax) in enumerate((((3, 1028), 0), ((2, 3, 5), 1), ((7,), -1), ((2, 1024), -1))):
        for j, rn in enumerate(("a6", "a4", "s8")):
            sd = 2000 + 10 * k + j
            modes.append(case(f"{shape}-{rn}-fixed-f32zp", shape, ax, rn, zp_kind="f32-negzero", seed=sd))
            modes.append(case(f"{shape}-{rn}-lsq", shape, ax, rn, mode="lsq", g=0.37, seed=sd))
            modes.append(case(f"{shape}-{rn}-lsqplus", shape, ax, rn, mode="lsqplus", g=2.0 ** -6, zp_kind="f32", seed=sd))
    # 64 channels: grad_scale's forward value (s - s * g) + s * g moves about one scale in ten by an ulp at g = 0.37
    modes.append(case("64x8-a6-lsq", (64, 8), 0, "a6", mode="lsq", g=0.37, seed=2900))
    modes.append(case("64x16-a4-lsqplus", (64, 16), 0, "a4", mode="lsqplus", g=2.0 ** -6, zp_kind="f32", seed=2901))
    groups["modes"] = modes
    return groups


GROUPS = _groups()


def lsqplus_fractional_zero_point(qmin, qmax, tries=400, seed=0):
    """Search of `tries` (zero point, grad factor) pairs for one whose LSQ+ effective zero point -- grad_scale's forward value
    (zp - zp * g) + zp * g of an INTEGER zp -- is not an integer in fp32.  Returns (zp, g) or None."""
    rng = np.random.default_rng(seed)
    for _ in range(tries):
        zp = F32(rng.integers(max(qmin, 1), qmax + 1))
        g = F32(1.0 / np.sqrt(float(rng.integers(2, 4096)) * qmax))
        _, z = FQ.lsqplus_effective_params(F32(1.0), zp, g)
        if float(z) != float(np.rint(z)):
            return float(zp), float(g)
    return None

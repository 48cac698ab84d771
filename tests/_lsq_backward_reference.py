"""Input recipes and launch shapes for the LSQ / LSQ+ backward tests (tests/test_gpu_lsq_backward_accuracy.py); every
condition a recipe promises is proved on the CPU by tests/test_oracle_lsq_backward_reference.py.

The four kernels (csrc/fake_quant.hip) sum ``ds_mul + ds_div`` into scale.grad and ``g_in + ng_mul`` into zero_point.grad
(oracle/fake_quant_oracle.py, lsq_backward_terms).  Two kinds of input:

DYADIC -- every summation order gives the same sum, so the expected gradient is ONE fp32 number and the check is on bits.
scale = 2^-3, an integer zero point (LSQ+: also k + 0.5, which the forward rounds half-to-even), x = scale * (k + f) with
integer k on both sides of [qmin, qmax] and f in {0, 1/4, 1/2, 3/4}, gy integers in [-8, 8].  Then x / s = k + f exactly,
g_mul = gy / 8, and every term is a multiple of 1/8 below 2^15 (ds_mul = gy * (xq - z): whole numbers; ds_div =
-gy * (k + f): quarters; g_in, ng_mul = +-gy / 8: eighths, at most 1): a sum of up to 2^25 of them is below 2^43
eighth-units and every partial sum is exact in float64; a run of 8 is below 2^21 eighth-units and exact in fp32 -- which
is all the order-free kernels add in fp32.  A whole fp32 summation (the strict tier) is exact too while 8 * A < 2^24
(A = the sum of the terms' magnitudes, so no partial sum in any order exceeds A; the zero point's terms are eighths,
hence 8 * A and not 4 * A).
The property is needed of the EFFECTIVE parameters: grad_scale's forward (t - t*g) + t*g may move t by an ulp, so
dyadic_factors() returns only factors that give the parameters back exactly.

RANDOM -- site / clipped / one-sign / cancelling data, judged against the correctly rounded sum (lsq_backward_exact) in
units of U = 2^-24 * g * A with the reference's own fp32 summation (..._reference_order) as the yardstick.
"""
import os
import re

import numpy as np

from oracle import fake_quant_oracle as FQ

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = os.path.join(ROOT, "outlier_suppression_amd", "csrc")


def _constant(path, pattern):
    with open(os.path.join(_SRC, path)) as f:
        m = re.search(pattern, f.read())
    assert m, (path, pattern)
    return int(m.group(1))


# the launch geometry of lsq_bwd_tensor_kernel, read from the sources (the release library holds bwd_blocks as a constant)
THREADS = _constant("fake_quant.hip", r"constexpr int kThreads = (\d+);")                  # 256
MAX_BLOCKS = _constant("osq_host.h", r"constexpr int kMaxBlocks = (\d+);")                # 2048: upper end of the knob
BWD_BLOCKS = _constant("fake_quant.hip", r"OSQ_AB_KNOB\(int, g_bwd_blocks, (\d+)\)")      # the knob's default (grid cap)
ORDERED_MAX_INNER = _constant("fake_quant.hip", r"sum_lanes && outer == 1 && inner <= (\d+)")   # LDS limit of the strict rows
TRIP = 2 * THREADS * 4 * BWD_BLOCKS       # elements one trip of the capped grid covers (two float4 per lane)


def per_tensor_lengths():
    """No float4 at all, tails of 1..3 with and without a capped grid, the three forms of a lane's loop (one trip with and
    without its second float4, several trips with a partial last one), and the two lengths the strict tests use."""
    small = [0, 1, 3, 4, 5, 7, 1023, 1024, 1025, 1026, 1027]
    edges = [TRIP // 2 - 1, TRIP // 2 + 1, TRIP - 1, TRIP + 1, 3 * TRIP - 1, 3 * TRIP + 1]
    return small + edges + [3145728 + 13, (1 << 24) + 32 * 1024 + 37]


def grid_of(n, cap=None):
    """Workgroups of the order-free per-tensor launch for n elements."""
    n4 = n // 4
    return max(1, min(-(-n4 // (2 * THREADS)), cap or BWD_BLOCKS))


def lane_forms(n, cap=None):
    """Which forms of the lane loop a length runs: (some lane's last trip has one float4, some lane's trip has two,
    some lane takes several trips) -- the loop of lsq_bwd_tensor_kernel walked for every lane."""
    n4, stride = n // 4, grid_of(n, cap) * THREADS
    i0 = np.arange(min(n4, stride), dtype=np.int64)
    if i0.size == 0:
        return False, False, False
    trips = -(-(n4 - i0) // (2 * stride))
    last = i0 + (trips - 1) * 2 * stride
    one = bool((last + stride >= n4).any())
    two = bool((last + stride < n4).any() or (trips > 1).any())
    return one, two, bool((trips > 1).any())


# (outer, channels, inner) of lsq_bwd_channel_kernel / lsq_bwd_channel_ordered_kernel
CHANNEL_SHAPES = [(1, 12, 20), (1, 768, 768), (1, 3072, 768), (1, 768, 3072), (1, 7, 3073), (1, 5, 7), (1, 3, 255),
                  (1, 3, 256), (1, 3, 257), (1, 3, 513), (4, 6, 5), (3, 64, 130), (2, 1, 1000), (8, 12, 1)]
CHANNEL_EMPTY = [(0, 4, 5), (3, 0, 5), (3, 4, 0), (1, 4, 0)]
CHANNEL_SIZED = [(1, 768, 768), (1, 768, 3072), (1, 7, 3073), (3, 64, 130)]       # the accuracy tests' shapes
TENSOR_SIZED = [1023, 98304 + 5, 3145728 + 13, 64 * 128 * 768]


def ordered_rows(outer, inner):
    """True when the strict per-channel call runs lsq_bwd_channel_ordered_kernel (else it hands over to the order-free one)."""
    return outer == 1 and inner <= ORDERED_MAX_INNER


# ----------------------------------------------------------------------------------------------------------------------
# dyadic
# ----------------------------------------------------------------------------------------------------------------------

DYADIC_SCALE = F32(0.125)
DYADIC_RANGES = ((0, 63), (-32, 31), (0, 255), (-8, 7))


def effective_is_exact(scale, zero_point, g, mode):
    """grad_scale's forward gives the parameters back bit for bit (zero point: its rounded value for LSQ+)."""
    s, z = FQ.lsq_effective(F32(scale), np.asarray(zero_point, F32), g, mode)
    want = np.round(np.asarray(zero_point, F32)) if FQ._mode_name(mode) == "lsqplus" else np.asarray(zero_point, F32)
    return bool(np.all(np.asarray(s, F32) == F32(scale)) and np.array_equal(np.asarray(z, F32).reshape(-1), want.reshape(-1)))


def dyadic_factors(n, qmax, zero_points, channels=None):
    """Grad factors for a dyadic case: a power of two and the module's own 1/sqrt(n * qmax) -- each kept only if the
    effective parameters of every mode are then exactly (2^-3, the integer)."""
    out = []
    for g in (2.0 ** -10, FQ.lsqplus_grad_factor(max(n, 1), qmax, channels)):
        if all(effective_is_exact(DYADIC_SCALE, zero_points, g, m) for m in FQ.MODES):
            out.append(g)
    return out


def dyadic_xy(rng, shape, qmin, qmax, zero_point, ch_axis=-1):
    """x, gy of the recipe.  zero_point: a number, or one per channel (then k is spread round that channel's range)."""
    n = int(np.prod(shape))
    z = np.round(np.asarray(zero_point, np.float64))
    if ch_axis != -1:
        shp = [1] * len(shape)
        shp[ch_axis] = shape[ch_axis]
        z = np.broadcast_to(z.reshape(shp), shape).reshape(-1)
    span = (qmax - qmin) // 2 + 4
    lo, hi = qmin - z - span, qmax - z + span                     # x_int = rint(k + f) + z reaches both sides of the range
    k = np.floor(lo + rng.random(n) * (hi - lo + 1))
    edge = rng.random(n) < 0.1                                    # exactly on the clamp boundaries, often
    k = np.where(edge, np.where(rng.random(n) < 0.5, qmin - z, qmax - z) + rng.integers(-1, 2, n), k)
    f = rng.integers(0, 4, n) / 4.0
    x = (np.float64(DYADIC_SCALE) * (k + f)).astype(F32)
    gy = rng.integers(-8, 9, n).astype(F32)
    return x.reshape(shape), gy.reshape(shape)


def dyadic_one_sign_xy(rng, n, qmax, zero_point):
    """The dyadic recipe with every term of scale.grad positive: gy in 1..8 and every x above the range, so ds_mul =
    gy * (qmax - z) are whole numbers of one sign and a lane's running sum GROWS -- beyond 2^24 (where fp32 drops odd
    numbers) once a lane has added enough of them, while any run of 8 stays exact.  A kernel that keeps an fp32
    accumulator across trips then misses the exact sum; float64 across trips does not."""
    k = qmax - np.round(np.float64(zero_point)) + 1 + rng.integers(0, 100, n)
    f = rng.integers(0, 4, n) / 4.0
    x = (np.float64(DYADIC_SCALE) * (k + f)).astype(F32)
    return x, rng.integers(1, 9, n).astype(F32)


def dyadic_expected(x, gy, zero_point, qmin, qmax, g, mode, ch_axis=-1):
    """(dx, ds, dz, A) with ds, dz the single fp32 numbers every summation order must give, [channels] each, and
    A = max(A_s, A_z) per channel."""
    e = FQ.lsq_backward_exact(x, gy, DYADIC_SCALE if ch_axis == -1 else np.full(x.shape[ch_axis], DYADIC_SCALE),
                              zero_point, qmin, qmax, g, mode, ch_axis, how="float64")
    return e.dx, e.dscale.astype(F32), e.dzp.astype(F32), np.maximum(e.A_s, e.A_z)


def fp32_sums_exact(A):
    """A whole fp32 summation of eighth-unit terms is exact in every order while 8 * A < 2^24."""
    return 8.0 * np.asarray(A) < 2.0 ** 24


# ----------------------------------------------------------------------------------------------------------------------
# random recipes
# ----------------------------------------------------------------------------------------------------------------------

def activation_like(rng, n):
    """Post-LayerNorm-like values with a few large columns (what tests/golden/make_golden.py quantizes)."""
    x = rng.standard_normal(n).astype(F32)
    x[rng.random(n) < 0.01] *= F32(12.0)
    return x


def span_qparams(x, bit, symmetric):
    """scale / zero point from the data's span, as calculate_qparams does it (observer.py:100-118)."""
    from oracle import observer_oracle as OB
    qmin, qmax = (-(1 << (bit - 1)), (1 << (bit - 1)) - 1) if symmetric else (0, (1 << bit) - 1)
    finite = x[np.isfinite(x)]
    lo, hi = (F32(finite.min()), F32(finite.max())) if finite.size else (F32(-1), F32(1))
    scale, zp = OB.calculate_qparams(lo, hi, qmin, qmax, symmetric)
    return F32(scale), F32(zp), qmin, qmax


SITE_VARIANTS = [(2, False), (4, True), (6, False), (8, True), (8, False)]
RECIPES = ("site", "clipped", "one-sign", "cancelling")


def recipe(name, seed, n, variant=0):
    """(x, gy, scale, zero_point, qmin, qmax) of one seeded case, flat fp32 arrays of n elements.

    site        activation_like / randn * 1.5, scale from the span, bits 2 / 4 / 6 / 8, both symmetries
    clipped     scale so small that >= 40 % of the elements lie outside EACH side: dz sums millions of terms
    one-sign    gy > 0 and every x above qmax * scale: every term of both sums has one sign, kappa = 1
    cancelling  gy alternating in sign along sorted |x|: kappa = A / |S| between 1e3 and 1e5"""
    rng = np.random.default_rng([seed, RECIPES.index(name), variant])
    if name == "site":
        bit, sym = SITE_VARIANTS[variant % len(SITE_VARIANTS)]
        x = activation_like(rng, n) if variant % 2 == 0 else (rng.standard_normal(n) * 1.5).astype(F32)
        gy = rng.standard_normal(n).astype(F32)
        scale, zp, qmin, qmax = span_qparams(x, bit, sym)
        return x, gy, scale, zp, qmin, qmax
    if name == "clipped":
        x = (rng.standard_normal(n) * 1.5).astype(F32)
        gy = rng.standard_normal(n).astype(F32)
        return x, gy, F32(0.004), F32(31.5 if variant % 2 else 32.0), 0, 63     # inside: |x| < ~0.13 = 0.085 sigma
    if name == "one-sign":
        gy = (rng.random(n) + 0.25).astype(F32)
        x = (F32(63 * 0.07) + F32(0.1) + np.abs(rng.standard_normal(n)) * 1.5).astype(F32)
        return x, gy, F32(0.07), F32(7.3), 0, 63
    if name == "cancelling":
        x = np.sort(np.abs(rng.standard_normal(n) * 1.5)).astype(F32)
        sign = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
        # +-1 on neighbours of the sorted |x| cancels (exactly where both are clipped); the small one-signed part sets |S|
        gy = (sign + 1e-3).astype(F32)
        return x, gy, F32(0.07), F32(31.4), 0, 63
    raise ValueError(name)


def kappa(e):
    """(kappa_s, kappa_z) = A / |S| of a lsq_backward_exact result (per channel)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return e.A_s / np.abs(e.S_s), e.A_z / np.abs(e.S_z)


# ----------------------------------------------------------------------------------------------------------------------
# the bar
# ----------------------------------------------------------------------------------------------------------------------

U24 = 2.0 ** -24
BAR_FACTOR = 3.0          # as tests/test_gpu_site_accuracy.py: 3x the reference's own fp32 error ...
BAR_FLOOR = 4.0           # ... with a floor of 4 units on the reference's figure


def units(value, exact, A, factor):
    """|value - exact| in units of U = 2^-24 * factor * A (0 where A is 0 and the value is right)."""
    value, exact = np.asarray(value, np.float64), np.asarray(exact, np.float64)
    u = U24 * abs(float(factor)) * np.asarray(A, np.float64)
    err = np.abs(value - exact)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(err == 0, 0.0, err / u)


def ulp32_units(exact, A, factor):
    """One fp32 ulp of the result (its final rounding), in the same unit."""
    exact = np.asarray(exact, np.float64)
    u = U24 * abs(float(factor)) * np.asarray(A, np.float64)
    ulp = np.spacing(np.abs(exact).astype(F32)).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(u > 0, ulp / u, 0.0)


def bar_units(e_ref, exact, A, factor):
    """What the kernel's error may be, in units: max(3 * e_ref, 4) + one ulp of the result."""
    return np.maximum(BAR_FACTOR * np.asarray(e_ref, np.float64), BAR_FLOOR) + ulp32_units(exact, A, factor)


# ----------------------------------------------------------------------------------------------------------------------
# specials
# ----------------------------------------------------------------------------------------------------------------------

SPECIAL_VALUES = (("x", np.nan), ("x", np.inf), ("x", -np.inf), ("gy", np.nan), ("gy", np.inf), ("gy", -np.inf),
                  ("x", -0.0), ("x", 1e-41), ("gy", -0.0), ("gy", 1e-41))


def special_positions(n, cap=None):
    """first float4, last float4, inside the tail, in the second grid-stride trip -- those that exist at length n."""
    n4 = n // 4
    pos = {"first float4": 1} if n4 else {}
    if n4:
        pos["last float4"] = 4 * (n4 - 1) + 2
    if n % 4:
        pos["tail"] = n - 1
    second = 2 * grid_of(n, cap) * THREADS * 4 + 5
    if second < 4 * n4:
        pos["second trip"] = second
    return pos

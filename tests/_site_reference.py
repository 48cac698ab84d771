"""float64 references of the three one-launch producer sites (csrc/layernorm.hip, csrc/attention.hip, the GELU instance
of csrc/fake_quant.hip) and the seeded input recipes the accuracy tests judge them on.  Plain NumPy / torch CPU; imported
by tests/test_oracle_site_reference.py (which pins the references to the reference project's own runs and proves every
recipe's conditions on the CPU) and by tests/test_gpu_site_accuracy.py.

What is float64 and what is not: the elementwise steps in front of a reduction (``x*gamma + hidden``, ``s*alpha + mask``)
are bit-defined fp32 operations of the eager code -- the kernels reproduce them word for word -- so they are formed in
fp32 here as well and are not part of what is judged.  Everything after them (moments, normalisation, affine pair; max,
exp, sum, division; erf) is float64."""
import math

import numpy as np
import torch

F32 = np.float32
U = 2.0 ** -24                      # unit roundoff of fp32


def _np32(t):
    if t is None:
        return None
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(t, dtype=F32))


# ---------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------

def residual_f32(x, hidden, gamma):
    """r of the eager ops (GammaResidual): ``a = x*gamma`` rounded, ``r = a + hidden`` rounded; x itself without a residual
    (gamma is only read next to a hidden operand, as in the kernel)."""
    x, hidden, gamma = _np32(x), _np32(hidden), _np32(gamma)
    if hidden is None:
        return x
    with np.errstate(all="ignore"):
        a = x * gamma if gamma is not None else x
        return (a + hidden).astype(F32)


def layernorm_site_f64(x, hidden, gamma, weight, bias, eps):
    """(y64 [rows, H], kappa [rows]) of ``layer_norm(x*gamma + hidden) * weight + bias``: r in fp32 (residual_f32), then
    mean, biased variance, (r - mean) / sqrt(var + eps), * weight, + bias in float64.  kappa = 1 + |mean| / sigma is the
    row's condition number for the moments (sigma from float64; inf where sigma == 0)."""
    r = residual_f32(x, hidden, gamma)
    h = r.shape[-1]
    r = r.reshape(-1, h).astype(np.float64)
    with np.errstate(all="ignore"):
        mean = r.mean(axis=1, keepdims=True)
        d = r - mean
        var = (d * d).mean(axis=1, keepdims=True)
        y = d / np.sqrt(var + float(eps))
        if weight is not None:
            y = y * _np32(weight).astype(np.float64)
        if bias is not None:
            y = y + _np32(bias).astype(np.float64)
        sigma = np.sqrt(var[:, 0])
        kappa = np.where(sigma > 0, 1.0 + np.abs(mean[:, 0]) / np.where(sigma > 0, sigma, 1.0), np.inf)
    return y, kappa


def pre_softmax_f32(scores, mask, alpha=None, divisor=None):
    """The value that enters the softmax, in fp32 and in the kernel's documented order: ``s*alpha`` or ``s/divisor``
    (alpha / divisor rounded to fp32 first, as the C ABI takes them), then ``+ mask`` (broadcast), each step rounded."""
    assert alpha is None or divisor is None
    v = _np32(scores)
    with np.errstate(all="ignore"):
        if alpha is not None:
            v = v * F32(alpha)
        elif divisor is not None:
            v = v / F32(divisor)
        if mask is not None:
            v = v + np.broadcast_to(_np32(mask), v.shape)
    return np.ascontiguousarray(v, dtype=F32)


def softmax_f64(v):
    """softmax over the last axis of fp32 values, in float64 (exp(v - max) / sum).  A NaN, a +inf or a row of -inf only
    gives a NaN row, as the formula does everywhere."""
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(all="ignore"):
        e = np.exp(v - v.max(axis=-1, keepdims=True))
        return e / e.sum(axis=-1, keepdims=True)


def softmax_site_f64(scores, mask, alpha=None, divisor=None):
    """(v32, p64): pre_softmax_f32 and its float64 softmax."""
    v = pre_softmax_f32(scores, mask, alpha, divisor)
    return v, softmax_f64(v)


def gelu_f64(x):
    """x/2 * (1 + erf(x / sqrt(2))) in float64 (torch's float64 erf)."""
    x = torch.as_tensor(_np32(x)).double()
    return (x * 0.5 * (1.0 + torch.erf(x * (1.0 / math.sqrt(2.0))))).numpy()


# ---------------------------------------------------------------------------------------------------------------------
# metrics
# ---------------------------------------------------------------------------------------------------------------------

def ln_error(y, y64, kappa):
    """max over rows of (max |y - y64| / max(1, max |y64|)) / kappa.  Rows with kappa == inf (sigma == 0) are judged by
    exact checks, not here.  A non-finite y where y64 is finite counts as an infinite error."""
    y = np.asarray(y, dtype=np.float64).reshape(y64.shape)
    err = np.abs(y - y64)
    err[~np.isfinite(err)] = np.inf
    per_row = err.max(axis=1) / np.maximum(1.0, np.abs(y64).max(axis=1))
    ok = np.isfinite(kappa)
    return float((per_row[ok] / kappa[ok]).max()) if ok.any() else 0.0


SOFTMAX_REL_FLOOR = 2.0 ** -100     # |p - p64| is relative to p64 at and above this, absolute below


def softmax_error(p, p64):
    """max of |p - p64| / p64 where p64 >= 2**-100 and of |p - p64| below; rows whose float64 result is NaN are skipped
    (they are compared as NaN patterns by the exact checks)."""
    p = np.asarray(p, dtype=np.float64).reshape(p64.shape)
    rows = ~np.isnan(p64).any(axis=-1)
    p, p64 = p[rows], p64[rows]
    if p.size == 0:
        return 0.0
    err = np.abs(p - p64)
    err[~np.isfinite(err)] = np.inf
    big = p64 >= SOFTMAX_REL_FLOOR
    err[big] = err[big] / p64[big]
    return float(err.max())


def bar_from(torch_cpu_figure, factor=3.0):
    """The asserted bound: ``factor`` x torch's CPU fp32 figure in the same metric, with a floor of 4u on that figure."""
    return factor * max(float(torch_cpu_figure), 4.0 * U)


# ---------------------------------------------------------------------------------------------------------------------
# LayerNorm site: cases and input recipes
# ---------------------------------------------------------------------------------------------------------------------

# every dispatch boundary of residual_layernorm_fq_kernel<R> (ceil(cols / 256) -> R in 1,2,3,4,8,16) and a partial last
# lane group on each side of it
LN_WIDTHS = (4, 8, 252, 256, 260, 508, 512, 516, 764, 768, 772, 1020, 1024, 1028, 1536, 2044, 2048, 2052, 3072, 4092, 4096)


def ln_template_r(cols):
    per_lane = (cols // 4 + 63) // 64
    for r in (1, 2, 3, 4, 8, 16):
        if per_lane <= r:
            return r
    raise ValueError(cols)


# name, residual, gamma on the shortcut, LayerNorm weight, bias -- the four forms the wrapped models launch
LN_COMBOS = (
    ("plain", False, False, True, True),             # embedding LayerNorm: no residual, affine pair
    ("residual_affine", True, False, True, True),    # before Gamma Migration
    ("gamma_shift", True, True, False, True),        # after it: shortcut * gamma, non-scaling LayerNorm + beta/gamma
    ("bare", False, False, False, False),
)
LN_EPS = (1e-12, 1e-5)
LN_CLASSES = ("randn", "outliers", "offset10", "offset1e3", "spike", "tiny", "huge", "gamma_outliers")
LN_ACC_ROWS = 96


def ln_inputs(cols, cls, combo, rows=LN_ACC_ROWS, seed=0):
    """(x, hidden, gamma, weight, bias) as torch fp32 CPU tensors (None where the combination has no such operand).

    randn            unit normal rows
    outliers         + six columns x 20 (the tests/_ln_site.py recipe)
    offset10/1e3     + a common offset of 10 / 1e3 standard deviations (on the sub-layer output when there is a residual,
                     so that gamma does not turn the offset into variance)
    spike            one 1e4 entry in an otherwise unit row
    tiny / huge      every activation x 1e-20 / x 1e15: squares in the subnormal range / near the top of fp32
    gamma_outliers   gamma and the LayerNorm weight carry 6.0 / 4.5 / 0.05 entries (what Gamma Migration exists for)"""
    name, use_hidden, use_gamma, use_weight, use_bias = combo
    gen = torch.Generator().manual_seed(7919 * cols + 101 * LN_CLASSES.index(cls) + 13 * [c[0] for c in LN_COMBOS].index(name) + seed)
    x = torch.randn(rows, cols, generator=gen)
    hidden = torch.randn(rows, cols, generator=gen) * 0.5
    idx = torch.randperm(cols, generator=gen)[:6]
    gamma = torch.rand(cols, generator=gen) * 1.5 + 0.2
    weight = torch.rand(cols, generator=gen) * 1.5 + 0.2
    bias = torch.randn(cols, generator=gen) * 0.3
    if cls == "outliers":
        x[:, idx] *= 20.0
    elif cls in ("offset10", "offset1e3"):
        (hidden if use_hidden else x).add_(10.0 if cls == "offset10" else 1e3)
    elif cls == "spike":
        x[torch.arange(rows), torch.randint(0, cols, (rows,), generator=gen)] = 1e4
    elif cls == "tiny":
        x *= 1e-20
        hidden *= 1e-20
    elif cls == "huge":
        x *= 1e15
        hidden *= 1e15
    elif cls == "gamma_outliers":
        special = torch.tensor([6.0, 4.5, 0.05])[:min(3, cols)]
        gamma[idx[:3]] = special
        weight[idx[:3]] = special
    return (x, hidden if use_hidden else None, gamma if (use_hidden and use_gamma) else None,
            weight if use_weight else None, bias if use_bias else None)


def eager_layernorm(r, weight, bias, eps):
    """The eager sequence of the wrappers on a formed residual r (torch tensor, any device): nn.LayerNorm with its affine
    pair (QuantizedLayerNorm), or the non-scaling LayerNorm followed by ``+= bias`` (QuantizedSplitLayerNorm)."""
    import torch.nn.functional as F
    h = r.shape[-1]
    if weight is not None:
        return F.layer_norm(r, (h,), weight, bias, eps)
    y = F.layer_norm(r, (h,), None, None, eps)
    if bias is not None:
        y = y + bias
    return y


def distinct_rows(k, cols, gen, scale=1.0):
    return torch.randn(k, cols, generator=gen) * scale * (1.0 + torch.arange(k, dtype=torch.float32)[:, None] * 0.25)


def row_map(rows, k, seed):
    """Row i of the large tensor is distinct row perm(i) mod k, for a seeded permutation of range(rows)."""
    return torch.randperm(rows, generator=torch.Generator().manual_seed(seed)) % k


# ---------------------------------------------------------------------------------------------------------------------
# softmax site: cases and input recipes
# ---------------------------------------------------------------------------------------------------------------------

SM_REGISTER_WIDTHS = (4, 8, 252, 256, 260, 508, 512, 516, 1020, 1024, 1028, 2044, 2048)   # R in 1,2,4,8, full and ragged
SM_GENERIC_WIDTHS = (6, 255, 1023, 2052, 4100)
SM_PRE = (("plain", {}), ("scale", {"alpha": 0.125}), ("divide", {"divisor": math.sqrt(48.0)}))
SM_KINDS = ("peaked", "flat")
SM_SHAPE = (2, 2, 12)               # batch, heads, queries of an accuracy case


def softmax_template_r(cols):
    per_lane = (cols // 4 + 63) // 64
    for r in (1, 2, 4, 8):
        if per_lane <= r:
            return r
    raise ValueError(cols)


def softmax_inputs(cols, kind, pre, seed=0):
    """(scores [B,h,T,S], mask [B,1,T,S]) as torch fp32 CPU tensors.  peaked: the tests/_attention_site.py recipe (pre-softmax
    values ~ 2 * randn with three hot keys + 4); flat: values within 0.02 of each other.  The mask hides a tail of every
    row -- with -inf in sample 0 (BART's causal value), -10000 in sample 1 (BERT's padding value) -- never the whole row."""
    b, h, t = SM_SHAPE
    gen = torch.Generator().manual_seed(104729 * cols + 17 * SM_KINDS.index(kind) + 5 * [p[0] for p in SM_PRE].index(pre[0]) + seed)
    back = 1.0 / pre[1]["alpha"] if "alpha" in pre[1] else pre[1].get("divisor", 1.0)     # undo the pre-softmax step
    if kind == "peaked":
        scores = torch.randn(b, h, t, cols, generator=gen) * (2.0 * back)
        hot = torch.randint(0, cols, (3,), generator=gen)
        scores[..., hot] += 4.0 * back
    else:
        scores = torch.randn(b, h, t, cols, generator=gen) * (0.01 * back)
    valid = torch.randint(1, cols + 1, (b, 1, t, 1), generator=gen)
    hidden = torch.arange(cols).view(1, 1, 1, cols) >= valid
    mask = torch.zeros(b, 1, t, cols)
    mask[0:1].masked_fill_(hidden[0:1], float("-inf"))
    mask[1:2].masked_fill_(hidden[1:2], -10000.0)
    return scores, mask


def softmax_edge_rows(cols, gen):
    """(scores [5, S], mask [5, S]): the edge rows of test_edge_rows_match_torch_cpu -- a NaN, a +inf, all -inf (through
    the mask), finfo.min on the whole row (through the mask), half the row -inf."""
    s = torch.randn(5, cols, generator=gen) * 4
    m = torch.zeros(5, cols)
    s[0, cols - 1] = float("nan")
    s[1, 0] = float("inf")
    m[2, :] = float("-inf")
    m[3, :] = torch.finfo(torch.float32).min
    m[4, cols // 2:] = float("-inf")
    return s, m


# ---------------------------------------------------------------------------------------------------------------------
# GELU site: inputs, integer reference, tie neighbourhood
# ---------------------------------------------------------------------------------------------------------------------

GELU_QUANT = ((0.037, 17, 6), (0.11, 29, 6), (0.0041, 40, 8))       # scale, zero point, bits
GELU_TIE_SHARE = 2e-3               # largest share of entries the tie neighbourhood may cover, per (input, scale)


def _ladder(lo, hi, step=64):
    """Every ``step``-th fp32 value of [lo, hi] (both of one sign): consecutive bit patterns are consecutive values."""
    a, b = np.array([lo, hi], dtype=F32).view(np.int32)
    a, b = (a, b) if a <= b else (b, a)
    return np.arange(int(a), int(b) + 1, step, dtype=np.int64).astype(np.int32).view(F32)


def gelu_inputs():
    """name -> fp32 array: 2**22 draws of 3 * randn; the dense ladders through the 1 + erf cancellation tail [-6, -2] and
    through [2**-10, 2]."""
    gen = torch.Generator().manual_seed(4201)
    return {
        "randn3": (torch.randn(1 << 22, generator=gen) * 3).numpy(),
        "ladder_tail": np.ascontiguousarray(_ladder(-6.0, -2.0)),
        "ladder_rise": np.ascontiguousarray(_ladder(2.0 ** -10, 2.0)),
    }


GELU_SPECIALS = (0.0, -0.0, 1e-40, -1e-40, 40.0, -40.0, float("inf"), float("-inf"), float("nan"))


def gelu_special_inputs():
    """[(x, positions)]: fp32 tensors of 3 * randn whose length leaves a scalar tail behind the float4 body (n % 4 == 3),
    with every special value at the head and in the vector body (starting off a float4 boundary, so that each of the four
    slots sees them), and, three at a time, in the three tail positions."""
    gen = torch.Generator().manual_seed(4202)
    sp = np.array(GELU_SPECIALS, dtype=F32)
    k = len(sp)
    n = 4096 + 3
    x = (torch.randn(n, generator=gen) * 3).numpy()
    pos = []
    for start in (0, 1029):
        x[start:start + k] = sp
        pos.extend(range(start, start + k))
    out = [(x, np.array(pos))]
    for j in range(0, k, 3):
        n = 1024 + 3
        x = (torch.randn(n, generator=gen) * 3).numpy()
        x[n - 3:] = sp[j:j + 3]
        out.append((x, np.arange(n - 3, n)))
    return out


def effective_params(scale, zp, bits, lsqplus, numel):
    """(s, z, qmin, qmax, grad_factor): the fp32 scale and zero point that reach the quantizer -- the values themselves
    (Fixed, int32 zero point) or after LSQ+'s round_ste / grad_scale (oracle/fake_quant_oracle.py)."""
    from oracle import fake_quant_oracle as FQ
    qmax = 2 ** bits - 1
    if not lsqplus:
        return F32(scale), F32(zp), 0, qmax, 1.0
    gf = FQ.lsqplus_grad_factor(numel, qmax)
    s, z = FQ.lsqplus_effective_params(F32(scale), F32(zp), gf)
    return F32(s), F32(z), 0, qmax, gf


def gelu_q64(g64, s, z, qmin, qmax):
    """(q64, distance): clamp(rint(g64 / s) + z) in float64 and each entry's distance |frac(g64 / s) - 1/2| * s from the
    nearest rounding boundary, in units of the GELU's value."""
    u = g64 / float(s)
    q = np.clip(np.rint(u) + float(z), qmin, qmax)
    dist = np.abs((u - np.floor(u)) - 0.5) * float(s)
    return q, dist


def gelu_delta(x):
    """2 x the largest |F.gelu (CPU fp32) - gelu_f64| on x: the half-width of the tie neighbourhood."""
    import torch.nn.functional as F
    g32 = F.gelu(torch.from_numpy(np.ascontiguousarray(x))).numpy().astype(np.float64)
    return 2.0 * float(np.abs(g32 - gelu_f64(x)).max())


def integers_of(y, s, z):
    """The integer tensor behind a fake-quantised y: y / s + z rounded (util_quant.py:14 inverted exactly)."""
    return np.rint(np.asarray(y, dtype=np.float64) / float(s) + float(z))

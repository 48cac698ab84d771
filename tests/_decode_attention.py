"""Float64 restatement of the attention of one decoding step (the reference's quant_bart.py:232-268 for one query token)
and TIE-FREE inputs for it: what tests/test_oracle_decode_attention.py (CPU) and tests/test_gpu_decode_attention.py share.

    s[j] = dot(q, k[j]) + mask[j];  p = softmax(s);  p' = fq_probs(p);  c = sum_j p'[j] * v[j];  out = fq_ctx(c)

Two fp32 evaluations of this chain that add in different orders give different last bits of p and c, and a fake-quantizer
turns a last-bit difference into a whole quantization step wherever ``u = value / scale`` sits on a rounding tie
(n + 0.5).  So the cases here are chosen such that no fp32 evaluation can reach a tie:

  * every quantity is computed in float64, together with a forward error bound ``g`` on the ``u`` that goes into ``rint``,
    valid for ANY fp32 summation order: gamma_n * sum|terms| for the two dot products (n = head_dim resp. kv_len,
    gamma_n = n u / (1 - n u), u = 2^-24), 4 ulp for expf, one rounding each for the subtraction of the row maximum, the
    reciprocal, the product with it and the division by the scale, propagated through the softmax;
  * a seeded case is kept only if every |u - nearest tie| > 4 g, else the next seed is tried.  The factor of four covers
    what the bound leaves out (the rounding of p' into c is in it; second-order terms and the difference between expf
    implementations are not).

On such inputs every correct fp32 evaluation yields the float64 integer codes exactly, and its outputs are
``(code - zp) * scale`` in fp32, word for word.  The bound is checked on the CPU (torch's eager sequence in two summation
orders), not on the kernel under test.

Masks hold 0 and finfo(float32).min only: ``dot + finfo.min`` is finfo.min in fp32 and in float64 alike (the dot is far
below half an ulp of it), so a masked score carries no error."""
import functools
from collections import namedtuple

import numpy as np

F32 = np.float32
U = 2.0 ** -24
FMIN = float(np.finfo(np.float32).min)
EPS32 = np.float32(np.finfo(np.float32).eps)

HEAD_DIMS = (16, 64, 128)
QUANTS = (("asym6", "fixed"), ("asym6", "lsqplus"), ("sym8", "fixed"), ("sym8", "lsqplus"))
MASKS = ("none", "pad", "full")
CAPS = ("eq", "plus7", "differ")
RANGES = {"asym6": (0, 63), "sym8": (-128, 127)}

Case = namedtuple("Case", "head_dim kv_len batch heads bits mode bad_params mask cap")


def rows_per_wave(head_dim):
    return 64 // (head_dim // 4)


def kv_lens(head_dim):
    """1: softmax of one; 3: less than one wave's rows; either side of one trip of the four waves; a second trip with a ragged
    tail; and one position more than four trips + one wave's rows (the kernel keeps four trips of loads in flight)."""
    r = rows_per_wave(head_dim)
    return (1, 3, 4 * r - 1, 4 * r, 4 * r + 1, 2 * 4 * r + 5, 4 * 4 * r + r + 1)


def table(head_dim):
    """The cases of one head size: every kv_len x batch*heads in {1, 6} x the four quantizer variants; the mask and cap
    variants and the bad raw parameters (negative scale, out-of-range zero point: LSQ+ only) rotate through them."""
    out = []
    for kv in kv_lens(head_dim):
        for batch, heads in ((1, 1), (2, 3)):
            for bits, mode in QUANTS:
                i = len(out)
                mask = MASKS[i % 3]
                out.append(Case(head_dim, kv, batch, heads, bits, mode, mode == "lsqplus" and (i // 4) % 2 == 1, mask,
                                CAPS[(i // 3) % 3]))
    return out


LIMIT_CASE = Case(16, 4096, 1, 1, "asym6", "lsqplus", False, "pad", "plus7")


def gamma(n):
    return n * U / (1 - n * U)


def grad_scale_value(t, g):
    t = F32(t)
    tg = t * F32(g)
    return F32(F32(t - tg) + tg)


class QuantGroup:
    """One quantizer of the site: the raw parameters as they are handed over, what OSQ_PARAM_SANITIZE leaves in them, and
    the effective (scale, zero point) that reach the quantizer (util_quant.py:48-51, fake_quant.py:188-191), all fp32."""

    def __init__(self, bits, mode, scale, zero_point, numel, bad):
        self.qmin, self.qmax = RANGES[bits]
        self.mode = mode
        self.grad_factor = float(F32(1.0 / (numel * self.qmax) ** 0.5)) if mode == "lsqplus" else 1.0
        self.scale_after, self.zp_after = F32(scale), F32(zero_point)
        self.scale_raw, self.zp_raw = self.scale_after, self.zp_after
        if mode == "lsqplus":
            if bad:
                self.scale_raw = F32(-self.scale_after)
            s = F32(max(abs(self.scale_raw), EPS32))
            z = F32(min(max(self.zp_raw, F32(self.qmin)), F32(self.qmax)))
            self.scale_after, self.zp_after = s, z
            z = F32(F32(np.round(z) - z) + z)
            self.scale_eff, self.zp_eff = grad_scale_value(s, self.grad_factor), grad_scale_value(z, self.grad_factor)
        else:
            self.scale_eff, self.zp_eff = self.scale_after, self.zp_after

    def quantize(self, u64):
        """fp32 x_quant (the integer codes, as util_quant.py:12-13 holds them) and the dequantised fp32 value for float64 u."""
        r = np.rint(u64)
        assert np.abs(r).max() < 2 ** 24
        x_int = r.astype(F32) + self.zp_eff
        xq = np.clip(x_int, F32(self.qmin), F32(self.qmax))
        return xq, ((xq - self.zp_eff) * self.scale_eff).astype(F32)


def tie_margin(u, g):
    """min over the entries of |u - nearest tie| - 4 g: positive = tie-free."""
    return float((np.abs(u - (np.floor(u) + 0.5)) - 4 * g).min())


def build_mask(case, rng):
    b, s = case.batch, case.kv_len
    if case.mask == "none":
        return None
    m = np.zeros((b, 1, 1, s), F32)
    for i in range(b):
        keep = s if s < 2 else int(rng.integers(1, s))           # a padding tail on every row ...
        m[i, 0, 0, keep:] = FMIN
    if case.mask == "full":
        m[b - 1] = FMIN                                           # ... and one row masked altogether
    return m


def evaluate(case, seed):
    rng = np.random.default_rng(seed)
    b, h, d, s = case.batch, case.heads, case.head_dim, case.kv_len
    # the model's query carries head_dim ** -0.5 (quant_bart.py:154); the softmax sharpens with kv_len, so that the sum of
    # all u of a row (1 / scale: what the relative part of the bound multiplies) stays of a size at which seeds pass.  At
    # the limit less so: about 170 of the 4096 probabilities keep a non-zero code
    q = (rng.standard_normal((b, h, 1, d)) * (d ** -0.5 * (1 + (0.3 if s < 1024 else 0.12) * np.log2(s)))).astype(F32)
    k = rng.standard_normal((b, h, s, d)).astype(F32)
    v = rng.standard_normal((b, h, s, d)).astype(F32)
    mask = build_mask(case, rng)
    q64, k64, v64 = q.astype(np.float64)[:, :, 0], k.astype(np.float64), v.astype(np.float64)

    # ---- scores and their bound
    dot = np.einsum("bhd,bhsd->bhs", q64, k64)
    err_s = gamma(d) * np.einsum("bhd,bhsd->bhs", np.abs(q64), np.abs(k64))
    if mask is not None:
        assert np.isin(mask, (0.0, F32(FMIN))).all()
        masked = np.broadcast_to(mask[:, :, 0] != 0, dot.shape)
        dot = np.where(masked, FMIN, dot)
        err_s = np.where(masked, 0.0, err_s)
    # ---- softmax: any constant may be subtracted, the kernel's is the maximum of ITS scores
    x = dot - dot.max(-1, keepdims=True)
    delta = err_s + U * (np.abs(x) + 2 * err_s.max(-1, keepdims=True))
    e = np.exp(x)
    err_e = e * (np.expm1(np.minimum(delta, 50.0)) + 8 * U) + 2.0 ** -148
    total = e.sum(-1, keepdims=True)
    err_total = gamma(s) * total + err_e.sum(-1, keepdims=True)
    rel_r = err_total / (total - err_total) + U
    p = e / total
    err_p = 1.01 * (err_e / total * (1 + rel_r) + p * (rel_r + U))
    # ---- probabilities quantizer
    bits_mode = (case.bits, case.mode)
    pmax = float(p.max())
    if case.bits == "asym6":
        pq = QuantGroup(*bits_mode, pmax / 63 * 1.05, 3, b * h * s, case.bad_params)
    else:
        pq = QuantGroup(*bits_mode, pmax / 127 * 0.9, 0, b * h * s, case.bad_params)
    u_p = p / float(pq.scale_eff)
    g_p = err_p / float(pq.scale_eff) + np.abs(u_p) * U
    p_codes, p_fq = pq.quantize(u_p)
    # ---- context and its bound (p' is exact once the codes are)
    terms = p_fq.astype(np.float64)[..., None] * v64
    c = terms.sum(2)
    err_c = gamma(s) * np.abs(terms).sum(2)
    cmax = max(float(np.abs(c).max()), 1e-3)
    if case.bits == "asym6":
        cq = QuantGroup(*bits_mode, cmax / 30 * 0.9, 31, b * h * d, False)
    else:
        cq = QuantGroup(*bits_mode, cmax / 127 * 0.9, 0, b * h * d, False)
    if case.bad_params:      # a negative scale and a zero point below the range: clamped to quant_min by the repair
        cq = QuantGroup(*bits_mode, -cq.scale_raw, cq.qmin - 4, b * h * d, True)
    u_c = c / float(cq.scale_eff)
    g_c = err_c / float(cq.scale_eff) + np.abs(u_c) * U
    c_codes, c_fq = cq.quantize(u_c)
    margin = min(tie_margin(u_p, g_p), tie_margin(u_c, g_c))
    return dict(case=case, seed=seed, q=q, k=k, v=v, mask=mask, probs_q=pq, ctx_q=cq, probs_codes=p_codes[:, :, None, :],
                probs=p_fq[:, :, None, :], ctx_codes=c_codes, out=c_fq.reshape(b, 1, h * d), margin=margin,
                p64=p, err_p=err_p, ctx64=c, err_ctx=err_c,      # float64 probabilities / context (from p') and their bounds
                worst_g=max(float(g_p.max()), float(g_c.max())))


@functools.lru_cache(maxsize=None)
def reference(case):
    """The first tie-free seeded instance of ``case`` (computed once per process; callers must not modify it)."""
    base = sum((i + 1) * int(f) for i, f in enumerate(case[:4])) + 7 * QUANTS.index((case.bits, case.mode))
    for seed in range(base * 100, base * 100 + 100):
        r = evaluate(case, seed)
        if r["margin"] > 0:
            return r
    raise AssertionError(f"no tie-free instance of {case} in 100 seeds")

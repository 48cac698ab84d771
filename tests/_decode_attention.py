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
below half an ulp of it), so a masked score carries no error.

The CODED variant (``Case.coded``) draws K and V as bytes of integer codes with a record (scale_eff, zp_eff, quant_min) per
tensor, as the coded KV cache holds them, and forms their fp32 values in numpy as
``((u + quant_min).astype(float32) - zp_eff) * scale_eff``: two correctly rounded fp32 operations (util_quant.py:14), the
word the fp32 cache holds.  The rest of the chain is the same.  Fixed cases hold 6-bit codes (quant_min 0), LSQ+ cases
8-bit ones (quant_min -128); the zero points are fractional -- an LSQ+ effective zero point is rounded before use, so the
fraction only tests the arithmetic.

ONE case, RELAXED_CASE (head_dim 256 at the limit of 4096), has no tie-free instance within reach: almost every entry is
clear of a tie and a few are not.  It is compared by ``sure_entries``: words where u is further than 4 g from a tie, at
most one quantization step elsewhere."""
import functools
from collections import namedtuple

import numpy as np

F32 = np.float32
U = 2.0 ** -24
FMIN = float(np.finfo(np.float32).min)
EPS32 = np.float32(np.finfo(np.float32).eps)

HEAD_DIMS = (4, 8, 16, 32, 64, 128, 256)
QUANTS = (("asym6", "fixed"), ("asym6", "lsqplus"), ("sym8", "fixed"), ("sym8", "lsqplus"))
MASKS = ("none", "pad", "full")
CAPS = ("eq", "plus7", "differ")
RANGES = {"asym6": (0, 63), "sym8": (-128, 127)}

SEED_BUDGET = 1000          # seeds tried per case, in order: the first hit stays the first hit whatever the budget

Case = namedtuple("Case", "head_dim kv_len batch heads bits mode bad_params mask cap coded", defaults=(False,))

# the record (scale_eff, zp_eff, quant_min) of K and of V, by the width of the codes.  V's zero point sits low in the range
# (values of about -0.4 .. 2.4): a row masked altogether averages V over up to 4096 positions, and an average near zero of
# terms near one leaves an 8-bit context grid no seed that is clear of a tie
KV_RECORDS = {6: ((0.06, 31.25, 0), (0.045, 9.5, 0)), 8: ((0.015, 3.25, -128), (0.011, -90.5, -128))}


def rows_per_wave(head_dim):
    return 64 // (head_dim // 4)


def trips_in_flight(coded):
    """Trips of loads the kernel issues before it reduces the first: KvWords::kInFlight / KvCodes::kInFlight."""
    return 16 if coded else 4


def kv_lens(head_dim, coded=False):
    """1: softmax of one; 3: less than one wave's rows; either side of one trip of the four waves; a second trip with a ragged
    tail; and one position more than the trips of loads in flight + one wave's rows (four trips for fp32 words; sixteen for
    code bytes, where that fits below the limit of 4096: the rule of tests/test_gpu_kv_codes.py::kv_lens)."""
    r = rows_per_wave(head_dim)
    return (1, 3, 4 * r - 1, 4 * r, 4 * r + 1, 2 * 4 * r + 5, min(trips_in_flight(coded) * 4 * r + r + 1, 4096))


def geometries(head_dim):
    """(batch, heads) pairs of a table.  At head_dim 256 batch * heads = 6 asks 1536 eight-bit context codes to be clear of a
    tie at once, which no seed within reach grants; two rows of one head and one row of two heads still exercise the mask-row
    and the head arithmetic."""
    return ((2, 1), (1, 2)) if head_dim == 256 else ((1, 1), (2, 3))


def table(head_dim, coded=False):
    """The cases of one head size: every kv_len x geometry x the four quantizer variants; the mask and cap variants and the
    bad raw parameters (negative scale, out-of-range zero point: LSQ+ only) rotate through them."""
    out = []
    for kv in kv_lens(head_dim, coded):
        for batch, heads in geometries(head_dim):
            for bits, mode in QUANTS:
                i = len(out)
                mask = MASKS[i % 3]
                out.append(Case(head_dim, kv, batch, heads, bits, mode, mode == "lsqplus" and (i // 4) % 2 == 1, mask,
                                CAPS[(i // 3) % 3], coded))
    return out


LIMIT_CASE = Case(16, 4096, 1, 1, "asym6", "lsqplus", False, "pad", "plus7")
# the limit at the other head sizes: R = 64 gives 16 trips of 256 positions, R = 1 (head_dim 256) 256 trips at 1024
LIMIT_CASES = (LIMIT_CASE,) + tuple(LIMIT_CASE._replace(head_dim=d, kv_len=s) for d, s in ((4, 4096), (8, 4096), (32, 4096), (256, 1024)))
# 1024 trips of four positions: no tie-free instance in 600 seeds (best margin -0.0025).  reference() gives the first instance
# whose probabilities are tie-free; a few of its 256 context codes are not, and the context is compared by sure_entries()
RELAXED_CASE = LIMIT_CASE._replace(head_dim=256, kv_len=4096)


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


# share of the code range K is drawn from at head_dim 256: uniform codes are wider than a normal K, and 256-term scores
# under an 8-bit probability grid leave no tie-free seed at the full range (narrowed until every case has an instance)
K_CODE_SPAN_256 = 0.25


def dequantize_codes(codes, record):
    """fp32 values of code bytes under a record: ((u + quant_min) as fp32 - zp_eff) * scale_eff, each operation rounded once."""
    scale_eff, zp_eff, quant_min = record
    return ((codes.astype(np.int32) + quant_min).astype(F32) - F32(zp_eff)) * F32(scale_eff)


def draw_codes(rng, shape, record, span):
    """Uniform code bytes from the middle ``span`` of the record's range (6-bit: bytes 0..63; 8-bit: 0..255) and their values."""
    n = 64 if record[2] == 0 else 256
    half = max(1, int(round(n * span / 2)))
    codes = rng.integers(n // 2 - half, n // 2 + half, shape).astype(np.uint8)
    values = dequantize_codes(codes, record)
    assert values.dtype == F32
    return codes, values


def evaluate(case, seed):
    rng = np.random.default_rng(seed)
    b, h, d, s = case.batch, case.heads, case.head_dim, case.kv_len
    # the model's query carries head_dim ** -0.5 (quant_bart.py:154); the softmax sharpens with kv_len, so that the sum of
    # all u of a row (1 / scale: what the relative part of the bound multiplies) stays of a size at which seeds pass.  At
    # the limit less so: about 170 of the 4096 probabilities keep a non-zero code
    # (coded cases keep the sharper factor at every length: their context bound counts non-zero terms only, see below)
    sharpen = 0.3 if s < 1024 or case.coded else 0.12
    q =(rng.standard_normal((b, h, 1, d)) * (d ** -0.5 * (1 + sharpen * np.log2(s)))).astype(F32)
    coded = {}
    if case.coded:
        k_rec, v_rec = KV_RECORDS[8 if case.mode == "lsqplus" else 6]
        k_codes, k = draw_codes(rng, (b, h, s, d), k_rec, K_CODE_SPAN_256 if d == 256 else 1.0)
        v_codes, v = draw_codes(rng, (b, h, s, d), v_rec, 1.0)
        coded = dict(k_codes=k_codes, v_codes=v_codes, k_record=k_rec, v_record=v_rec)
    else:
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
    # coded cases reach kv_len 4096 at batch * heads = 6, where gamma(kv_len) alone covers a seventh of an 8-bit step: there
    # the bound counts the terms that round at all (adding an exact zero, a position whose p' is 0, rounds nothing).  The
    # fp32 cases keep the coarser gamma(kv_len) their instances were found under.
    n_terms = np.maximum((p_fq != 0).sum(-1), 1)[..., None] if case.coded else s
    err_c = gamma(n_terms) * np.abs(terms).sum(2)
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
                worst_g=max(float(g_p.max()), float(g_c.max())),
                probs_margin=tie_margin(u_p, g_p), u_ctx=u_c, g_ctx=g_c, **coded)


def sure_entries(ref):
    """For RELAXED_CASE, whose context is not tie-free: ``sure`` [B, 1, h * d], true where the float64 u of the context is
    further than 4 g from a tie -- there every correct fp32 evaluation has the float64 code -- and the largest 4 g of the
    other entries: while that stays below 0.5 such an entry is at most one quantization step off.  (The probabilities of
    the instance ARE tie-free, so p' is exact and the context's bound holds as it stands.)"""
    case = ref["case"]
    assert ref["probs_margin"] > 0
    u, g = ref["u_ctx"], ref["g_ctx"]
    sure = np.abs(u - (np.floor(u) + 0.5)) > 4 * g
    return sure.reshape(case.batch, 1, case.heads * case.head_dim), float((4 * g)[~sure].max(initial=0.0))


def first_seed(case):
    base = sum((i + 1) * int(f) for i, f in enumerate(case[:4])) + 7 * QUANTS.index((case.bits, case.mode))
    return base * 100


@functools.lru_cache(maxsize=None)
def reference(case):
    """The first tie-free seeded instance of ``case`` (computed once per process; callers must not modify it).  RELAXED_CASE
    alone has none: for it, the first instance whose PROBABILITIES are tie-free; its context goes by sure_entries()."""
    first = first_seed(case)
    for seed in range(first, first + SEED_BUDGET):
        r = evaluate(case, seed)
        if (r["probs_margin"] if case == RELAXED_CASE else r["margin"]) > 0:
            return r
    raise AssertionError(f"no tie-free instance of {case} in {SEED_BUDGET} seeds")


# ---- non-finite inputs: NaN and infinity as DATA.  What each does is a property of the formula, stated here as a pattern
# and checked against the eager fp32 sequence on the CPU (tests/test_oracle_decode_attention.py) before any kernel sees it.
NONFINITE_KINDS = ("nan_k", "nan_q", "inf_k", "neg_inf_some", "neg_inf_row", "nan_v_at_zero_prob")
NONFINITE_AT = (1, 1)          # the (batch row, head) that is touched


def nonfinite_cases():
    """head_dim 4 / 64 / 256 (LPR 1 / 16 / 64), batch x heads 2 x 3, kv_len 3 and one position beyond a trip; a padding mask."""
    return [Case(d, s, 2, 3, "asym6", "fixed", False, "pad", "plus7") for d in (4, 64, 256) for s in (3, kv_lens(d)[4])]


def nonfinite(ref, kind):
    """The inputs of a tie-free instance with one non-finite change, and what the formula makes of it:

      nan_k / nan_q   one NaN in position 0 of K, or in q, of NONFINITE_AT: its score is NaN, so is the sum of the exps, so are
                      all probabilities of that (b, h) and its head_dim columns of out;
      inf_k           +inf in K under a positive element of q: the score is +inf and so the maximum; inf - inf is NaN: the same;
      neg_inf_some    -inf at the odd positions of mask row 0: exp(-inf) is the 0 that exp(finfo.min - max) is, so the words
                      are those of ``twin_mask``, which holds finfo.min there;
      neg_inf_row     mask row 1 is -inf everywhere: the maximum is -inf, -inf - -inf is NaN: every head of that batch row is
                      NaN (finfo.min instead gives the uniform row);
      nan_v_at_zero_prob   one NaN in V at the last position, which the padding mask gives probability 0 and the asymmetric
                      quantizer the value (zp - zp) * scale = 0: 0 * NaN is NaN in that one column of out, nothing else.

    Returns dict(q, k, v, mask, twin_mask, nan_probs [B, h, 1, S] bool, nan_out [B, 1, h * d] bool): every word outside the two
    NaN patterns is the clean instance's (the twin's for neg_inf_some)."""
    case = ref["case"]
    b, h, d, s = case.batch, case.heads, case.head_dim, case.kv_len
    b0, h0 = NONFINITE_AT
    x = {n: ref[n].copy() for n in ("q", "k", "v", "mask")}
    x["twin_mask"] = None
    nan_probs, nan_out = np.zeros((b, h, 1, s), bool), np.zeros((b, h, d), bool)
    if kind in ("nan_k", "nan_q", "inf_k"):
        col = int(np.argmax(x["q"][b0, h0, 0]))                     # a positive element of q: +inf * it is +inf
        assert x["q"][b0, h0, 0, col] > 0
        if kind == "nan_q":
            x["q"][b0, h0, 0, col] = np.nan
        else:
            x["k"][b0, h0, 0, col] = np.nan if kind == "nan_k" else np.inf
        nan_probs[b0, h0], nan_out[b0, h0] = True, True
    elif kind == "neg_inf_some":
        assert x["mask"][0, 0, 0, 0] == 0
        x["twin_mask"] = x["mask"].copy()
        x["mask"][0, 0, 0, 1::2] = -np.inf
        x["twin_mask"][0, 0, 0, 1::2] = FMIN
    elif kind == "neg_inf_row":
        x["mask"][1] = -np.inf
        nan_probs[1], nan_out[1] = True, True
    else:
        assert kind == "nan_v_at_zero_prob" and ref["probs"][b0, h0, 0, s - 1] == 0
        x["v"][b0, h0, s - 1, d - 1] = np.nan
        nan_out[b0, h0, d - 1] = True
    x["nan_probs"], x["nan_out"] = nan_probs, nan_out.reshape(b, 1, h * d)
    return x

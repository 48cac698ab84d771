"""Float64 restatement of an attention block over a whole sequence (quant_bert.py:169-188, quant_bart.py:232-268 for T
query tokens) with a per-entry error bound, and the case tables that tests/test_oracle_attention_block*.py (CPU) and
tests/test_gpu_attention_block*.py share: ``table`` (the tile edges of T and S) and ``edge_table`` (the S classes of the
kernel and the boundaries of its score and context loops, with masks of every stride pattern and finite mask values).

    s[j] = dot(q[t], k[j]);  v[j] = pre(s[j]) + mask[t, j];  p = softmax(v);  p' = fq_probs(p)
    c    = sum_j p'[j] * V[j];  out = fq_ctx(c) in the merged [B, T, h * d] layout

As in tests/_decode_attention.py (whose gamma, QuantGroup and mask conventions are imported, not copied) every quantity is
computed in float64 together with a bound ``g`` on the value ``u`` that goes into ``rint``, valid for ANY fp32 summation
order, fused multiply-adds included (they round less, not more): gamma_n * sum|terms| for the two products, 4 ulp for expf,
one rounding each for the scaling, the subtraction of the row maximum, the reciprocal, the product with it and the division
by the scale, propagated through the softmax.

A table of T x S x head_dim up to S = 1024 has no tie-free instances within reach of a seed search, so EVERY case goes by
the rule of DA.sure_entries: where ``|u - nearest tie| > 4 g`` a correct fp32 evaluation has the float64 integer code and
its output is ``(code - zp) * scale`` word for word; elsewhere it is at most one quantization step off.  The share of
entries that are not sure is capped (UNSURE_CAP, a condition on the CASES: a case that cannot meet it takes the next seed).

The context is restated from the PROBABILITY WORDS of the evaluation under test (its own p', exact fp32 numbers) times V:
a probability that sits near a tie cannot spoil the context comparison, whose bound is that of the second product alone.

A quantizer that is None passes its values through; they are then compared with the float64 value within 4 x the bound."""
import functools
from collections import namedtuple

import numpy as np

from _decode_attention import F32, FMIN, QUANTS, U, QuantGroup, gamma

TQ = 32                     # ops.ATTENTION_TQ / kBlkTQ of csrc/attention_block.hip (tests/test_gpu_attention_block.py asserts it)
TK = 32                     # ops.ATTENTION_TK / kBlkTK
HEAD_DIMS = (16, 32, 64, 128)
TOKENS = (1, TQ - 1, TQ, TQ + 1, 2 * TQ + 3)
KV_LENS = (1, 3, TK - 1, TK, TK + 1, 2 * TK + 5, 1024)
GEOMETRIES = ((1, 1), (2, 3))
MASKS = ("none", "pad", "causal")          # pad: [B, 1, 1, S]; causal: causal + pad, [B, 1, T, S]
PRES = ("none", "alpha", "divisor")
SITES = ("both", "both", "no_probs", "no_ctx", "neither")     # which quantizers the launch gets
UNSURE_CAP = 0.10
SELECT_CAP = 0.07           # what an instance is chosen under: the context is restated from the words under test, and a few
                            # entries may change sides between two evaluations
SEED_BUDGET = 20

# ---- the edge table: lengths chosen from the constants of csrc/attention_block.hip, not from the workload
WAVES = 4                   # kBlkWaves: key tiles go round them; the context's steps are split among WAVES / chunks segments
IN_FLIGHT = 16              # kBlkInFlight: steps of the context a lane loads at once, one batch ahead
S_CLASSES = (128, 256, 512, 1024)          # floats of LDS per score row: one kernel instance each
# 9: five steps, split 2 2 1 0 among four segments, 3 2 among two; 63..65 and 127..129: a segment of IN_FLIGHT steps and of
# one more with two and with four segments (with fewer segments: of two batches and of one step more); 128/129, 256/257,
# 512/513: the class switches, 129 and 257 also the first key tile past one and past two rounds of the waves; 127, 255, 511,
# 1023: the odd tops of the classes, where position S (the +0 partner of the last step) is the last word of the score row
EDGE_KV_LENS = (9, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023)
EDGE_TOKENS = (1, TQ + 1)
# head: [1, h, T, S] (batch stride 0, head stride not); bias: [B, h, T, S] of finite values; neginf: [1, 1, T, S] with -inf
EDGE_MASKS = ("head", "bias", "neginf", "none", "pad", "causal")
EDGE_PRES = ("none", "alpha", "divisor", "alpha_d")           # alpha_d: float32(d ** -0.5) as it is, a power of two or not

Case = namedtuple("Case", "head_dim tokens kv_len batch heads bits mode bad_params mask pre sites")


def table(head_dim):
    """T x S of one head size; geometry, the four quantizer variants, bad raw parameters (LSQ+ only), masks, pre-scaling and
    absent quantizers rotate through them."""
    out = []
    for t in TOKENS:
        for s in KV_LENS:
            i = len(out)
            bits, mode = QUANTS[i % 4]
            batch, heads = GEOMETRIES[(i // len(KV_LENS) + i % len(KV_LENS)) % 2]
            out.append(Case(head_dim, t, s, batch, heads, bits, mode, mode == "lsqplus" and (i // 4) % 2 == 1, MASKS[i % 3],
                            PRES[(i // 3) % 3], SITES[i % 5]))
    return out


def segments(head_dim):
    """Segments the context's steps are split into: a wave per 32-column chunk of the context and segment."""
    return WAVES // max(head_dim // 32, 1)


def steps_per_segment(head_dim, kv_len):
    """``per`` of the kernel's context loop: ceil(S / 2) steps (the matrix instruction sums two positions), split evenly."""
    return -(-(-(-kv_len // 2)) // segments(head_dim))


def key_tiles(kv_len, tk=TK):
    """``ktiles`` of the kernel's score loop."""
    return -(-kv_len // tk)


def s_class(kv_len):
    """The kernel instance a length runs: the smallest class that holds its score row."""
    return next(c for c in S_CLASSES if kv_len <= c)


def edge_table(head_dim):
    """EDGE_TOKENS x EDGE_KV_LENS of one head size.  Geometry, quantizers, bad parameters and sites rotate as in table(); the
    six masks start at the head size's index and the four pre-scalings shift by one every six cases, so that over the
    table every mask meets every pre-scaling."""
    out = []
    shift = HEAD_DIMS.index(head_dim)
    for t in EDGE_TOKENS:
        for s in EDGE_KV_LENS:
            i = len(out)
            bits, mode = QUANTS[i % 4]
            batch, heads = GEOMETRIES[(i // len(EDGE_KV_LENS) + i % len(EDGE_KV_LENS)) % 2]
            out.append(Case(head_dim, t, s, batch, heads, bits, mode, mode == "lsqplus" and (i // 4) % 2 == 1,
                            EDGE_MASKS[(i + shift) % 6], EDGE_PRES[(i + i // 6) % 4], SITES[i % 5]))
    return out


def build_mask(case, rng):
    b, h, t, s = case.batch, case.heads, case.tokens, case.kv_len
    if case.mask == "none":
        return None
    if case.mask == "head":                                      # per head, about 30 % closed; position 0 stays open
        m = np.where(rng.random((1, h, t, s)) < 0.3, F32(FMIN), F32(0.0))
        m[..., 0] = 0.0
        return m
    if case.mask == "bias":                                      # a finite bias everywhere, and the -10000 of older BERT code
        m = (0.5 * rng.standard_normal((b, h, t, s))).astype(F32)
        for i in range(b):
            keep = s if s < 2 else int(rng.integers(1, s))
            m[i, :, :, keep:] = -10000.0
        return m
    if case.mask == "neginf":                                    # torch's causal mask: -inf ahead of the diagonal
        m = np.zeros((1, 1, t, s), F32)
        m[0, 0][np.arange(s)[None, :] > np.arange(t)[:, None] + max(s - t, 0)] = -np.inf
        return m
    m = np.zeros((b, 1, t if case.mask == "causal" else 1, s), F32)
    for i in range(b):
        keep = s if s < 2 else int(rng.integers(1, s))           # a padding tail on every row; position 0 stays open
        m[i, :, :, keep:] = FMIN
    if case.mask == "causal":
        ahead = np.arange(s)[None, :] > np.arange(t)[:, None] + max(s - t, 0)
        m[:, 0][np.broadcast_to(ahead, (b, t, s))] = FMIN
    return m


def pre_args(case):
    """(alpha, divisor) as the launch gets them, and the factor q is drawn with so that pre(s) has the model's size."""
    d = case.head_dim
    if case.pre == "alpha":
        alpha = 2.0 ** round(np.log2(d ** -0.5))                 # a power of two, as callers pass
        return alpha, None, d ** -0.5 / alpha
    if case.pre == "divisor":
        return None, float(F32(d ** 0.5)), 1.0
    if case.pre == "alpha_d":                                    # the model's scaling as one fp32 factor: rounds unless d is 4 ** n
        return float(F32(d ** -0.5)), None, 1.0
    return None, None, d ** -0.5


def _softmax_with_bound(dot, err_s, s):
    x = dot - dot.max(-1, keepdims=True)
    delta = err_s + U * (np.abs(x) + 2 * err_s.max(-1, keepdims=True))
    e = np.exp(x)
    err_e = e * (np.expm1(np.minimum(delta, 50.0)) + 8 * U) + 2.0 ** -148
    total = e.sum(-1, keepdims=True)
    err_total = gamma(s) * total + err_e.sum(-1, keepdims=True)
    rel_r = err_total / (total - err_total) + U
    p = e / total
    return p, 1.01 * (err_e / total * (1 + rel_r) + p * (rel_r + U))


def probabilities64(q, k, mask, alpha, divisor):
    """float64 probabilities [B, h, T, S] of fp32 inputs and their bound.  ``mask``: fp32, broadcastable to [B, h, T, S].  An
    entry <= finfo.min (-inf included) closes its position: ``dot + finfo.min`` is finfo.min in fp32 and float64 alike, the
    score carries no error, and its probability is exactly 0 while the row has an open position.  Adding a zero entry is
    exact.  Any other entry m gives dot + m, rounded once (or not at all where the add is fused into the scaling)."""
    d, s = q.shape[-1], k.shape[2]
    q64, k64 = q.astype(np.float64), k.astype(np.float64)
    dot = np.einsum("bhtd,bhsd->bhts", q64, k64)
    err_s = gamma(d) * np.einsum("bhtd,bhsd->bhts", np.abs(q64), np.abs(k64))
    if alpha is not None:
        dot, err_s = dot * alpha, err_s * alpha
        if np.frexp(alpha)[0] != 0.5:                            # a power of two is exact; any other factor rounds once
            err_s = err_s + np.abs(dot) * U
    elif divisor is not None:
        dot, err_s = dot / divisor, err_s / divisor
        err_s = err_s + np.abs(dot) * U
    if mask is not None:
        assert mask.dtype == F32 and not np.isnan(mask).any() and not (mask == np.inf).any()
        m = np.broadcast_to(mask, dot.shape)
        closed = m <= F32(FMIN)
        finite = ~closed & (m != 0)
        if finite.any():
            added = dot + np.where(finite, m, 0.0).astype(np.float64)
            dot, err_s = np.where(finite, added, dot), np.where(finite, err_s + np.abs(added) * U, err_s)
        dot = np.where(closed, FMIN, dot)
        err_s = np.where(closed, 0.0, err_s)
    return _softmax_with_bound(dot, err_s, s)


def context64(probs_words, v):
    """float64 context [B, h, T, d] of fp32 probability WORDS times fp32 V, and the bound of that product alone."""
    p64, v64 = probs_words.astype(np.float64), v.astype(np.float64)
    c = np.einsum("bhts,bhsd->bhtd", p64, v64)
    return c, gamma(v.shape[2]) * np.einsum("bhts,bhsd->bhtd", np.abs(p64), np.abs(v64))


def merged(x):
    b, h, t, d = x.shape
    return x.transpose(0, 2, 1, 3).reshape(b, t, h * d)


class Expect:
    """What a correct fp32 evaluation may give for one output: ``words`` (fp32), ``sure`` (bool: word-equal there),
    ``slack`` (how far the other entries may be off) and ``share`` of entries that are not sure."""

    def __init__(self, value64, err, group):
        if group is None:                 # no quantizer: the value itself, within 4 x its bound and its own rounding
            self.words = value64.astype(F32)
            self.sure = np.zeros(value64.shape, bool)
            self.slack = 4 * err + 2 * U * np.abs(value64) + 2.0 ** -148
            self.share, self.worst = 0.0, 0.0
            return
        u = value64 / float(group.scale_eff)
        g = err / float(group.scale_eff) + np.abs(u) * U
        self.words = group.quantize(u)[1]
        self.sure = np.abs(u - (np.floor(u) + 0.5)) > 4 * g
        # one step between neighbouring codes; each of the two words (code - zp) * scale is rounded once on its own
        step = float(group.scale_eff)
        self.slack = step + 2 * U * (np.abs(self.words.astype(np.float64)) + step)
        self.share = float(1.0 - self.sure.mean())
        self.worst = float((4 * g)[~self.sure].max(initial=0.0))      # below 0.5: an unsure entry is at most one step off

    def mismatch(self, got):
        """None, or what is wrong with fp32 ``got``."""
        if got.shape != self.words.shape or got.dtype != F32:
            return f"shape / dtype {got.shape} {got.dtype}"
        if np.isnan(got).any():
            return f"{int(np.isnan(got).sum())} NaN"
        a, b = got[self.sure], self.words[self.sure]
        if not (a == b).all():
            return f"{int((a != b).sum())} of {a.size} sure entries differ"
        off = np.abs(got.astype(np.float64) - self.words.astype(np.float64))
        if not (off <= self.slack).all():
            return f"{int((off > self.slack).sum())} entries beyond the slack, worst {float((off / self.slack).max()):.3f} of it"
        if self.share > UNSURE_CAP or self.worst >= 0.5:
            return f"unsure share {self.share:.4f} (cap {UNSURE_CAP}), largest 4 g {self.worst:.3f}"
        return None


def _groups(case, p, c):
    """The two quantizers, sized on the float64 probabilities and context of the instance (None where the case has none)."""
    b, h, t, s = p.shape
    d = case.head_dim
    bits_mode = (case.bits, case.mode)
    pmax = float(p.max())
    if case.bits == "asym6":
        pq = QuantGroup(*bits_mode, pmax / 63 * 1.05, 3, b * h * t * s, case.bad_params)
    else:
        pq = QuantGroup(*bits_mode, pmax / 127 * 0.9, 0, b * h * t * s, case.bad_params)
    cmax = max(float(np.abs(c).max()), 1e-3)
    if case.bits == "asym6":
        cq = QuantGroup(*bits_mode, cmax / 30 * 0.9, 31, b * t * h * d, False)
    else:
        cq = QuantGroup(*bits_mode, cmax / 127 * 0.9, 0, b * t * h * d, False)
    if case.bad_params:      # a negative scale and a zero point below the range: clamped to quant_min by the repair
        cq = QuantGroup(*bits_mode, -cq.scale_raw, cq.qmin - 4, b * t * h * d, True)
    return pq, cq


def evaluate(case, seed):
    rng = np.random.default_rng(seed)
    b, h, t, s, d = case.batch, case.heads, case.tokens, case.kv_len, case.head_dim
    alpha, divisor, factor = pre_args(case)
    sharpen = 0.3 if s < 1024 else 0.12                          # as DA.evaluate: the softmax sharpens with the length
    q = (rng.standard_normal((b, h, t, d)) * (factor * (1 + sharpen * np.log2(s)))).astype(F32)
    k = rng.standard_normal((b, h, s, d)).astype(F32)
    v = rng.standard_normal((b, h, s, d)).astype(F32)
    mask = build_mask(case, rng)
    p, err_p = probabilities64(q, k, mask, alpha, divisor)
    # the quantizers are sized on the float64 chain: p' of the float64 probabilities, then the context of those words
    pq, cq = _groups(case, p, context64(p.astype(F32), v)[0])
    if case.sites in ("no_probs", "neither"):
        pq = None
    else:
        _, cq = _groups(case, p, context64(pq.quantize(p / float(pq.scale_eff))[1], v)[0])
    if case.sites in ("no_ctx", "neither"):
        cq = None
    probs = Expect(p, err_p, pq)
    ref = dict(case=case, seed=seed, q=q, k=k, v=v, mask=mask, alpha=alpha, divisor=divisor, probs_q=pq, ctx_q=cq, probs=probs)
    ref["ctx"] = expect_context(ref, probs.words)               # of the float64 chain's own words: what the cap is asked of
    return ref


def expect_context(ref, probs_words):
    """Expect of the merged output [B, T, h * d] given the probability words [B, h, T, S] of the evaluation under test."""
    c, err_c = context64(probs_words, ref["v"])
    return Expect(merged(c), merged(err_c), ref["ctx_q"])


def first_seed(case):
    return 1000 * sum((i + 1) * int(f) for i, f in enumerate(case[:5])) + 7 * QUANTS.index((case.bits, case.mode))


@functools.lru_cache(maxsize=None)
def reference(case):
    """The first seeded instance of ``case`` whose two outputs keep to SELECT_CAP (below UNSURE_CAP) with every unsure entry within one step
    (computed once per process; callers must not modify it)."""
    first = first_seed(case)
    for seed in range(first, first + SEED_BUDGET):
        r = evaluate(case, seed)
        if all(e.share <= SELECT_CAP and e.worst < 0.5 for e in (r["probs"], r["ctx"])):
            return r
    raise AssertionError(f"no instance of {case} within the cap in {SEED_BUDGET} seeds")


def report():
    """The per-case unsure shares, as profiles/attention_block_accuracy.txt holds them: table(), then edge_table()."""
    lines = ["head_dim T S B h quant mask pre sites seed(+offset) | unsure share probs / ctx | largest 4 g among unsure probs / ctx"]
    for case in [c for cases in (table, edge_table) for d in HEAD_DIMS for c in cases(d)]:
        r = reference(case)
        lines.append(f"{case.head_dim} {case.tokens} {case.kv_len} {case.batch} {case.heads} {case.bits}-{case.mode}"
                     f"{'-bad' if case.bad_params else ''} {case.mask} {case.pre} {case.sites} {r['seed']}(+{r['seed'] - first_seed(case)}) | "
                     f"{r['probs'].share:.4f} {r['ctx'].share:.4f} | {r['probs'].worst:.3f} {r['ctx'].worst:.3f}")
    return "\n".join(lines)


if __name__ == "__main__":
    print(report())

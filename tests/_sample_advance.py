"""What tests/test_sample_advance_cpu.py and tests/test_gpu_sample_advance*.py share: a float64 numpy restatement of one step of
osq_sample_advance (include/osq_hip.h) -- the banned tokens, z = x / T in fp32, the survivors in contract order, their weights,
the top-p cut, the running sums and the token a uniform selects, then the pad / eos lines and the stopping word of
tests/_greedy_advance.py -- and makers of cases that assert, on the CPU, the conditions their tests rely on.

A case is a _greedy_advance case (generate()'s settings) with ``temperature``, ``top_k`` and ``top_p`` beside it."""
from types import SimpleNamespace as NS

import numpy as np

import _greedy_advance as GA

MARGIN = 1e-3          # of W: how far a planted draw, or a top-p threshold, lies from every boundary
EPS = 2e-5             # of W: the band of the kernel's fp32 sums (profiles/beam_select_accuracy.txt: the same sums)


def make(rng, bsz, vocab, max_length, cur, temperature=1.0, top_k=0, top_p=1.0, **kw):
    return dict(GA.make(rng, bsz, vocab, max_length, cur, **kw), temperature=temperature, top_k=top_k, top_p=top_p)


def banned(case, b):
    """The tokens rule 2 bans in row b at the case's cur (not the NaN ones)."""
    kw, cur, vocab = GA.kernel_arguments(case), case["cur"], case["logits"].shape[1]
    out = {int(i) for i in kw["ban_ids"] if 0 <= i < vocab}
    n = case["ngram"]
    if n > 0 and cur >= n:
        s = case["seq"][b, :cur]
        suffix = s[cur - n + 1:cur]
        for i in range(cur - n + 1):
            last = int(s[i + n - 1])
            if np.array_equal(s[i:i + n - 1], suffix) and 0 <= last < vocab:
                out.add(last)
    return out


def survivors(x, ban, temperature, top_k, top_p):
    """Rules 2-7 for one row: NS(tokens, C, W, ranked, above) -- the kept survivors in contract order, their float64 running
    sums and total; ``ranked`` the survivors before the top-p cut and ``above`` each one's sum_{j<i} w_j / sum_j w_j."""
    z = (np.asarray(x, dtype=np.float32) / np.float32(temperature)).astype(np.float64)
    out = np.isnan(z) | np.isneginf(z)
    out[list(ban)] = True
    alive = np.flatnonzero(~out)
    if top_k >= 1 or top_p < 1.0:                                       # the nucleus without top_k (the eager form) ranks every token
        order = alive[np.argsort(-z[alive], kind="stable")]            # larger first, equal values by smaller token
        alive = order[:min(top_k, len(x)) if top_k >= 1 else len(x)]
    if alive.size == 0:
        return NS(tokens=alive, C=np.zeros(0), W=0.0, ranked=alive, above=np.zeros(0))
    m = z[alive].max()
    with np.errstate(invalid="ignore"):
        w = np.where(z[alive] == m, 1.0, np.exp(z[alive] - m))
    total = w.sum()
    above = (np.cumsum(w) - w) / total
    ranked = alive
    if top_p < 1.0:
        stay = above < top_p
        stay[0] = True
        alive, w = alive[stay], w[stay]
    C = np.cumsum(w)
    return NS(tokens=alive, C=C, W=float(C[-1]), ranked=ranked, above=above)


def pick(sv, u):
    """Rule 8: the first kept survivor with C_i > u * W, the last when none; token 0 without a survivor."""
    if sv.tokens.size == 0:
        return 0, -1
    i = int(np.searchsorted(sv.C, float(u) * sv.W, side="right"))
    i = min(i, sv.tokens.size - 1)
    return int(sv.tokens[i]), i


def row(case, b):
    return survivors(case["logits"][b], banned(case, b), case["temperature"], case["top_k"], case["top_p"])


def reference_case(case, u):
    """One step with the draws ``u`` [bsz]: (token, seq_out, unfinished_out, go_on), as _greedy_advance.reference."""
    kw = GA.kernel_arguments(case)
    bsz = case["logits"].shape[0]
    forced = kw["forced"]
    picked = np.array([forced if forced is not None and forced >= 0 else pick(row(case, b), u[b])[0] for b in range(bsz)])
    one_hot = np.full(case["logits"].shape, -1.0, dtype=np.float32)     # the greedy restatement does the rest: arg-max of a one-hot row
    one_hot[np.arange(bsz), picked] = 1.0
    return GA.reference(one_hot, case["seq"], case["cur"], case["max_length"], forced=forced, eos_ids=kw["eos_ids"],
                        pad=kw["pad"], unfinished=case["unfinished"])


def assert_kth_distinct(case):
    """Every row's top_k-th and (top_k + 1)-th surviving values differ: the survivor set does not hang on the tie rule."""
    k = case["top_k"]
    for b in range(case["logits"].shape[0]):
        everyone = survivors(case["logits"][b], banned(case, b), case["temperature"], case["logits"].shape[1], 1.0).tokens
        if k >= 1 and everyone.size > k:
            z = case["logits"][b][everyone] / np.float32(case["temperature"])
            assert z[k - 1] != z[k], (b, k)


def assert_top_p_margin(case):
    """No rank's threshold sum_above / W lies within MARGIN of top_p: fp32 sums decide every rank as float64 does."""
    for b in range(case["logits"].shape[0]):
        assert case["top_p"] == 1.0 or (np.abs(row(case, b).above - case["top_p"]) >= MARGIN).all(), b


def midpoint(sv, i):
    """The uniform at the middle of survivor i's interval, which is at least MARGIN * W wide on either side of it."""
    lo, hi = (sv.C[i - 1] if i else 0.0), sv.C[i]
    assert hi - lo >= 2 * MARGIN * sv.W, (i, lo, hi, sv.W)
    u = np.float32((lo + hi) / 2 / sv.W)
    assert 0.0 <= u < 1.0 and lo + MARGIN * sv.W * 0.99 <= float(u) * sv.W <= hi - MARGIN * sv.W * 0.99
    return u


def away_from_boundaries(sv, u):
    """The draw u lies at least MARGIN * W from every running sum."""
    return sv.tokens.size == 0 or bool((np.abs(sv.C - float(u) * sv.W) >= MARGIN * sv.W).all())


def excursion(sv, token, u):
    """How far (in units of W) the draw lies outside the float64 interval of ``token``; 0 inside; inf for no survivor."""
    if sv.tokens.size == 0:
        return 0.0 if token == 0 else np.inf
    at = np.flatnonzero(sv.tokens == token)
    if at.size == 0:
        return np.inf
    i = int(at[0])
    lo, hi, t = (sv.C[i - 1] if i else 0.0), sv.C[i], float(u) * sv.W
    return max(lo - t, t - hi, 0.0) / sv.W


def spread_logits(rng, bsz, vocab, heavy, lo=0.0, hi=2.0, tail=-30.0):
    """Rows whose ``heavy`` [bsz, n] tokens hold distinct values in [lo, hi] (every one of them weighs at least
    exp(lo - hi) / n of the row) over a tail of distinct values near ``tail``."""
    x = (tail - rng.permutation(vocab)[None, :] * 1e-3 - np.zeros((bsz, 1))).astype(np.float32)
    heavy = np.asarray(heavy)
    n = heavy.shape[1]
    for b in range(bsz):
        values = rng.uniform(lo, hi, n).astype(np.float32)
        assert np.unique(values).size == n
        x[b, heavy[b]] = values
    return x

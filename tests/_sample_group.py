"""What tests/test_sample_group_cpu.py and tests/test_gpu_sample_group*.py share: the grouped uniforms from the Philox words,
a float64 numpy restatement of the log-probability of a drawn token (include/osq_hip.h, "seeded sampling") over the survivors
of tests/_sample_advance.py, its bound, and the restatement's own list of cases.

    lp = (z_tok - m) - ln W, the first term 0 where z_tok == m (m = +inf included); z in fp32, as on both sides, everything
    after it in float64; W the total of the kept survivors; -inf for a row without a survivor.

The bound on |lp - lp64| is 2e-5 + 2**-21 * (|z_tok - m| + |ln W|): 2e-5 for a fixed-order fp32 W (profiles/sample_*_accuracy.txt),
the second term for the subtraction, logf and the final rounding."""
import math

import numpy as np

import _sample_advance as SA


def uniform_words(seed, inputs, cur, group):
    """The 24-bit words of the draws of ``inputs`` x ``group`` rows at history length cur: row b * group + j from the counter
    (b, cur, j, 0)."""
    from outlier_suppression_amd.model import sampling
    seed &= 0xFFFFFFFFFFFFFFFF
    key = (seed & 0xFFFFFFFF, seed >> 32)
    return [sampling.philox4x32((b, cur, j, 0), key)[0] >> 8 for b in range(inputs) for j in range(group)]


def uniforms(seed, inputs, cur, group):
    return (np.array(uniform_words(seed, inputs, cur, group), dtype=np.float64) * 2.0 ** -24).astype(np.float32)


def bound(dz, ln_w):
    return 2e-5 + 2.0 ** -21 * (abs(dz) + abs(ln_w))


def logprob64(x, ban, temperature, top_k, top_p, token):
    """(lp64, its bound) of ``token`` drawn from the row ``x``; (-inf, 0) for a row without a survivor.  The token must be a
    kept survivor."""
    sv = SA.survivors(x, ban, temperature, top_k, top_p)
    if sv.tokens.size == 0:
        return -math.inf, 0.0
    assert int(token) in sv.tokens.tolist(), (token, sv.tokens)
    z = (np.asarray(x, dtype=np.float32) / np.float32(temperature)).astype(np.float64)
    m, zt = z[sv.tokens].max(), z[int(token)]
    dz = 0.0 if zt == m else float(zt - m)
    ln_w = math.log(sv.W)
    return dz - ln_w, bound(dz, ln_w)


def case_logprob64(case, b, token):
    return logprob64(case["logits"][b], SA.banned(case, b), case["temperature"], case["top_k"], case["top_p"], token)


def within(lp, want, label=None):
    """lp against (lp64, bound): equal where lp64 is infinite.  Returns the excursion."""
    lp64, tol = want
    if math.isinf(lp64):
        assert lp == lp64, (label, lp, lp64)
        return 0.0
    off = abs(float(lp) - lp64)
    assert off <= tol, (label, float(lp), lp64, off, tol)
    return off


def lp_cases():
    """(label, row [vocab] fp32, temperature, top_k, top_p): the restatement's own cases."""
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    rng = np.random.default_rng(17)
    out = []
    for T in (0.7, 1.5):
        out.append((f"random row, the whole vocabulary, T {T}", rng.standard_normal(37).astype(np.float32), T, 0, 1.0))
        out.append((f"random row, top-k 5, T {T}", rng.standard_normal(37).astype(np.float32) * 3, T, 5, 1.0))
        x = SA.spread_logits(rng, 1, 300, [rng.choice(300, 8, replace=False)])[0]
        for k, kept, label in ((8, 3, "top-k 8"), (0, 6, "the whole vocabulary")):    # top_p midway between two thresholds
            above = SA.survivors(x, (), T, k or x.size, 1.0).above         # ranked
            assert above[kept] - above[kept - 1] >= 2 * SA.MARGIN
            out.append((f"a top-p cut that removes weight, {label}, T {T}", x, T, k, float(above[kept - 1] + above[kept]) / 2))
    x = rng.standard_normal(20).astype(np.float32)
    x[[3, 7, 11, 15]] = 2.5                                # four equal values at the k-th place: exactly k = 6 survive
    x[[1, 2, 5, 6]] = (4.0, 3.5, 3.0, 2.75)
    out.append(("ties at the k-th value", x, 0.7, 6, 1.0))
    above = SA.survivors(x, (), 1.5, 6, 1.0).above         # the cut keeps one of the two tied survivors
    out.append(("ties at the k-th value under a cut", x, 1.5, 6, float(above[4] + above[5]) / 2))
    x = rng.standard_normal(20).astype(np.float32)
    x[[4, 9, 10]] = inf
    out.append(("m = +inf, a tie group of three", x, 1.5, 0, 1.0))
    out.append(("m = +inf, top-k 2 of the three", x, 0.7, 2, 1.0))
    out.append(("m = +inf under a cut", x, 0.7, 0, 0.5))
    x = rng.standard_normal(20).astype(np.float32)
    x[[0, 6]] = nan
    x[12] = -inf
    out.append(("NaN and -inf are out", x, 1.5, 0, 1.0))
    out.append(("a row without a survivor", np.full(20, -inf, dtype=np.float32), 0.7, 4, 0.9))
    out.append(("a row of NaN: without a survivor", np.full(20, nan, dtype=np.float32), 1.5, 0, 1.0))
    out.append(("one survivor", np.where(np.arange(20) == 13, np.float32(-3.0), -inf).astype(np.float32), 0.7, 0, 1.0))
    return out

"""What tests/test_token_logprob_cpu.py and tests/test_gpu_token_logprob*.py share: a float64 numpy restatement of the
teacher-forced scoring rule (include/osq_hip.h, "teacher-forced scoring"), forward and backward, its bounds and the case
builders.

    m = the row's maximum (a NaN is no maximum); W = sum exp(z - m), -inf weighing 0; lse = m + ln W;
    lp = (z_t - m) - ln W, the first term 0 where z_t == m; 0 for an ignored row, NaN for a label outside the vocabulary;
    z in fp32 as on both sides, everything after it in float64.  A row whose maximum is not finite or that holds a NaN gives
    what IEEE arithmetic gives: NaN.

The forward bound on |lp - lp64| is tests/_sample_group.py's: 2e-5 + 2**-21 * (|z_t - m| + |ln W|) -- 2e-5 for a fixed-order
fp32 W, the second term for the subtraction, logf and the final rounding.  For lse the same with the rounding of m + ln W to
fp32 in the place of the subtraction: 2e-5 + 2**-21 * |ln W| + 2**-23 * |lse|.

The backward bound, derived from the forward one (backward_bound below): the kernel forms p = expf(z - lse) from the fp32 lse.
    the exponent is off by at most d = (the lse bound) + 2**-24 * |z - lse|   (lse, and the rounding of the subtraction)
    so p is off by the factor e**d, and by expf's own error, taken as 2 ulp:   |p - p64| <= p64 * ((e**d - 1) + 2**-22 * e**d)
    p - [v == t] and the product with coef round once each, and coef = upstream / scored is itself a rounded fp32 quotient:
                                                                                2**-22 * |p64 - [v == t]|, relative to coef
    an expf result below the smallest normal number may be flushed:            2**-126
    |dlogits - dlogits64| <= |coef| * (p64 * ((e**d - 1) + 2**-22 * e**d) * (1 + 2**-22) + 2**-22 * |p64 - [v == t]| + 2**-126)
A row of at most 4096 tokens is divided by the kernel's own fp32 sum S of its p: that takes the common factor e**d out again
and adds the rounding of S (at most 16 + 8 additions deep, 24 * 2**-24) and of the quotient (2**-24), together below 1.5e-6
relative to p64 -- far inside the e**d - 1 >= 2e-5 the bound above already grants, so one bound serves both forms.
"""
import numpy as np

CHUNK = 4096            # kBsChunk of csrc/token_argmax.h: one workgroup's tokens
QUAD_RUN = 1024         # tokens 4 (i + 256 k) + e: the k-th 128-bit access of the 256 threads covers 1024 tokens
VOCABS = (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8193, 50265, 57345)
ROWS = (1, 2, 3, 255, 257)
IGNORE = -100


def bound(dz, ln_w):
    return 2e-5 + 2.0 ** -21 * (np.abs(dz) + np.abs(ln_w))


def lse_bound(ln_w, lse):
    return 2e-5 + 2.0 ** -21 * np.abs(ln_w) + 2.0 ** -23 * np.abs(lse)


def forward64(logits, labels, ignore_index=IGNORE):
    """The restatement over fp32 logits [R, V] and int64 labels [R]: a dict of float64 arrays lp, lse, tol (the bound on lp),
    lse_tol, m, ln_w, and scored / bad (bool [R]), loss, loss_tol."""
    z = np.asarray(logits, dtype=np.float32).astype(np.float64)
    labels = np.asarray(labels, dtype=np.int64)
    rows, vocab = z.shape
    with np.errstate(all="ignore"):
        m = np.fmax.reduce(z, axis=1, initial=-np.inf)                   # fmax: a NaN is no maximum
        w = np.exp(z - m[:, None])                                       # exp(-inf) = 0; -inf - -inf and inf - inf: NaN
        ln_w = np.log(w.sum(axis=1))
        lse = m + ln_w
        ignored = labels == ignore_index
        inside = (labels >= 0) & (labels < vocab)
        scored, bad = ~ignored & inside, ~ignored & ~inside
        zt = z[np.arange(rows), np.where(inside, labels, 0)]
        dz = np.where(zt == m, 0.0, zt - m)
        lp = np.where(ignored, 0.0, np.where(inside, dz - ln_w, np.nan))
        tol = np.where(scored & np.isfinite(lp), bound(dz, ln_w), 0.0)
        n = int(scored.sum())
        loss = -lp.sum() / n if n else np.nan
        loss_tol = tol[scored].mean() if n else 0.0
    return dict(lp=lp, lse=lse, tol=tol, lse_tol=lse_bound(ln_w, lse), m=m, ln_w=ln_w, scored=scored, bad=bad, loss=loss,
                loss_tol=loss_tol)


def backward64(logits, labels, coef, ignore_index=IGNORE):
    """(dlogits64 [R, V], its elementwise bound) for per-row coefficients ``coef`` (float64 [R]): coef * (exp(z - lse) - onehot),
    0 for a row that is ignored or whose label lies outside the vocabulary."""
    f = forward64(logits, labels, ignore_index)
    z = np.asarray(logits, dtype=np.float32).astype(np.float64)
    rows, vocab = z.shape
    onehot = np.zeros_like(z)
    live = f["scored"]
    onehot[np.arange(rows)[live], np.asarray(labels)[live]] = 1.0
    coef = np.where(live, np.asarray(coef, dtype=np.float64), 0.0)[:, None]
    with np.errstate(all="ignore"):
        p = np.exp(z - f["lse"][:, None])
        d = np.where(live[:, None], coef * (p - onehot), 0.0)
    return d, backward_bound(z, f["lse"], f["lse_tol"], p, onehot, coef) * live[:, None]


def backward_bound(z, lse, lse_tol, p, onehot, coef):
    """The derivation in the module docstring."""
    with np.errstate(all="ignore"):
        d = lse_tol[:, None] + 2.0 ** -24 * np.abs(z - lse[:, None])
        grow = np.expm1(d)
        return np.abs(coef) * (p * (grow + 2.0 ** -22 * (1.0 + grow)) * (1.0 + 2.0 ** -22) + 2.0 ** -22 * np.abs(p - onehot)
                               + 2.0 ** -126)


def seams(vocab):
    """The tokens at which the layout changes hands: the row's ends, the first and last token of every chunk, the ends of a
    128-bit access and of the 1024 tokens one access of the workgroup covers."""
    at = {0, vocab - 1, 3, 4, QUAD_RUN - 1, QUAD_RUN}
    for c0 in range(0, vocab, CHUNK):
        at.update((c0, min(c0 + CHUNK, vocab) - 1))
    return sorted(p for p in at if 0 <= p < vocab)


def random_case(rng, rows, vocab, ignored=0.2, scale=3.0):
    """(logits [rows, vocab] fp32, labels [rows] int64): normal logits, about ``ignored`` of the labels IGNORE."""
    logits = (rng.standard_normal((rows, vocab)) * scale).astype(np.float32)
    labels = rng.integers(0, vocab, rows).astype(np.int64)
    labels[rng.uniform(size=rows) < ignored] = IGNORE
    return logits, labels


def planted_case(rng, vocab):
    """Rows with the label on every seam, the row's maximum on the same token and, in a second set, on the seam after it."""
    at = seams(vocab)
    logits = (rng.standard_normal((2 * len(at), vocab)) * 2.0).astype(np.float32)
    labels = np.array(at + at, dtype=np.int64)
    for i, p in enumerate(at):
        logits[i, p] = 9.0
        logits[len(at) + i, at[(i + 1) % len(at)]] = 9.0
    return logits, labels


def constructed_case(rng, vocab):
    """(logits, labels, notes): the rows the rule names one by one.  notes[r] tells what row r is; see expect_constructed."""
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    lone = vocab // 2
    other = (lone + 1) % vocab
    rows, labels, notes = [], [], []

    def add(note, row, label):
        rows.append(np.asarray(row, dtype=np.float32))
        labels.append(label)
        notes.append(note)
    survivor = np.where(np.arange(vocab) == lone, np.float32(-3.25), -inf)
    add("survivor, label on it", survivor, lone)
    if vocab > 1:
        add("survivor, label elsewhere", survivor, other)
    add("all -inf", np.full(vocab, -inf), lone)
    x = rng.standard_normal(vocab).astype(np.float32)
    x[vocab - 1] = nan
    add("a NaN", x, 0)
    x = rng.standard_normal(vocab).astype(np.float32)
    x[lone] = inf
    add("+inf", x, lone)
    for sign in (1.0, -1.0):                                   # a spread of a few units in the last place of 1e30
        base = np.float32(sign * 1e30)
        step = np.spacing(base)
        add(f"near {sign * 1e30:g}", base + step * rng.integers(-8, 9, vocab).astype(np.float32), other)
    add("ordinary, ignored", rng.standard_normal(vocab).astype(np.float32), IGNORE)
    add("ordinary", rng.standard_normal(vocab).astype(np.float32) * 4, other)
    add("label -1", rng.standard_normal(vocab).astype(np.float32), -1)
    add("label V", rng.standard_normal(vocab).astype(np.float32), vocab)
    add("ordinary, last", rng.standard_normal(vocab).astype(np.float32) * 4, vocab - 1)
    return np.stack(rows), np.array(labels, dtype=np.int64), notes


def check_forward(lp, lse, want, label=""):
    """Device words against forward64's: inside the bounds, NaN and infinities where the restatement has them.  Returns the
    largest (excursion, its bound) of lp."""
    lp, lse = np.asarray(lp, dtype=np.float64), np.asarray(lse, dtype=np.float64)
    worst = (0.0, 0.0)
    for r in range(lp.shape[0]):
        for got, ref, tol, what in ((lp[r], want["lp"][r], want["tol"][r], "lp"), (lse[r], want["lse"][r], want["lse_tol"][r], "lse")):
            if np.isnan(ref):
                assert np.isnan(got), (label, what, r, got, ref)
            elif np.isinf(ref):
                assert got == ref, (label, what, r, got, ref)
            else:
                off = abs(got - ref)
                assert off <= tol, (label, what, r, got, ref, off, tol)
                if what == "lp" and off > worst[0]:
                    worst = (off, tol)
    return worst

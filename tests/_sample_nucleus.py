"""What tests/test_sample_nucleus_cpu.py and tests/test_gpu_sample_nucleus*.py share: a numpy restatement of the SEARCH by which
osq_sample_nucleus (include/osq_hip.h, "a nucleus over the whole vocabulary") finds its token -- the ordered 32-bit keys of z,
S(k) = the sum of the weights above a key, the two bisections over keys, the tie arithmetic -- with float64 sums, beside the
sort-and-cumulate restatement of tests/_sample_advance.py (``survivors`` / ``pick``), which is the yardstick; and makers of
cases that assert, on the CPU, the conditions their tests rely on.

The kernel's layout, which the cases aim at: 1024 threads, thread t owning tokens 50 t .. 50 t + 49, 64 threads to a wave."""
import numpy as np

import _sample_advance as SA

THREADS, PER, WAVE = 1024, 50, 64
MAX_VOCAB = THREADS * PER                      # kSnMaxVocab
LAST_U = np.float32(1 - 2.0 ** -24)
BAND = 10 * SA.EPS                             # how far a dense case keeps its threshold and its draws from every boundary


def ordered_keys(z):
    """beam_key of fp32 values: an order-preserving map to 32 bits (as uint64, so that differences do not wrap)."""
    u = np.asarray(z, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return np.where(u & 0x80000000, ~u & 0xFFFFFFFF, u | 0x80000000)


def search(x, ban, temperature, top_p, u):
    """The header's search for one row: (token, kept) -- the token the draw u selects and how many ranks the cut keeps."""
    z = np.asarray(x, dtype=np.float32) / np.float32(temperature)
    out = np.isnan(z) | np.isneginf(z)
    out[list(ban)] = True
    z = z + np.float32(0.0)                                             # -0.0 taken as +0.0
    key = np.where(out, 0, ordered_keys(z)).astype(np.uint64)
    if not key.any():
        return 0, 0
    top = int(key.max())
    m = np.float64(z[key == top][0])
    with np.errstate(invalid="ignore", over="ignore"):
        w = np.where(key == 0, 0.0, np.where(z == m, 1.0, np.exp(z.astype(np.float64) - m)))
    order = np.argsort(key, kind="stable")
    sorted_keys, tail = key[order], np.concatenate([np.cumsum(w[order][::-1])[::-1], [0.0]])
    above = lambda k: float(tail[np.searchsorted(sorted_keys, k, side="right")])   # noqa: E731  S(k): the weights of keys > k
    weight = lambda k: float(w[key == k][0])                                        # noqa: E731
    bound = float(np.float32(top_p)) * above(0)
    lo, cut, s_cut = 0, top, 0.0
    while cut - lo > 1:
        mid = lo + (cut - lo) // 2
        s = above(mid)
        if s < bound:
            cut, s_cut = mid, s
        else:
            lo = mid
    group = np.flatnonzero(key == cut)                                   # in token order
    assert group.size >= 1, "the cut is a key that is present"
    kept = int(np.sum(s_cut + np.arange(group.size) * weight(cut) < bound))
    assert kept >= 1
    target = float(u) * (s_cut + kept * weight(cut))
    lo, hit, s_hit = cut - 1, top, 0.0
    while hit - lo > 1:
        mid = lo + (hit - lo) // 2
        s = above(mid)
        if s <= target:
            hit, s_hit = mid, s
        else:
            lo = mid
    group = np.flatnonzero(key == hit)
    assert group.size >= 1, "the draw's key is present"
    limit = kept if hit == cut else group.size
    passed = np.flatnonzero(s_hit + (np.arange(limit) + 1) * weight(hit) > target)
    total_kept = int(np.sum(key > cut)) + kept
    return int(group[passed[0] if passed.size else limit - 1]), total_kept


def midpoint(sv, i, band=SA.MARGIN):
    """The uniform at the middle of survivor i's interval, at least ``band`` * W inside it."""
    lo, hi = (sv.C[i - 1] if i else 0.0), sv.C[i]
    u = np.float32((lo + hi) / 2 / sv.W)
    assert 0.0 <= u < 1.0 and lo + band * sv.W <= float(u) * sv.W <= hi - band * sv.W, (i, lo, hi, sv.W)
    return u


def between(above, r, band=SA.MARGIN):
    """A top_p that keeps ranks 0 .. r - 1 and drops rank r: the middle of above[r - 1] and above[r], ``band`` from both."""
    p = float((above[r - 1] + above[r]) / 2)
    assert 0.0 < p < 1.0 and (np.abs(above - p) >= band).all(), (r, above[r - 1], above[r])
    return p


def repeat_rows(case, n):
    rep = lambda a: np.repeat(a[:1], n, axis=0)            # noqa: E731
    return dict(case, logits=rep(case["logits"]), seq=rep(case["seq"]), unfinished=rep(case["unfinished"]))


def cut_case(rng, vocab, place, kept=3, heavy=6, temperature=0.9):
    """One row of ``heavy`` distinct heavy tokens over a light tail whose ``kept``-th rank (0-based kept - 1, the last one the
    cut keeps) is the token ``place``; top_p between two consecutive ``above`` values.  Returns (case of four equal rows, the
    draws, the tokens they must give): the midpoints of rank 0, of the rank before the last kept and of the last kept, and
    u = 1 - 2^-24.  One rank too many or too few kept moves W, and with it every target, by a whole interval."""
    others = rng.choice(np.setdiff1d(np.arange(vocab), [place]), heavy - 1, replace=False)
    tokens = np.concatenate([[place], others]).astype(np.int64)
    x = SA.spread_logits(rng, 1, vocab, [tokens])
    by_value = tokens[np.argsort(-x[0, tokens])]
    x[0, place], x[0, by_value[kept - 1]] = x[0, by_value[kept - 1]], x[0, place]
    case = SA.make(rng, 1, vocab, 6, 3, temperature, 0, 0.5, logits=x, eos=(min(1, vocab - 1),), pad=0)
    everyone = SA.survivors(x[0], SA.banned(case, 0), temperature, 0, 1.0 - 1e-12)
    assert everyone.ranked[kept - 1] == place
    case["top_p"] = between(everyone.above, kept)
    sv = SA.row(case, 0)
    assert sv.tokens.size == kept and sv.tokens[-1] == place
    u = np.array([midpoint(sv, 0), midpoint(sv, kept - 2), midpoint(sv, kept - 1), LAST_U], dtype=np.float32)
    want = [int(sv.tokens[0]), int(sv.tokens[kept - 2]), place, place]
    return repeat_rows(case, 4), u, want


def places(vocab):
    """Tokens at every seam of the kernel's layout that a row of ``vocab`` tokens has: (label, token)."""
    last_thread = (vocab - 1) // PER
    last_wave = last_thread // WAVE
    out = [("thread 0, first element", 0), ("thread 0, last element", PER - 1), ("a thread's first element", 7 * PER),
           ("a thread's last element", 7 * PER + PER - 1), ("lane 63 of the first wave", (WAVE - 1) * PER + 3),
           ("lane 0 of the second wave", WAVE * PER), ("lane 0 of the last wave", last_wave * WAVE * PER + 1),
           ("lane 63 of a middle wave", (8 * WAVE - 1) * PER + PER - 1), ("the last thread, first element", last_thread * PER),
           ("the last valid element", vocab - 1)]
    return [(label, t) for label, t in out if 0 <= t < vocab]


def dense_case(rng, vocab=50265, heavy=1500, kept=600, temperature=1.0):
    """About ``heavy`` tokens of near-equal weight (values in [0, 0.2]), ``kept`` of them inside the nucleus, top_p midway
    between two consecutive ``above`` values; every rank's threshold and every planted draw at least BAND from a boundary."""
    tokens = rng.choice(vocab, heavy, replace=False).astype(np.int64)
    x = SA.spread_logits(rng, 1, vocab, [tokens], lo=0.0, hi=0.2)
    case = SA.make(rng, 1, vocab, 6, 3, temperature, 0, 0.5, logits=x)
    everyone = SA.survivors(x[0], set(), temperature, 0, 1.0 - 1e-12)
    case["top_p"] = between(everyone.above, kept, BAND)
    sv = SA.row(case, 0)
    assert sv.tokens.size == kept
    ranks = [0, kept // 2, kept - 2, kept - 1]
    u = np.array([midpoint(sv, i, BAND) for i in ranks] + [LAST_U], dtype=np.float32)
    want = [int(sv.tokens[i]) for i in ranks] + [int(sv.tokens[-1])]
    return repeat_rows(case, len(u)), u, want


def flat_case(rng, vocab, top_p):
    """Every logit equal: the kept set is tokens 0 .. r - 1 with r = ceil(top_p * vocab) (all sums are small integers, exact
    in fp32 and float64 alike; top_p * vocab is asserted to lie away from an integer).  Draws for the first, a middle and the
    last of them."""
    x = np.full((1, vocab), 1.25, dtype=np.float32)
    case = SA.make(rng, 1, vocab, 6, 3, 0.7, 0, top_p, logits=x)
    exact = float(np.float32(top_p)) * vocab
    assert abs(exact - round(exact)) > 1e-2 * max(1.0, exact / 4096), exact
    r = int(np.ceil(exact))
    sv = SA.row(case, 0)
    assert sv.tokens.tolist() == list(range(r))
    picks = [0, r // 2, r - 1]
    u = np.array([np.float32((j + 0.5) / r) for j in picks] + [LAST_U], dtype=np.float32)
    for j, v in zip(picks, u):
        assert j + 0.25 < float(v) * r < j + 0.75
    return repeat_rows(case, len(u)), u, picks + [r - 1]


def tie_group_case(rng, vocab=4100, first=WAVE * PER - 2, n=5, kept=3):
    """Two heavier distinct tokens, then ``n`` equal ones at ``first`` .. ``first + n - 1`` -- across the boundary between two
    threads that is also the boundary between two waves -- with the cut keeping ``kept`` of the group."""
    x = SA.spread_logits(rng, 1, vocab, [[5, vocab - 3]], lo=1.0, hi=2.0)
    x[0, first:first + n] = 0.5
    case = SA.make(rng, 1, vocab, 6, 3, 1.0, 0, 0.5, logits=x)
    everyone = SA.survivors(x[0], set(), 1.0, 0, 1.0 - 1e-12)
    assert everyone.ranked[2:2 + n].tolist() == list(range(first, first + n))
    case["top_p"] = between(everyone.above, 2 + kept)
    sv = SA.row(case, 0)
    assert sv.tokens.size == 2 + kept and sv.tokens[2:].tolist() == list(range(first, first + kept))
    u = np.array([midpoint(sv, i) for i in range(2 + kept)] + [LAST_U], dtype=np.float32)
    return repeat_rows(case, len(u)), u, sv.tokens.tolist() + [first + kept - 1]

"""What tests/test_greedy_advance_cpu.py and tests/test_gpu_greedy_advance*.py share: a numpy restatement of one step of
osq_greedy_advance (include/osq_hip.h) -- the banned tokens, numpy's arg-max (the first maximum, NaN above every number, -0.0
equal to +0.0: torch.argmax's order), the pad / eos lines, the stopping word -- and seeded makers of cases.

A case is a dict at the level of generate()'s settings (min_length, the forced ids, the eos ids): ``kernel_arguments`` derives
what the host passes to the static entry point at the case's ``cur``, ``reference_case`` the expected outputs."""
import numpy as np

SETTINGS = dict(ngram=0, min_length=0, eos=(), pad=0, forced_bos=None, forced_eos=None)


def reference(logits, seq, cur, max_length, ngram=0, ban_ids=(), forced=None, eos_ids=(), pad=0, unfinished=None):
    """One step at history length cur: (token [bsz] int64, seq_out, unfinished_out, go_on).  ``seq`` is [bsz, >= max_length]
    with the history in [:, :cur]; ``unfinished`` [bsz] uint8, returned as it came when there is no eos id."""
    logits = np.asarray(logits, dtype=np.float32)
    bsz, vocab = logits.shape
    seq_out = seq.copy()
    unfinished_out = None if unfinished is None else unfinished.copy()
    token = np.zeros(bsz, dtype=np.int64)
    eos_ids = [int(e) for e in eos_ids]
    for b in range(bsz):
        if forced is not None and forced >= 0:
            t = int(forced)
        else:
            row = logits[b].copy()
            for i in ban_ids:
                if 0 <= i < vocab:
                    row[i] = -np.inf
            if ngram > 0 and cur >= ngram:
                s = seq[b, :cur]
                suffix = s[cur - ngram + 1:cur]
                for i in range(cur - ngram + 1):
                    last = int(s[i + ngram - 1])
                    if np.array_equal(s[i:i + ngram - 1], suffix) and 0 <= last < vocab:
                        row[last] = -np.inf
            t = int(np.argmax(row))
        if eos_ids:
            if not unfinished[b]:
                t = int(pad)
            unfinished_out[b] = 1 if (unfinished[b] and t not in eos_ids) else 0
        token[b] = t
        seq_out[b, cur] = t
    go_on = int(cur + 1 < max_length and (not eos_ids or bool(unfinished_out.any())))
    return token, seq_out, unfinished_out, go_on


def kernel_arguments(case):
    """What the host passes to the static entry point at the case's cur: dict(ngram, ban_ids, forced, eos_ids, pad)."""
    cur, max_length = case["cur"], case["max_length"]
    forced = case["forced_bos"] if cur == 1 else None
    if case["forced_eos"] is not None and cur == max_length - 1:
        forced = case["forced_eos"]                     # the later processor wins
    ban = tuple(case["eos"]) if (case["min_length"] > 0 and cur < case["min_length"]) else ()
    return dict(ngram=case["ngram"], ban_ids=ban, forced=forced, eos_ids=tuple(case["eos"]), pad=case["pad"])


def reference_case(case):
    return reference(case["logits"], case["seq"], case["cur"], case["max_length"], unfinished=case["unfinished"],
                     **kernel_arguments(case))


def make(rng, bsz, vocab, max_length, cur, logits=None, history=None, unfinished=None, **settings):
    """A case: random logits (or the given ones), a random history over few distinct tokens (so that windows repeat), every
    row unfinished unless told otherwise; the tail of seq holds -7, which a step must leave but for column cur."""
    case = dict(SETTINGS, **settings)
    if logits is None:
        logits = rng.standard_normal((bsz, vocab)).astype(np.float32)
    seq = np.full((bsz, max_length), -7, dtype=np.int64)
    seq[:, :cur] = rng.integers(0, min(vocab, 3), size=(bsz, cur)) if history is None else history
    case.update(logits=np.ascontiguousarray(logits, dtype=np.float32), seq=seq, cur=cur, max_length=max_length,
                unfinished=np.ones(bsz, dtype=np.uint8) if unfinished is None else np.asarray(unfinished, dtype=np.uint8))
    return case


def planted(rng, bsz, vocab, at, value=50.0):
    """Random logits in [-4, 4) with ``value`` planted at index ``at`` of every row."""
    x = rng.uniform(-4, 4, size=(bsz, vocab)).astype(np.float32)
    x[:, at] = value
    return x


def order_cases(rng, vocab=37, bsz=3, max_length=9, cur=4):
    """(label, case): the order of the arg-max -- ties, signed zeros, NaN, -inf -- and the bans that change the winner."""
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    full = lambda v: np.full((bsz, vocab), v, dtype=np.float32)          # noqa: E731
    out = [("random rows", make(rng, bsz, vocab, max_length, cur))]
    x = rng.integers(-3, 4, size=(bsz, vocab)).astype(np.float32)        # integer-valued: every row has its maximum several times
    out.append(("duplicated maxima", make(rng, bsz, vocab, max_length, cur, logits=x)))
    out.append(("a constant row", make(rng, bsz, vocab, max_length, cur, logits=full(1.5))))
    for first, second, label in ((-0.0, 0.0, "-0.0 before +0.0"), (0.0, -0.0, "+0.0 before -0.0")):
        x = full(-2.0)
        x[:, 5], x[:, 11] = first, second
        out.append((label, make(rng, bsz, vocab, max_length, cur, logits=x)))
    x = planted(rng, bsz, vocab, 3)
    x[:, 20] = nan
    out.append(("one NaN", make(rng, bsz, vocab, max_length, cur, logits=x)))
    x = x.copy()
    x[:, 9] = nan
    out.append(("two NaNs", make(rng, bsz, vocab, max_length, cur, logits=x)))
    x = planted(rng, bsz, vocab, 3)
    x[:, 2] = nan
    out.append(("a banned NaN (min-length)", make(rng, bsz, vocab, max_length, cur, logits=x, eos=(2,), pad=1, min_length=8)))
    history = np.tile(np.array([2, 1, 2, 1], dtype=np.int64), (bsz, 1))  # suffix (1,): the windows (1, 2) ban 2
    out.append(("a banned NaN (n-gram)", make(rng, bsz, vocab, max_length, cur, logits=x, history=history, ngram=2)))
    out.append(("an all -inf row", make(rng, bsz, vocab, max_length, cur, logits=full(-inf))))
    history = np.tile(np.array([0, 1, 2, 1], dtype=np.int64), (bsz, 1))
    out.append(("every token banned", make(rng, bsz, 3, max_length, cur, history=history, ngram=1)))
    return out


def ngram_cases(rng, vocab=37, bsz=3):
    """(label, case): n-gram sizes 1 / 2 / 3 at cur = n - 1, n, n + 1 (a history has at least its start token: cur >= 1).  Row b's
    history alternates between tokens 0 and 1, starting with b % 2, and the logits put 0 first and 1 second: once a window
    repeats, the ban takes the winner of some row."""
    out = []
    for n in (1, 2, 3):
        for cur in sorted({max(1, n - 1), n, n + 1}):
            x = rng.standard_normal((bsz, vocab)).astype(np.float32)
            x[:, 0], x[:, 1] = 9.0, 8.0
            history = np.array([[(b + i) % 2 for i in range(cur)] for b in range(bsz)], dtype=np.int64)
            out.append((f"ngram {n} at cur {cur}", make(rng, bsz, vocab, cur + 3, cur, logits=x, history=history, ngram=n)))
    return out


def finish_cases(rng, vocab=37, bsz=3, max_length=9):
    """(label, case): min-length either side of its bound, the forced tokens, finished rows, the last position."""
    out = []
    for eos in ((4,), (4, 0, 30)):
        for cur in (4, 5, 6):                            # min_length 6: banned at 4 and 5, free at 6
            x = planted(rng, bsz, vocab, eos[-1])
            x[:, eos[0]] = 40.0
            out.append((f"min-length 6 with {len(eos)} eos at cur {cur}",
                        make(rng, bsz, vocab, max_length, cur, logits=x, eos=eos, pad=1, min_length=6)))
    nan_rows = np.full((bsz, vocab), np.nan, dtype=np.float32)
    out.append(("forced bos", make(rng, bsz, vocab, max_length, 1, forced_bos=7, forced_eos=2, eos=(2,), pad=1)))
    out.append(("forced bos over NaN rows", make(rng, bsz, vocab, max_length, 1, logits=nan_rows, forced_bos=7)))
    out.append(("forced bos does not fire at cur 2", make(rng, bsz, vocab, max_length, 2, forced_bos=7, forced_eos=2)))
    out.append(("forced eos", make(rng, bsz, vocab, max_length, max_length - 1, forced_bos=7, forced_eos=2, eos=(2,), pad=1)))
    out.append(("both forced at max_length 2", make(rng, bsz, vocab, 2, 1, forced_bos=7, forced_eos=2, eos=(2,), pad=1)))
    out.append(("both forced at max_length 2, no eos", make(rng, bsz, vocab, 2, 1, forced_bos=7, forced_eos=2)))
    x = planted(rng, bsz, vocab, 4)
    x[1, 4] = -9.0                                       # row 1 does not pick the eos
    for unfinished, label in (((1, 1, 1), "rows finish now"), ((0, 1, 0), "rows already finished"),
                              ((0, 0, 0), "every row finished"), ((1, 0, 0), "only the first row unfinished"),
                              ((0, 0, 1), "only the last row picks the eos")):
        out.append((label, make(rng, bsz, vocab, max_length, 4, logits=x, unfinished=unfinished, eos=(4, 30), pad=1)))
    out.append(("no eos: unfinished untouched", make(rng, bsz, vocab, max_length, 4, logits=x, unfinished=(0, 1, 0))))
    out.append(("the last position", make(rng, bsz, vocab, max_length, max_length - 1, eos=(4,), pad=1)))
    out.append(("the last position, no eos", make(rng, bsz, vocab, max_length, max_length - 1)))
    return out


def all_cases(seed=0):
    rng = np.random.default_rng(seed)
    return order_cases(rng) + ngram_cases(rng) + finish_cases(rng)


def has_nan(case):
    return bool(np.isnan(case["logits"]).any())

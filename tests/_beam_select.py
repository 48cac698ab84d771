"""What tests/test_beam_select_cpu.py and tests/test_gpu_beam_select*.py share: a float64 restatement of the contract of
osq_beam_select (include/osq_hip.h) in numpy, the gap that entitles a test to compare indices exactly, and seeded cases.

    value(b, j, t) = (x - m) - L + running[b, j]     m = max_t x, L = log(sum_t exp(x - m)) over the whole row
                     -inf + running[b, j]            where t is banned in row r = b * nb + j
    banned           every id of ban_ids; with n = ngram > 0 and cur >= n, seq[r, i + n - 1] for every i in [0, cur - n] whose
                     window seq[r, i : i + n - 1] equals the suffix seq[r, cur - n + 1 : cur]; ids outside [0, vocab) ban nothing
    order            larger value first, equal values by smaller flat index j * vocab + t, NaN above every number
"""
import numpy as np
import torch


def banned(seq, cur, ngram, ban_ids, rows, vocab):
    """The ban rule as the plain double loop: bool [rows, vocab]."""
    out = np.zeros((rows, vocab), dtype=bool)
    for r in range(rows):
        if ngram > 0 and cur >= ngram:
            for i in range(cur - ngram + 1):
                same = True
                for k in range(ngram - 1):
                    if int(seq[r, i + k]) != int(seq[r, cur - ngram + 1 + k]):
                        same = False
                        break
                t = int(seq[r, i + ngram - 1])
                if same and 0 <= t < vocab:
                    out[r, t] = True
        for t in ban_ids:
            if 0 <= int(t) < vocab:
                out[r, int(t)] = True
    return out


def values(logits, running, seq=None, cur=0, ngram=0, ban_ids=()):
    """float64 [bsz, nb * vocab]: every element's value."""
    x = np.asarray(logits, dtype=np.float64)
    run = np.asarray(running, dtype=np.float64)
    bsz, nb = run.shape
    rows, vocab = x.shape
    assert rows == bsz * nb
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        m = x.max(axis=1, keepdims=True)
        lp = (x - m) - np.log(np.exp(x - m).sum(axis=1, keepdims=True))
        lp[banned(None if seq is None else np.asarray(seq), cur, ngram, ban_ids, rows, vocab)] = -np.inf
        return (lp.reshape(bsz, nb, vocab) + run[:, :, None]).reshape(bsz, nb * vocab)


def order(v):
    """The indices of one batch row's values in the contract's order."""
    nan = np.isnan(v)
    with np.errstate(invalid="ignore"):
        return np.lexsort((np.arange(v.size), -np.where(nan, 0.0, v), ~nan))


def reference(logits, running, keep, seq=None, cur=0, ngram=0, ban_ids=()):
    """(top_value float64 [bsz, keep], top_index int64 [bsz, keep]) of the contract."""
    v = values(logits, running, seq, cur, ngram, ban_ids)
    idx = np.stack([order(row)[:keep] for row in v]).astype(np.int64)
    return np.take_along_axis(v, idx, axis=1), idx


def gap(logits, running, keep, seq=None, cur=0, ngram=0, ban_ids=()):
    """The smallest float64 difference between two DISTINCT consecutive values among ranks 1 .. keep + 1 of any batch row
    (exact ties -- identical inputs, two -inf -- do not count; NaN has no distance)."""
    v = values(logits, running, seq, cur, ngram, ban_ids)
    best = np.inf
    for row in v:
        top = row[order(row)[:keep + 1]]
        with np.errstate(invalid="ignore"):
            d = top[:-1] - top[1:]
        d = d[np.isfinite(d) & (d > 0)]
        if d.size:
            best = min(best, float(d.min()))
    return best


def case(seed, bsz, nb, vocab, cur=0, alphabet=None):
    """Seeded inputs: logits [bsz * nb, vocab] = randn * 4, running [bsz, nb] = randn, and (cur > 0) token histories
    [bsz * nb, cur] drawn from an alphabet of 5 ids, so that windows repeat."""
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(bsz * nb, vocab, generator=g) * 4
    running = torch.randn(bsz, nb, generator=g)
    seq = None
    if cur > 0:
        ids = torch.arange(5) if alphabet is None else torch.as_tensor(alphabet, dtype=torch.int64)
        seq = ids[torch.randint(0, ids.numel(), (bsz * nb, cur), generator=g)]
    return logits, running, seq

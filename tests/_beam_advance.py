"""What tests/test_beam_advance_cpu.py and tests/test_gpu_beam_advance*.py share: a numpy restatement of one step of
osq_beam_advance (include/osq_hip.h) -- integers and np.float32 operations, one per torch op of
generation._advance_beams_torch, the strict order of ties, both forms of the division -- and seeded states and selections.

A state is a dict of numpy arrays: running / finished int64 [bsz, nb, L], running_scores / scores float32 [bsz, nb],
finished_len int64 [bsz, nb], done bool [bsz, nb], improvable bool [bsz]."""
import numpy as np

STATE = ("running", "running_scores", "finished", "scores", "finished_len", "done", "improvable")
OUTPUTS = STATE + ("beam_idx", "next_tokens", "go_on")
F = np.float32
BIG = F(-1.0e9)


def order(v):
    """The indices of v in the order of the kernels' top-k: NaN first, then larger values, equal values (-0.0 equals +0.0)
    by smaller index."""
    v = np.asarray(v)
    return sorted(range(len(v)), key=lambda i: (0, 0.0, i) if np.isnan(v[i]) else (1, -float(v[i]), i))


def divisors(cur, max_length, early_stopping, length_penalty, prompt=1):
    """(len_div, best_div) of the step at length cur, as the Python lines of the torch function compute them."""
    best_len = (max_length - prompt) if (early_stopping == "never" and length_penalty > 0.0) else (cur + 1 - prompt)
    return (cur + 1 - prompt) ** length_penalty, best_len ** length_penalty


def _divide(v, div, reciprocal):
    """v / div by the Python scalar div: v * float32(1 / div) with the reciprocal taken in double (torch on the GPU), or the
    correctly rounded v / float32(div) (torch on the CPU)."""
    with np.errstate(all="ignore"):
        return v * F(1.0 / float(div)) if reciprocal else v / F(div)


def reference(top_lp, top_idx, state, cur, vocab, eos=(), early_stopping=False, length_penalty=1.0, reciprocal=False):
    """One step at length cur (prompt of one token): the dict of every output of osq_beam_advance (OUTPUTS)."""
    top_lp, top_idx = np.asarray(top_lp, dtype=F), np.asarray(top_idx, dtype=np.int64)
    bsz, keep = top_lp.shape
    _, nb, L = state["running"].shape
    len_div, best_div = divisors(cur, L, early_stopping, length_penalty)
    out = {name: np.zeros_like(state[name]) for name in STATE}
    out["beam_idx"] = np.zeros(bsz * nb, dtype=np.int64)
    out["next_tokens"] = np.zeros(bsz * nb, dtype=np.int64)
    out["_cat"] = np.zeros((bsz, nb + keep), dtype=F)           # scores | cand before the merge: for a test's tie check
    all_hits, all_done = True, True
    with np.errstate(all="ignore"):
        for b in range(bsz):
            beam, token = top_idx[b] // vocab, top_idx[b] % vocab
            beam = np.clip(beam, 0, nb - 1)
            top_seq = state["running"][b][beam].copy()
            top_seq[:, cur] = token
            hits = np.full(keep, cur + 1 >= L) | np.isin(token, np.asarray(eos, dtype=np.int64))
            trl = top_lp[b] + hits.astype(F) * BIG
            nxt = order(trl)[:nb]
            out["running"][b] = top_seq[nxt]
            out["running_scores"][b] = trl[nxt]
            out["beam_idx"][b * nb:(b + 1) * nb] = beam[nxt] + b * nb
            out["next_tokens"][b * nb:(b + 1) * nb] = token[nxt]
            just = hits & (np.arange(keep) < nb)
            cand = _divide(top_lp[b], len_div, reciprocal)
            full = bool(state["done"][b].all()) and early_stopping is True
            cand = cand + F(full) * BIG
            cand = cand + F(not state["improvable"][b]) * BIG
            cand = cand + (~just).astype(F) * BIG
            cat = np.concatenate((state["scores"][b], cand))
            out["_cat"][b] = cat
            merged = order(cat)[:nb]
            out["finished"][b] = np.concatenate((state["finished"][b], top_seq))[merged]
            out["scores"][b] = cat[merged]
            out["finished_len"][b] = np.concatenate((state["finished_len"][b], np.full(keep, cur, dtype=np.int64)))[merged]
            out["done"][b] = np.concatenate((state["done"][b], just))[merged]
            best_running = _divide(out["running_scores"][b, 0], best_div, reciprocal)
            worst_done = np.where(out["done"][b], np.min(out["scores"][b]), BIG)
            out["improvable"][b] = state["improvable"][b] and bool(np.any(best_running > worst_done))
            all_hits, all_done = all_hits and bool(hits.all()), all_done and bool(out["done"][b].all())
    go_on = bool(out["improvable"].any()) and not (all_done and early_stopping is True) and not all_hits
    out["go_on"] = np.array([go_on], dtype=np.int32)
    return out


def random_state(rng, bsz, nb, L, cur, vocab, kind="nothing", eos=()):
    """A state at length cur.  kind: "nothing" done, "some" done (row r: a different number of finished beams), "all" done,
    "stale" (some done and row 1, or the only row, no longer improvable).  Tokens avoid ``eos``; the real scores are
    pairwise distinct, the others -1e9 as a search starts them."""
    free = np.array([t for t in range(vocab) if t not in set(eos)], dtype=np.int64)
    state = {"running": np.full((bsz, nb, L), 1, dtype=np.int64), "finished": np.full((bsz, nb, L), 1, dtype=np.int64)}
    state["running"][:, :, :cur] = rng.choice(free, size=(bsz, nb, cur))
    state["running_scores"] = -np.sort(rng.permutation(64 * bsz * nb)[:bsz * nb].reshape(bsz, nb).astype(F) / F(16), axis=1)
    state["scores"] = np.full((bsz, nb), BIG, dtype=F)
    state["finished_len"] = np.zeros((bsz, nb), dtype=np.int64)
    state["done"] = np.zeros((bsz, nb), dtype=bool)
    state["improvable"] = np.ones(bsz, dtype=bool)
    for b in range(bsz):
        count = {"nothing": 0, "all": nb}.get(kind, (0 if nb == 1 else 1, max(1, nb // 2), max(1, nb - 1))[b % 3])
        real = -np.sort(rng.permutation(640)[:count].astype(F) / F(64) + F(0.2537))     # descending, distinct, in (-11, 0)
        state["scores"][b, :count] = real
        state["done"][b, :count] = True
        for j in range(count):
            n = int(rng.integers(1, cur + 1))
            state["finished"][b, j, :n] = rng.choice(free, size=n)
            state["finished_len"][b, j] = n - 1 if n > 1 else 1
    if kind == "stale":
        state["improvable"][min(1, bsz - 1)] = False
    return state


def random_selection(rng, bsz, nb, keep, vocab, eos=(), wide=False, hits=True):
    """top_lp [bsz, keep] pairwise distinct per row, in random order -- in (-20, 0), or with ``wide`` at least 128 apart (a
    sum with -1e9 keeps them apart) -- and top_idx with random beams and tokens that avoid ``eos``, except, with ``hits``,
    an eos planted in row 0 at candidate 0 (among the first nb), in row 1 at the last candidate (beyond them) and in row 2 at
    both where nb candidates stay free."""
    free = np.array([t for t in range(vocab) if t not in set(eos)], dtype=np.int64)
    top_lp = np.zeros((bsz, keep), dtype=F)
    for b in range(bsz):
        ranks = rng.permutation(1024)[:keep].astype(F)
        top_lp[b] = -(ranks + F(1)) * F(200) - rng.random(keep).astype(F) if wide else -(ranks + F(1)) / F(64)
    token = rng.choice(free, size=(bsz, keep))
    if hits and len(eos):
        for b in range(bsz):
            at = ((0,), (keep - 1,), (0, keep - 1) if keep - 2 >= nb else ())[b % 3]
            for k in at:
                token[b, k] = eos[int(rng.integers(len(eos)))]
    beam = rng.integers(0, nb, size=(bsz, keep))
    return top_lp, (beam * vocab + token).astype(np.int64)

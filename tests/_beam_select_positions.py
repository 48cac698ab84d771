"""What tests/test_beam_select_positions_cpu.py and tests/test_gpu_beam_select_positions.py share: where osq_beam_select
(csrc/beam_select.hip, csrc/token_argmax.h) keeps a token and a candidate, a recipe that plants the winners of a step where
a case wants them, and the table of cases.  No GPU: numpy and torch on the CPU.  The contract is tests/_beam_select.py.

Ownership, from the kernels' text.  beam_chunk_kernel: one 256-thread workgroup per (row, chunk of 4096 tokens), element
i = threadIdx.x + j * 256 in register j of its thread; beam_merge_kernel: one workgroup per batch row over
n = nb * chunks * keep candidate slots, slot p read (and, once taken, cleared and rescanned) by thread p & 255 in trip p >> 8:

    chunk = t // 4096          i = t % 4096               length of a chunk  min(4096, vocab - 4096 * chunk)
    thread = i % 256           register = i // 256        wave = thread // 64        lane = thread % 64
    p = (beam * chunks + chunk) * keep + rank_in_chunk    merge_thread = p % 256     merge_trip = p // 256

Planting.  Noise randn * 0.5 everywhere; the q-th plant of a beam (in the order the case lists them) is the logit
40 - 0.37 q; a beam with a plant runs at -0.11 * beam, every other beam at -100.  Log-softmax normalises each row by itself,
so a plant competes with the other beams' plants through (x - m) - L, never through x: counting q per beam makes every
planted row's m the same 40, its L at most log(1 / (1 - exp(-0.37))) = 1.18, its plants (x - m) - L >= -0.37 * 63 - 1.18 =
-24.5 and its noise (x - m) - L <= 2.7 - 40 = -37.3 (2.7: 5.4 sigma; 6.4e6 draws reach about 5.2).  With the
running scores (>= -6.93) the last plant of any beam stays 5.9 above the noise of every beam, two plants of one beam stay
0.37 apart and the q-th plants of two beams 0.11 * (their distance) +- (L of one - L of the other): distinct, and decided
by the merge.  tests/test_beam_select_positions_cpu.py checks all of it on the float64 restatement, case by case: the set,
the gap (>= 1e-4) and the magnitudes (<= 64) that the value bound of tests/test_gpu_beam_select.py is derived for.
A top of 20 would let 64 plants sink into the noise: not used."""
import functools
from typing import Callable, NamedTuple, Optional

import numpy as np
import torch

import _beam_select as BS

CHUNK, THREADS, PER, WAVE = 4096, 256, 16, 64
TOP, STEP, NOISE, LEAD, AWAY = 40.0, 0.37, 0.5, 0.11, -100.0


# ------------------------------------------------------------------------------------------------ ownership

class Owner(NamedTuple):
    chunk: int
    i: int
    thread: int
    register: int
    wave: int
    lane: int


def chunks_of(vocab):
    return (vocab + CHUNK - 1) // CHUNK


def chunk_len(vocab, chunk):
    return min(CHUNK, vocab - CHUNK * chunk)


def owner(t):
    """Where beam_chunk_kernel keeps token ``t`` of a row."""
    i = t % CHUNK
    thread = i % THREADS
    return Owner(t // CHUNK, i, thread, i // THREADS, thread // WAVE, thread % WAVE)


def tok(chunk, thread, register=0):
    """The token that register ``register`` of thread ``thread`` holds in chunk ``chunk``."""
    return chunk * CHUNK + register * THREADS + thread


def merge_slot(beam, chunk, rank, chunks, keep):
    return (beam * chunks + chunk) * keep + rank


def merge_owner(p):
    """(thread, trip) of beam_merge_kernel for candidate slot ``p``."""
    return p % THREADS, p // THREADS


# ------------------------------------------------------------------------------------------------ planting

def per_row(plants, bsz):
    """``plants`` as one list per batch row: a flat list of (beam, token) plants every row alike."""
    if plants and isinstance(plants[0], list):
        assert len(plants) == bsz
        return plants
    return [list(plants)] * bsz


def planted(seed, bsz, nb, vocab, plants, top=TOP, step=STEP, noise=NOISE, lead=LEAD, away=AWAY):
    """(logits [bsz * nb, vocab], running [bsz, nb]) of the recipe above.  ``plants``: (beam, token) pairs, one list for
    every batch row or a list of ``bsz`` lists."""
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(bsz * nb, vocab, generator=g) * noise
    running = torch.full((bsz, nb), away)
    for b, row in enumerate(per_row(plants, bsz)):
        count = {}
        assert len(set(row)) == len(row), "a plant twice"
        for beam, token in row:
            q = count.get(beam, 0)
            count[beam] = q + 1
            logits[b * nb + beam, token] = top - step * q
            running[b, beam] = -lead * beam
    return logits, running


# ------------------------------------------------------------------------------------------------ the table

class Case(NamedTuple):
    label: str                      # its first letter is the group
    bsz: int
    nb: int
    vocab: int
    keep: int
    plants: list                    # (beam, token) in planted rank order; one list, or one per batch row
    classes: tuple                  # ownership classes (names of ``classes_hit``) the case is there for
    seed: int = 0
    ban_ids: tuple = ()
    make: Optional[Callable] = None     # (case) -> (logits, running) where the recipe alone does not say it (F, G)
    index: Optional[list] = None        # top_index [bsz][keep] where the case's point is one stated order
    pipeline: bool = True               # tie-free and all finite: torch's own pipeline is a second reference

    @property
    def group(self):
        return self.label[0]


def _arrange(tokens, how, seed=0):
    """``tokens`` in planted rank order: rank running ``with`` the position, ``against`` it, or ``shuffled`` by seed."""
    tokens = sorted(tokens)
    if how == "against":
        return tokens[::-1]
    if how == "shuffled":
        return [tokens[k] for k in np.random.default_rng(seed).permutation(len(tokens))]
    assert how == "with"
    return tokens


ORDERS = ("with", "against", "shuffled")
EDGES = (0, 63, 64, 255, 256, 3839, 3840, 4095)
TABLE = []


def _add(label, bsz, nb, vocab, keep, plants, classes=(), **kw):
    assert all(c.label != label for c in TABLE), label
    TABLE.append(Case(label, bsz, nb, vocab, keep, plants, tuple(classes), **kw))


# ---- A: positions in one chunk
for n, how in enumerate(ORDERS):
    _add(f"A edges of 4096, rank {how} position", 1, 2, 4096, 8, [(1, t) for t in _arrange(EDGES, how, n)],
         ("register 0", "register 15", "wave 0 lane 0", "wave 0 lane 63", "wave 1 lane 0", "wave 3 lane 63",
          "first token of a full chunk", "last token of a full chunk", "chunk supplies keep", "chunk supplies 0"), seed=n)
    _add(f"A edges of chunk 1 of 8193, rank {how} position", 2, 2, 8193, 8,
         [(n % 2, CHUNK + t) for t in _arrange(EDGES, how, 10 + n)],
         ("register 0", "register 15", "first token of a full chunk", "last token of a full chunk"), seed=10 + n)

# ---- B: one thread owns them all
for thread in (0, 63, 64, 255):
    for n, how in enumerate(ORDERS):
        _add(f"B 16 of thread {thread}, rank {how} register", 1, 2, 4096, 16,
             [(1, t) for t in _arrange([tok(0, thread, r) for r in range(PER)], how, thread + n)],
             ("thread owns 16", "register 0", "register 15"), seed=20 + n)
    how = ORDERS[(thread // 63) % 3]
    _add(f"B 12 of 16 planted in thread {thread}, rank {how} register", 1, 1, 4096, 12,
         [(0, t) for t in _arrange([tok(0, thread, r) for r in range(PER)], how, thread)], ("thread owns 12",), seed=24)
# a ragged last chunk of 1380 tokens: thread 0 holds six tokens in range, thread 255 five
_add("B ragged chunk, the 6 of thread 0", 1, 2, CHUNK + 1380, 6,
     [(1, t) for t in _arrange([tok(1, 0, r) for r in range(6)], "against")], ("first token of a ragged chunk",), seed=25)
_add("B ragged chunk, the 5 of thread 255", 1, 2, CHUNK + 1380, 5,
     [(0, t) for t in _arrange([tok(1, 255, r) for r in range(5)], "shuffled", 3)], (), seed=26)
_add("B ragged chunk, 5 of the 6 of thread 91", 1, 1, CHUNK + 1380, 5,
     [(0, t) for t in _arrange([tok(1, 91, r) for r in range(6)], "with")], (), seed=27)

# ---- C: one wave, one lane
for wave, register, chunk, vocab, how in ((1, 15, 0, 4096, "shuffled"), (2, 0, 0, 4096, "against"), (0, 7, 1, 8193, "with"),
                                          (3, 3, 1, 8193, "shuffled")):
    _add(f"C the 64 lanes of wave {wave} at register {register}", 1, 2, vocab, 64,
         [(1, t) for t in _arrange([tok(chunk, wave * WAVE + lane, register) for lane in range(WAVE)], how, wave)],
         (f"wave {wave} lane 0", f"wave {wave} lane 63", "chunk supplies keep"), seed=30 + wave)
for n, how in enumerate(ORDERS):
    _add(f"C lane 0 of four waves x 16 registers, rank {how} position", 1, 2, 4096, 64,
         [(0, t) for t in _arrange([tok(0, w * WAVE, r) for w in range(4) for r in range(PER)], how, n)],
         ("wave 0 lane 0", "wave 1 lane 0", "wave 2 lane 0", "wave 3 lane 0", "thread owns 16"), seed=35 + n)

# ---- D: chunks
_add("D first and last token of every chunk of 8193", 2, 2, 8193, 5,
     [(1, t) for t in _arrange([0, 4095, 4096, 8191, 8192], "shuffled", 1)],
     ("first token of a ragged chunk", "last token of a ragged chunk", "chunk supplies 1", "chunk supplies fewer than keep"),
     seed=40)
_add("D first and last token of every chunk of 50265", 1, 3, 50265, 26,
     [(c % 3, t) for c in range(13) for t in (c * CHUNK, c * CHUNK + chunk_len(50265, c) - 1)],
     ("first token of a ragged chunk", "last token of a ragged chunk", "chunk supplies fewer than keep"), seed=41)
_add("D the last chunk of 8193 alone", 2, 3, 8193, 1, [(2, 8192)], ("chunk supplies 1", "merge slot n-1"), seed=42)
_add("D all winners in the last chunk of 50265", 2, 2, 50265, 12,
     [(1, t) for t in _arrange([49152, 49153, 49215, 49216, 49407, 49408, 49663, 50000, 50175, 50176, 50263, 50264], "shuffled", 2)],
     ("first token of a ragged chunk", "last token of a ragged chunk", "chunk supplies keep", "merge slot n-1"), seed=43)
_add("D 4097, token 4096 first of 12", 1, 2, 4097, 12,
     [(1, 4096)] + [(1, t) for t in (5, 255, 256, 1000, 2047, 2048, 3000, 3839, 3840, 4000, 4095)],
     ("chunk supplies 1", "first token of a ragged chunk", "last token of a ragged chunk"), seed=44)
_add("D 4101, five in the tail and seven elsewhere", 2, 2, 4101, 12,
     [(0, 7), (0, 4100), (0, 4098), (0, 300), (0, 4096), (0, 4095), (0, 4099), (0, 2222), (0, 4097), (0, 1), (0, 263), (0, 64)],
     ("chunk supplies fewer than keep", "last token of a ragged chunk", "thread owns 2"), seed=45)      # thread 7: 7 and 263

# ---- E: the merge
_add("E 36 slots, four winners a beam", 1, 3, 4096, 12,
     [(k % 3, t) for k, t in enumerate((9, 100, 511, 777, 1024, 1500, 2000, 2500, 3000, 3500, 4000, 4094))],
     ("merge slot 0", "chunk supplies fewer than keep"), seed=50)
_add("E 36 slots, all from the last beam", 1, 3, 4096, 12, [(2, 11 + 340 * k) for k in range(12)], ("merge slot n-1",), seed=51)
_add("E 256 slots, sixteen winners a beam", 1, 4, 4096, 64, [(k % 4, 3 + 63 * k) for k in range(64)], ("merge slot 0",), seed=52)
_add("E 256 slots, all from the last beam", 1, 4, 4096, 64, [(3, 4095 - 61 * k) for k in range(64)],
     ("merge slot 255", "merge slot n-1"), seed=53)
_add("E 288 slots, slots 0..6 and 252..256", 2, 8, 8193, 12,
     [[(0, 10 * k) for k in range(7)] + [(7, 4000 - 100 * k) for k in range(5)],
      [(7, 33 * k) for k in range(5)] + [(0, 50 + k) for k in range(7)]],
     ("merge slot 0", "merge slot 255", "merge slot 256", "merge trip >= 1", "merge thread owns >= 2"), seed=54)
_add("E 288 slots, all from the last chunk of the last beam", 1, 12, CHUNK + 300, 12,
     [(11, t) for t in _arrange([CHUNK + 25 * k for k in range(11)] + [CHUNK + 299], "against")],
     ("merge slot n-1", "merge trip >= 1", "last token of a ragged chunk"), seed=55)
_add("E 64 beams keep 64 at 4097, one winner a beam", 2, 64, 4097, 64,
     [[(j, 4096 if j % 9 == 0 else (61 * j) % 4096) for j in range(64)], [(63 - j, (4096 - 67 * j) % 4097) for j in range(64)]],
     ("nb 64 and keep 64", "merge trip >= 1", "chunk supplies 1"), seed=56)
_add("E 64 beams keep 64 at 4097, all in beam 63", 1, 64, 4097, 64,
     [(63, t) for t in _arrange([4096] + [65 * k for k in range(63)], "shuffled", 4)],
     ("nb 64 and keep 64", "merge trip >= 1"), seed=57)
_add("E 64 beams keep 64 at 50265, one winner a beam", 2, 64, 50265, 64,
     [[(j, (j % 13) * CHUNK + (997 * j) % chunk_len(50265, j % 13)) for j in range(64)],
      [(63 - j, ((j + 5) % 13) * CHUNK + (131 * j) % chunk_len(50265, (j + 5) % 13)) for j in range(64)]],
     ("nb 64 and keep 64", "merge trip >= 1"), seed=58)
_add("E 64 beams keep 64 at 50265, all in beam 37", 1, 64, 50265, 64,
     [(37, t) for t in _arrange([(k % 13) * CHUNK + (211 * k) % chunk_len(50265, k % 13) for k in range(63)] + [50264], "shuffled", 5)],
     ("nb 64 and keep 64", "merge trip >= 1", "last token of a ragged chunk"), seed=59)


# ---- F: exact ties (bitwise-equal logits in one row; identical rows with equal running scores)
def _equal(tokens, others=(), same_beams=(), seed=0):
    """A maker: the recipe, then ``tokens`` of beam ``same_beams[0]`` (of every batch row) all at 41, then the rows and
    running scores of ``same_beams[1:]`` made that beam's."""
    def make(case):
        beams = same_beams or (0,)
        logits, running = planted(case.seed, case.bsz, case.nb, case.vocab, [(beams[0], t) for t in others])
        for b in range(case.bsz):
            row = b * case.nb + beams[0]
            logits[row, list(tokens)] = 41.0
            running[b, beams[0]] = -LEAD * beams[0]
            for j in beams[1:]:
                logits[b * case.nb + j] = logits[row]
                running[b, j] = running[b, beams[0]]
        return logits, running
    return make


V2 = 8193
_add("F equal winners at tokens 4095 and 4096", 2, 2, V2, 4, [], seed=60, pipeline=False,
     make=_equal((4095, 4096), others=(17, 5000), same_beams=(1,)), index=[[V2 + 4095, V2 + 4096, V2 + 17, V2 + 5000]] * 2)
_add("F equal winners in chunk 1 of beam 0 and chunk 0 of beam 1", 2, 3, V2, 5, [], seed=61, pipeline=False,
     make=_equal((300, 6000), others=(4444,), same_beams=(0, 1)), index=[[300, 6000, V2 + 300, V2 + 6000, 4444]] * 2)
_add("F twenty equal at 4086..4105, keep 12", 1, 2, V2, 12, [], seed=62, pipeline=False,
     make=_equal(range(4086, 4106), same_beams=(1,)), index=[[V2 + t for t in range(4086, 4098)]])
_add("F twenty equal at 4086..4105 in three identical beams", 2, 3, V2, 12, [], seed=63, pipeline=False,
     make=_equal(range(4086, 4106), same_beams=(0, 1, 2)), index=[list(range(4086, 4098))] * 2)
_add("F sixteen equal in the registers of thread 63, keep 12", 1, 2, 4096, 12, [], seed=64, pipeline=False,
     make=_equal([tok(0, 63, r) for r in range(PER)], same_beams=(1,)), index=[[4096 + tok(0, 63, r) for r in range(12)]])
_add("F equal winners in four waves", 1, 1, 4096, 3, [], seed=65, pipeline=False,
     make=_equal((63, 64, 128, 192)), index=[[63, 64, 128]])


def _three_beams_256_slots_apart(case):
    """Beams 0, 4 and 8 of nine identical, 22 plants each, keep 64 over one chunk: the q-th plants tie at the slots q,
    256 + q and 512 + q, the three of one merge thread."""
    logits, running = planted(case.seed, case.bsz, case.nb, case.vocab, [(0, 7 + 173 * q) for q in range(22)])
    for j in (4, 8):
        logits[j] = logits[0]
        running[0, j] = running[0, 0]
    return logits, running


_add("F identical beams 0, 4 and 8 of nine: ties 256 slots apart", 1, 9, 4096, 64, [], seed=66, pipeline=False,
     make=_three_beams_256_slots_apart, classes=("merge thread owns >= 2", "merge trip >= 1"),
     index=[[j * 4096 + 7 + 173 * q for q in range(22) for j in (0, 4, 8)][:64]])


# ---- G: special values as data
INF, NAN = float("inf"), float("nan")
V3 = 2 * CHUNK + 808                        # three chunks, the last ragged


def _with(plants, edit):
    def make(case):
        logits, running = planted(case.seed, case.bsz, case.nb, case.vocab, plants)
        edit(logits, running)
        return logits, running
    return make


def _fill(row, lo, hi, value):
    def edit(logits, running):
        logits[row, lo:hi] = value
    return edit


G_PLANTS = [(0, 100), (1, 5000), (0, 8500), (1, 8999), (0, 4096), (1, 4095)]
for name, lo, hi in (("first", 0, CHUNK), ("middle", CHUNK, 2 * CHUNK), ("ragged last", 2 * CHUNK, V3)):
    plants = [(j, t) for j, t in G_PLANTS if not (j == 1 and lo <= t < hi)]
    _add(f"G the {name} chunk of beam 1 holds only -inf", 1, 2, V3, 4, plants, seed=70, pipeline=False,
         make=_with(plants, _fill(1, lo, hi, -INF)))


def _all_but_three(logits, running):
    keep = {0: (1, 4, 4097), 1: (0, 4095, 4199), 2: (3, 5, 4096), 3: (2, 4098, 4198)}
    for row, tokens in keep.items():
        saved = logits[row, list(tokens)].clone()
        logits[row] = -INF
        logits[row, list(tokens)] = saved
    running[:] = torch.tensor([[-0.25, -0.5], [-0.75, -0.125]])


_add("G all but three tokens of a row -inf", 2, 2, 4200, 12, [], seed=71, pipeline=False, make=_with([], _all_but_three))


def _set(row, token, value):
    def edit(logits, running):
        logits[row, token] = value
    return edit


def _run(b, beam, value):
    def edit(logits, running):
        running[b, beam] = value
    return edit


G_ROWS = [[(0, 10), (1, 4100), (2, 4999)], [(2, 20), (0, 4097), (1, 300)], [(1, 4095), (2, 4096), (0, 30)]]
V4 = 5000
_add("G one +inf logit", 3, 3, V4, 4, G_ROWS, seed=72, pipeline=False, make=_with(G_ROWS, _set(4, 4500, INF)),
     index=[None, [V4, V4 + 1, V4 + 2, V4 + 3], None])
_add("G a row of -inf only", 3, 3, V4, 4, G_ROWS, seed=73, pipeline=False, make=_with(G_ROWS, _fill(8, 0, V4, -INF)),
     index=[None, None, [2 * V4, 2 * V4 + 1, 2 * V4 + 2, 2 * V4 + 3]])
_add("G clean", 3, 3, V4, 4, G_ROWS, seed=74)
_add("G one NaN logit in beam 1 of 3", 3, 3, V4, 4, G_ROWS, seed=74, pipeline=False, make=_with(G_ROWS, _set(4, 4098, NAN)),
     index=[None, [V4, V4 + 1, V4 + 2, V4 + 3], None])
_add("G a running score of NaN", 3, 3, V4, 4, G_ROWS, seed=75, pipeline=False, make=_with(G_ROWS, _run(0, 2, NAN)),
     index=[[2 * V4, 2 * V4 + 1, 2 * V4 + 2, 2 * V4 + 3], None, None])
_add("G a running score of -inf", 3, 3, V4, 4, G_ROWS, seed=76, pipeline=False, make=_with(G_ROWS, _run(1, 0, -INF)))
_add("G a running score of +inf", 3, 3, V4, 4, G_ROWS, seed=77, pipeline=False, make=_with(G_ROWS, _run(2, 1, INF)),
     index=[None, None, [V4, V4 + 1, V4 + 2, V4 + 3]])
NAN_CASE, CLEAN_CASE = "G one NaN logit in beam 1 of 3", "G clean"

# ---- H: bans on plants (ban_ids ban a token in every row)
H1_BANS = (31, 32, 4095, CHUNK + 31, CHUNK + 32, 8191, 8192, 7000)
_add("H bans at tokens 31 | 32 of two chunks and at three chunk ends", 2, 2, 8193, 12,
     [(k % 2, t) for k, t in enumerate((31, 600, 32, 4095, 33, 4127, 30, 4128, 8191, 4129, 8192, 4126, 8190, 4094, 1, 4096,
                                        5555, 64, 3840))],
     ("chunk supplies fewer than keep",), seed=80, ban_ids=H1_BANS)
H2_BANS = tuple(sorted([CHUNK + 299, CHUNK + 31, CHUNK + 32, 0, 255, 256] + [1000 + 7 * k for k in range(10)]))
_add("H sixteen ban_ids, a ragged chunk's last token among them", 1, 3, CHUNK + 300, 4,
     [(2, CHUNK + 299), (1, CHUNK + 298), (2, 0), (0, CHUNK + 32), (1, 255), (2, CHUNK + 33), (0, 256), (1, 1007), (0, 1008),
      (2, CHUNK + 31), (1, 4095)],
     ("chunk supplies 1",), seed=81, ban_ids=H2_BANS)
_add("H the three best of one thread banned", 1, 2, 4096, 12,
     [(1, tok(0, 200, r)) for r in (3, 0, 15, 7, 1, 2, 4, 5, 6, 8, 9, 10, 11, 12, 13)], ("thread owns 12",), seed=82,
     ban_ids=(tok(0, 200, 3), tok(0, 200, 0), tok(0, 200, 15)))

GROUPS = "ABCDEFGH"
PLANTED_GROUPS = "ABCDEH"
BY_LABEL = {c.label: c for c in TABLE}


def cases(group):
    return [c for c in TABLE if c.group == group]


# ------------------------------------------------------------------------------------------------ inputs and the reference

@functools.lru_cache(maxsize=None)
def _inputs(label):
    case = BY_LABEL[label]
    if case.make is not None:
        logits, running = case.make(case)
    else:
        logits, running = planted(case.seed, case.bsz, case.nb, case.vocab, case.plants)
    assert logits.shape == (case.bsz * case.nb, case.vocab) and running.shape == (case.bsz, case.nb)
    return logits, running


def inputs(case):
    """(logits, running) of a case: computed once, shared, not to be written to."""
    return _inputs(case.label)


@functools.lru_cache(maxsize=None)
def _expected(label):
    case = BY_LABEL[label]
    logits, running = inputs(case)
    args = (logits.numpy(), running.numpy(), case.keep, None, 0, 0, case.ban_ids)
    want_v, want_i = BS.reference(*args)
    return want_v, want_i, BS.gap(*args)


def expected(case):
    """(top_value float64, top_index, gap) of BS.reference and BS.gap: computed once, shared, not to be written to."""
    return _expected(case.label)


def unbanned_plants(case):
    """Per batch row, the flat indices of the plants no ban_id bans."""
    return [sorted(beam * case.vocab + t for beam, t in row if t not in case.ban_ids) for row in per_row(case.plants, case.bsz)]


# ------------------------------------------------------------------------------------------------ coverage

CLASSES = (("register 0", "register 15")
           + tuple(f"wave {w} lane {lane}" for w in range(4) for lane in (0, 63))
           + ("first token of a full chunk", "last token of a full chunk", "first token of a ragged chunk",
              "last token of a ragged chunk", "thread owns 2", "thread owns 12", "thread owns 16",
              "chunk supplies 0", "chunk supplies 1", "chunk supplies fewer than keep", "chunk supplies keep",
              "merge slot 0", "merge slot 255", "merge slot 256", "merge slot n-1", "merge trip >= 1",
              "merge thread owns >= 2", "nb 64 and keep 64"))


def classes_hit(case):
    """The ownership classes that the winners of a case -- the reference's top ``keep`` of every batch row -- fall into."""
    logits, running = inputs(case)
    _, want_i, _ = expected(case)
    v = BS.values(logits.numpy(), running.numpy(), ban_ids=case.ban_ids)
    chunks, keep, vocab = chunks_of(case.vocab), case.keep, case.vocab
    n = case.nb * chunks * keep
    hit = set()
    if case.nb == 64 and keep == 64:
        hit.add("nb 64 and keep 64")
    for b in range(case.bsz):
        per_thread, per_chunk, per_merge_thread = {}, {}, {}
        for idx in want_i[b].tolist():
            beam, t = divmod(idx, vocab)
            o = owner(t)
            length = chunk_len(vocab, o.chunk)
            if o.register in (0, PER - 1):
                hit.add(f"register {o.register}")
            if o.lane in (0, WAVE - 1):
                hit.add(f"wave {o.wave} lane {o.lane}")
            kind = "full" if length == CHUNK else "ragged"
            if o.i == 0:
                hit.add(f"first token of a {kind} chunk")
            if o.i == length - 1:
                hit.add(f"last token of a {kind} chunk")
            c0 = beam * vocab + o.chunk * CHUNK
            first = BS.order(v[b, c0:c0 + length])[:keep].tolist()      # the chunk's candidate list, as the chunk kernel leaves it
            p = merge_slot(beam, o.chunk, first.index(o.i), chunks, keep)
            thread, trip = merge_owner(p)
            for slot, name in ((0, "0"), (255, "255"), (256, "256"), (n - 1, "n-1")):
                if p == slot:
                    hit.add(f"merge slot {name}")
            if trip >= 1:
                hit.add("merge trip >= 1")
            per_thread[beam, o.chunk, o.thread] = per_thread.get((beam, o.chunk, o.thread), 0) + 1
            per_chunk[beam, o.chunk] = per_chunk.get((beam, o.chunk), 0) + 1
            per_merge_thread[thread] = per_merge_thread.get(thread, 0) + 1
        for count in per_thread.values():
            if count in (2, 12, 16):
                hit.add(f"thread owns {count}")
        if len(per_chunk) < case.nb * chunks:
            hit.add("chunk supplies 0")
        for count in per_chunk.values():
            hit.add("chunk supplies 1" if count == 1 else "chunk supplies keep" if count == keep
                    else "chunk supplies fewer than keep")
        if max(per_merge_thread.values()) >= 2:
            hit.add("merge thread owns >= 2")
    return hit

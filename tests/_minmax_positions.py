"""Where an element of the input is read by the min/max kernels of csrc/observer.hip, and planted inputs that put the
extremum at every such place: observe_flat_kernel, observe_rows_kernel, observe_channels_kernel, token_minmax_vec_kernel
(single segment and head split), token_minmax_generic_kernel and token_minmax_multi_kernel.  No GPU and no torch device
is needed to import this module; tests/test_oracle_minmax_positions.py holds the index models against brute-force
walkers of the same loops on the CPU, tests/test_gpu_minmax_positions.py runs the cases.

A CLASS of an access is a tuple (part, axis, value): `part` names the loop that reads the element (unrolled body trip 1 /
trip >= 2 with the load a..d or u = 0..2, remainder loop trip, scalar tail trip, ...), `axis` one coordinate of the reader
(granule element, lane, wave, workgroup, token slot, ...) and `value` its class (first / last / interior, a number).  A
kernel that skips one element skips it by its loop and ONE of those coordinates, so the cases must reach every such triple;
the full product of all coordinates would be thousands of launches per size and adds nothing a skipped element can hide in.

Every value is exact in fp32, bf16 and fp16: data is built as float32 and converts to the 16-bit types without rounding.
"""
import numpy as np

from oracle import observer_oracle as OB

F32 = np.float32

# ------------------------------------------------------------------ the launchers' constants, each with the line it restates
THREADS = 256           # observer.hip: constexpr int kThreads = 256;
WAVE = 64               # osq_device.h: #define OSQ_WAVE 64
WAVES = THREADS // WAVE     # observer.hip: constexpr int kWavesPerBlock = kThreads / OSQ_WAVE;
OBS_BLOCKS = 768        # observer.hip: OSQ_AB_KNOB(int, g_obs_blocks, 768);
MAX_BLOCKS = 2048       # osq_host.h:   constexpr int kMaxBlocks = 2048;
FLAT_UNROLL = 4         # observer.hip: for (; i + 3 * stride < ng; i += 4 * stride)   and  grid_for(..., kThreads * 4, g_obs_blocks)
GRANULE = {4: 4, 2: 8}      # osq_device.h: Granule<float>::kPer = 4, Granule<T>::kPer = 8 (bf16 / fp16), by itemsize
ROW_LOADS = {4: 4, 2: 2}    # osq_device.h: Granule<float>::kRowLoads = 4, Granule<T>::kRowLoads = 2
TOK_PER_WAVE = 4        # observer.hip: constexpr int kTokPerWave = 4;
TOK_PER_BLOCK = 16      # observer.hip: constexpr int kTokPerBlock = kTokPerWave * kWavesPerBlock;
TOK_STEP = 3            # observer.hip: for (; j + 2 * OSQ_WAVE < inner_g; j += 3 * OSQ_WAVE)   (also both vector loops of the multi kernel)
ROWS_CAP = MAX_BLOCKS * 4   # observer.hip: grid_for(channels, kWavesPerBlock, kMaxBlocks * 4)
TOKEN_CAP = MAX_BLOCKS * 8  # observer.hip: grid_for(v.batch * v.tokens, kWavesPerBlock, kMaxBlocks * 8)   (generic token kernel, multi kernel)
FINISH_PER = MAX_BLOCKS // THREADS   # observer.hip: constexpr int kPer = kMaxBlocks / kThreads;   (raw[j], j = 0..7, of the finishing workgroup)
# the one-launch step (fused_step.h); its grid is one workgroup per CU (observer.hip, persistent_grid_for: return cus[dev];)
FUSED_THREADS = 1024    # fused_step.h: constexpr int kFusedThreads = 1024;
FUSED_WAVES = FUSED_THREADS // WAVE     # fused_step.h: constexpr int kFusedWaves = kFusedThreads / OSQ_WAVE;
FUSED_HOLD_REGS = 18    # fused_step.h: constexpr int kFusedHoldRegs = 18;   (SR = kFusedHoldRegs / NV tokens of a wave stay in registers)
FUSED_HOLD_LDS = 9      # fused_step.h: constexpr int kFusedHoldLds = 9;     (SL = kFusedHoldLds / NV more in LDS; the rest is streamed)


def grid_for(items, per_block, cap=MAX_BLOCKS):
    """osq_host.h: grid_for."""
    return max(1, min(cap, (items + per_block - 1) // per_block))


def lg_group(inner_g):
    """observer.hip: lgG = 0; while ((1 << lgG) < inner_g && lgG < 6) ++lgG;   (head-split form; 6 for one segment)."""
    lg = 0
    while (1 << lg) < inner_g and lg < 6:
        lg += 1
    return lg


def edge(i, n):
    """first / last / interior of 0..n-1 (a single one is `first`)."""
    return "first" if i == 0 else ("last" if i == n - 1 else "mid")


def trip_name(t):
    return "1" if t == 0 else "2+"


def unrolled_part(v, cnt, unroll, names="abcd"):
    """The v-th of the cnt visits one thread makes in  `for (; i + (U-1)*S < n; i += U*S) body;  for (; i < n; i += S) rem;`:
    the body takes cnt // U trips of U loads, the remainder loop the rest."""
    body = (cnt // unroll) * unroll
    if v < body:
        return "body%s%s" % (trip_name(v // unroll), names[v % unroll])
    return "rem%d" % (v - body + 1)


# ================================================================== observe_flat_kernel

FLAT_PARTS = (["body%s%s" % (t, l) for t in ("1", "2+") for l in "abcd"] + ["rem1", "rem2", "rem3", "tail1", "tail2+"])
_EDGE_CODE = {"first": 0, "last": 1, "mid": 2}
_EDGE_NAME = {v: k for k, v in _EDGE_CODE.items()}


def flat_geometry(n, itemsize, aligned=True, blocks=OBS_BLOCKS):
    """observer.hip, observe_flat(): ng = aligned16(x) ? n / kPer : 0;  grid_for(ng ? ng : ceil(n / kPer), kThreads * 4, g_obs_blocks)."""
    per = GRANULE[itemsize]
    ng = n // per if aligned else 0
    grid = grid_for(ng if ng else (n + per - 1) // per, THREADS * FLAT_UNROLL, blocks)
    return per, ng, grid


def _wg_code(wg, grid):
    """Workgroup class as an integer: 0 first, 1 last, 2 interior, else the workgroup's own number when it lies next to a
    multiple of kThreads (m*256 - 1, m*256, m*256 + 1: either side of the step from raw[m - 1] to raw[m] in the finisher)."""
    wg = np.asarray(wg, np.int64)
    code = np.full(wg.shape, 2, np.int64)
    r = wg % THREADS
    near = (wg >= THREADS - 1) & ((r == 0) | (r == 1) | (r == THREADS - 1))
    code = np.where(near, wg + 16, code)
    code = np.where(wg == grid - 1, 1, code)
    return np.where(wg == 0, 0, code)


def wg_name(code):
    return _EDGE_NAME[int(code)] if code < 16 else str(int(code) - 16)


def _lane_code(lane):
    lane = np.asarray(lane, np.int64)
    return np.where(lane == 0, 0, np.where(lane == WAVE - 1, 1, 2))


def flat_model(n, itemsize, aligned=True, blocks=OBS_BLOCKS):
    """int64 [ng + tail, 4] = (part, lane class, wave, workgroup class) of the access that reads each UNIT, in closed form:
    unit u < ng is granule u (elements u * kPer .. u * kPer + kPer - 1, one 16-byte load), unit ng + k is tail element
    ng * kPer + k (one scalar load)."""
    per, ng, grid = flat_geometry(n, itemsize, aligned, blocks)
    S = grid * THREADS
    u = np.arange(ng + (n - ng * per), dtype=np.int64)
    vec = u < ng
    tid = np.where(vec, u % S, (u - ng) % S)
    visit = np.where(vec, u // S, (u - ng) // S)
    cnt = (ng - tid + S - 1) // S                                  # granules this thread visits
    body = (cnt // FLAT_UNROLL) * FLAT_UNROLL
    part_body = np.where(visit // FLAT_UNROLL == 0, 0, 4) + visit % FLAT_UNROLL          # body1a..d = 0..3, body2+a..d = 4..7
    part_rem = 8 + (visit - body)                                                         # rem1..3 = 8..10
    part_tail = np.where(visit == 0, 11, 12)
    out = np.empty((u.size, 4), np.int64)
    out[:, 0] = np.where(vec, np.where(visit < body, part_body, part_rem), part_tail)
    out[:, 1] = _lane_code(tid % WAVE)
    out[:, 2] = (tid % THREADS) // WAVE
    out[:, 3] = _wg_code(tid // THREADS, grid)
    return out


def flat_walk(n, itemsize, aligned=True, blocks=OBS_BLOCKS):
    """The same by running the kernel's three loops for every thread of the grid at once (one array entry per thread)."""
    per, ng, grid = flat_geometry(n, itemsize, aligned, blocks)
    S = grid * THREADS
    out = np.full((ng + n - ng * per, 4), -9, np.int64)
    tid = np.arange(S, dtype=np.int64)
    who = np.stack([_lane_code(tid % WAVE), (tid % THREADS) // WAVE, _wg_code(tid // THREADS, grid)], 1)

    def mark(active, unit, part):
        out[unit[active], 0] = part
        out[unit[active], 1:] = who[active]

    i, trip = tid.copy(), 0
    while True:                                                   # for (; i + 3 * stride < ng; i += 4 * stride)
        act = i + 3 * S < ng
        if not act.any():
            break
        for l in range(FLAT_UNROLL):
            mark(act, i + l * S, (0 if trip == 0 else 4) + l)
        i = np.where(act, i + 4 * S, i)
        trip += 1
    r = 0
    while True:                                                   # for (; i < ng; i += stride)
        act = i < ng
        if not act.any():
            break
        mark(act, i, 8 + r)
        i = np.where(act, i + S, i)
        r += 1
    j, trip = ng * per + tid, 0
    while True:                                                   # for (j = ng * kPer + tid; j < n; j += stride)
        act = j < n
        if not act.any():
            break
        mark(act, ng + (j - ng * per), 11 if trip == 0 else 12)
        j = j + S
        trip += 1
    return out


def flat_representatives(n, itemsize, aligned=True, blocks=OBS_BLOCKS, table=None):
    """[(element index, (part, elem, lane, wave, wg))]: per part, greedily the unit that covers most (axis, value) pairs not
    covered yet, then further units until the part has seen every granule element 0..kPer-1.  Works on the distinct rows of
    the table, so a table of millions of units costs one np.unique."""
    per, ng, _ = flat_geometry(n, itemsize, aligned, blocks)
    if table is None:
        table = flat_model(n, itemsize, aligned, blocks)
    key = ((table[:, 0] * 4 + table[:, 1]) * 4 + table[:, 2]) * 4096 + table[:, 3]
    _, first = np.unique(key, return_index=True)
    rows = table[first]
    reps = []
    for p in np.unique(rows[:, 0]):
        sel = np.flatnonzero(rows[:, 0] == p)
        need = [set(np.unique(rows[sel, a]).tolist()) for a in range(1, 4)]
        picked = []
        while any(need):
            score = np.zeros(sel.size, np.int64)
            for a in range(3):
                score += np.isin(rows[sel, a + 1], list(need[a]))
            k = sel[int(np.argmax(score))]
            for a in range(3):
                need[a].discard(int(rows[k, a + 1]))
            picked.append(k)
        vec = p < 11
        m = 0
        while vec and len(picked) < per:                          # more units of this part, so that every element gets its turn
            picked.append(sel[m % sel.size])
            m += 1
        for q, k in enumerate(picked):
            unit = int(first[k])
            e = q % per if vec else -1
            idx = unit * per + e if vec else ng * per + (unit - ng)
            reps.append((idx, (FLAT_PARTS[int(p)], e, _EDGE_NAME[int(rows[k, 1])], int(rows[k, 2]), wg_name(rows[k, 3]))))
    return reps


def flat_classes(reps):
    """The (part, axis, value) triples a list of representatives reaches."""
    out = set()
    for _, (p, e, lane, wave, wg) in reps:
        if e >= 0:
            out.add((p, "elem", e))
        out |= {(p, "lane", lane), (p, "wave", wave), (p, "wg", wg)}
    return out


def flat_class_of(idx, n, itemsize, aligned=True, blocks=OBS_BLOCKS):
    """The class tuple of ONE element index, by the closed form (what the dropped-element check names)."""
    per, ng, grid = flat_geometry(n, itemsize, aligned, blocks)
    S = grid * THREADS
    if idx < ng * per:
        g, e = divmod(idx, per)
        tid, v = g % S, g // S
        part = unrolled_part(v, (ng - tid + S - 1) // S, FLAT_UNROLL)
    else:
        e = -1
        tid, v = (idx - ng * per) % S, (idx - ng * per) // S
        part = "tail" + trip_name(v)
    return (part, e, edge(tid % WAVE, WAVE), (tid % THREADS) // WAVE, wg_name(int(_wg_code(tid // THREADS, grid))))


def flat_all_classes(itemsize, blocks=OBS_BLOCKS):
    """Every class observe_flat_kernel has on a grid capped at `blocks` workgroups, with what no input can reach left out
    (and said why): the list the cases' union is held against."""
    per = GRANULE[itemsize]
    wgs = {"first"}
    if blocks > 1:
        wgs.add("last")
    if blocks > 2:
        wgs.add("mid")
    for m in range(1, FINISH_PER + 1):
        for w in (m * THREADS - 1, m * THREADS, m * THREADS + 1):
            if 0 < w < blocks - 1:
                wgs.add(str(w))
    out = set()
    for p in FLAT_PARTS:
        if not p.startswith("tail"):
            out |= {(p, "elem", e) for e in range(per)}
        out |= {(p, "lane", v) for v in ("first", "last", "mid")}
        out |= {(p, "wave", w) for w in range(WAVES)}
        out |= {(p, "wg", w) for w in wgs}
    return out


# (shape name) -> (n as a function of kPer, aligned).  S = 768 * 256 granules is one stride of the capped grid.
_S = OBS_BLOCKS * THREADS
FLAT_SIZES = [
    ("n1", lambda per: 1, True), ("per-1", lambda per: per - 1, True), ("per", lambda per: per, True), ("per+1", lambda per: per + 1, True),
    ("ng1023", lambda per: 1023 * per, True), ("ng1024", lambda per: 1024 * per, True),             # ng 1024: one unrolled trip on grid 1
    ("ng1025+1", lambda per: 1025 * per + 1, True),                                                  # grid 2: no unrolled trip, a tail
    ("ng2047", lambda per: 2047 * per, True), ("ng2048", lambda per: 2048 * per, True),
    ("grid257", lambda per: (256 * 1024 + 1) * per + 3, True),                                       # workgroups 255 / 256 (last)
    ("grid259", lambda per: (258 * 1024 + 1) * per, True),                                           # ... and 257 as an interior one
    ("capped", lambda per: (8 * _S + _S // 2 + 37) * per + per - 1, True),                           # second unrolled trip + remainder + tail
    ("capped_rem3", lambda per: (7 * _S + 5) * per, True),                                           # three remainder trips behind one body trip
    ("misaligned", lambda per: 4099, False),
    ("misaligned_grid515", lambda per: 514 * 1024 * per + 5, False),                                 # the scalar loop on every workgroup class, many trips
]
FLAT_LARGE = {"grid257", "grid259", "capped", "capped_rem3", "misaligned_grid515"}


def flat_knob_sizes(blocks, per):
    """Sizes for a grid capped at `blocks` workgroups (tunable build): two and a half unrolled trips plus a tail, three
    remainder trips; for 2048 one size that fills the grid (the finishing workgroup's whole raw[] read)."""
    S = blocks * THREADS
    if blocks == MAX_BLOCKS:
        return [((blocks - 1) * 1024 + 1) * per + 1]
    return [(8 * S + S // 2 + 37) * per + per - 1, (7 * S + 5) * per, (4 * S) * per]


# ================================================================== planted values

def grid_values(rng, shape):
    """Base data: multiples of 2^-6 in [-1, 1], exact in bf16 (8 significant bits) and fp16."""
    return (rng.integers(-64, 65, size=shape).astype(F32) / F32(64.0)).astype(F32)


def next_above_one(itemsize, lowp="bf16"):
    """The format's next value beyond 1.0."""
    if itemsize == 4:
        return F32(1.0) + F32(2.0 ** -23)
    return F32(1.0 + (2.0 ** -7 if lowp == "bf16" else 2.0 ** -10))


SUBNORMAL = F32(1e-40)


def kinds_for(itemsize, lowp="bf16"):
    """The planted kinds as (name, base sign, planted maximum, planted minimum).  Base sign 0: the data as drawn, +1: its
    magnitude (data >= +0.0, zeros +0.0), -1: minus its magnitude (data <= -0.0, zeros -0.0).  A planted minimum of None
    leaves the base value where the minimum would go."""
    u = next_above_one(itemsize, lowp)
    ks = [
        ("finite", 0, F32(3.5), F32(-2.75)),
        ("ulp", 0, u, -u),
        ("neg_zero_min", +1, F32(3.5), F32(-0.0)),        # data >= +0.0 with zeros, one -0.0: the minimum is the word 0x80000000
        ("pos_zero_max", -1, F32(0.0), F32(-3.5)),        # data <= -0.0 with zeros, one +0.0: the maximum is the word 0x00000000
        ("inf", 0, F32(np.inf), F32(-np.inf)),
        ("nan", 0, F32(np.nan), None),                    # a NaN where the maximum would go: both outputs NaN
    ]
    if itemsize == 4:
        ks.append(("subnormal", -1, SUBNORMAL, F32(-3.5)))   # an fp32 subnormal as the only positive value
    return ks


def signed_base(base, sign):
    """The base data of a kind: as drawn, or its magnitude with one sign (zeros take that sign too)."""
    if sign == 0:
        return base
    a = np.abs(base)
    return a if sign > 0 else -a          # -(+0.0) = -0.0


def expected_pair(values):
    """(min, max) of the oracle (IEEE rule for the zeros, NaN poisons both) of a flat fp32 array."""
    v = np.asarray(values, F32).reshape(-1)
    if np.isnan(v).any():
        return F32(np.nan), F32(np.nan)
    return OB.aminmax(v)


def flat_pairs(reps):
    """[(index of the planted maximum, index of the planted minimum or None)]: every representative holds the maximum once
    and, half the list further on, the minimum once."""
    idx = [i for i, _ in reps]
    m = len(idx)
    out = []
    for k, i in enumerate(idx):
        j = idx[(k + m // 2 + 1) % m]
        out.append((i, j if j != i else None))
    return out


def plant_flat(base, kind, imax, imin):
    """(array, expected min, expected max) for one launch: base with the kind's sign, the kind's maximum at imax and its
    minimum at imin.  With both planted the extremes are known by construction (the planted values lie outside the base
    range; the zeros outside it by their sign); with one element only the other extreme is the oracle's over the array."""
    name, sign, vmax, vmin = kind
    x = signed_base(base, sign).copy()
    x[imax] = vmax
    if imin is not None and vmin is not None:
        x[imin] = vmin
    if name == "nan":
        return x, F32(np.nan), F32(np.nan)
    if imin is not None and vmin is not None:
        return x, vmin, vmax
    return x, OB.aminmax(x)[0], vmax


def ordered_key(a):
    """int64 keys that order fp32 values the way the oracle's min / max do: by value, -0.0 below +0.0 (no NaN in base data)."""
    b = np.ascontiguousarray(a, F32).view(np.int32).astype(np.int64)
    return np.where(b < 0, -(b & 0x7FFFFFFF) - 1, b)


def flat_ends(x, k=3):
    """(indices of the k smallest, indices of the k largest) elements of x in the oracle's order, each list in order."""
    key = ordered_key(x)
    k = min(k, x.size)
    lo = np.argpartition(key, k - 1)[:k]
    hi = np.argpartition(-key, k - 1)[:k]
    return lo[np.argsort(key[lo], kind="stable")], hi[np.argsort(-key[hi], kind="stable")]


def flat_rest_pair(x, ends, skip):
    """(min, max) of x without the elements at the indices `skip` (at most two), from flat_ends(x, 3)."""
    lo, hi = ends
    return x[[i for i in lo if i not in skip][0]], x[[i for i in hi if i not in skip][0]]


def flat_base(n, seed):
    """Base data of a flat case; sizes of eight or more hold both ends of the range and a zero somewhere, so that `ulp` (one
    step beyond +-1.0) is the NEXT value up and a planted zero meets a zero of the other sign.  Below eight elements there is
    no room beside the planted pair: there `ulp` is merely a larger value."""
    x = grid_values(np.random.default_rng(seed), n)
    if n >= 8:
        x[n // 3], x[n // 3 + 1] = 1.0, -1.0
        x[n // 5] = 0.0
    return x


# ================================================================== token_minmax_multi_kernel (fp32)

def multi_column_parts(vec, feat_outer, feat_inner):
    """Loop part of every feature of a site's token.  Vector descriptors walk the F4 = feat_outer * feat_inner / 4 float4s
    of the token three steps of 64 at a time (one loop for feat_outer == 1, one with the segment division for head-split
    views); scalar descriptors walk the F elements 64 at a time."""
    if vec:
        parts = column_parts(feat_outer * feat_inner // 4, TOK_STEP, "012")
        kind = "one" if feat_outer == 1 else "split"
        return ["%s_%s" % (kind, p) for p in parts for _ in range(4)]
    return ["scalar_trip%s" % ("1" if j < WAVE else "2+") for j in range(feat_outer * feat_inner)]


def multi_all_parts():
    vec = ["body%s%s" % (t, u) for t in ("1", "2+") for u in "012"] + ["rem1", "rem2"]
    return {"%s_%s" % (k, p) for k in ("one", "split") for p in vec} | {"scalar_trip1", "scalar_trip2+"}


# ================================================================== per-row kernels: column classes

def column_parts(inner_g, unroll, names="abcd"):
    """Per granule 0..inner_g-1 of a row walked by one wave (lane = g % 64, U loads per trip): the loop part."""
    out = []
    for g in range(inner_g):
        lane, v = g % WAVE, g // WAVE
        cnt = (inner_g - lane + WAVE - 1) // WAVE
        out.append(unrolled_part(v, cnt, unroll, names))
    return out


def column_parts_walk(inner_g, unroll, names="abcd"):
    """The same by running `for (; j + (U-1)*64 < inner_g; j += U*64) ...; for (; j < inner_g; j += 64) ...` per lane."""
    out = [None] * inner_g
    for lane in range(WAVE):
        j, trip = lane, 0
        while j + (unroll - 1) * WAVE < inner_g:
            for u in range(unroll):
                out[j + u * WAVE] = "body%s%s" % (trip_name(trip), names[u])
            j += unroll * WAVE
            trip += 1
        r = 0
        while j < inner_g:
            out[j] = "rem%d" % (r + 1)
            j += WAVE
            r += 1
    return out


# ---- observe_rows_kernel: wave (blockIdx.x * 256 + threadIdx.x) / 64 walks rows wave, wave + nwaves, ...
def rows_inner_g(L):
    """The issue's list plus (L - 1) * 64: the only size at which the LAST remainder trip runs on every lane (fp32: 192)."""
    return tuple(sorted({1, 63, 64, 65, (L - 1) * 64, L * 64 - 1, L * 64, L * 64 + 1, 2 * L * 64 + 1}))


ROWS_COUNTS = (1, 3, 4, 5)
ROWS_TRIP2 = ROWS_CAP * WAVES + 3             # rows above 4 * kMaxBlocks * 4 with inner_g = 1: the row loop's second trip


def rows_row_class(r, rows):
    grid = grid_for(rows, WAVES, ROWS_CAP)
    nw = grid * WAVES
    wave = r % nw
    return {("row", "wave", wave % WAVES), ("row", "wg", edge(wave // WAVES, grid)), ("row", "trip", trip_name(r // nw))}


def rows_all_classes(itemsize):
    per, L = GRANULE[itemsize], ROW_LOADS[itemsize]
    parts = ["body%s%s" % (t, l) for t in ("1", "2+") for l in "abcd"[:L]] + ["rem%d" % k for k in range(1, L)]
    out = set()
    for p in parts:
        out |= {(p, "elem", e) for e in range(per)} | {(p, "lane", v) for v in ("first", "last", "mid")}
    out |= {("row", "wave", w) for w in range(WAVES)} | {("row", "wg", v) for v in ("first", "last", "mid")}
    out |= {("row", "trip", "1"), ("row", "trip", "2+")}
    return out


# ---- observe_channels_kernel: workgroup = channel; thread j % 256 reads p[j], trip j / 256, for every outer index
CHANNELS_INNER = (1, 255, 256, 257, 513)
CHANNELS_OUTER = (1, 2, 3)


def channels_column_class(o, j, outer, inner):
    t = j % THREADS
    p = "trip%s" % ("1" if j < THREADS else ("2" if j < 2 * THREADS else "3+"))
    return {(p, "lane", edge(t % WAVE, WAVE)), (p, "wave", t // WAVE), (p, "outer", edge(o, outer))}


def channels_column_walk(outer, inner):
    """{(o, j): (trip, thread)} by running the kernel's two loops for the 256 threads."""
    out = {}
    for o in range(outer):
        for t in range(THREADS):
            j, trip = t, 0
            while j < inner:
                out[(o, j)] = (trip, t)
                j += THREADS
                trip += 1
    return out


def channels_all_classes():
    """Not reachable: trip3+ on lanes and waves other than the first -- the listed inner sizes end at 513, whose third trip
    is thread 0 alone."""
    out = set()
    for p in ("trip1", "trip2", "trip3+"):
        out |= {(p, "lane", v) for v in ("first", "last", "mid")} | {(p, "wave", w) for w in range(WAVES)}
        out |= {(p, "outer", v) for v in ("first", "last", "mid")}
    return out - {("trip3+", "lane", "last"), ("trip3+", "lane", "mid"), ("trip3+", "wave", 1), ("trip3+", "wave", 2), ("trip3+", "wave", 3)}


# ================================================================== token kernels

# the issue's list plus 130: the second remainder trip on interior lanes (65 has it on lane 0 only, 191 on lane 63 only)
TOKEN_SINGLE_INNER_G = (1, 63, 64, 65, 130, 191, 192, 193, 384, 385)
TOKEN_HEAD_INNER_G = (1, 2, 3, 4, 16, 64, 65)
TOKEN_GENERIC_F = (1, 63, 64, 65, 129)
TOKEN_LENGTHS = (0, 1, 2, 3, 4, 5, 15, 16, 17)        # and T
GENERIC_TRIP2_TOKENS = TOKEN_CAP * WAVES + 7          # more than 8 * kMaxBlocks * 4 tokens (F = 5): the token loop's second trip


def token_slot_class(b, t, length, T):
    """Classes of token t (< length) of sample b in token_minmax_vec_kernel: slot k of its wave, how many tokens that wave
    has, the wave, the chunk, and whether the chunk rotation moved the chunk off its own blockIdx.x."""
    chunks = (T + TOK_PER_BLOCK - 1) // TOK_PER_BLOCK
    chunk, w, k = t // TOK_PER_BLOCK, (t % TOK_PER_BLOCK) // TOK_PER_WAVE, t % TOK_PER_WAVE
    t0 = t - k
    ntok = min(TOK_PER_WAVE, length - t0)
    bx = (chunk - b) % chunks                          # chunk = (blockIdx.x + blockIdx.y) % gridDim.x
    return {("tok", "slot", (k, ntok)), ("tok", "wave", w), ("tok", "chunk", edge(chunk, chunks)),
            ("tok", "rotated", bx != chunk)}


def token_slot_walk(lengths, T):
    """{(b, t): (k, ntok, w, chunk, blockIdx.x)} by running the kernel's index arithmetic for every (blockIdx, wave)."""
    chunks = (T + TOK_PER_BLOCK - 1) // TOK_PER_BLOCK
    out = {}
    for by, ln in enumerate(lengths):
        ln = min(ln, T)
        for bx in range(chunks):
            chunk = (bx + by) % chunks
            for w in range(WAVES):
                t0 = chunk * TOK_PER_BLOCK + w * TOK_PER_WAVE
                if t0 >= ln:
                    continue
                ntok = min(ln - t0, TOK_PER_WAVE)
                for lane in range(ntok):                       # if (lane < ntok) store slot b * T + t0 + lane
                    out[(by, t0 + lane)] = (lane, ntok, w, chunk, bx)
    return out


def token_all_slot_classes():
    out = {("tok", "slot", (k, n)) for n in range(1, TOK_PER_WAVE + 1) for k in range(n)}
    out |= {("tok", "wave", w) for w in range(WAVES)} | {("tok", "chunk", v) for v in ("first", "last", "mid")}
    return out | {("tok", "rotated", False), ("tok", "rotated", True)}


def single_all_classes(itemsize):
    per = GRANULE[itemsize]
    parts = ["body%s%s" % (t, u) for t in ("1", "2+") for u in "012"] + ["rem1", "rem2"]
    out = set()
    for p in parts:
        out |= {(p, "elem", e) for e in range(per)} | {(p, "lane", v) for v in ("first", "last", "mid")}
    return out


def head_column(o, g, feat_outer, inner_g):
    """Head-split form: feature segment o, granule g of it -> (lgG, lane, part).  grp = lane >> lgG walks segments grp,
    grp + ngrp, ...; li = lane & (gl - 1) walks granules li, li + gl, ..."""
    lg = lg_group(inner_g)
    gl, ngrp = 1 << lg, WAVE >> lg
    grp, li = o % ngrp, g % gl
    part = "seg%s_g%s" % (trip_name(o // ngrp), trip_name(g // gl))
    return lg, grp * gl + li, part, grp, li


def head_classes(o, g, feat_outer, inner_g):
    lg, lane, part, grp, li = head_column(o, g, feat_outer, inner_g)
    gl, ngrp = 1 << lg, WAVE >> lg
    return {(part, "lgG", lg), (part, "grp", edge(grp, ngrp)), (part, "li", edge(li, gl)), (part, "lane", edge(lane, WAVE))}


def head_walk(feat_outer, inner_g):
    """{(o, g): (lane, segment trip, granule trip)} by running the kernel's two loops for the 64 lanes."""
    lg = lg_group(inner_g)
    gl, ngrp = 1 << lg, WAVE >> lg
    out = {}
    for lane in range(WAVE):
        grp, li = lane >> lg, lane & (gl - 1)
        o, ot = grp, 0
        while o < feat_outer:
            j, jt = li, 0
            while j < inner_g:
                out[(o, j)] = (lane, ot, jt)
                j += gl
                jt += 1
            o += ngrp
            ot += 1
    return out


def head_feat_outers(inner_g):
    """feat_outer below, at and above 64 >> lgG (at least 2: one segment is the single-segment kernel)."""
    ngrp = WAVE >> lg_group(inner_g)
    return sorted({max(2, ngrp - 1), max(2, ngrp), ngrp + 1, 2 * ngrp + 1})


def generic_column_class(j):
    p = "trip%s" % ("1" if j < WAVE else ("2" if j < 2 * WAVE else "3+"))
    return {(p, "lane", edge(j % WAVE, WAVE))}


# ---- token cases: (name, kind, B, T, feat_outer, feat_inner in elements as a function of kPer)
def token_cases(itemsize):
    """[(name, kind, lengths, T, feat_outer, feat_inner)]: kind "single" ([B,T,F]), "head" ([B,T,h,d] memory, seq_pos 1),
    "generic" ([B,T,F] from a misaligned pointer), "keyview" (a [B,h,d,T] tensor read with seq_pos 3: stride_inner = T).  T alternates between 32 (two chunks)
    and 37 (three, the last one short); the sample count between 10 / 11 / 12, co-prime and not with the chunk count."""
    per = GRANULE[itemsize]
    cases, k = [], 0

    def lengths_for(T, B):
        base = [min(l, T) for l in TOKEN_LENGTHS] + [T]
        return (base + [T, T - 1, 7, 0, T, 9])[:B]

    combos = ((32, 10), (37, 10), (37, 12), (32, 11))
    for ig in TOKEN_SINGLE_INNER_G:
        T, B = combos[k % 4]; k += 1
        cases.append(("single_ig%d" % ig, "single", lengths_for(T, B), T, 1, ig * per))
    for ig in TOKEN_HEAD_INNER_G:
        for fo in head_feat_outers(ig):
            if ig >= 64 and fo > 3:
                continue                                   # lgG = 6: one group of 64 lanes, every segment a new trip; 2 and 3 segments do
            T, B = combos[k % 4]; k += 1
            cases.append(("head_ig%d_h%d" % (ig, fo), "head", lengths_for(T, B), T, fo, ig * per))
    # seven segments of 64 granules: more than 384 float4 per fp32 token, the second 3-step trip of the multi kernel's head-split loop
    cases.append(("head_ig64_h7", "head", lengths_for(37, 10), 37, 7, 64 * per))
    for F in TOKEN_GENERIC_F:
        T, B = combos[k % 4]; k += 1
        cases.append(("generic_F%d" % F, "generic", lengths_for(T, B), T, 1, F))
    cases.append(("generic_keyview", "keyview", lengths_for(37, 10), 37, 3, 2 * per))      # [B, 3, 2 * kPer, T], seq_pos 3
    return cases


def token_kernel_of(kind, feat_outer, feat_inner, itemsize):
    """The launcher's choice (observer.hip, token_minmax()) for the layouts token_cases builds: the "generic" layout lies one
    element past a 16-byte boundary (aligned16(x) fails whatever F is), the key view has stride_inner = T."""
    if kind in ("keyview", "generic"):
        return "generic"
    assert feat_inner % GRANULE[itemsize] == 0
    return "single" if feat_outer == 1 else "head"


# ================================================================== planted per-row inputs

PAD_VALUES = (F32(np.nan), F32(np.inf), F32(-np.inf), F32(1e30), F32(-1e30))
SENTINEL = np.uint32(0x7FC5A5A5)        # a quiet NaN whose payload no arithmetic here produces


def rows_launches(n_valid, F, n_kinds, max_launches=24):
    """Launch list [(column offset, kind shift)]: valid row number i gets its maximum at column (i + offset) % F and kind
    (i + shift) % K.  Offsets step by the number of valid rows until every column has held the maximum (and, F/2 + 1 further
    on, the minimum); every offset runs with every shift while that stays within max_launches, else the shift cycles with
    the offset (kinds then meet every column CLASS rather than every column; the CPU test checks that they do)."""
    offs = list(range(0, F, max(n_valid, 1))) if n_valid < F else [0]
    if len(offs) * n_kinds <= max_launches:
        return [(o, s) for o in offs for s in range(n_kinds)]
    return [(o, k % n_kinds) for k, o in enumerate(offs)] + ([] if len(offs) >= n_kinds else [(0, s) for s in range(len(offs), n_kinds)])


def plant_rows(base, valid, offset, shift, kinds):
    """base [R, F] fp32 (grid values); valid [R] bool.  Returns (x [R, F], min [R], max [R], columns of the planted maxima,
    columns of the planted minima, kind index per row); rows that are not valid are filled with PAD_VALUES (NaN, +-inf,
    +-1e30 in turn) and expect nothing."""
    R, F = base.shape
    x = base.copy()
    rank = np.cumsum(valid) - 1
    cmax = (rank + offset) % F
    cmin = (cmax + F // 2 + 1) % F
    kidx = (rank + shift) % len(kinds)
    emin, emax = np.zeros(R, F32), np.zeros(R, F32)
    for r in range(R):
        if not valid[r]:
            x[r] = PAD_VALUES[r % len(PAD_VALUES)]
            continue
        name, sign, vmax, vmin = kinds[kidx[r]]
        if sign:
            x[r] = signed_base(x[r], sign)
        a, b = int(cmax[r]), int(cmin[r])
        if F >= 4:                                         # the neighbours that make the planted value the NEXT one, not just a far one
            na, nb = (a + 1) % F, (b + 1) % F
            if name == "ulp":
                x[r, na], x[r, nb] = 1.0, -1.0
            elif name == "neg_zero_min":
                x[r, nb] = 0.0
            elif name == "pos_zero_max":
                x[r, na] = -0.0
        x[r, a] = vmax
        two = vmin is not None and a != b
        if two:
            x[r, b] = vmin
        if name == "nan":
            emin[r] = emax[r] = np.nan
        elif two:
            emin[r], emax[r] = vmin, vmax
        else:                                              # F == 1: the one element is both
            emax[r] = vmax
            emin[r] = OB.zmin(x[r])
    return x, emin, emax, cmax, cmin, kidx


def oracle_rows(x):
    """Per-row (min, max) of the oracle; a NaN poisons both of its row."""
    mn, mx = OB.token_min_max(x)
    bad = np.isnan(x).any(axis=1)
    mn, mx = np.asarray(mn, F32).copy(), np.asarray(mx, F32).copy()
    mn[bad] = np.nan
    mx[bad] = np.nan
    return mn, mx


def dropped_rows_unchanged(x, emin, emax, cmax, cmin, valid):
    """The dropped-element check: with the planted maximum (minimum) removed from its row, that row's oracle maximum
    (minimum) must differ as a word.  Returns the (row, column, side) where it does not."""
    R, F = x.shape
    if F == 1:
        return []                                           # nothing is left of a one-column row: the answer goes with it
    rows = np.flatnonzero(valid)
    xs, bad = x[rows], []
    for side, cols, want in ((1, cmax, emax), (0, cmin, emin)):
        k = np.ones(xs.shape, bool)
        k[np.arange(rows.size), cols[rows]] = False
        rest = xs[k].reshape(rows.size, F - 1)
        got = oracle_rows(rest)[side]
        w, g = want[rows].copy().view(np.uint32), got.view(np.uint32)
        same = (w == g) | (np.isnan(want[rows]) & np.isnan(got))
        if side == 0:
            same &= ~(np.isnan(want[rows]) | (cmin[rows] == cmax[rows]))      # the NaN sits where the maximum goes only
        bad += [(int(rows[i]), int(cols[rows[i]]), side) for i in np.flatnonzero(same)]
    return bad


# ================================================================== the per-row cases

ROWS_MAX = 260          # rows / channels of a case whose columns outnumber them: the offsets cycle instead


def row_cases(itemsize):
    """Every per-row / per-token case of one element size: dicts with the kernel, the [R, F] row matrix geometry, which rows
    are valid, and how the rows are laid out in the tensor the entry point is given (test_gpu_minmax_positions.build_tensor)."""
    per, L = GRANULE[itemsize], ROW_LOADS[itemsize]
    out = []
    # observe_rows_kernel
    for ig in rows_inner_g(L):
        F = ig * per
        out.append(dict(name="rows_ig%d" % ig, kernel="rows", R=min(max(F, 9), ROWS_MAX), F=F, inner_g=ig))
    for rc in ROWS_COUNTS:
        for ig in (1, 65):
            out.append(dict(name="rows_r%d_ig%d" % (rc, ig), kernel="rows", R=rc, F=ig * per, inner_g=ig))
    out.append(dict(name="rows_trip2", kernel="rows", R=ROWS_TRIP2, F=per, inner_g=1, shifts=2))
    # observe_channels_kernel
    for inner in CHANNELS_INNER:
        for outer in CHANNELS_OUTER:
            out.append(dict(name="channels_i%d_o%d" % (inner, outer), kernel="channels", R=min(max(outer * inner, 5), ROWS_MAX),
                            F=outer * inner, outer=outer, inner=inner, misalign=(outer == 1 and inner % per == 0)))
    # the token kernels
    for name, kind, lengths, T, fo, fi in token_cases(itemsize):
        valid = np.concatenate([np.arange(T) < min(l, T) for l in lengths])
        out.append(dict(name="token_" + name, kernel=token_kernel_of(kind, fo, fi, itemsize), layout=kind, R=len(lengths) * T,
                        F=fo * fi, T=T, lengths=list(lengths), feat_outer=fo, feat_inner=fi, valid=valid))
    out.append(dict(name="token_generic_trip2", kernel="generic", layout="generic", R=GENERIC_TRIP2_TOKENS, F=5, T=GENERIC_TRIP2_TOKENS,
                    lengths=[GENERIC_TRIP2_TOKENS - 2], feat_outer=1, feat_inner=5, shifts=2,
                    valid=np.arange(GENERIC_TRIP2_TOKENS) < GENERIC_TRIP2_TOKENS - 2))
    for c in out:
        c.setdefault("valid", np.ones(c["R"], bool))
    return out


def case_seed(name):
    return sum((k + 1) * ord(ch) for k, ch in enumerate(name)) % (2 ** 31)


def case_launches(case, kinds):
    """Yield (x [R, F], expected min, expected max, cmax, cmin, kind index per row) for every launch of a case."""
    base = grid_values(np.random.default_rng(case_seed(case["name"])), (case["R"], case["F"]))
    launches = rows_launches(int(case["valid"].sum()), case["F"], len(kinds))
    if "shifts" in case:
        launches = launches[:case["shifts"]]
    for off, shift in launches:
        yield plant_rows(base, case["valid"], off, shift, kinds)


def column_classes(case, itemsize):
    """Per column 0..F-1 of a case's rows: the set of (part, axis, value) classes of the access that reads it."""
    per, k = GRANULE[itemsize], case["kernel"]
    F = case["F"]
    if k == "rows":
        parts = column_parts(case["inner_g"], ROW_LOADS[itemsize])
        return [{(parts[j // per], "elem", j % per), (parts[j // per], "lane", edge((j // per) % WAVE, WAVE))} for j in range(F)]
    if k == "channels":
        return [channels_column_class(j // case["inner"], j % case["inner"], case["outer"], case["inner"]) for j in range(F)]
    if k == "single":
        parts = column_parts(F // per, TOK_STEP, "012")
        return [{(parts[j // per], "elem", j % per), (parts[j // per], "lane", edge((j // per) % WAVE, WAVE))} for j in range(F)]
    if k == "head":
        fi = case["feat_inner"]
        return [head_classes(j // fi, (j % fi) // per, case["feat_outer"], fi // per) | {("head", "elem", j % per)} for j in range(F)]
    return [generic_column_class(j) for j in range(F)]


# ================================================================== the multi-site table of the fp32 token cases

def multi_launch_count(runs):
    """Table launches of the multi-site test: as many as the site with the most launches has (runs: per site its launch list);
    table launch l takes launch l % len of every site, so every launch of every site is used."""
    return max(len(r) for r in runs)

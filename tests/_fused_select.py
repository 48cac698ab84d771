"""The selectors of the one-launch observe + fake-quant step (csrc/fused_step.h: fused_select<CH>, and select_from_registers of
csrc/token_select.h behind it): a model of the chunk geometry, a model of the DECISIONS of the selection, the enumeration of
the tokens, and the case tables.  No GPU and no torch device is needed to import this module;
tests/test_oracle_fused_select.py holds the models against a brute-force walk of the kernel's loads and asserts what the
tables reach, tests/test_gpu_fused_select.py runs the cases.

Expected values never come from here: the statistics are the oracle's (oracle/observer_oracle.py), y is the oracle's
(oracle/fake_quant_oracle.py).  select_path() only says WHICH branch a case takes, so that a case's name can be asserted.
"""
import numpy as np

import _minmax_positions as MP
from oracle import observer_oracle as OB

F32 = np.float32
WAVE = MP.WAVE
NC = MP.FUSED_WAVES         # fused_step.h:113  constexpr int NC = kFusedWaves;   (chunks per selector wave)
NG = 2                      # fused_step.h:140  #define OSQ_FUSED_GROUPS 2
GC = NC // NG               # fused_step.h:142  constexpr int NG = OSQ_FUSED_GROUPS, GC = NC / NG;
MAX_CH = 3                  # observer.hip, launch_fused: (B*T + grid - 3) / (grid - 2) > 3 * OSQ_WAVE -> three launches
MAX_NWG = NC * NC           # observer.hip, launch_fused: grid - 2 > kFusedWaves * kFusedWaves -> three launches
MAX_SLOTS = 32768           # observer.hip, osq_observe_tokens_fake_quant: slots <= 4 * 8 * kSelThreads
MAX_BATCH = 1024            # fused_step.h:40   constexpr int kFusedMaxBatch = 1024;
FUSED_NV = (3, 4, 12, 16)   # observer.hip: nv == 3 || nv == 4 || nv == 12 || nv == 16   (H = 256 * nv)
SEL_BINS = 2048             # observer.hip: constexpr int kSelBins = 2048;
SEL_BITS = 11               # observer.hip: constexpr int kSelBits = 11;
LIST_CAP = 1024             # observer.hip: constexpr int kListCap = 1024;
SENTINEL_Y = 0x7FC0BEEF     # a quiet NaN whose payload no arithmetic here produces: what y holds before every launch


# ================================================================== chunk geometry (fused_step.h:125-152)

def geometry(nwg, total, V):
    """fused_step.h:125-152 as plain integers, and fused_step.h:394-398 for CH."""
    qt, rt = divmod(total, nwg)                 # :126  chunk g starts at g * qt + min(g, rt)
    qv, rv = divmod(V, nwg)                     # :127  ... and holds qv + (g < rv) valid values
    cmax = qv + (1 if rv else 0)                # :144
    CH = 1 if cmax <= WAVE else (2 if cmax <= 2 * WAVE else 3)      # :396-398
    tlen = cmax - WAVE * (CH - 1)               # :145
    lt = 0 if tlen <= 1 else (tlen - 1).bit_length()                # :146
    cpr = GC if (64 >> lt) >= GC else 64 >> lt  # :147
    ntg = GC // cpr                             # :148
    return dict(nwg=nwg, total=total, V=V, qt=qt, rt=rt, qv=qv, rv=rv, cmax=cmax, CH=CH, tlen=tlen, lt=lt, cpr=cpr, ntg=ntg,
                RG=GC * (CH - 1) + GC)          # :150  registers per group


def chunk_start(geo, g):
    return g * geo["qt"] + min(g, geo["rt"])


def nv_of(geo, g):
    return geo["qv"] + (1 if g < geo["rv"] else 0)


def locate(geo, j):
    """Enumeration index j (< V) -> where a selector holds its extremum.  fused_step.h:425-426 (j = local * G + bp),
    :98 (wave g % 16 takes chunks g, g + 16, ...), :133 (groups of GC chunks), :228 (main blocks), :233-235 (tails)."""
    nwg, CH, lt, cpr, RG = geo["nwg"], geo["CH"], geo["lt"], geo["cpr"], geo["RG"]
    g, local = j % nwg, j // nwg
    wave, i = g % NC, g // NC
    group, e = i // GC, i % GC
    out = dict(g=g, local=local, wave=wave, i=i, group=group, slot=chunk_start(geo, g) + local)
    if local < WAVE * (CH - 1):
        c, lane = local // WAVE, local % WAVE
        out.update(kind="main", c=c, lane=lane, reg=RG * group + e * (CH - 1) + c)
    else:
        tl = local - WAVE * (CH - 1)
        t, ci = e // cpr, e % cpr
        out.update(kind="tail", t=t, ci=ci, tl=tl, lane=(ci << lt) | tl, reg=RG * group + GC * (CH - 1) + t)
    return out


def walk_selector(geo):
    """Every (wave, register, lane) a selector side loads, by running the loops of fused_step.h:217-258 for the sixteen waves:
    {(wave, reg, lane): (slot offset, absorbed as valid)}."""
    nwg, CH, lt, cpr, ntg, RG = (geo[k] for k in ("nwg", "CH", "lt", "cpr", "ntg", "RG"))
    out = {}
    for wv in range(NC):
        want = 0
        for i in range(NC):
            g = wv + NC * i
            if g < nwg and nv_of(geo, g) > 0:
                want |= 1 << i
        for j in range(NG):
            for lane in range(WAVE):
                ci, tl = lane >> lt, lane & ((1 << lt) - 1)
                for e in range(GC):
                    g = wv + NC * (GC * j + e)
                    off = chunk_start(geo, g)
                    for c in range(CH - 1):
                        out[(wv, RG * j + e * (CH - 1) + c, lane)] = (off + lane + c * WAVE, bool((want >> (GC * j + e)) & 1))
                for t in range(GC):
                    if t < ntg:
                        i = GC * j + t * cpr + ci
                        g = wv + NC * i
                        off = chunk_start(geo, g) + WAVE * (CH - 1) + tl
                        ok = ci < cpr and g < nwg and WAVE * (CH - 1) + tl < nv_of(geo, g)
                        out[(wv, RG * j + GC * (CH - 1) + t, lane)] = (off, ok)
    return out


def written_slots(geo):
    """Slot -> enumeration index of what a streaming workgroup publishes there this launch (fused_step.h:504-505, 532-533)."""
    return {chunk_start(geo, g) + local: local * geo["nwg"] + g for g in range(geo["nwg"]) for local in range(nv_of(geo, g))}


def eligible(B, T, H, nwg):
    """Whether the call takes the one-launch form on a grid of nwg + 2 workgroups (observer.hip: osq_observe_tokens_fake_quant,
    launch_fused)."""
    total = B * T
    return (H % 256 == 0 and H // 256 in FUSED_NV and 1 <= B <= MAX_BATCH and T >= 1 and total % 4 == 0 and total <= MAX_SLOTS
            and 1 <= nwg <= MAX_NWG and (total + nwg - 1) // nwg <= MAX_CH * WAVE)


# ================================================================== token enumeration (fused_step.h:446-464)

def enumeration_rows(lengths, T):
    """rows[j] = b * T + t of enumeration index j: the valid tokens sample-major, the padded ones after them."""
    valid, padded = [], []
    for b, ln in enumerate(lengths):
        ln = min(max(int(ln), 0), T)
        valid += [b * T + t for t in range(ln)]
        padded += [b * T + t for t in range(ln, T)]
    return np.array(valid + padded, np.int64), len(valid)


def shape_for(V):
    """(B, T) of a small tensor with B <= 1024, (B * T) % 4 == 0 and B * T >= V: T = 4 ceil(V / 4096), B = ceil(V / T) -- fewer
    than T padded slots."""
    T = 4 * max(1, -(-V // 4096))
    return max(1, -(-V // T)), T


def lengths_for(B, T, V):
    """Lengths that sum to V: every sample full, then single tokens taken off samples 1, 4, 7, ... until V is left."""
    L = [T] * B
    d, i = B * T - V, 0
    assert 0 <= d
    while d > 0:
        b = (1 + 3 * i) % B
        if L[b] > 0:
            L[b] -= 1
            d -= 1
        i += 1
    return L


# ================================================================== planted extrema

def grids(V, seed):
    """(maxima, minima magnitudes) at enumeration positions 0..V-1: seeded permutations of two ascending grids, all distinct,
    exact in fp32: maxima 1 + r 2^-15 in [1, 2), minima -(2 + r 2^-14) in (-4, -2]."""
    rng = np.random.default_rng(seed)
    a = (F32(1.0) + rng.permutation(V).astype(F32) * F32(2.0 ** -15)).astype(F32)
    m = (F32(2.0) + rng.permutation(V).astype(F32) * F32(2.0 ** -14)).astype(F32)
    return a, m


def exact_percentile(N, k):
    """An fp32 p with fp32(p) * fp32(N - 1) == k exactly (the rank both the oracle and the kernel compute in fp32), so that
    floor == ceil == k and the threshold IS the key at rank k."""
    if N <= 1 or k == 0:
        return F32(0.0) if N > 1 else F32(0.5)
    if k == N - 1:
        return F32(1.0)
    p = F32(k / (N - 1))
    for cand in (p, np.nextafter(p, F32(1)), np.nextafter(p, F32(0))):
        if F32(cand * F32(N - 1)) == F32(k):
            return F32(cand)
    raise AssertionError(("no exact percentile", N, k))


def plant(vals, j, k):
    """vals with the value of rank k moved to position j (a swap): position j then holds the key at rank k."""
    out = vals.copy()
    holder = int(np.argsort(vals, kind="stable")[k])
    out[j], out[holder] = vals[holder], vals[j]
    return out


def plant_positions(geo):
    """Enumeration indices to plant at: chunks g = 0, rv - 1, rv, nwg - 1, one of wave 15 and one of the second group (where
    they exist) x the first and last lane of every main block and tail positions 0, tlen - 2, tlen - 1 (where valid)."""
    nwg, rv, CH, tlen = geo["nwg"], geo["rv"], geo["CH"], geo["tlen"]
    chunks = {0, rv - 1, rv, nwg - 1}
    if nwg >= NC:
        chunks.add(NC - 1 + NC * ((nwg - NC) // NC))                     # the last chunk of wave 15
    if nwg > NC * GC:
        chunks.add(NC * GC + (nwg - NC * GC - 1) // 2)                   # a chunk of the second group
    locals_ = set()
    for c in range(CH - 1):
        locals_ |= {WAVE * c, WAVE * c + WAVE - 1}
    locals_ |= {WAVE * (CH - 1) + t for t in (0, tlen - 2, tlen - 1) if t >= 0}
    out = []
    for g in sorted(c for c in chunks if 0 <= c < nwg):
        for local in sorted(locals_):
            if local < nv_of(geo, g):
                out.append(local * nwg + g)
    return out


def plant_launches(geo, limit=None):
    """[(j0, j1, k, p, hinted)], one launch per position: the key of rank k goes to position j0 of the maxima and to j1 of the
    minima (j1 is the position half the list further on); k cycles through ranks near 0.9, 0.5 and 0.97 of V and p is exact
    for it; every other launch runs with a running statistic whose window holds the rank (hinted)."""
    pos = plant_positions(geo)
    V = geo["V"]
    out, n = [], len(pos)
    for i, j0 in enumerate(pos):
        k = int((0.9, 0.5, 0.97)[i % 3] * (V - 1))
        out.append((j0, pos[(i + n // 2 + 1) % n], k, exact_percentile(V, k), i % 2 == 1))
    return out if limit is None else out[:limit]


HINT_MAX, HINT_MIN = F32(1.5), F32(-3.0)      # windows [0.75, 2.25] and [1.5, 4.5]: every key of grids() lies inside


def poisoned_thresholds(tmin, tmax, p, j, side):
    """The oracle's (lo, up) when the extremum at position j of one side is DROPPED from the selection while the count stays
    (a NaN-poisoned register: its key lies above every other, it is in no `v <= thr`)."""
    tmin, tmax = tmin.copy(), tmax.copy()
    if side == 0:
        tmax[j] = np.inf
    else:
        tmin[j] = -np.inf
    with np.errstate(all="ignore"):
        try:
            return OB.prune_thresholds(tmin, tmax, p)
        except ValueError:              # the rank falls on the poisoned key: the threshold is NaN and nothing lies below it
            return F32(np.nan), F32(np.nan)


# ================================================================== the case tables: chunk geometry

TAILS = (1, 2, 3, 5, 9, 17, 33)               # tlen with lt = 0 .. 6
RELEASE_CLASSES = (["ch%d_lt%d" % (ch, lt) for ch in (1, 2) for lt in range(7)] + ["ch3_t1", "ch3_t2"] +
                   ["v1", "below_nwg", "v64n", "v64n+1", "v128n", "v128n+1"])


def release_case(name, nwg):
    """(V, B, T) of a release-grid class on nwg streaming workgroups, or None where the device cannot hold it."""
    cap = min(MAX_SLOTS, MAX_CH * WAVE * nwg)
    pad = True
    if name.startswith("ch"):
        ch, k = int(name[2]), int(name.rsplit("t", 1)[1])
        cmax = WAVE * (ch - 1) + (TAILS[k] if ch < 3 else k)
        # rv = 0, 1, about half, nwg - 1 in turn
        V = [cmax * nwg, (cmax - 1) * nwg + 1, (cmax - 1) * nwg + max(1, nwg // 2), (cmax - 1) * nwg + max(1, nwg - 1)][(k + ch + 3) % 4]
        if -(-V // 4) * 4 > cap:
            V = (cmax - 1) * nwg + 1
    else:
        V = {"v1": 1, "below_nwg": max(1, nwg - 1), "v64n": 64 * nwg, "v64n+1": 64 * nwg + 1, "v128n": 128 * nwg, "v128n+1": 128 * nwg + 1}[name]
        pad = name not in ("v64n", "v128n")
    if pad:
        B, T = shape_for(V)
    else:
        B, T = nwg, V // nwg
    if V < 1 or B * T > cap or B > MAX_BATCH:
        return None
    return V, B, T


KNOB_NWG = (1, 2, 15, 16, 17, 33, 130)


def knob_cmax(nwg):
    """cmax values run on a grid of nwg + 2 workgroups: all 21 (CH, lt) classes at nwg = 1 (at most 192 tokens), a spread of
    them elsewhere (every one of them again across nwg = 2 .. 33), 130 workgroups: both groups of a wave, shared tails."""
    all21 = [WAVE * ch + t for ch in range(3) for t in TAILS]
    if nwg == 1:
        return all21 + [4, 64, 128, 192]
    if nwg == 130:
        return [1, 2, 5, 33, 66, 73, 130, 161, 192]
    k = KNOB_NWG.index(nwg)
    return sorted(set(all21[(k + 5 * i) % 21] for i in range(5)) | {192})


def knob_cases(nwg):
    """[(V, B, T)] for a grid of nwg + 2 workgroups, at most 192 nwg slots each."""
    out = []
    for n, cmax in enumerate(knob_cmax(nwg)):
        rvs = [0, 1, max(1, nwg // 2), nwg - 1]
        rv = rvs[n % 4] if nwg > 1 else 0
        V = cmax * nwg if rv == 0 else (cmax - 1) * nwg + rv
        cap = MAX_CH * WAVE * nwg
        total = min(cap, -(-(V + (3 if n % 2 else 0)) // 4) * 4)       # every other case with a few padded slots more
        if V > total:
            V = total
        B = next(b for b in (7, 5, 4, 3, 2, 1) if total % b == 0)
        out.append((V, B, total // B))
    return out


# ================================================================== the decisions of select_from_registers (token_select.h)

def level_shift(width):
    """observer.hip: level_shift."""
    bits = 0 if width <= 1 else (width - 1).bit_length()
    return bits - SEL_BITS if bits > SEL_BITS else 0


def _bits(f):
    return int(np.array([f], F32).view(np.uint32)[0])


def hint_window(hint, prune=True):
    """token_select.h:98-107."""
    h = F32(hint)
    if prune and h > F32(1e-30) and h < F32(1e30):
        lo = _bits(F32(h * F32(0.5)))
        wd = _bits(F32(h * F32(1.5))) - lo + 1
        return dict(on=True, lo=lo, wd=wd, sh=level_shift(wd))
    return dict(on=False, lo=0, wd=0, sh=0)


def select_path(values, p, hint):
    """Which branches select_from_registers (token_select.h:220-475) takes on one side's values (token_max, or -token_min) with
    prune on and no NaN among them.  Reports decisions only."""
    v = np.ascontiguousarray(values, F32)
    keys = (v.view(np.uint32) & np.uint32(0x7FFFFFFF)).astype(np.int64)
    neg = (v.view(np.uint32) >> 31).astype(bool)
    N = v.size
    rank = F32(F32(p) * F32(N - 1))
    rlo = np.floor(rank)
    k_lo, k_hi, w = int(rlo), int(np.ceil(rank)), F32(rank - rlo)
    win = hint_window(hint)
    n_below = int((keys < win["lo"]).sum()) if win["on"] else 0
    prehist = win["on"] and n_below <= k_lo
    rep = dict(window=win["on"], rejected="below" if win["on"] and not prehist else None, eq_below=win["on"] and n_below == k_lo,
               eq_above=False, k_eq=k_hi == k_lo, w_lt_half=bool(w < F32(0.5)), need_next=None, shortcut=False, reaches_hi=None,
               hi_listed=None, pos=0, next_needed=None)
    kmin, kmax = int(keys.min()), int(keys.max())
    if prehist:
        lo, width, srank, shift, le = win["lo"], win["wd"], k_lo - n_below, win["sh"], n_below
    else:
        lo, width = kmin, kmax - kmin + 1
        srank, shift, le = k_lo, level_shift(width), 0
    count, done, listed, levels, level = N, False, False, 0, 0
    while level < 3 and not done:
        if level > 0 and count <= LIST_CAP:
            listed = True
            break
        d = keys - lo
        m = (d >= 0) & (d < width)
        inside = int(m.sum())
        if level == 0 and prehist and srank >= inside:
            rep["rejected"], rep["eq_above"], prehist = "above", srank == inside, False
            lo, width = kmin, kmax - kmin + 1
            srank, shift, le = k_lo, level_shift(width), 0
            continue
        levels += 1
        hist = np.bincount(d[m] >> shift, minlength=SEL_BINS)
        cum = np.cumsum(hist)
        b = int(np.searchsorted(cum, srank, side="right"))
        below_b, cnt = int(cum[b] - hist[b]), int(hist[b])
        off = b << shift
        lo += off
        count = cnt
        if shift == 0:
            le += below_b + cnt
            width, done = 0, True
        else:
            rest, cap = width - off, 1 << shift
            le += below_b
            srank -= below_b
            width = min(rest, cap)
            shift = level_shift(width)
        level += 1
    rep.update(prehist=bool(prehist), levels=levels, exit="listed" if (not done and listed) else "all_levels")
    if rep["exit"] == "listed":
        inb = (keys - lo >= 0) & (keys - lo < width)
        order = np.argsort(keys[inb], kind="stable")
        L, Lneg = keys[inb][order], neg[inb][order]
        need_next = k_hi != k_lo and srank + 1 >= count
        v_lo = int(L[srank])
        pos = (1 if (~Lneg[L == v_lo]).any() else 0)
        hi_listed = srank + 1 < L.size
        if hi_listed:
            v_hi = int(L[srank + 1])
            pos |= 2 if (~Lneg[L == v_hi]).any() else 0
        else:
            above = keys[keys >= lo + width]
            v_hi = int(above.min()) if need_next and above.size else 0xFFFFFFFF
        lo_f = np.array([v_lo], np.uint32).view(F32)[0]
        hi_f = lo_f if k_hi == k_lo else np.array([v_hi], np.uint32).view(F32)[0]
        with np.errstate(all="ignore"):
            dd = F32(hi_f - lo_f)
            t = OB.fma_f32(w, dd, lo_f) if w < F32(0.5) else OB.fma_f32(F32(w - F32(1)), dd, hi_f)
        reaches = bool(hi_f > lo_f and t >= hi_f)
        rep.update(need_next=bool(need_next), hi_listed=bool(hi_listed), pos=pos, reaches_hi=reaches,
                   shortcut=bool((pos & 1) and (not reaches or hi_listed)))
    else:
        rep["next_needed"] = bool(k_hi != k_lo and le <= k_hi)
    return rep


# ================================================================== the case tables: selection paths

def spread(n, lo=0.6, hi=1.45):
    """n distinct ascending multiples of 2^-13 in [lo, hi]."""
    s = np.unique(np.round(np.linspace(lo, hi, n) * 8192.0)) / 8192.0
    assert s.size == n
    return s.astype(F32)


def _below(x):
    return np.nextafter(F32(x), F32(0))


def path_cases():
    """[dict(name, vals, p, cnt, hint, expect)]: `vals` are one side's values in ascending order of |value| (the test permutes
    them over the tokens), hint the magnitude of that side's running statistic (cnt = 0: the state is +-inf), expect the
    decisions select_path must report.  A window around hint 1.0 is [0.5, 1.5] in bins of 8192 keys (2^-10 in [1, 2))."""
    cases = []

    def add(name, vals, p, hint, cnt=1, **expect):
        cases.append(dict(name=name, vals=np.asarray(vals, F32), p=F32(p), cnt=cnt, hint=F32(hint), expect=expect))

    s200, s500 = spread(200), spread(500, 0.3, 1.45)
    add("off_first_batch", s200, 0.9, np.inf, cnt=0, window=False, exit="listed", levels=1, w_lt_half=True, k_eq=False)
    add("off_zero_hint", spread(64), 0.9, 0.0, window=False)
    add("off_denormal_hint", spread(8), 0.9, 1e-40, window=False)
    add("off_huge_hint", spread(64), 0.9, 1e31, window=False)
    add("hit", s500, 0.9, 1.0, window=True, prehist=True, rejected=None, eq_below=False, levels=1, exit="listed")
    add("below", s200, 0.9, 8.0, window=True, prehist=False, rejected="below", levels=1)
    add("above", s200, 0.9, 0.25, window=True, prehist=False, rejected="above", eq_above=False, levels=1)
    k = int(np.floor(F32(0.9) * F32(199)))
    add("eq_below", s200, 0.9, 2.0 * s200[k], window=True, prehist=True, eq_below=True)
    h = F32(s200[k - 1] / F32(1.5))
    while _bits(F32(h * F32(1.5))) < _bits(s200[k - 1]):
        h = np.nextafter(h, F32(np.inf))
    add("eq_above", s200, 0.9, h, window=True, prehist=False, rejected="above", eq_above=True)
    crowd = (F32(1.25) + np.arange(1500).astype(F32) * F32(2.0 ** -21)).astype(F32)
    crowded = np.concatenate([spread(750, 0.6, 1.2), crowd, spread(750, 1.3, 1.45)])
    add("crowded_listed", crowded, 0.4, 1.0, window=True, prehist=True, levels=2, exit="listed")
    add("crowded_listed_off", crowded, 0.4, np.inf, cnt=0, window=False, levels=2, exit="listed")
    dups = np.concatenate([spread(450, 0.6, 1.2), np.full(1100, 1.25, F32), spread(450, 1.3, 1.45)])
    add("all_levels_inner", dups, 0.5, 1.0, window=True, prehist=True, levels=3, exit="all_levels", next_needed=False)
    add("all_levels_edge", dups, 0.775, 1.0, window=True, prehist=True, levels=3, exit="all_levels", next_needed=True)
    add("all_levels_off", dups, 0.5, np.inf, cnt=0, window=False, levels=3, exit="all_levels")
    add("sparse_need_next", (0.55 * 1.01 ** np.arange(90)).astype(F32), 0.9, 1.0, window=True, exit="listed", need_next=True, shortcut=True,
        reaches_hi=False)
    add("dense_no_next", (F32(1.0) + np.arange(600).astype(F32) * F32(2.0 ** -16)).astype(F32), 0.5, 1.0, window=True, exit="listed",
        need_next=False, hi_listed=True, shortcut=True, w_lt_half=False)
    s300 = spread(300).copy()
    s300[int(np.floor(F32(0.9) * F32(299)))] *= F32(-1)
    add("sign_refuses_shortcut", s300, 0.9, 1.0, exit="listed", pos=0, shortcut=False)
    s101 = spread(101)
    near = s101.copy()
    near[76] = np.nextafter(near[75], F32(2))
    add("reaches_hi_listed", near, 0.7575, 1.0, exit="listed", w_lt_half=False, reaches_hi=True, hi_listed=True, shortcut=True, pos=3)
    edge = s101.copy()
    edge[76] = F32(np.ceil(edge[75] * 1024.0 + 1.0) / 1024.0)            # a bin's first key ...
    edge[75] = _below(edge[76])                                          # ... and the last key of the bin below it
    add("reaches_hi_unlisted", edge, 0.7575, 1.0, exit="listed", reaches_hi=True, hi_listed=False, need_next=True, shortcut=False)
    nearneg = near.copy()
    nearneg[76] *= F32(-1)
    add("reaches_hi_negative", nearneg, 0.7575, 1.0, exit="listed", reaches_hi=True, hi_listed=True, shortcut=True, pos=1)
    add("integral_rank", s101, 0.5, 1.0, k_eq=True, exit="listed")
    add("p_zero", spread(50), 0.0, 1.0, k_eq=True)
    add("p_one", spread(50), 1.0, 1.0, k_eq=True)
    add("all_negative", -spread(100), 0.9, 1.0, window=True, pos=0, shortcut=False)
    return cases


# every branch class of select_from_registers the cases must reach, as (field, value) of select_path's report
PATH_CLASSES = [("window", False), ("window", True), ("prehist", True), ("rejected", "below"), ("rejected", "above"), ("eq_below", True),
                ("eq_above", True), ("levels", 1), ("levels", 2), ("levels", 3), ("exit", "listed"), ("exit", "all_levels"),
                ("need_next", True), ("need_next", False), ("next_needed", True), ("next_needed", False), ("shortcut", True),
                ("shortcut", False), ("pos", 0), ("reaches_hi", True), ("reaches_hi", False), ("hi_listed", False), ("k_eq", True),
                ("k_eq", False), ("w_lt_half", True), ("w_lt_half", False)]


def path_tokens(case, side, seed):
    """(token_min, token_max, hint state (min_val, max_val), cnt) of a selection-path case run on `side`: that side carries the
    case's values in a seeded order, the other one distinct plain values far enough out that min <= max holds per token."""
    rng = np.random.default_rng(seed)
    n = case["vals"].size
    mine = case["vals"][rng.permutation(n)]
    other = (F32(4.0) + rng.permutation(n).astype(F32) * F32(2.0 ** -10)).astype(F32)
    tmax, tmin = (mine, -other) if side == 0 else (other, -mine)
    if case["cnt"] == 0:
        state = (F32(np.inf), F32(-np.inf))
    else:
        state = (F32(-5.0), case["hint"]) if side == 0 else (-case["hint"], F32(5.0))
    return tmin.astype(F32), tmax.astype(F32), state, case["cnt"]


def side_values(tmin, tmax, side):
    return tmax if side == 0 else -tmin


def token_rows(tmin, tmax, H, seed):
    """[V, H] fp32 rows whose minimum is tmin (column 1) and maximum tmax (column 0), every other column between them."""
    rng = np.random.default_rng(seed)
    u = rng.integers(1, 8, size=(tmin.size, H)).astype(F32) / F32(8.0)
    span = (tmax - tmin)[:, None].astype(F32)
    x = np.clip(tmin[:, None] + span * u, tmin[:, None], tmax[:, None]).astype(F32)
    x[:, 0], x[:, 1] = tmax, tmin
    return x


def base_rows(total, H, seed):
    """[total, H] rows of magnitude at most 0.5 (multiples of 2^-7); every row is then given its carriers or a padding value."""
    rng = np.random.default_rng(seed)
    return (rng.integers(-64, 65, size=(total, H)).astype(F32) / F32(128.0)).astype(F32)


def fill_padding(x, rows, V):
    """Padded rows hold what would show if it were observed: NaN, +-inf, +-1e30 in turn."""
    for n, r in enumerate(rows[V:]):
        x[r] = MP.PAD_VALUES[n % len(MP.PAD_VALUES)]


# ================================================================== row mapping

ROW_B = (1, 63, 64, 65, 1024)
ROW_PATTERNS = ("full", "zero", "leading", "trailing", "alternating", "one_last")


def pattern_lengths(pattern, B, T):
    third = max(1, B // 3)
    out = []
    for b in range(B):
        out.append({"full": T, "zero": 0, "leading": 0 if b < third else max(0, T - b % 3),
                    "trailing": 0 if b >= B - third else max(0, T - b % 3), "alternating": 0 if b % 2 else max(0, T - b % 5),
                    "one_last": 1 if b == B - 1 else 0}[pattern])
    return out


def held_tokens(nv, nwg):
    """Tokens the streaming waves keep (fused_step.h:333-335: S = 18 / NV + 9 / NV slots of 16 nwg waves): the rest is streamed."""
    return (MP.FUSED_HOLD_REGS // nv + MP.FUSED_HOLD_LDS // nv) * NC * nwg


def row_mapping_T(B, pattern, nv, nwg):
    """Smallest T (a multiple of 4) at which both valid and padded tokens of the pattern are streamed, where the pattern and
    the 32768-slot limit allow it; None where not even padded ones can be (NV = 3 on a full grid)."""
    need = held_tokens(nv, nwg) + NC * nwg // 2
    first = None
    for T in range(4, MAX_SLOTS // B + 1, 4):
        V, total = sum(pattern_lengths(pattern, B, T)), B * T
        if total <= need:
            continue
        if first is None:
            first = T
        if V > need or pattern in ("zero", "one_last"):
            return T
    return first

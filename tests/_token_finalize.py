"""The three implementations of osq_token_range_finalize (csrc/observer.hip, csrc/token_select.h): models of their DECISIONS,
the placement of a case's values on a [B, T] geometry, and the case tables.  No GPU and no torch device is needed to import
this module; tests/test_oracle_token_finalize.py asserts what the tables reach, tests/test_gpu_token_finalize.py runs them.

  select   token_select_kernel<R4> (token_select.h:609), R4 = 1, 2, 4, 8: two workgroups, one per side, a rendezvous word
  single   token_finalize_kernel<SLOTS> (observer.hip:503-810), SLOTS = 4, 8, 16, 32, 0: one workgroup, both sides at once
  wide     wide_hist_kernel -> wide_collect_kernel -> wide_select_kernel (observer.hip:905-1228)

Expected values never come from here: `cur` is the oracle's prune_thresholds plus the clip rule, the finish step is
OB.ObserverState.  The models only say WHICH branch a problem takes, so that what a table reaches can be asserted.

A threshold lies between the keys at ranks floor(rank) and ceil(rank); the statistic max(v[v <= thr]) only moves with the
upper key when the threshold REACHES it.  The `edge` cases therefore put rank r + 1 one ulp above rank r with w = 0.75: the
fused multiply-add rounds the threshold onto the upper key, and a wrong source of rank r + 1 changes the result's words."""
import numpy as np

import _fused_select as FS
from oracle import observer_oracle as OB

F32 = np.float32
SEL_THREADS = 1024          # token_select.h:27    constexpr int kSelThreads = 1024;
FINAL_THREADS = 1024        # observer.hip         kFinalThreads (slot = tid + i * 1024, :528)
LIST_CAP = FS.LIST_CAP      # observer.hip:454
SEL_BINS = FS.SEL_BINS      # observer.hip:452
WIDE_BLOCK = 512            # observer.hip:853     constexpr int kWideSlotsPerBlock = 512;
COARSE_SHIFT = 20           # observer.hip:854     constexpr int kCoarseShift = 20;
WIDE_DEFAULT = 32769        # observer.hip:838     OSQ_SWITCH(int64_t, g_wide_min_slots, 32769);
WIDE_FLOOR = 1024           # observer.hip:1731    osq_set_wide_min_slots refuses a threshold below 1024 slots
SELECT_MAX = 4 * 8 * SEL_THREADS        # observer.hip:1236   S <= 4 * 8 * kSelThreads
SENTINEL = 0x7FC0BEEF       # a quiet NaN whose payload no arithmetic here produces: what cur holds before every launch
HUGE = F32(3.0e38)          # a padded slot read as valid would become the largest key of its side


# ================================================================== expected result

def quantile_is_nan(tmin, tmax, p):
    with np.errstate(all="ignore"):
        return bool(np.isnan(OB.torch_quantile_linear(np.abs(tmax), p)) or np.isnan(OB.torch_quantile_linear(np.abs(tmin), p)))


def expected_cur(tmin, tmax, p):
    """(cur_min, cur_max) of the oracle for the VALID tokens' extrema: prune_thresholds, then aminmax(clip(value, lo, up)) =
    (up if lo > up else lo, up) (observer.py:68, 227).  A NaN among them makes both quantiles' order undefined: (NaN, NaN)."""
    if quantile_is_nan(tmin, tmax, p):
        return np.array([np.nan, np.nan], F32)
    lo, up = OB.prune_thresholds(tmin, tmax, p)
    return np.array([up if lo > up else lo, up], F32)


def expected_finish(cur, rule, cnt, state, bit, sym):
    """(min_val, max_val, scale, zero_point) after the finish step, by OB.ObserverState (as expected_stats of
    tests/test_gpu_fused_select.py); rule 0 / 1 / 2 = none / running / average (_hip.UPDATE_*)."""
    st = OB.ObserverState(bit=bit, symmetric=sym)
    st.min_val, st.max_val, st.cnt = np.asarray(F32(state[0])), np.asarray(F32(state[1])), cnt
    with np.errstate(all="ignore"):
        if rule == 2:
            st._avg_update(F32(cur[0]), F32(cur[1]))
        elif rule == 1:
            st._running_update(F32(cur[0]), F32(cur[1]))
        else:
            st.min_val, st.max_val = np.asarray(F32(cur[0])), np.asarray(F32(cur[1]))
        scale, zp = st.qparams()
    return F32(st.min_val), F32(st.max_val), F32(scale), F32(zp)


# ================================================================== dispatch (observer.hip:1233-1238, 1454-1481)

def select_fast_ok(B, T, final_fast=1, off_min=0, off_max=0, workspace=True):
    """observer.hip:1233: select_fast_ok for one problem (stride 0); off_* = the arrays' distance from a 16-byte boundary in
    elements."""
    S = B * T
    return bool(workspace and final_fast and T >= 4 and S % 4 == 0 and S <= SELECT_MAX and off_min % 4 == 0 and off_max % 4 == 0)


def dispatch(B, T, final_fast=1, wide_min=WIDE_DEFAULT, off_min=0, off_max=0, prune=True, have_list=True):
    """osq_token_range_finalize, observer.hip:1455-1481: which implementation runs, and which instantiation."""
    S = B * T
    if S >= wide_min and (have_list or not prune):
        return "wide", -(-S // WIDE_BLOCK)
    if select_fast_ok(B, T, final_fast, off_min, off_max):
        gpt = (S // 4 + SEL_THREADS - 1) // SEL_THREADS                 # observer.hip:1258
        return "select", 1 if gpt <= 1 else 2 if gpt <= 2 else 4 if gpt <= 4 else 8
    per = (S + FINAL_THREADS - 1) // FINAL_THREADS                      # observer.hip:1454
    return "single", 4 if per <= 4 else 8 if per <= 8 else 16 if per <= 16 else 32 if per <= 32 else 0


def clamp_lengths(lengths, T):
    """All three kernels clamp a length to [0, T] (observer.hip:546, :581, :897 t < T; token_select.h:510)."""
    return [min(max(int(l), 0), T) for l in lengths]


def valid_mask(B, T, lengths):
    L = np.asarray(clamp_lengths(lengths, T))
    return (np.arange(T)[None, :] < L[:, None]).reshape(-1)


# ================================================================== shared rank arithmetic

def ranks(N, p):
    """observer.hip:635-639 / :1020 / token_select.h: rank = fp32(p) * fp32(N - 1)."""
    rank = F32(F32(p) * F32(N - 1))
    rlo = np.floor(rank)
    return int(rlo), int(np.ceil(rank)), F32(rank - rlo)


def keys_of(values):
    v = np.ascontiguousarray(values, F32)
    return (v.view(np.uint32) & np.uint32(0x7FFFFFFF)).astype(np.int64), (v.view(np.uint32) >> 31).astype(bool)


def key_float(k):
    return np.array([k], np.uint32).view(F32)[0]


def reaches_hi(v_lo, v_hi, w):
    """Whether the interpolated threshold equals the upper key (so that the statistic depends on it)."""
    lo_f, hi_f = key_float(v_lo), key_float(v_hi)
    with np.errstate(all="ignore"):
        d = F32(hi_f - lo_f)
        t = OB.fma_f32(w, d, lo_f) if w < F32(0.5) else OB.fma_f32(F32(w - F32(1)), d, hi_f)
    return bool(hi_f > lo_f and t >= hi_f)


def sign_tie(keys, neg, *wanted):
    """Equal keys of opposite sign at one of the wanted keys."""
    return any(bool(neg[keys == k].any() and (~neg[keys == k]).any()) for k in wanted)


# ================================================================== select: the loader select_side (token_select.h:481-586)

def select_side_model(B, T, lengths):
    """The validity select_side gives every slot, by its own arithmetic (rem_a / rem_b / wrap per 16-byte group,
    token_select.h:498-515, :545-571), and what the geometry makes it do."""
    S = B * T
    groups = S >> 2                                                 # :489
    gpt = (groups + SEL_THREADS - 1) // SEL_THREADS
    R4 = 1 if gpt <= 1 else 2 if gpt <= 2 else 4 if gpt <= 4 else 8
    straddle = T % 4 != 0                                           # :491
    L = clamp_lengths(lengths if lengths is not None else [T] * B, T)
    ok = np.zeros(S, bool)
    valid_to_pad = pad_to_valid = False
    for g in range(groups):
        bb, tt = divmod(4 * g, T)                                   # :501, kept in step by :516-518
        ia = L[min(bb, B - 1)]                                      # :507
        ib = L[min(bb + 1, B - 1)] if straddle else ia              # :508
        to_end = T - tt                                             # :512
        rem_a, rem_b, wrap = ia - tt, ib + to_end, to_end           # :513-515
        for k in range(4):
            if not straddle:
                ok[4 * g + k] = k < rem_a                           # :564
            else:
                ok[4 * g + k] = (k < rem_a) if k < wrap else (k < rem_b)        # :568
        if straddle and wrap < 4:
            before, after = ok[4 * g + wrap - 1], ok[4 * g + wrap]
            valid_to_pad |= bool(before and not after)
            pad_to_valid |= bool(after and not before)
    return dict(R4=R4, straddle=straddle, valid_to_pad=valid_to_pad, pad_to_valid=pad_to_valid,
                tail_clamp=groups % SEL_THREADS != 0,               # :514, :527  g < groups
                whole_wave_valid=bool(not straddle and ok.all()),   # :545
                ok=ok)


def select_report(values, p):
    """FS.select_path without a window (the stand-alone kernel has none), plus the rank arithmetic."""
    rep = FS.select_path(values, p, np.inf)
    k_lo, k_hi, w = ranks(np.asarray(values).size, p)
    rep.update(k_lo=k_lo, k_hi=k_hi, w=w)
    return rep


# ================================================================== single: token_finalize_kernel (observer.hip:503-810)

def single_path(side0, side1, p, slots):
    """Both sides' decisions in token_finalize_kernel: side0 = token_max, side1 = -token_min (only |.| and the sign matter).
    Returns [report of side 0, report of side 1]."""
    per = (slots + FINAL_THREADS - 1) // FINAL_THREADS
    SLOTS = 4 if per <= 4 else 8 if per <= 8 else 16 if per <= 16 else 32 if per <= 32 else 0       # :1477-1481
    K, NEG = zip(*(keys_of(v) for v in (side0, side1)))
    N = K[0].size
    k_lo, k_hi, w = ranks(N, p)
    st = []
    for a in range(2):                                              # :641-649
        lo, width = int(K[a].min()), int(K[a].max()) - int(K[a].min()) + 1
        st.append(dict(lo=lo, width=width, rank=k_lo, shift=FS.level_shift(width), le=0, done=False, count=N, levels=0))
    listed = False
    for level in range(3):                                          # :654
        if st[0]["done"] and st[1]["done"]:                         # :655
            break
        if level > 0 and all(s["done"] or s["count"] <= LIST_CAP for s in st):      # :656
            listed = True
            break
        for a in range(2):
            s = st[a]
            if s["done"]:                                           # :684  active
                continue
            s["levels"] += 1
            d = K[a] - s["lo"]
            m = (d >= 0) & (d < s["width"])                         # :667  d0 < w0 (unsigned)
            hist = np.bincount(d[m] >> s["shift"], minlength=SEL_BINS)
            cum = np.cumsum(hist)
            b = int(np.searchsorted(cum, s["rank"], side="right"))
            below, cnt = int(cum[b] - hist[b]), int(hist[b])
            off = b << s["shift"]
            s["lo"] += off                                          # :691
            s["count"] = cnt
            if s["shift"] == 0:                                     # :693
                s["le"] += below + cnt
                s["width"], s["done"] = 0, True
            else:                                                   # :697-702
                rest, cap = s["width"] - off, 1 << s["shift"]
                s["le"] += below
                s["rank"] -= below
                s["width"] = min(rest, cap)
                s["shift"] = FS.level_shift(s["width"])
    out = []
    for a in range(2):
        s, other = st[a], st[1 - a]
        keys, neg = K[a], NEG[a]
        srt = np.sort(keys)
        v_lo, v_hi = int(srt[k_lo]), int(srt[k_hi])
        if k_hi == k_lo:                                            # :771
            src = "none"
        elif listed and not s["done"]:                              # :749  s_found[a][1], else s_next
            src = "list" if s["rank"] + 1 < s["count"] else "s_next"
        else:                                                       # :749 / :767  le > k_hi ? v : s_next
            src = "dups" if s["le"] > k_hi else "s_next"
        rep = dict(SLOTS=SLOTS, levels=s["levels"], exit="listed" if listed else "all_levels",
                   mixed=("this_done" if s["done"] else "other_done" if other["done"] else None) if listed else None,
                   hi_source=src, k_eq=k_hi == k_lo, w_lt_half=bool(w < F32(0.5)), k_lo=k_lo, k_hi=k_hi, w=w,
                   reaches_hi=reaches_hi(v_lo, v_hi, w), sign_tie=sign_tie(keys, neg, v_lo, v_hi),
                   list_sign_tie=False)
        if listed and not s["done"]:
            inl = (keys - s["lo"] >= 0) & (keys - s["lo"] < s["width"])
            assert int(inl.sum()) == s["count"] and int(np.sort(keys[inl])[s["rank"]]) == v_lo
            rep["list_sign_tie"] = sign_tie(keys[inl], neg[inl], v_lo, v_hi)
        else:
            assert s["lo"] == v_lo and s["le"] == int((keys <= v_lo).sum())
        rep["source_decides"] = rep["reaches_hi"] and src != "none"
        out.append(rep)
    return out


# ================================================================== wide: observer.hip:905-1228

def wide_path(values, p):
    """One side's decisions in wide_collect_kernel / list_select2 / wide_select_kernel."""
    keys, neg = keys_of(values)
    N = keys.size
    k_lo, k_hi, w = ranks(N, p)
    srt = np.sort(keys)
    coarse = srt >> COARSE_SHIFT
    c = int(coarse[k_lo])                                           # pick_coarse_bin, :970
    below, count = int((coarse < c).sum()), int((coarse == c).sum())
    r = k_lo - below                                                # :1172  rank inside the list
    lst = srt[below:below + count]
    top = int((lst[r] >> 9) & 0x7FF)                                # :1108  first-level bin
    top_below = int((((lst >> 9) & 0x7FF) < top).sum())
    top_count = int((((lst >> 9) & 0x7FF) == top).sum())
    want = r - top_below                                            # :1131
    if k_hi == k_lo:                                                # :1180
        src = "none"
    elif r + 1 < count:                                             # :1135
        src = "same_bin" if want + 1 < top_count else "s_above"     # :1136-1140
    else:
        src = "next_inv"                                            # :1180
    v_lo, v_hi = int(srt[k_lo]), int(srt[k_hi])
    rep = dict(coarse_bin=c, coarse_count=count, first_of_coarse=k_lo == below, last_of_coarse=k_lo == below + count - 1,
               first_level_bin=top, hi_source=src, all_in_list=count == N, k_eq=k_hi == k_lo, w_lt_half=bool(w < F32(0.5)),
               coarse_slot=((c & 15) << 7) | (c >> 4),              # :903
               k_lo=k_lo, k_hi=k_hi, w=w, reaches_hi=reaches_hi(v_lo, v_hi, w), sign_tie=sign_tie(keys, neg, v_lo, v_hi))
    rep["source_decides"] = rep["reaches_hi"] and src != "none"
    return rep


def wide_geometry(B, T, lengths):
    """Workgroups, and where their 512-slot boundaries fall (inside a sample's valid run / inside its padding)."""
    S = B * T
    ok = valid_mask(B, T, lengths if lengths is not None else [T] * B)
    in_valid = in_pad = False
    for m in range(WIDE_BLOCK, S, WIDE_BLOCK):
        if m % T:                                                   # slots m - 1 and m belong to one sample
            in_valid |= bool(ok[m - 1] and ok[m])
            in_pad |= bool(not ok[m - 1] and not ok[m])
    return dict(workgroups=-(-S // WIDE_BLOCK), boundary_in_valid=in_valid, boundary_in_padding=in_pad,
                last_block_partial=S % WIDE_BLOCK != 0)


# ================================================================== value cases

def from_keys(k):
    return np.asarray(k, np.uint32).view(F32).copy()


def edge_values(N, E, step_lo=37, step_hi=41):
    """N distinct ascending values: N // 2 keys E, E - step_lo, ... below and the others E + 1, E + 1 + step_hi, ... above: ranks
    N // 2 - 1 and N // 2 are the adjacent keys E and E + 1."""
    n_lo = N // 2
    lo = E - step_lo * np.arange(n_lo - 1, -1, -1, dtype=np.int64)
    hi = E + 1 + step_hi * np.arange(N - n_lo, dtype=np.int64)
    return from_keys(np.concatenate([lo, hi]))


def frac_percentile(N, k, frac=0.75):
    """An fp32 p whose rank fp32(p) * fp32(N - 1) has floor k and fraction near `frac`."""
    if N < 2:
        return F32(0.5)
    p = F32((k + frac) / (N - 1))
    k_lo, _, w = ranks(N, p)
    assert k_lo == k and abs(float(w) - frac) < 0.2, (N, k, float(w))
    return p


E_COARSE = 0x3F9FFFFF        # the last key of coarse bin 0x3F9 (1.2499999); E + 1 = 1.25 opens coarse bin 0x3FA
E_LEVEL1 = 0x3FA401FF        # the last key of a first-level bin (bits 8:0 all ones) inside coarse bin 0x3FA
E_INSIDE = 0x3FA40100        # E and E + 1 share their first-level bin
DUP_KEY = 0x3FA40100


def dup_values(N, n_dup, at):
    """n_lo distinct keys ending one below DUP_KEY, n_dup copies of DUP_KEY, then DUP_KEY + 1 and distinct keys above."""
    n_lo = (N - n_dup) // 2
    lo = DUP_KEY - 1 - 37 * np.arange(n_lo - 1, -1, -1, dtype=np.int64)
    hi = DUP_KEY + 1 + 41 * np.arange(N - n_dup - n_lo, dtype=np.int64)
    vals = from_keys(np.concatenate([lo, np.full(n_dup, DUP_KEY, np.int64), hi]))
    k = {"inside": n_lo + n_dup // 2, "last": n_lo + n_dup - 1, "below": n_lo - 1}[at]
    return vals, k


FUSED_CASES_KEPT = ("off_first_batch", "crowded_listed_off", "all_levels_inner", "all_levels_edge", "sparse_need_next", "dense_no_next",
                    "sign_refuses_shortcut", "reaches_hi_listed", "reaches_hi_unlisted", "reaches_hi_negative", "integral_rank",
                    "p_zero", "p_one", "all_negative")          # the others of FS.path_cases() differ only in their window


def default_other(n):
    """The other side's magnitudes: distinct plain values far enough out that min <= max holds per token."""
    return (F32(4.0) + np.arange(n).astype(F32) * F32(2.0 ** -10)).astype(F32)


def value_cases():
    """[dict(name, vals, other, p, finite, aims)]: `vals` are the magnitudes-with-sign of the side the case is run on (token_max
    on side 0, -token_min on side 1), `other` those of the opposite side; `aims` names the classes the case is meant to reach."""
    cases = []

    def add(name, vals, p, other=None, aims=()):
        vals = np.asarray(vals, F32)
        other = default_other(vals.size) if other is None else np.asarray(other, F32)
        assert other.size == vals.size
        cases.append(dict(name=name, vals=vals, other=other, p=F32(p), finite=True, aims=tuple(aims)))

    for c in FS.path_cases():
        if c["name"] in FUSED_CASES_KEPT:
            add(c["name"], c["vals"], c["p"], aims=("select_from_registers: " + c["name"],))
    N = 3000
    add("edge_next_coarse_bin", edge_values(N, E_COARSE), frac_percentile(N, N // 2 - 1),
        aims=("wide: last key of a coarse bin, rank r + 1 from next_inv", "single: rank r + 1 from s_next"))
    add("edge_first_of_coarse_bin", edge_values(N, E_COARSE), frac_percentile(N, N // 2, 0.25), aims=("wide: first key of a coarse bin",))
    add("edge_next_first_level_bin", edge_values(N, E_LEVEL1), frac_percentile(N, N // 2 - 1), aims=("wide: rank r + 1 from s_above",))
    add("edge_same_first_level_bin", edge_values(N, E_INSIDE), frac_percentile(N, N // 2 - 1),
        aims=("wide: rank r + 1 in the same first-level bin", "single: rank r + 1 from the list"))
    for at in ("inside", "last", "below"):
        vals, k = dup_values(N, 1100, at)
        add("dups_rank_" + at, vals, frac_percentile(N, k), aims=("more than 1024 duplicates: rank %s the run" % at,))
    vals, k = dup_values(N, 1100, "last")
    add("dups_rank_last_beside_constant", vals, frac_percentile(N, k), other=np.full(N, 4.0, F32),
        aims=("single: all levels on both sides, rank r + 1 from s_next",))
    far = vals.copy()
    far[0], far[-1] = F32(1e-3), F32(100.0)                       # a wide key range: three histogram levels
    add("dups_rank_last_wide_range", far, frac_percentile(N, k), other=np.full(N, 4.0, F32),
        aims=("single: three levels, rank r + 1 from s_next",))
    lone = edge_values(N, E_INSIDE, 64, 20)
    lone[0] = key_float(E_INSIDE - 64 * (N // 2) + 1)           # E is then the LAST key of its level-0 bin of 64 keys, alone in it
    add("edge_next_level0_bin", lone, frac_percentile(N, N // 2 - 1), aims=("single: listed, rank r + 1 from s_next",))
    crowd = (F32(1.25) + np.arange(1500).astype(F32) * F32(2.0 ** -21)).astype(F32)
    crowded = np.concatenate([FS.spread(750, 0.6, 1.2), crowd, FS.spread(750, 1.3, 1.45)])
    add("crowded_beside_constant", crowded, 0.4, other=np.full(N, 4.0, F32), aims=("single: listed with the other side done (duplicates)",))
    two = from_keys(np.where(np.arange(N) < N // 2, 0x40800000, 0x40800001))
    add("crowded_beside_two_keys", crowded, frac_percentile(N, N // 2 - 1), other=two,
        aims=("single: listed with the other side done, its rank r + 1 from s_next",))
    dup3, k = dup_values(N, 1100, "inside")
    add("duplicates_beside_sparse", dup3, frac_percentile(N, k), other=np.resize(FS.spread(40, 3.0, 5.0), N),
        aims=("two sides that differ: three levels beside a sparse side",))
    add("clip_rule_lo_above_up", FS.spread(200), 0.9, other=-default_other(200), aims=("lo > up: (up, up)",))
    z = FS.spread(100).copy()
    z[:40] = np.where(np.arange(40) % 3 == 0, F32(0.0), F32(-0.0))
    add("zeros_of_both_signs", z, frac_percentile(100, 20, 0.25), aims=("+-0.0 at the wanted rank",))
    zn = FS.spread(100).copy()
    zn[:40] = F32(-0.0)
    add("zeros_negative_only", zn, frac_percentile(100, 20, 0.25), aims=("-0.0 at the wanted rank",))
    t = FS.spread(300).copy()
    t[201] = -t[200]
    add("sign_tie_at_rank", t, frac_percentile(300, 200, 0.25), aims=("equal keys of opposite sign in the list",))
    add("sign_tie_at_rank_upper", t, frac_percentile(300, 199, 0.75), aims=("equal keys of opposite sign at rank r + 1",))
    add("all_equal", np.full(700, 1.25, F32), 0.9, aims=("all values equal",))
    add("all_equal_both_sides", np.full(700, 1.25, F32), 0.9, other=np.full(700, 4.0, F32), aims=("all values equal on both sides",))
    add("one_token", [1.25], 0.9, aims=("one valid token",))
    add("two_tokens", [1.0, 1.5], 0.9, aims=("N = 2",))
    add("two_tokens_adjacent", from_keys([0x3F800000, 0x3F800001]), 0.75, aims=("N = 2, the threshold reaches the upper key",))
    return cases


def scalable_values(kind, V, seed=0):
    """(vals, p) of `kind` for any V >= 1: what the size classes are filled with."""
    if V < 4 or kind == "spread":
        rng = np.random.default_rng(seed + V)
        vals = np.sort((F32(0.5) + rng.permutation(max(V, 1)).astype(F32)[:V] * F32(2.0 ** -12)).astype(F32))
        return vals, (frac_percentile(V, int(0.9 * (V - 1)), 0.5) if V > 2 else F32(0.9))
    if kind == "dups" and V >= 8:
        n_dup = min(1100, V // 2)
        vals, k = dup_values(V, n_dup, "last")
        return vals, frac_percentile(V, k)
    E = {"edge_coarse": E_COARSE, "edge_level1": E_LEVEL1, "edge_inside": E_INSIDE, "dups": E_INSIDE}[kind]
    return edge_values(V, E), frac_percentile(V, V // 2 - 1)


SCALABLE_KINDS = ("edge_coarse", "edge_level1", "edge_inside", "dups", "spread")


# ================================================================== placement

def place(vals, other, side, B, T, lengths, seed, pad):
    """(token_min, token_max) of B * T slots: the case's values, in a seeded permutation, on the valid tokens (side 0: token_max
    = vals, token_min = -other; side 1: token_min = -vals, token_max = other); padded slots hold NaN (pad = "nan") or a huge
    finite value of the sign that would win (pad = "huge")."""
    ok = valid_mask(B, T, lengths if lengths is not None else [T] * B)
    V = int(ok.sum())
    assert V == np.asarray(vals).size == np.asarray(other).size, (V, np.asarray(vals).size)
    rng = np.random.default_rng(seed)
    mine, oth = np.asarray(vals, F32)[rng.permutation(V)], np.asarray(other, F32)[rng.permutation(V)]
    tmax = np.full(B * T, np.nan if pad == "nan" else HUGE, F32)
    tmin = np.full(B * T, np.nan if pad == "nan" else -HUGE, F32)
    if side == 0:
        tmax[ok], tmin[ok] = mine, -oth
    else:
        tmax[ok], tmin[ok] = oth, -mine
    return tmin, tmax, ok


def lengths_summing_to(B, T, V):
    return FS.lengths_for(B, T, V)


def value_geometry(impl, N, n):
    """(B, T, lengths, knobs) on which value case number n of N tokens runs under `impl`: a few padded slots wherever N allows.
    select: T = 8 or (odd n) a straddling T = 6; single: reached through final_fast = 0 on a select-shaped layout (even n) or
    through an odd slot count (odd n); wide: wide_min_slots = 1024 and at least 1024 slots."""
    if impl == "select":
        T = 6 if n % 2 else 8
        B = max(2, -(-(N + 3) // T))
        B += B % 2                                                   # B * T % 4 == 0
        return B, T, lengths_summing_to(B, T, N), dict(final_fast=1, wide_min=WIDE_DEFAULT)
    if impl == "single":
        if n % 2:
            T = 7
            B = max(1, -(-(N + 2) // T))
            B += 1 - B % 2                                           # odd B * T
            return B, T, lengths_summing_to(B, T, N), dict(final_fast=1, wide_min=WIDE_DEFAULT)
        T = 8
        B = max(1, -(-(N + 3) // T))
        return B, T, lengths_summing_to(B, T, N), dict(final_fast=0, wide_min=WIDE_DEFAULT)
    T = 96 if n % 2 else 100
    B = max(-(-WIDE_FLOOR // T), -(-(N + 5) // T))
    return B, T, spread_lengths(B, T, N), dict(final_fast=1, wide_min=WIDE_FLOOR)


def spread_lengths(B, T, V):
    """Lengths summing to V with the padding spread over the samples (so that block boundaries meet valid runs and padding)."""
    assert 0 <= V <= B * T
    base, extra = divmod(V, B)
    return [base + (1 if b < extra else 0) for b in range(B)]


# ================================================================== size classes

LENGTH_PATTERNS = ("full", "one_token", "alternating", "t_minus_1", "ones", "beyond_T")


def pattern_lengths(pattern, B, T):
    """full; all zero except one token; zero and full alternating (sample 0 full); T - 1; 1; and lengths beyond T (2 T + 3 on
    every third sample, clamped to T by all three kernels; the others T - 2)."""
    return {"full": [T] * B,
            "one_token": [1 if b == B // 2 else 0 for b in range(B)],
            "alternating": [T if b % 2 == 0 else 0 for b in range(B)],
            "t_minus_1": [T - 1] * B,
            "ones": [1] * B,
            "beyond_T": [2 * T + 3 if b % 3 == 0 else max(T - 2, 0) for b in range(B)]}[pattern]


# (B, T): slots 4, 4096, 4100, 8192, 8196, 16384, 16388, 32768 (both sides of every R4 threshold), and T = 5, 6, 7, 101 straddling
SELECT_SIZES = ((1, 4), (128, 32), (1025, 4), (256, 32), (2049, 4), (128, 128), (4097, 4), (256, 128),
                (8, 5), (820, 5), (1366, 6), (2340, 7), (324, 101))
# (B, T, how single is reached): slots 1, 3, 4095, 4096, 4097, 8193, 16385, 32768, 32769
SINGLE_SIZES = ((1, 1, "t_below_4"), (1, 3, "t_below_4"), (1365, 3, "t_below_4"), (819, 5, "odd_slots"), (128, 32, "final_fast_0"),
                (128, 32, "tmin_off_16"), (128, 32, "tmax_off_16"), (17, 241, "odd_slots"), (8193, 1, "t_below_4"), (3277, 5, "odd_slots"),
                (256, 128, "final_fast_0"), (3641, 9, "wide_min_raised"))
# (B, T): 1024, 1025 and 12288 slots; 513 slots cannot be reached: osq_set_wide_min_slots refuses a threshold below 1024
WIDE_SIZES = ((8, 128), (16, 64), (25, 41), (5, 205), (96, 128), (64, 192))


def single_knobs(how):
    """(final_fast, wide_min, off_min, off_max) that reach single `how`."""
    return dict(final_fast=0 if how == "final_fast_0" else 1, wide_min=(1 << 40) if how == "wide_min_raised" else WIDE_DEFAULT,
                off_min=1 if how == "tmin_off_16" else 0, off_max=1 if how == "tmax_off_16" else 0)


def size_problems(impl, B, T):
    """[(pattern, lengths, kind, pad)] run at one size class: every length pattern, the scalable kinds and the padding values
    in turn."""
    out = []
    for i, pattern in enumerate(LENGTH_PATTERNS):
        L = pattern_lengths(pattern, B, T)
        if sum(clamp_lengths(L, T)) == 0:
            continue
        out.append((pattern, L, SCALABLE_KINDS[(i + B + T) % len(SCALABLE_KINDS)], ("nan", "huge")[(i + B) % 2]))
    return out


# ================================================================== coverage constants

WINDOW_FIELDS = ("window", "prehist", "rejected", "eq_below", "eq_above")      # the stand-alone kernel has no hinted window
SELECT_CLASSES = ([("path", "window", False)] + [("path", f, v) for f, v in FS.PATH_CLASSES if f not in WINDOW_FIELDS] +
                  [("path", "source_decides", True)] + [("loader", "R4", r) for r in (1, 2, 4, 8)] +
                  [("loader", f, v) for f in ("straddle", "valid_to_pad", "pad_to_valid", "tail_clamp", "whole_wave_valid") for v in (True, False)])
SINGLE_CLASSES = ([("SLOTS", s) for s in (4, 8, 16, 32, 0)] + [("levels", n) for n in (1, 2, 3)] + [("exit", "listed"), ("exit", "all_levels")] +
                  [("mixed", "this_done"), ("mixed", "other_done"), ("mixed", None)] +
                  [("hi_source", s) for s in ("list", "s_next", "dups", "none")] +
                  [("k_eq", True), ("k_eq", False), ("w_lt_half", True), ("w_lt_half", False), ("sign_tie", True), ("list_sign_tie", True)] +
                  [("decides", "list"), ("decides", "s_next"), ("decides", "listed_done_s_next"), ("decides", "all_levels_s_next")])
WIDE_CLASSES = ([("hi_source", s) for s in ("same_bin", "s_above", "next_inv", "none")] +
                [("decides", s) for s in ("same_bin", "s_above", "next_inv")] +
                [("first_of_coarse", True), ("last_of_coarse", True), ("first_of_coarse", False), ("last_of_coarse", False),
                 ("all_in_list", True), ("all_in_list", False), ("coarse_count_above_1024", True), ("sign_tie", True),
                 ("k_eq", True), ("w_lt_half", True), ("w_lt_half", False)] +
                [("geometry", f, True) for f in ("boundary_in_valid", "boundary_in_padding", "last_block_partial", "workgroups_2", "workgroups_24")])


def single_classes_of(reps):
    """The SINGLE_CLASSES entries the two sides' reports of one problem reach."""
    out = set()
    for r in reps:
        out |= {(f, r[f]) for f in ("SLOTS", "levels", "exit", "mixed", "hi_source", "k_eq", "w_lt_half")}
        out |= {(f, True) for f in ("sign_tie", "list_sign_tie") if r[f]}
        if r["source_decides"]:
            if r["exit"] == "listed" and r["mixed"] != "this_done":
                out.add(("decides", r["hi_source"]))
            elif r["exit"] == "listed":
                out.add(("decides", "listed_done_" + r["hi_source"]))
            else:
                out.add(("decides", "all_levels_" + r["hi_source"]))
    return out


def wide_classes_of(rep, geo=None):
    out = {(f, rep[f]) for f in ("hi_source", "first_of_coarse", "last_of_coarse", "all_in_list", "k_eq", "w_lt_half")}
    if rep["source_decides"]:
        out.add(("decides", rep["hi_source"]))
    if rep["coarse_count"] > LIST_CAP:
        out.add(("coarse_count_above_1024", True))
    if rep["sign_tie"]:
        out.add(("sign_tie", True))
    if geo is not None:
        out |= {("geometry", f, True) for f in ("boundary_in_valid", "boundary_in_padding", "last_block_partial") if geo[f]}
        if geo["workgroups"] == 2:
            out.add(("geometry", "workgroups_2", True))
        if geo["workgroups"] >= 24:
            out.add(("geometry", "workgroups_24", True))
    return out


def select_classes_of(rep, loader=None):
    out = {("path", f, rep[f]) for f, _ in FS.PATH_CLASSES if f in rep}
    if rep.get("exit") == "listed" and rep.get("reaches_hi") and not rep["k_eq"]:
        out.add(("path", "source_decides", True))
    if loader is not None:
        out |= {("loader", f, loader[f]) for f in ("R4", "straddle", "valid_to_pad", "pad_to_valid", "tail_clamp", "whole_wave_valid")}
    return out

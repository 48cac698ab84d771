"""Seeded table recipes and CPU references for the table-driven multi-tensor kernels: osq_fake_quant_weights_multi,
osq_token_minmax_multi and osq_token_range_finalize_batched (tests/test_oracle_multi_tables.py checks what the recipes
promise, tests/test_gpu_multi_tables.py runs them).  Everything here is NumPy: a recipe is a handful of flat arrays plus
one small record per entry, so that the many tiny tensors of a table are carved out of ONE device allocation.

The constants below restate the kernels' launch shapes (csrc/fake_quant.hip, csrc/observer.hip, csrc/osq_host.h); the
recipes are built around them: a table either side of the LDS limit, a total one grid-stride trip cannot hold, rows one
float4 either side of an unrolled trip.
"""
import functools

import numpy as np

from oracle import fake_quant_oracle as FQ
from oracle import observer_oracle as OB

F32 = np.float32

K_MAX_BLOCKS = 2048                         # osq_host.h kMaxBlocks
WAVES_PER_BLOCK = 4                         # 256 threads / 64 lanes
LDS_WEIGHTS, LDS_SITES = 1024, 512          # kMultiLdsWeights, kMultiLdsSites: longer tables are bisected in global memory
WEIGHT_GRID_WAVES = K_MAX_BLOCKS * 4 * WAVES_PER_BLOCK      # 32768 rows per grid-stride trip
TOKEN_GRID_WAVES = K_MAX_BLOCKS * 8 * WAVES_PER_BLOCK       # 65536 token slots per grid-stride trip
WEIGHT_TRIP = 4 * 64 * 4                    # kUnroll * wave float4 = 1024 floats of a row per unrolled trip
TOKEN_TRIP = 3 * 64 * 4                     # 768 features per unrolled trip

ZP_INT32, ZP_FLOAT32 = 0, 1
FIXED, LSQ, LSQPLUS = 0, 1, 2

GUARD = 4                                   # floats between two entries' outputs (keeps every output row 16-byte aligned)
SENTINEL_BITS = 0x4B1D4B1D                  # an ordinary finite float (1.0296e7): what guard words and untouched slots hold
SENTINEL = np.array([SENTINEL_BITS], np.uint32).view(F32)[0]

WEIGHT_INNERS = (4, 252, 256, 260, 1020, 1024, 1028, 2052)
WEIGHT_LENGTHS = (1, 2, 77, 1024, 1025, 1300)
WEIGHT_TABLES = tuple(f"n{n}" for n in WEIGHT_LENGTHS) + ("second_trip", "zero_rows", "all_zero_rows")


def bits(a):
    """uint32 words of an fp32 array, every NaN mapped to one pattern (payloads are not part of the contract)."""
    a = np.ascontiguousarray(np.asarray(a, dtype=F32))
    w = a.view(np.uint32).copy()
    w[np.isnan(a)] = np.uint32(0x7FC00000)
    return w


# ------------------------------------------------------------------------------------------- weights

def _quant_range(bit, symmetric):
    return (-(1 << (bit - 1)), (1 << (bit - 1)) - 1) if symmetric else (0, (1 << bit) - 1)


def _weight_entry(i, rng, big=False, rows=None, inner=None, layout=None):
    """Geometry and quantizer of entry i.  The 40 (inner, rows) pairs cycle with i; `big` forces the shapes whose rows
    take more than one unrolled trip and whose channel index wraps; rows / inner / layout override the cycle."""
    kind = ("one", "two", "three", "sixtyfour", "wrap")[(i // 8) % 5]
    mode = (FIXED, LSQ, LSQPLUS)[i % 3]
    if big:
        inner, kind, mode = (2052, 1028)[i % 2], ("wrap", "sixtyfour")[(i // 2) % 2], (LSQPLUS, FIXED, LSQ)[i % 3]
    if inner is None:
        inner = WEIGHT_INNERS[i % 8]
    if rows is None:
        rows = {"one": 1, "two": 2, "three": 3, "sixtyfour": 64, "wrap": 3 * (2, 5, 7)[i % 3]}[kind]
        layout = "wrap" if kind == "wrap" else layout
    if layout is None:
        layout = ("per_row", "per_tensor")[(i // 3) % 2]             # channels == rows / channels == 1
    if rows == 0:
        layout = "per_tensor"
    channels = {"per_row": rows, "per_tensor": 1, "wrap": rows // 3}[layout]    # wrap: row % channels wraps twice
    bit, symmetric = (2, 4, 6, 8)[(i // 3) % 4], bool((i // 5) % 2)
    zp_type = ZP_FLOAT32 if mode == LSQPLUS else (ZP_INT32, ZP_FLOAT32)[(i // 7) % 2]
    qmin, qmax = _quant_range(bit, symmetric)
    # powers of two (x / scale exact: the planted ties ARE ties) next to arbitrary scales
    scale = np.where(rng.random(channels) < 0.5, 2.0 ** rng.integers(-6, 0, channels), rng.uniform(0.01, 0.2, channels)).astype(F32)
    zp = rng.integers(qmin, qmax + 1, channels).astype(np.float64)
    if symmetric:
        zp[:] = 0
    if mode == LSQPLUS:
        zp = zp + rng.uniform(-0.45, 0.45, channels)                # a non-integer float zero point: LSQ+ rounds it itself
    grad_factor = 1.0 if mode == FIXED else float(1.0 / np.sqrt(max(rows, 1) * inner * max(qmax, 1)))
    return dict(rows=rows, channels=channels, inner=inner, layout=layout, mode=mode, bit=bit, symmetric=symmetric,
                zp_type=zp_type, quant_min=qmin, quant_max=qmax, scale=scale, zp=zp, grad_factor=grad_factor)


SPECIAL_KINDS = ("nan", "+inf", "-inf", "+0", "-0", "tie", "far")


def _special(kind, scale, k):
    if kind == "tie":
        return F32((k % 5 - 2 + 0.5) * float(scale))                # exactly .5 * scale away from a grid point
    return {"nan": F32(np.nan), "+inf": F32(np.inf), "-inf": F32(-np.inf), "+0": F32(0.0), "-0": F32(-0.0),
            "far": F32(3.0e38 if k % 2 else -1.0e30)}[kind]


def classify_special(v, scale):
    """The kind of special a planted value is, or None."""
    v = F32(v)
    if np.isnan(v):
        return "nan"
    if np.isinf(v):
        return "+inf" if v > 0 else "-inf"
    if v == 0:
        return "-0" if np.signbit(v) else "+0"
    if abs(v) > 1e29:
        return "far"
    q = float(v) / float(scale)
    return "tie" if abs(q - np.floor(q) - 0.5) < 1e-6 else None


def _plant(x, e, i):
    """Specials at the first and last float of the first and last row of the entry, the kinds cycling with i."""
    rows, inner = x.shape
    for c, (r, j) in enumerate(((0, 0), (0, inner - 1), (rows - 1, 0), (rows - 1, inner - 1))):
        kind = SPECIAL_KINDS[(i + 2 * c) % len(SPECIAL_KINDS)]
        x[r, j] = _special(kind, e["scale"][r % e["channels"]], i + c)


def _finish_weight_table(name, entries, seed):
    rng = np.random.default_rng(seed)
    x_off = y_off = p_off = 0
    xs, scales, zps_i, zps_f = [], [], [], []
    for i, e in enumerate(entries):
        rows, inner, ch = e["rows"], e["inner"], e["channels"]
        x = (rng.standard_normal((rows, inner)) * (e["scale"][np.arange(rows) % ch][:, None] * (1 << (e["bit"] - 1)))).astype(F32)
        if rows:
            _plant(x, e, i)
        e.update(index=i, x_off=x_off, y_off=y_off + GUARD, p_off=p_off)
        xs.append(x.reshape(-1))
        scales.append(e["scale"])
        zps_i.append(np.rint(e["zp"]).astype(np.int32))
        zps_f.append(e["zp"].astype(F32))
        x_off += rows * inner
        y_off += GUARD + rows * inner
        p_off += ch
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)   # noqa: E731
    row_end = np.cumsum([e["rows"] for e in entries]).astype(np.int64)
    return dict(name=name, entries=entries, x=cat(xs, F32), scale=cat(scales, F32), zp_i32=cat(zps_i, np.int32),
                zp_f32=cat(zps_f, F32), row_end=row_end, total_rows=int(row_end[-1]) if len(entries) else 0,
                y_len=y_off + GUARD)


@functools.lru_cache(maxsize=None)
def weight_table(name):
    """One table of osq_fake_quant_weights_multi: flat input x, flat parameters, per-entry records with offsets into them
    and into the guarded output (GUARD sentinel floats before every entry and after the last)."""
    seed = 1000 + WEIGHT_TABLES.index(name)
    rng = np.random.default_rng(seed)
    if name == "second_trip":
        # 32768 + 5 rows of inner = 4: the last five rows (per-row parameters) belong to the grid's second trip
        shapes = ((2, "per_row"), (2, "per_tensor"), (3, "per_row"), (8190, "wrap"), (8192, "per_tensor"), (8192, "per_row"),
                  (8192, "per_row"))
        return _finish_weight_table(name, [_weight_entry(i, rng, rows=r, inner=4, layout=l) for i, (r, l) in enumerate(shapes)], seed)
    if name in ("zero_rows", "all_zero_rows"):
        # empty entries at the front, in the middle (two in a row) and at the end; or nothing but empty entries
        pattern = (0, 0, 3, 0, 0, 64, 2, 0, 1, 0) if name == "zero_rows" else (0, 0, 0)
        return _finish_weight_table(name, [_weight_entry(i, rng, rows=r, layout=("per_row", "per_tensor")[i % 2])
                                           for i, r in enumerate(pattern)], seed)
    n = int(name[1:])
    corners = {0, n - 1, LDS_WEIGHTS - 1, LDS_WEIGHTS}             # the last entry of the LDS copy and the first beyond it
    entries = []
    for i in range(n):
        if n > 100 and i >= 40 and i not in corners:
            entries.append(_weight_entry(i, rng, rows=(1, 2, 3)[i % 3]))      # long tables: tiny beyond the first full cycle
        else:
            entries.append(_weight_entry(i, rng, big=i in corners and n > 2))
    return _finish_weight_table(name, entries, seed)


def weight_entry_x(table, e):
    return table["x"][e["x_off"]:e["x_off"] + e["rows"] * e["inner"]].reshape(e["rows"], e["inner"])


def weight_entry_zp(table, e):
    src = table["zp_i32"] if e["zp_type"] == ZP_INT32 else table["zp_f32"]
    return src[e["p_off"]:e["p_off"] + e["channels"]]


@functools.lru_cache(maxsize=None)
def weight_reference(name):
    """The guarded output the launch must leave, as uint32 words: every entry through oracle/fake_quant_oracle.py
    (lsq_effective for the mode, then quantize_affine / dequantize_affine per channel = row % channels), sentinels in
    between.  Computed once per table."""
    t = weight_table(name)
    out = np.full(t["y_len"], SENTINEL, F32)
    for e in t["entries"]:
        if e["rows"] == 0:
            continue
        ch = e["channels"]
        x = weight_entry_x(t, e).reshape(e["rows"] // ch, ch, e["inner"])
        s, z = FQ.lsq_effective(t["scale"][e["p_off"]:e["p_off"] + ch], weight_entry_zp(t, e).astype(F32), F32(e["grad_factor"]),
                                e["mode"])
        s, z = np.asarray(s, F32).reshape(1, ch, 1), np.asarray(z, F32).reshape(1, ch, 1)
        xq = FQ.quantize_affine(x, s, z, e["quant_min"], e["quant_max"])
        out[e["y_off"]:e["y_off"] + x.size] = FQ.dequantize_affine(xq, s, z).reshape(-1)
    return bits(out)


def weight_guard_mask(table):
    m = np.ones(table["y_len"], bool)
    for e in table["entries"]:
        m[e["y_off"]:e["y_off"] + e["rows"] * e["inner"]] = False
    return m


# ------------------------------------------------------------------------------------------- token sites

SITE_COUNTS = (1, 2, 96, 512, 513, 700)
SITE_TABLES = tuple(f"n{n}" for n in SITE_COUNTS) + ("second_trip",)
BTH_FEATURES = (4, 252, 256, 260, 764, 768, 772, 1540)
HEAD_SPLITS = ((191, 4), (12, 64), (193, 4), (2, 8), (3, 68))      # h * d / 4 = 191, 192, 193 (one trip and a float4 either side), 4, 51
SITE_KINDS = ("bth", "bhtd", "bhdt", "odd33", "one_feature", "strided", "unaligned")
LENGTH_KINDS = ("null", "zero", "full", "ragged", "shared")


def _site_geometry(kind, i, pick=None):
    """(memory shape, permutation, slicer, seq_pos, vec) of a site of `kind`; batch, tokens and width cycle with i
    (`pick` forces the width)."""
    B, T = (1, 2, 3)[(i // 2) % 3], (1, 3, 4, 5, 7)[(i // 3) % 5]            # T mostly no multiple of 4; B in pairs (shared lengths)
    k = (i // 7) if pick is None else pick
    if kind == "bth":
        return (B, T, BTH_FEATURES[k % 8]), None, None, 1, 1
    if kind in ("bhtd", "bhdt"):
        h, d = HEAD_SPLITS[k % 5]
        # [B,T,h,d] memory seen as [B,h,T,d] (seq_pos 2) or [B,h,d,T] (seq_pos 3): outer = h, inner = d (deferred.py)
        return (B, T, h, d), ((0, 2, 1, 3) if kind == "bhtd" else (0, 2, 3, 1)), None, (2 if kind == "bhtd" else 3), 1
    if kind == "odd33":
        return (B, T, 33), None, None, 1, 0
    if kind == "one_feature":
        return (B, T, 1), None, None, 1, 0
    if kind == "strided":                                                    # every other float: stride_inner == 2
        return (B, T, 2 * (5, 8, 66)[k % 3]), None, (slice(None), slice(None), slice(None, None, 2)), 1, 0
    return (B, T, 8), None, None, 1, 0                                       # "unaligned": starts one float off a 16-byte line


def site_view(flat, s):
    """The site's tensor as a view of the flat buffer `flat` (a NumPy array or a torch tensor: same steps)."""
    n = int(np.prod(s["mem_shape"]))
    v = flat[s["x_off"]:s["x_off"] + n].reshape(s["mem_shape"])
    if s["perm"] is not None:
        v = v.transpose(s["perm"]) if isinstance(v, np.ndarray) else v.permute(s["perm"])
    if s["slicer"] is not None:
        v = v[s["slicer"]]
    return v


def site_lengths(table, s):
    return None if s["len_off"] is None else table["lengths"][s["len_off"]:s["len_off"] + s["B"]]


def site_valid(table, s):
    """[B, T] bool: the token slots the kernel must write."""
    L = site_lengths(table, s)
    if L is None:
        return np.ones((s["B"], s["T"]), bool)
    return np.arange(s["T"])[None, :] < L[:, None]


def _fill_site(x4, valid, i, rng):
    """x4: the site's data as [B, T, F] (tokens x flattened features, a copy).  Every token's maximum and minimum sit at
    the first / last / a random feature, so that no element can be skipped unnoticed; then the specials."""
    B, T, Fn = x4.shape
    x4[...] = rng.standard_normal(x4.shape).astype(F32)
    for b in range(B):
        for t in range(T):
            k = b * T + t + i
            hi = (0, Fn - 1, int(rng.integers(Fn)))[k % 3]
            lo = (Fn - 1, 0, int(rng.integers(Fn)))[(k // 3) % 3]
            x4[b, t, hi] = F32(50 + rng.random())
            if lo != hi:
                x4[b, t, lo] = F32(-50 - rng.random())
    planted = set()
    vb, vt = np.nonzero(valid)
    pb, pt = np.nonzero(~valid)
    if len(vb):
        b, t = int(vb[i % len(vb)]), int(vt[i % len(vb)])
        what = i % 4
        if what == 0:                                   # a NaN in a valid token, at the first or the last feature
            x4[b, t, (0, Fn - 1)[(i // 4) % 2]] = np.nan
            planted.add("nan_valid")
        elif what == 1:                                 # infinities come through
            x4[b, t, Fn - 1] = np.inf
            x4[b, t, 0] = -np.inf if Fn > 1 else np.inf
            planted.add("inf_valid")
        elif what == 2:                                 # a token of zeros of both signs: the extremum IS a zero
            x4[b, t, :] = 0.0
            x4[b, t, ::2] = -0.0
            planted.add("zero_extremum")
    if len(pb) and i % 2:
        b, t = int(pb[i % len(pb)]), int(pt[i % len(pb)])
        x4[b, t, :] = (np.nan, np.inf, -np.inf)[(i // 2) % 3]      # padded tokens change nothing
        planted.add("special_padded")
    return planted


def _finish_site_table(name, sites, seed):
    rng = np.random.default_rng(seed)
    x_off = o_off = len_off = 0
    lens, prev = [], None
    for i, s in enumerate(sites):
        B, T = s["mem_shape"][0], s["mem_shape"][1]
        x_off += (-x_off) % 4                           # every site starts on a 16-byte line ...
        if s["kind"] == "unaligned":
            x_off += 1                                  # ... but these
        lk = s["length_kind"]
        if lk == "shared" and (prev is None or prev["B"] != B or prev["len_off"] is None):
            lk = "ragged"
        if lk == "null":
            off = None
        elif lk == "shared":
            off = prev["len_off"]                       # the very same device vector as the site before
        else:
            L = {"zero": np.zeros(B, np.int64), "full": np.full(B, T + (i % 2) * 2, np.int64),      # lengths beyond T: every token
                 "ragged": rng.integers(0, T + 1, B)}[lk].astype(np.int64)
            if lk == "ragged" and B > 1:
                L[i % B] = 0
                L[(i + 1) % B] = max(1, T - 1)
            if s.get("last_full"):
                L[-1] = T
            lens.append(L)
            off, len_off = len_off, len_off + B
        s.update(index=i, B=B, T=T, x_off=x_off, out_off=o_off + 1 + i % 3, len_off=off, length_kind=lk)
        x_off += int(np.prod(s["mem_shape"]))
        o_off = s["out_off"] + B * T
        prev = s
    # what no site owns (alignment gaps, the skipped floats of strided sites) holds +-1000: read by mistake it would win
    flat = np.where((np.arange(x_off) // 2) % 2 == 0, F32(1000), F32(-1000)).astype(F32)
    table = dict(name=name, sites=sites, lengths=np.concatenate(lens) if lens else np.zeros(0, np.int64), out_len=o_off + 2, x=flat)
    tok_end, total = [], 0
    for i, s in enumerate(sites):
        view = site_view(flat, s)                       # [B, ..., T, ...] as the observer sees it
        order = [0, s["seq_pos"]] + [a for a in range(view.ndim) if a not in (0, s["seq_pos"])]
        moved = np.empty((s["B"], s["T"], int(np.prod([view.shape[a] for a in order[2:]]))), F32)     # tokens x features
        s["planted"] = _fill_site(moved, site_valid(table, s), i, rng)
        view[...] = np.transpose(moved.reshape([view.shape[a] for a in order]), np.argsort(order))
        total += s["B"] * s["T"]
        tok_end.append(total)
    table.update(tok_end=np.asarray(tok_end, np.int64), total_tokens=total)
    return table


@functools.lru_cache(maxsize=None)
def site_table(name):
    """One table of osq_token_minmax_multi: flat data, flat lengths, per-site records (memory shape, permutation, slice,
    sequence axis, offsets).  Outputs of consecutive sites are 1-3 floats apart (out_off)."""
    seed = 2000 + SITE_TABLES.index(name)
    if name == "second_trip":
        # features = 4, 65536 + 61 token slots: the second trip ends inside the last site, on valid tokens
        shapes = ((3, 7), (8, 4100), (8, 4097))
        sites = [dict(kind="bth", mem_shape=(B, T, 4), perm=None, slicer=None, seq_pos=1, vec=1,
                      length_kind=("null", "ragged", "ragged")[k], last_full=True) for k, (B, T) in enumerate(shapes)]
        return _finish_site_table(name, sites, seed)
    n = int(name[1:])
    sites = []
    for i in range(n):
        kind, pick, lk = (SITE_KINDS[i % 7] if n > 2 else ("bth", "bhdt")[i]), None, LENGTH_KINDS[(i // 2) % 5]
        if n > 2 and i in (0, n - 1, LDS_SITES - 1, LDS_SITES):
            # the ends of the table and both sides of the LDS limit: rows of more than one trip, ragged lengths
            kind, pick, lk = ("bth", "bhtd")[i % 2], (7, 2)[i % 2], "ragged"
        shape, perm, slicer, seq_pos, vec = _site_geometry(kind, i, pick)
        sites.append(dict(kind=kind, mem_shape=shape, perm=perm, slicer=slicer, seq_pos=seq_pos, vec=vec, length_kind=lk,
                          last_full=pick is not None))
    return _finish_site_table(name, sites, seed)


@functools.lru_cache(maxsize=None)
def site_reference(name):
    """(token_min, token_max, written): NumPy min / max over the feature axes of every site at its output offset (a NaN in a
    token makes both NaN, as np.min / np.max do), SENTINEL everywhere else; `written` marks the valid slots."""
    t = site_table(name)
    mn = np.full(t["out_len"], SENTINEL, F32)
    mx = np.full(t["out_len"], SENTINEL, F32)
    written = np.zeros(t["out_len"], bool)
    for s in t["sites"]:
        view = site_view(t["x"], s)
        axes = tuple(a for a in range(view.ndim) if a not in (0, s["seq_pos"]))
        valid = site_valid(t, s).reshape(-1)
        sl = slice(s["out_off"], s["out_off"] + s["B"] * s["T"])
        with np.errstate(invalid="ignore"):
            mn[sl] = np.where(valid, view.min(axis=axes).reshape(-1), SENTINEL)
            mx[sl] = np.where(valid, view.max(axis=axes).reshape(-1), SENTINEL)
        written[sl] = valid
    return mn, mx, written


def site_features(s):
    """Elements per token, and whether the 16-byte path may be promised (`vec`)."""
    shape = list(s["mem_shape"])
    if s["slicer"] is not None:
        shape[2] //= 2
    return int(np.prod(shape[2:])), s["vec"]


# ------------------------------------------------------------------------------------------- batched finaliser

FINAL_SHAPES = tuple((q, b) for q in (1, 3, 40) for b in (1, 3))
FINAL_PERCENTILES = (0.0, 0.5, 0.9, 1.0)
FINAL_GEOMETRY = {False: (8, 16), True: (16, 64)}   # batch x tokens: 128 slots, and 1024 = the lowest wide switch point the library takes
FINAL_WIDE_MIN = 1024
FINAL_SLACK = 8                             # problem_stride = B * T + 8: the batched entry must step by the stride


@functools.lru_cache(maxsize=None)
def final_table(n_q, n_b, wide=False):
    """Per-token extrema of n_q quantizers x n_b batches with FINAL_SLACK floats of slack behind every problem (NaN behind
    token_min, +inf behind token_max: read by mistake they would show), every quantizer its own lengths, prune flags of
    both kinds; problem 0 is all padding (when there is more than one) and the last one has a single valid token."""
    rng = np.random.default_rng(3000 + 10 * n_q + n_b + 500 * wide)
    FINAL_B, FINAL_T = FINAL_GEOMETRY[bool(wide)]
    S = FINAL_B * FINAL_T
    stride = S + FINAL_SLACK
    tmax = (np.abs(rng.standard_normal((n_q, n_b, stride))) * rng.choice([1.0, 1.0, 8.0], (n_q, n_b, stride)) + 0.5).astype(F32)
    tmin = (tmax - 1.0 - np.abs(rng.standard_normal((n_q, n_b, stride))) * 3).astype(F32)
    dup = rng.random((n_q, n_b)) < 0.3                                   # heavy duplicates: a few distinct values
    tmax[dup] = np.round(tmax[dup])
    tmin[dup] = np.round(tmin[dup])
    tmin[..., S:] = np.nan
    tmax[..., S:] = np.inf
    lengths = rng.integers(0, FINAL_T + 1, (n_q, n_b, FINAL_B)).astype(np.int64)
    lengths[:, :, 0] = FINAL_T
    if n_q * n_b > 1:
        lengths[0, 0, :] = 0                                             # all padding: its row of cur_table stays as it was
    lengths[-1, -1, :] = 0
    lengths[-1, -1, FINAL_B // 2] = 1                                    # a single valid token
    flags = np.asarray([0 if (q % 4 == 1) else 1 for q in range(n_q)], np.int32)
    return dict(n_q=n_q, n_b=n_b, B=FINAL_B, T=FINAL_T, stride=stride, tmin=tmin, tmax=tmax, lengths=lengths, flags=flags)


@functools.lru_cache(maxsize=None)
def final_reference(n_q, n_b, percentile, wide=False):
    """cur_table [n_b, n_q, 2] as uint32 words: observer_oracle.prune_thresholds over the valid tokens (plain extrema where
    the quantizer does not prune), SENTINEL where nothing is valid."""
    t = final_table(n_q, n_b, wide)
    cur = np.full((n_b, n_q, 2), SENTINEL, F32)
    for q in range(n_q):
        for b in range(n_b):
            valid = (np.arange(t["T"])[None, :] < t["lengths"][q, b][:, None]).reshape(-1)
            if not valid.any():
                continue
            mn, mx = t["tmin"][q, b, :valid.size][valid], t["tmax"][q, b, :valid.size][valid]
            if t["flags"][q]:
                lo, up = OB.prune_thresholds(mn, mx, percentile)
                cur[b, q] = (up if lo > up else lo, up)
            else:
                cur[b, q] = (OB.zmin(mn), OB.zmax(mx))
    return bits(cur)

"""Launch shapes, case tables and planted elements for the sixteen kernels of csrc/msefast.hip (tests/test_oracle_msefast_shapes.py
checks on the CPU what the tables promise, tests/test_gpu_msefast_shapes.py runs them on the device).  Everything here is
NumPy and the oracle; no device code is imported.

The constants restate the launchers; the predictors mirror their decision text; the case tables are built round every
threshold the predictors know.  A whole Brent search is a weak detector of a dropped element (the search may land on the same
range anyway), so the cases that look for an off-by-one PLANT one element of V sigma at the position a bug would lose: with
that element's loss contribution removed (extrema kept) the oracle's own search finds a range at least 1.5 times away
(`decides`), so a kernel that loses the element cannot return the oracle's words.
"""
import functools

import numpy as np

from oracle import observer_oracle as OB

F32 = np.float32

# ---- per-channel rows: osq_msefast_rows / msefast_rows_kernel<MAXV, ATEN>
WAVE = 64                       # OSQ_WAVE: one wave per row, lane l caches columns l, l + 64, ...
ROW_WAVES = 4                   # kWavesPerBlock = kThreads / OSQ_WAVE: rows per workgroup
ROW_MAXV = (4, 16, 48)          # cols <= 64 * 4 / 64 * 16 / 64 * 48
ROW_LONG_MAX = 32767            # order && cols > 64 * 48 && cols < 32768: the long-row form, cols * 4 bytes of dynamic LDS
ROW_FALLBACK = 32768            # from here the order-free sum ("mse_sum_order" 8 / 16: OSQ_ERR_UNSUPPORTED)
# ---- streaming forms: osq_msefast_tensor_evals_flat / _tokens
THREADS = 256                   # kThreads
MAX_BLOCKS = 2048               # kMaxBlocks (osq_host.h)
# ---- resident forms: osq_msefast_tensor_search / _search_multi
RES_THREADS = 512               # kResThreads
RES_STAGE = 8                   # kResStage: slots staged through LDS per turn of resident_fill
RES_LADDER = (1, 2, 4, 8, 16, 24, 32)       # OSQ_RESIDENT(K)
RES_MULTI_LADDER = (8, 16, 24, 32)          # OSQ_RESIDENT_MULTI(KT)
RES_MULTI_REG_SLOTS = 24        # KR = KT > 24 ? 24 : KT: slots 24 .. 31 of the 32-slot form live in LDS
RES_MAX_SLOTS = 32              # kResMaxSlots
RES_MAX_BATCH = 512             # kResMaxBatch = kResThreads
RES_MAX_SITES = 16              # kResidentMaxSites (osq_host.h)
RES_MAX_BLOCKS = 512            # kResidentMaxBlocks (osq_host.h)
NOMINAL_PER_K = 256 * RES_THREADS * 4       # per_k of a grid of 256 workgroups (one per CU of an MI355X): the CPU tests' stand-in


def ceil_div(a, b):
    return -(-a // b)


def grid_for(work_items, per_block, max_blocks=MAX_BLOCKS):
    """osq_host.h: grid_for."""
    return max(1, min(ceil_div(work_items, per_block), max_blocks))


# =========================================================================================== predictors

def predict_rows(cols, rows_order=8, sum_order=0):
    """osq_msefast_rows -> (form, MAXV, short_path).  form: "ordered" (msefast_rows_kernel<MAXV, true>), "ordered-long"
    (<0, true>, one wave per workgroup), "order-free" (<MAXV>), "unsupported".  short_path: the row is shorter than one SIMD
    vector of the order and takes aten_sum_short."""
    forced = sum_order in (8, 16)
    order = sum_order if forced else rows_order
    if order and cols > 64 * 48 and cols < 32768:
        return "ordered-long", 0, False
    if forced and cols >= 32768:
        return "unsupported", None, False
    maxv = 4 if cols <= 64 * 4 else 16 if cols <= 64 * 16 else 48 if cols <= 64 * 48 else 0
    if order and cols <= 64 * 48:
        return "ordered", maxv, cols < order
    return "order-free", maxv, False


def flat_stride(n):
    """float4s between two loads of one thread of msefast_flat_loss_kernel: gridDim.x * kThreads."""
    return grid_for(n // 4, THREADS * 2) * THREADS


def predict_flat(n):
    """osq_msefast_tensor_evals_flat + the loop of msefast_flat_loss_kernel -> (grid, parts reached).  "pair": a trip whose
    second float4 exists (`two`); "single": one whose second does not; "second trip": i += 2 * stride stays below n4;
    "tail1..3": n % 4 elements read by workgroup 0."""
    n4 = n // 4
    grid = grid_for(n4, THREADS * 2)
    stride = grid * THREADS
    parts = set()
    if n4 > stride:
        parts.add("pair")
    if n4 % (2 * stride):
        parts.add("single")
    if n4 > 2 * stride:
        parts.add("second trip")
    if n % 4:
        parts.add("tail%d" % (n % 4))
    return grid, parts


def token_geometry(x, seq_pos, n_lengths):
    """ops.token_view restated for a NumPy array (element strides)."""
    seq_pos %= x.ndim
    others = [d for d in range(x.ndim) if d != seq_pos]
    st = [s // x.itemsize for s in x.strides]
    if len(others) == 3:
        outer, inner, s_outer, s_inner = x.shape[others[1]], x.shape[others[2]], st[others[1]], st[others[2]]
    else:
        outer, inner, s_outer, s_inner = 1, x.shape[others[1]], 0, st[others[1]]
    return dict(batch=min(x.shape[0], n_lengths), tokens=x.shape[seq_pos], feat_outer=outer, feat_inner=inner,
                stride_batch=st[0], stride_token=st[seq_pos], stride_outer=s_outer, stride_inner=s_inner)


def predict_tokens(view, aligned=True):
    """osq_msefast_tensor_evals_tokens -> (vec, grid, parts): one wave per token, a second trip when the capped grid has
    fewer waves than there are tokens."""
    v = view
    vec = bool(v["stride_inner"] == 1 and v["feat_inner"] % 4 == 0 and aligned and v["stride_batch"] % 4 == 0 and
               v["stride_token"] % 4 == 0 and (v["feat_outer"] == 1 or v["stride_outer"] % 4 == 0))
    ntok = v["batch"] * v["tokens"]
    grid = grid_for(ntok, ROW_WAVES)
    return vec, grid, ({"second trip"} if ntok > grid * ROW_WAVES else set())


def predict_resident(elems, per_k):
    """osq_msefast_tensor_search -> K of msefast_resident_kernel<K>, 0: falls back to the streaming form."""
    need = ceil_div(elems, per_k)
    if need > RES_MAX_SLOTS:
        return 0
    return next(k for k in RES_LADDER if need <= k)


def predict_resident_multi(slot_list):
    """osq_msefast_tensor_search_multi -> (KT, indices of the sites with a slot kept in LDS); (0, ()) when the group does not
    fit (more than 16 sites, more than 32 slots)."""
    total = sum(slot_list)
    if len(slot_list) > RES_MAX_SITES or total > RES_MAX_SLOTS or min(slot_list) < 1:
        return 0, ()
    kt = next(k for k in RES_MULTI_LADDER if total <= k)
    lds, slot0 = [], 0
    for i, s in enumerate(slot_list):
        if kt > RES_MULTI_REG_SLOTS and slot0 + s > RES_MULTI_REG_SLOTS:
            lds.append(i)
        slot0 += s
    return kt, tuple(lds)


# =========================================================================================== planted elements

def plant_value(n):
    """V for n observed elements of sigma 1 (4 or 6 bit): large enough that the oracle's search follows the element
    (tests/test_oracle_msefast_shapes.py holds `decides` >= 1.5 for every case built with it), and, from 10^5 elements on,
    small enough that the search WITHOUT the element still sees the bulk: scipy's bounded search starts at 0.382 V and
    0.618 V, and at 6 bits every element of the bulk rounds to zero there once V exceeds about 870 sigma -- two equal
    losses, and the search walks to V with or without the element (V = 3000 at 4.2 M elements: ratio 1.000)."""
    for limit, v in ((300, 12.0), (1100, 20.0), (8000, 40.0), (40000, 120.0), (80000, 200.0)):
        if n <= limit:
            return v
    return 700.0


@functools.lru_cache(maxsize=64)
def normal(shape, sigma=1.0, seed=0):
    """The seeded normal fp32 tensor every planted case of one shape starts from (read-only)."""
    shape = (shape,) if isinstance(shape, int) else tuple(shape)
    rng = np.random.default_rng([7101, seed, *shape])
    x = (rng.standard_normal(shape, dtype=F32) * F32(sigma)).astype(F32)
    x.setflags(write=False)
    return x


def planted(n_or_shape, positions, sigma, V, seed=0):
    """One tensor per position: normal(sigma) data with the single element `position` (a flat index or an index tuple) set to
    V.  A generator: the tensors of the largest case are 17 MB each."""
    base = normal(n_or_shape, sigma, seed)
    for p in positions:
        x = base.copy()
        x[p] = F32(V)
        yield p, x


def flat_positions(n):
    """Element 0, the last element (the tail's last when n % 4), and the elements on either side of 4 * stride (where a
    thread's second float4 of a trip begins) and of 8 * stride (where the second trip begins) -- those that exist."""
    s = flat_stride(n)
    return tuple(sorted({p for p in (0, n - 1, 4 * s - 1, 4 * s, 8 * s - 1, 8 * s) if 0 <= p < n}))


def resident_positions(n, per_k, first_slot=0):
    """The last element of slot k - 1 and the first of slot k for k in 1, 2, 4, 8, 16, 24 (where resident_fill's staging
    loop turns over, the ladder changes form and the multi-site kernel leaves the registers) from slot `first_slot` on, and
    the last valid element."""
    out = {n - 1}
    for k in (1, 2, 4, 8, 16, 24):
        if k >= max(first_slot, 1):
            out.update(p for p in (k * per_k - 1, k * per_k) if p < n)
    return tuple(sorted(out))


def row_positions(cols, rows_order):
    """Columns 0, 63, 64 (the lane loop's turn-over), 64 * MAXV - 1 (the last cached column of each instantiation) and
    cols - 1; under an ordered form also the first column of the cols % width scalar tail and of the cols % (4 * width)
    remainder of the four interleaved accumulators."""
    out = {0, 63, 64, cols - 1} | {64 * m - 1 for m in ROW_MAXV}
    if rows_order:
        if cols % rows_order:
            out.add(cols - cols % rows_order)
        if cols % (4 * rows_order):
            out.add(cols - cols % (4 * rows_order))
    return tuple(sorted(p for p in out if 0 <= p < cols))


def scheme_state(bit, symmetric, x=None, ch_axis=-1):
    st = OB.ObserverState(bit=bit, symmetric=symmetric, ch_axis=ch_axis)
    if x is not None:
        st.one_side_dist = OB.one_side_dist(x)
    return st


def found_range(x, x_min, x_max, st):
    search = OB.msefast_search_1d if (st.one_side_dist != "no" or st.symmetric) else OB.msefast_search_2d
    lo, hi = search(np.ascontiguousarray(x, dtype=F32).reshape(-1), x_min, x_max, st)
    return float(hi) - float(lo)


def decides(x, position, st, row_vec=None):
    """Ratio (>= 1) of the ranges the oracle's own search finds on x and on x with the planted element's contribution removed
    (the element set to 0, whose squared error is 0 under every candidate; x_min / x_max of x kept).  row_vec: the row
    summation order of a per-channel search (None: the exact mean)."""
    x = np.asarray(x, dtype=F32)
    x_min, x_max = OB.aminmax(x)
    without = x.copy()
    without[position] = F32(0)
    old = OB.MEAN_LIKE_TORCH
    if row_vec is not None and x.size < ROW_FALLBACK:
        from oracle.aten_sum import aten_mean_f32
        OB.MEAN_LIKE_TORCH = lambda sq: aten_mean_f32(sq, row_vec)      # noqa: E731
    try:
        a, b = found_range(x, x_min, x_max, st), found_range(without, x_min, x_max, st)
    finally:
        OB.MEAN_LIKE_TORCH = old
    return max(a / b, b / a) if a > 0 and b > 0 else float("inf")


# =========================================================================================== a. rows

ROW_ORDERS = (8, 16, 0)         # "mse_rows_order"; the oracle's ROW_SUM_VEC: 8, 16, None
ROW_COLS_FORMS = (1, 2, 255, 256, 257, 1023, 1024, 1025, 3071, 3072, 3073, 32767, 32768)
ROW_COLS_WIDTHS = (7, 8, 9, 15, 16, 17, 31, 32, 33)
ROW_COLS_SHORT16 = (10, 11, 12, 13, 14)         # with 8, 9 and 15 above: every row of 8 to 15 columns
ROW_COLS = tuple(sorted(ROW_COLS_FORMS + ROW_COLS_WIDTHS + ROW_COLS_SHORT16))
ROW_SCHEMES = (("sym", 4, True), ("asym", 4, False))
ROW_ASYM_MAX_COLS = 3073
ROW_PLANTED_COLS = (9, 17, 33, 100, 256, 257, 1024, 1025, 3072, 3073, 32767, 32768)
ROW_PLANTED_ASYM_COLS = (257, 1025)


def row_vec(rows_order):
    return rows_order or None


def row_counts(cols):
    """1 (a lone wave), 3 (a partly filled workgroup), 4 (a full one), 5 (a second, partly filled)."""
    return (1, 2) if cols >= ROW_LONG_MAX else (1, 3, 4, 5)


@functools.lru_cache(maxsize=None)
def row_weights(cols):
    return normal((max(row_counts(cols)), cols), 1.0, 1)


def row_units():
    """(cols, rows_order, scheme name) of the plain row cases."""
    return [(c, o, s[0]) for c in ROW_COLS for o in ROW_ORDERS for s in ROW_SCHEMES if s[0] == "sym" or c <= ROW_ASYM_MAX_COLS]


def row_planted_units():
    """(cols, rows_order, scheme name) of the planted row cases; row_planted_cases lists the tensors of one."""
    return [(c, o, s[0]) for c in ROW_PLANTED_COLS for o in ROW_ORDERS for s in ROW_SCHEMES
            if s[0] == "sym" or c in ROW_PLANTED_ASYM_COLS]


def row_planted_cases(cols, rows_order):
    """[(column, weights)]: the element planted at `column` of the FIRST and of the LAST row of one tensor."""
    w = row_weights(cols)
    out = []
    for p in row_positions(cols, rows_order):
        x = w.copy()
        x[0, p] = x[-1, p] = F32(plant_value(cols))
        out.append((p, x))
    return out


def degenerate_rows(cols=40):
    """An all-zero row, a constant positive row, a constant negative row and a row with one non-zero element between normal rows."""
    w = normal((7, cols), 1.0, 2).copy()
    w[1] = F32(0)
    w[2] = F32(0.37)
    w[4] = F32(-1.25)
    w[5] = F32(0)
    w[5, cols // 3] = F32(-2.5)
    return w


_row_memo = {}


def oracle_row(row, bit, symmetric, side, vec):
    """(min, max, evaluations) of the oracle's per-channel search of one row, summed on `vec` lanes (None: the exact mean).
    observe_msefast itself on a one-row tensor; memoised by the row's bytes: rows shared between cases are searched once."""
    row = np.ascontiguousarray(row, dtype=F32).reshape(1, -1)
    key = (row.tobytes(), bit, symmetric, side, vec)
    if key not in _row_memo:
        st = OB.ObserverState(bit=bit, symmetric=symmetric, ch_axis=0)
        st.one_side_dist = side
        counter = [0]
        old = OB.ROW_SUM_VEC
        OB.ROW_SUM_VEC = vec
        try:
            OB.observe_msefast(st, row, counter=counter)
        finally:
            OB.ROW_SUM_VEC = old
        _row_memo[key] = (F32(st.min_val[0]), F32(st.max_val[0]), counter[0])
    return _row_memo[key]


def oracle_rows(w, bit, symmetric, vec):
    """-> (min[rows], max[rows], evaluations[rows]); the sidedness is the whole tensor's (observer.py:528-529)."""
    side = OB.one_side_dist(w)
    got = [oracle_row(r, bit, symmetric, side, vec) for r in w]
    return (np.array([g[0] for g in got], F32), np.array([g[1] for g in got], F32), np.array([g[2] for g in got], np.int32))


# =========================================================================================== b. streaming flat form

FLAT_LENGTHS = (1, 2, 3, 4, 5, 7, 1023, 1027, 4 * 512 * 3, 4 * 512 * 3 + 1, 4 * 512 * 3 + 2, 4 * 512 * 3 + 3, 7200)
FLAT_SINGLE_AND_PAIR = 7200                     # 1800 float4s on a stride of 1024: threads 0..775 pair, the rest single
FLAT_BIG = 4 * (2 * MAX_BLOCKS * THREADS) + 1203        # the capped grid's second trip (300 float4s) and a tail of 3
FLAT_PLANTED_LENGTHS = tuple(n for n in FLAT_LENGTHS if n >= 1023) + (FLAT_BIG,)
FLAT_SCHEMES = (("sym", 6, True), ("asym", 6, False))
FLAT_MISALIGNED = 4099                          # observed from a base 4 bytes off a 16-byte boundary


def flat_data(n):
    return normal(n, 1.0, 3)


def flat_planted_positions(n):
    """flat_positions; the 4.2 M-element case keeps the four only it can reach (its oracle search takes seconds)."""
    if n == FLAT_BIG:
        s = flat_stride(n)
        return (4 * s, 8 * s - 1, 8 * s, n - 1)
    return flat_positions(n)


def oracle_tensor(x, bit, symmetric, lengths=None, seq_pos=-1, calls=1, mean=None):
    """[(min_val, max_val, evaluations)] after each of `calls` calls of a fresh MSEFastObserver on x (the second call runs
    in float64, observer.py:524); mean: OB.MEAN_LIKE_TORCH for the duration (None: the correctly rounded mean)."""
    st = OB.ObserverState(bit=bit, symmetric=symmetric)
    old = OB.MEAN_LIKE_TORCH
    OB.MEAN_LIKE_TORCH = mean
    out = []
    try:
        for _ in range(calls):
            counter = [0]
            OB.observe_msefast(st, x, lengths, seq_pos, counter=counter)
            out.append((np.float64(st.min_val), np.float64(st.max_val), counter[0]))
    finally:
        OB.MEAN_LIKE_TORCH = old
    return out


# =========================================================================================== c. streaming token form

class TokenCase:
    """mem: the dense array in memory; view(a): the observed view (basic indexing / transposes: serves NumPy and torch);
    lengths / seq_pos as the observer gets them."""

    def __init__(self, mem_shape, view, lengths, seq_pos, seed):
        self.mem_shape, self.view, self.seq_pos, self.seed = tuple(mem_shape), view, seq_pos, seed
        self.lengths = np.asarray(lengths, dtype=np.int64)

    def mem(self):
        return normal(self.mem_shape, 1.0, self.seed).copy()

    def geometry(self):
        return token_geometry(self.view(self.mem()), self.seq_pos, self.lengths.size)

    def tokens_first(self, a):
        """[B, T, F]-shaped index helper: the view with the sequence axis second, features flattened (a copy)."""
        return OB._tokens_first(self.view(a), self.seq_pos % self.view(a).ndim)

    def last_valid(self):
        """(sample, token) of the last valid token of the last non-empty sample, T."""
        T = self.view(self.mem()).shape[self.seq_pos]
        n = min(self.lengths.size, self.view(self.mem()).shape[0])
        b = max(i for i in range(n) if self.lengths[i] > 0)
        return b, int(min(self.lengths[b], T)) - 1, T

    def plant(self, a, where, V):
        """Set one element of the dense array `a` (NumPy, in place) through the view: where = "valid" (last feature of the
        last valid token of the last non-empty sample) or "padded" (first feature of the token after it)."""
        b, t, T = self.last_valid()
        v = self.view(a)
        sp = self.seq_pos % v.ndim
        idx = [slice(None)] * v.ndim
        idx[0], idx[sp] = b, (t if where == "valid" else t + 1)
        assert idx[sp] < T
        sub = v[tuple(idx)]                         # a view of `a`: the remaining feature axes
        sub[(-1,) * sub.ndim if where == "valid" else (0,) * sub.ndim] = F32(V)


_BT = lambda a: a                                   # noqa: E731
TOKEN_CASES = {
    # lengths hold 0, T and a value above T (clamped by the kernels, sliced by the oracle); the last non-empty sample stops short of T
    "dense_F4": TokenCase((5, 7, 4), _BT, (0, 7, 9, 3, 0), 1, 10),
    "dense_F6": TokenCase((5, 7, 6), _BT, (7, 0, 9, 1, 5), 1, 11),
    "dense_F64": TokenCase((5, 7, 64), _BT, (0, 9, 7, 2, 6), 1, 12),
    "dense_F68": TokenCase((5, 7, 68), _BT, (3, 7, 0, 9, 4), 1, 13),
    "head_split": TokenCase((4, 9, 3, 8), lambda a: a.transpose(0, 2, 1, 3) if isinstance(a, np.ndarray) else a.permute(0, 2, 1, 3),
                            (9, 0, 11, 4), 2, 14),                  # [B, h, T, d] over [B, T, h, d] memory: feat_outer 3, vector loads
    "key_view": TokenCase((5, 3, 8, 9), _BT, (2, 9, 0, 12, 7), 3, 15),     # [B, h, d, T] in memory: the inner axis has stride T, scalar loads
    "zip_3d": TokenCase((12, 6, 20), _BT, (6, 0, 8, 3), 1, 16),         # [B * h, T, S] with B lengths: zip() stops at the mask
    "grid_cap": TokenCase((1171, 7, 4), _BT, tuple(int(v) for v in np.random.default_rng(7102).integers(0, 9, 1169)) + (7, 5), 1, 17),
    "grid_cap_F6": TokenCase((1171, 7, 6), _BT, tuple(int(v) for v in np.random.default_rng(7103).integers(0, 9, 1169)) + (7, 4), 1, 18),
}                                                                    # 8197 tokens: past the 2048-workgroup cap, vector and scalar loads


def token_observed(case, mem=None):
    return OB.remove_padding(case.view(case.mem() if mem is None else mem), case.lengths, case.seq_pos)


# =========================================================================================== d. / e. resident forms

def resident_sizes(per_k):
    """{K: (K_prev * per_k + 1, K * per_k - 3, K * per_k)} for every K of the ladder."""
    return {k: (kp * per_k + 1, k * per_k - 3, k * per_k) for kp, k in zip((0,) + RES_LADDER, RES_LADDER)}


def resident_planted_positions(n, per_k, k_prev):
    """The positions this K adds to the smaller ones: the slot boundaries from K_prev on, the last valid element; the first
    element stands in when there is no boundary inside."""
    pos = resident_positions(n, per_k, first_slot=max(k_prev, 1))
    return pos if len(pos) > 1 else tuple(sorted({0} | set(pos)))


# slots of each site of a multi-site group (a site of s slots holds between (s - 1) * per_k + 1 and s * per_k elements)
MULTI_GROUPS = {
    "sum8": (3, 5), "sum9": (4, 5), "sum16": (7, 9), "sum17": (9, 8), "sum24": (12, 12),
    "sum25_straddle": (23, 2),          # site 1 holds slots 23 and 24: its first in registers, its second in LDS
    "sum32_lds_site": (10, 14, 8),      # site 2 lies wholly in slots 24 .. 31; the planted element is in it
    "sixteen_ones": (1,) * 16, "sixteen_twos": (2,) * 16,
    "masked_inside": (2, 1, 3),         # site 1 is a masked [B, T, F] site
}
MULTI_REJECTED = {"seventeen_sites": (1,) * 17, "sum33": (16, 17)}


def multi_site_elems(slots, i, per_k):
    """Elements of site i of a group: full, three short of full, or one past the previous slot, in turn."""
    return (slots * per_k, slots * per_k - 3, (slots - 1) * per_k + 1)[i % 3]

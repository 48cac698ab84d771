"""Case tables, float64 references and bounds for the kernels of csrc/observers_extra.hip: the moments of LSQPlusObserver,
the histogram of AvgQuantileObserver, the grid of MSEObserver / AvgMSEObserver (tests/test_oracle_extra_observers.py checks
what the tables promise with the references alone, tests/test_gpu_extra_observers.py runs them on the device).  Everything
here is NumPy / CPU torch; no device code is imported.

The constants restate the launch shapes of the kernels; the cases are built around them: a flat tensor of more float4s than
the capped grid holds in one trip, a base 4 bytes off a 16-byte boundary (scalar loads), a tail of 1 to 3 elements, rows of
whole 256-float pieces (the "pieces" dealing of mse_grid_all_kernel) and every way of missing that predicate.
"""
import functools

import numpy as np
import torch

from oracle import observer_oracle as OB

F32 = np.float32

THREADS = 256                   # kThreads
MOMENT_MAX_BLOCKS = 1024        # osq_observe_moments: make_source(..., 1024)
HIST_MAX_BLOCKS = 256           # osq_observe_quantile / osq_mse_grid_tensor: make_source(..., 256)
HIST_BINS = 2048                # kHistBins; 8 consecutive bins per thread of the finaliser, 512 per wave
GRID_ALL_WAVES = 16             # kGridAllThreads / 64
GRID_ALL_MAX_BLOCKS = 256       # kGridAllMaxBlocks
GRID_ALL_MAX_BATCH = 1024       # kGridAllMaxBatch: prefix sums of the lengths in LDS
PIECE = 256                     # floats of one piece: one float4 per lane
FAST_DIVIDEND_MIN = F32(8.6736174e-19)      # div_fast_dividend: smaller non-zero magnitudes take the true division


def ulp32(v):
    """Spacing of fp32 at |v|."""
    return np.float64(np.spacing(np.abs(F32(v))))


# =========================================================================================== 1. moments (LSQ+)

MOMENT_PAIRS = ((0.0, 1.0), (1.0, 0.02), (1.0, 0.001), (10.0, 0.1), (100.0, 0.01), (-100.0, 0.01))     # (mean, std)
MOMENT_NS = (1, 2, 3, 5, 1023, 1024, 1027, 4096, 20483)
MOMENT_BIG_N = 4 * 1024 * 1024 + 3          # 1025 workgroups' worth of float4s: the 1024-block cap and a second trip, tail of 3
MOMENT_CONSTANTS = (0.1, -3.7, 0.0)         # constant data: std exactly 0
MOMENT_CONSTANT_NS = (2, 5, 1027, 20483)
MOMENT_CHANNEL_CASES = (((7, 300), 0), ((5, 9, 1), 1), ((3, 4, 257), 1), ((4, 1), 0))     # (shape, ch_axis)


def moment_data(n, mean, std, seed=0):
    rng = np.random.default_rng([7001, seed, n])
    return (mean + std * rng.standard_normal(n)).astype(F32)


def moment_channel_data(shape, ch_axis, seed=0):
    """Channel c is drawn with MOMENT_PAIRS[c % 6]."""
    rng = np.random.default_rng([7002, seed, *shape])
    x = rng.standard_normal(shape)
    bshape = [1] * len(shape)
    bshape[ch_axis] = shape[ch_axis]
    pairs = np.array([MOMENT_PAIRS[c % len(MOMENT_PAIRS)] for c in range(shape[ch_axis])])
    return (pairs[:, 0].reshape(bshape) + pairs[:, 1].reshape(bshape) * x).astype(F32)


def moment_range(mean64, std64):
    """(min, max, bound) from float64 moments: mean32 = f32(mean64), std32 = f32(std64), min / max = mean32 -+ f32(3) * std32
    in fp32 (observer.py:171-172, as oracle.observe_lsqplus).

    bound = 4 ulp32(|mean32| + 3 std32).  A result computed from correctly rounded moments may still take mean32 and std32
    one ulp away when the float64 values sit near a rounding boundary: 1 ulp(mean) + 3 ulp(std) -- and 3 ulp(std) <= 1.5 ulp
    of the product 3 std, an fp32 number of twice to four times the magnitude -- plus the two roundings of 3 * std and of the
    sum, half an ulp each.  All four are at most one ulp of |mean32| + 3 std32, which bounds the magnitude of every term."""
    mean32 = np.asarray(mean64, dtype=np.float64).astype(F32)
    std32 = np.asarray(std64, dtype=np.float64).astype(F32)
    three = F32(3) * std32
    with np.errstate(invalid="ignore"):
        bound = 4.0 * np.spacing(np.abs(mean32).astype(F32) + three).astype(np.float64)
    return (mean32 - three).astype(F32), (mean32 + three).astype(F32), bound


def moment_reference(x, ch_axis=-1):
    """Two-pass float64 moments (unbiased std; NaN for one element, as torch.std) -> (min, max, bound)."""
    x = np.asarray(x, dtype=F32)
    rows = (x.reshape(1, -1) if ch_axis == -1 else OB._to_channel_rows(x, ch_axis)).astype(np.float64)
    mean = rows.mean(axis=1)
    dev = rows - mean[:, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        std = np.sqrt((dev * dev).sum(axis=1) / np.float64(rows.shape[1] - 1)) if rows.shape[1] > 1 else np.full(rows.shape[0], np.nan)
    mn, mx, bound = moment_range(mean, std)
    return (mn[0], mx[0], bound[0]) if ch_axis == -1 else (mn, mx, bound)


def moment_within(got, want, bound):
    """|got - want| <= bound elementwise; NaN where and only where the reference is NaN."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and (np.abs(got - want)[~nan] <= np.broadcast_to(bound, want.shape)[~nan]).all())


def moment_thread_sequences(x, misaligned=False):
    """The elements each thread of moments_flat_kernel adds, in its order: [threads, longest] zero-padded at the END (a
    trailing zero changes no sum).  Aligned base: float4 i goes to thread i mod (grid * 256), the 1 to 3 tail elements to
    threads 0..2 of workgroup 0 after their float4s; misaligned base: element i to thread i mod (grid * 256)."""
    x = np.asarray(x, dtype=F32).ravel()
    n = x.size
    grid = min(MOMENT_MAX_BLOCKS, max(1, (n // 4 + 1 + 4 * THREADS - 1) // (4 * THREADS)))
    T = grid * THREADS
    e = np.arange(n)
    if misaligned:
        thread, pos = e % T, e // T
    else:
        n4 = n // 4
        i = e // 4
        thread, pos = i % T, 4 * (i // T) + e % 4
        t = e[4 * n4:] - 4 * n4                                    # the tail: thread t, after its (n4 - t + T - 1) // T float4s
        thread[4 * n4:], pos[4 * n4:] = t, 4 * np.maximum((n4 - t + T - 1) // T, 0)
    seq = np.zeros((T, int(pos.max()) + 1), dtype=F32)
    seq[thread, pos] = x
    return seq


def moment_emulation(x, form, misaligned=False):
    """(min, max) of the per-tensor kernel's arithmetic in NumPy.  form "fp32-products": v * v and runs of 32 in fp32, float64
    totals, var = (sumsq - n mean^2) / (n - 1) -- the kernel before this suite.  form "f64-shifted": float64 sums of
    d = v - x[0] and d * d -- the kernel now (float64 additions in NumPy's order rather than the grid's: the order moves a
    float64 sum of these sizes by parts in 1e-13, five orders below the bound)."""
    x = np.asarray(x, dtype=F32).ravel()
    n = np.float64(x.size)
    if form == "fp32-products":
        seq = moment_thread_sequences(x, misaligned)
        a0, a1 = np.zeros(seq.shape[0]), np.zeros(seq.shape[0])
        for r0 in range(0, seq.shape[1], 32):
            s1, s2 = np.zeros(seq.shape[0], F32), np.zeros(seq.shape[0], F32)
            for k in range(r0, min(r0 + 32, seq.shape[1])):
                v = seq[:, k]
                s1 = (s1 + v).astype(F32)
                s2 = (s2 + (v * v).astype(F32)).astype(F32)
            a0, a1 = a0 + s1, a1 + s2
        shift, s, ss = 0.0, a0.sum(), a1.sum()
    elif form == "f64-shifted":
        shift = np.float64(x[0])
        d = x.astype(np.float64) - shift
        s, ss = d.sum(), (d * d).sum()
    else:
        raise ValueError(form)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean_s = s / n
        var = (ss - n * mean_s * mean_s) / (n - 1.0) if n > 1 else np.float64(np.nan)
        sd = F32(np.sqrt(var if var > 0 else (0.0 if var == var else var)))
    mean = F32(shift + mean_s)
    three = F32(F32(3) * sd)
    return F32(mean - three), F32(mean + three)


# =========================================================================================== views shared by 2. and 3.

def token_geometry(x, seq_pos, n_lengths):
    """ops.token_view restated for a NumPy array: dict of batch, tokens, feat_outer, feat_inner and the element strides."""
    seq_pos %= x.ndim
    others = [d for d in range(x.ndim) if d != seq_pos]
    st = [s // x.itemsize for s in x.strides]
    if len(others) == 3:
        outer, inner, s_outer, s_inner = x.shape[others[1]], x.shape[others[2]], st[others[1]], st[others[2]]
    else:
        outer, inner, s_outer, s_inner = 1, x.shape[others[1]], 0, st[others[1]]
    return dict(batch=min(x.shape[0], n_lengths), tokens=x.shape[seq_pos], feat_outer=outer, feat_inner=inner,
                stride_batch=st[0], stride_token=st[seq_pos], stride_outer=s_outer, stride_inner=s_inner)


def vector_path(g):
    """make_source's `vec` for a 16-byte aligned base."""
    return (g["stride_inner"] == 1 and g["feat_inner"] % 4 == 0 and g["stride_batch"] % 4 == 0 and g["stride_token"] % 4 == 0
            and (g["feat_outer"] == 1 or g["stride_outer"] % 4 == 0))


def pieces_path(g):
    """The predicate of mse_grid_all_kernel's dealing by pieces."""
    return vector_path(g) and g["feat_outer"] == 1 and g["feat_inner"] % PIECE == 0 and g["batch"] <= GRID_ALL_MAX_BATCH


def _activations(rng, shape, scale=1.0):
    x = rng.standard_normal(shape).astype(F32) * F32(scale)
    x[..., 3 % shape[-1]] *= F32(7)                   # an outlier feature: clipping pays, the best candidate is inside the grid
    return x


class Site:
    """One observed tensor: `mem` is the dense array in memory, `view(a)` the observed view of it (basic slicing only: the same
    call serves a NumPy array and a torch tensor), lengths / seq_pos as the observer gets them (None / -1: a flat tensor),
    `offset` floats between a 16-byte boundary and the base of a flat tensor."""

    def __init__(self, mem, lengths=None, seq_pos=-1, view=None, offset=0):
        self.mem, self.seq_pos, self.offset = np.ascontiguousarray(mem, dtype=F32), seq_pos, offset
        self.lengths = None if lengths is None else np.asarray(lengths, dtype=np.int64)
        self.view = view or (lambda a: a)

    def observed(self):
        """The [valid tokens, features] (or flat) array the reference observes (observer.py:72-84)."""
        x = self.view(self.mem)
        return x.reshape(-1) if self.lengths is None else OB.remove_padding(x, self.lengths, self.seq_pos)

    def geometry(self):
        return None if self.lengths is None else token_geometry(self.view(self.mem), self.seq_pos, self.lengths.size)

    def mapped(self, fn):
        return Site(fn(self.mem), self.lengths, self.seq_pos, self.view, self.offset)


# =========================================================================================== 2. quantile

QUANTILE_FLAT_NS = (1, 7, 1024, 262147, 1100003)
QUANTILE_THRESHOLDS = (0.99999, 0.9, 1.0)
QUANTILE_CASES = tuple(f"flat{n}{s}" for n in QUANTILE_FLAT_NS for s in ("", "_off")) + (
    "dense_4x9x256", "view_seq2", "view_seq3", "short_mask", "edges_pow2", "edges_13bit", "quarters", "all_zero")


def _edge_data(rng, n, hi):
    """Magnitudes k * f32(hi / 2048), k in 0..2048: every element on a bin edge; 0 and hi itself present.  hi has at most 13
    significant bits, so every k * hi / 2048 is exact in fp32 and the edges are the same numbers however they are computed.
    (With more bits they are not: torch.histc takes its edges from torch.linspace, whose CPU kernel forms them vector by
    vector -- for hi = 3.7, 210 of the 2049 edges of torch 2.10 on an AVX-512 host are one ulp away from the scalar form the
    oracle and the kernel use.  Which bin an element exactly on such an edge falls into is the build's, not the
    reference's, so no case asks.)"""
    k = rng.integers(0, HIST_BINS + 1, n)
    k[:4] = (0, HIST_BINS, 1, HIST_BINS - 1)
    sign = np.where(rng.random(n) < 0.5, F32(-1), F32(1))
    return (k.astype(F32) * F32(F32(hi) / F32(HIST_BINS)) * sign).astype(F32)


@functools.lru_cache(maxsize=None)
def quantile_case(name):
    """-> (three Sites, thresholds).  The three batches differ, so the average rule has something to average."""
    rng = np.random.default_rng([7003, QUANTILE_CASES.index(name)])
    thresholds = QUANTILE_THRESHOLDS
    if name.startswith("flat"):
        n, off = int(name[4:].split("_")[0]), int(name.endswith("_off"))
        sites = [Site(rng.standard_normal(n) * (1.0 + 0.5 * it), offset=off) for it in range(3)]
    elif name == "dense_4x9x256":
        sites = [Site(_activations(rng, (4, 9, 256), 1.0 + it), (0, 9, 4, 2), 1) for it in range(3)]
    elif name == "view_seq2":            # [B, h, T, d]: feat_outer > 1 on the vector path
        sites = [Site(_activations(rng, (3, 4, 10, 32), 1.0 + it), (10, 0, 7), 2) for it in range(3)]
    elif name == "view_seq3":            # [B, h, d, T]: the inner axis is strided, scalar loads
        sites = [Site(_activations(rng, (3, 4, 33, 10), 1.0 + it), (3, 10, 0), 3) for it in range(3)]
    elif name == "short_mask":           # three lengths for a batch of five: zip() stops at the mask (observer.py:82)
        sites = [Site(_activations(rng, (5, 6, 64), 1.0 + it), (6, 0, 2), 1) for it in range(3)]
    elif name in ("edges_pow2", "edges_13bit"):
        hi = (8.0, 3.75)[name == "edges_13bit"]
        sites = [Site(_edge_data(rng, 5000, hi * (1 + it))) for it in range(3)]
    elif name == "quarters":             # mass spread over the whole range: a target bin in every wave of the finaliser
        sites = [Site(rng.uniform(-1.0, 1.0, 20000) * (1.0 + it)) for it in range(3)]
        cum = np.cumsum(quantile_hist(sites[0].observed())[0].astype(np.float64))
        thresholds = tuple(float((cum[b - 1] + cum[b]) / 2 / 20000) for b in (100, 700, 1300, 1900)) + (1.0, 1.5)
    elif name == "all_zero":
        sites = [Site(np.zeros(777)) for it in range(3)]
    else:
        raise KeyError(name)
    return sites, thresholds


def quantile_hist(x):
    """(counts, min, max, max_hist_range) with the reference's own call: torch.histc on the CPU (observer.py:262-263)."""
    x = np.ascontiguousarray(x, dtype=F32).reshape(-1)
    mn, mx = OB.aminmax(x)
    max_range = F32(max(F32(-mn), mx))
    hist = torch.histc(torch.from_numpy(np.abs(x)), bins=HIST_BINS, min=0.0, max=float(max_range)).numpy()
    return hist, mn, mx, max_range


def quantile_bin(hist, numel, threshold):
    """Index of the first bin whose fp32 running total reaches fp32(threshold * numel); HIST_BINS when none does."""
    cur, target = F32(0), F32(threshold * numel)
    for i in range(HIST_BINS):
        cur = F32(cur + hist[i])
        if cur >= target:
            return i
    return HIST_BINS


def quantile_observe(st, x, threshold):
    """AvgQuantileObserver.forward on the observed values x (observer.py:253-282): torch.histc, the oracle's clip and update."""
    hist, mn, mx, max_range = quantile_hist(x)
    clip = OB.quantile_clip_from_hist(hist, x.size, threshold, max_range, HIST_BINS)
    st._avg_update(F32(max(mn, F32(-clip))), F32(min(mx, clip)))


@functools.lru_cache(maxsize=None)
def quantile_reference(name):
    """{threshold: [(min_val, max_val) after batch 1, 2, 3]}."""
    sites, thresholds = quantile_case(name)
    out = {}
    for thr in thresholds:
        st = OB.ObserverState(bit=6, symmetric=False)
        out[thr] = []
        for s in sites:
            quantile_observe(st, s.observed(), thr)
            out[thr].append((F32(st.min_val), F32(st.max_val)))
    return out


# =========================================================================================== 3. MSE grid

LOSS_RTOL = 2.0 ** -19          # device loss against the oracle's, per candidate (derivation: grid_reference)
NEAR_MIN = 1.0 + 2.0 ** -18     # two candidates whose oracle losses are closer than this may swap places
GRID_KINDS = ("sym", "side", "asym")         # 1-D symmetric (6 bit), 1-D one-sided (4 bit), 2-D asymmetric (4 bit, 1600 candidates)
GRID_CASES = ("flat1", "flat5", "flat4099", "flat4099_off", "flat1100003", "dense_3x5x256", "dense_4x8x768", "dense_2x40x512",
              "slice_3x5x320", "batch1025", "dense_3x5x260", "view_seq2", "view_seq3", "short_mask", "tiny_values")
GRID_1D_ONLY = ("flat1100003", "batch1025")  # more than ~32k observed elements: no 1600-candidate search
GRID_PIECES = ("dense_3x5x256", "dense_4x8x768", "dense_2x40x512", "slice_3x5x320", "short_mask", "tiny_values")
GRID_SECOND_TRIP = ("dense_4x8x768", "dense_2x40x512")          # more pieces than the grid has waves
GRID_2D_MAX_ELEMS = 32768
GRID_UNITS = tuple((c, k) for c in GRID_CASES for k in GRID_KINDS if not (k == "asym" and c in GRID_1D_ONLY))
ROW_SHAPES = ((9, 1), (5, 63), (4, 65), (3, 300))


def grid_scheme(kind):
    """-> (bit, symmetric)."""
    return (6, True) if kind == "sym" else (4, False)


@functools.lru_cache(maxsize=None)
def grid_case(name):
    """Two Sites (two-sided data)."""
    rng = np.random.default_rng([7004, GRID_CASES.index(name)])
    two = lambda make: [make(1.0), make(1.3)]        # noqa: E731
    if name.startswith("flat"):
        n, off = int(name[4:].split("_")[0]), int(name.endswith("_off"))
        return two(lambda s: Site(_activations(rng, (n,), s) if n > 8 else rng.standard_normal(n) * s, offset=off))
    if name == "dense_3x5x256":
        return two(lambda s: Site(_activations(rng, (3, 5, 256), s), (5, 2, 4), 1))
    if name == "dense_4x8x768":          # a sample of length 0 first: equal neighbouring prefix sums
        return two(lambda s: Site(_activations(rng, (4, 8, 768), s), (0, 8, 3, 1), 1))
    if name == "dense_2x40x512":
        return two(lambda s: Site(_activations(rng, (2, 40, 512), s), (40, 17), 1))
    if name == "slice_3x5x320":          # token stride 320, 256 features observed
        return two(lambda s: Site(_activations(rng, (3, 5, 320), s), (5, 0, 3), 1, view=lambda a: a[:, :, :256]))
    if name == "batch1025":              # more samples than the LDS prefix table holds: one token per wave
        L = (rng.random(1025) < 0.7).astype(np.int64)
        L[:3] = (1, 0, 1)
        return two(lambda s: Site(_activations(rng, (1025, 1, 256), s), L, 1))
    if name == "dense_3x5x260":          # rows that are no whole pieces
        return two(lambda s: Site(_activations(rng, (3, 5, 260), s), (0, 5, 2), 1))
    if name == "view_seq2":
        return two(lambda s: Site(_activations(rng, (3, 4, 10, 32), s), (10, 0, 7), 2))
    if name == "view_seq3":
        return two(lambda s: Site(_activations(rng, (3, 4, 33, 10), s), (3, 10, 0), 3))
    if name == "short_mask":
        return two(lambda s: Site(_activations(rng, (5, 6, 256), s), (6, 0, 2), 1))
    if name == "tiny_values":            # a few magnitudes below the reciprocal route's guard, in some pieces only

        def make(s):
            x = _activations(rng, (3, 5, 256), s)
            x[0, 1, [0, 17, 200]] = F32(1e-30)
            x[2, 0, 64] = F32(-1e-30)
            return Site(x, (5, 5, 5), 1)
        return two(make)
    raise KeyError(name)


def grid_sites(name, kind):
    """The case's two batches as the kind observes them: one-sided searches get |x| (even cases) or -|x| (odd cases)."""
    sites = grid_case(name)
    if kind != "side":
        return sites, "no"
    neg = GRID_CASES.index(name) % 2 == 1
    return [s.mapped(lambda a: -np.abs(a) if neg else np.abs(a)) for s in sites], ("neg" if neg else "pos")


def grid_candidates(x_min, x_max, quant_min, quant_max, symmetric, side, num=100, channel=False):
    """(lo[k], hi[k]) of perform_1D_search / perform_2D_search (observer.py:314-361) in candidate order, fp32 throughout --
    the loops of oracle.mse_grid_search as arrays (pinned to it in tests/test_oracle_extra_observers.py).  channel: the
    per-channel 2-D search widens the extrema to include zero first (observer.py:319-320)."""
    x_min, x_max = F32(x_min), F32(x_max)
    i = np.arange(1, num + 1).astype(F32)
    if side != "no" or symmetric:
        thres = (F32(F32(max(abs(x_min), x_max)) / F32(num)) * i).astype(F32)
        zero = np.zeros(num, dtype=F32)
        return (zero if side == "pos" else -thres), (zero if side == "neg" else thres)
    if channel:
        x_min, x_max = F32(OB.zminimum(x_min, F32(0))), F32(OB.zmaximum(x_max, F32(0)))
    tmp_max = (F32(F32(x_max - x_min) / F32(num)) * i).astype(F32)[:, None]
    delta = (tmp_max / F32(float(quant_max - quant_min))).astype(F32)
    zd = (np.arange(quant_min, quant_max + 1).astype(F32)[None, :] * delta).astype(F32)
    lo = np.maximum((F32(0) - zd).astype(F32), x_min)
    hi = np.minimum((tmp_max - zd).astype(F32), x_max)
    return lo.reshape(-1).astype(F32), hi.reshape(-1).astype(F32)


def grid_search_reference(x, quant_min, quant_max, symmetric, side, channel=False):
    """Every candidate of one search against oracle.mse_grid_loss -> dict:
      lo, hi      the candidates' ranges
      loss        the oracle's loss of each: fp32 squared errors, float64 mean, rounded to fp32 once
      best        first strict minimum (the oracle's choice), best_range its range
      separated   every candidate of another range has a loss above loss[best] * NEAR_MIN
      near        bool per candidate: loss <= loss[best] * NEAR_MIN

    The device adds the same fp32 squared errors (all >= 0) in fp32 runs of 16 inside a float64 total: a run's relative error
    is at most 15 roundings of 2^-24, the final rounding of the mean to fp32 adds one more on either side: 16 * 2^-24 =
    2^-20; LOSS_RTOL doubles it.  Sums of non-negative terms: a loss of 0 has only zero terms, so it must come out as 0."""
    x = np.ascontiguousarray(x, dtype=F32).reshape(-1)
    x_min, x_max = OB.aminmax(x)
    lo, hi = grid_candidates(x_min, x_max, quant_min, quant_max, symmetric, side, channel=channel)
    memo, loss = {}, np.empty(lo.size, dtype=F32)
    for k in range(lo.size):
        key = (lo[k].tobytes(), hi[k].tobytes())
        if key not in memo:
            memo[key] = OB.mse_grid_loss(x, lo[k], hi[k], quant_min, quant_max, symmetric)
        loss[k] = memo[key]
    best = int(np.argmin(loss))                     # first occurrence of the minimum == first strict minimum below 1e10
    assert loss[best] < 1e10
    near = loss.astype(np.float64) <= np.float64(loss[best]) * NEAR_MIN
    other = (OB_bits(lo) != OB_bits(lo[best])) | (OB_bits(hi) != OB_bits(hi[best]))
    return dict(lo=lo, hi=hi, loss=loss, best=best, best_range=(lo[best], hi[best]), near=near, x_min=x_min, x_max=x_max,
                separated=not bool((near & other).any()))


def OB_bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=F32)).view(np.uint32)


@functools.lru_cache(maxsize=None)
def grid_reference(name, kind):
    """[reference of batch 1, of batch 2] for one unit of GRID_UNITS; computed once, read by every test."""
    bit, symmetric = grid_scheme(kind)
    quant_min, quant_max = OB.quant_range(bit, symmetric)
    sites, side = grid_sites(name, kind)
    return [grid_search_reference(s.observed(), quant_min, quant_max, symmetric, side) for s in sites]


def update_chain(ranges, average):
    """[(min_val, max_val) after each batch] of the observer's update rule (observer.py:377-378 / 401-409) over the ranges."""
    st, out = OB.ObserverState(), []
    for lo, hi in ranges:
        (st._avg_update if average else st._running_update)(np.asarray(F32(lo)), np.asarray(F32(hi)))
        out.append((F32(st.min_val), F32(st.max_val)))
    return out


@functools.lru_cache(maxsize=None)
def rows_case(shape):
    """A weight whose rows are all positive (row 0), all negative (row 1) and mixed (the rest)."""
    rng = np.random.default_rng([7005, *shape])
    w = (rng.standard_normal(shape) * 0.05).astype(F32)
    w[0] = np.abs(w[0]) + F32(1e-3)
    w[1] = -np.abs(w[1]) - F32(1e-3)
    return w


@functools.lru_cache(maxsize=None)
def rows_reference(shape, kind):
    """Per-row references of mse_grid_rows.  kind "side" observes |w| (every row positive)."""
    bit, symmetric = grid_scheme(kind)
    quant_min, quant_max = OB.quant_range(bit, symmetric)
    w = np.abs(rows_case(shape)) if kind == "side" else rows_case(shape)
    side = "pos" if kind == "side" else "no"
    return w, side, [grid_search_reference(r, quant_min, quant_max, symmetric, side, channel=True) for r in w]

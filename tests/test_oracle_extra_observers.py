"""What tests/_extra_observers.py promises, shown with the references alone (CPU only): the helpers agree with torch.std,
torch.histc and oracle/observer_oracle.py; every case reaches the launch shape it is named for and stays inside the caps
(element counts, lengths, finite data, separated minima); and the moment bound is sharp -- a NumPy emulation of the fp32-product
arithmetic that moments_flat_kernel used to run misses it wherever |mean| >= 1, the float64 form passes everywhere."""
import warnings

import numpy as np
import pytest
import torch

import _extra_observers as EO
from oracle import observer_oracle as OB

F32 = np.float32


# ----------------------------------------------------------------------------------- 1. moments

def test_moment_reference_is_torch_std_in_double():
    for n in (2, 5, 1027, 20483):
        for k, (mean, std) in enumerate(EO.MOMENT_PAIRS):
            x = EO.moment_data(n, mean, std, k)
            t = torch.from_numpy(x).double()
            want = EO.moment_range(t.mean().item(), t.std().item())
            got = EO.moment_reference(x)
            assert got[0] == want[0][()] and got[1] == want[1][()] and got[2] == want[2][()], (n, mean, std)
    mn, mx, bound = EO.moment_reference(EO.moment_data(1, 1.0, 0.02))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                 # torch warns about the one-element std it returns NaN for
        assert np.isnan(mn) and np.isnan(mx) and torch.isnan(torch.ones(1).std())
    for c in EO.MOMENT_CONSTANTS:
        mn, mx, _ = EO.moment_reference(np.full(1027, c, dtype=F32))
        assert mn == F32(c) and mx == F32(c)


def test_moment_reference_is_the_oracle_lsqplus():
    for shape, axis in EO.MOMENT_CHANNEL_CASES:
        x = EO.moment_channel_data(shape, axis)
        st = OB.ObserverState(bit=4, symmetric=True, ch_axis=axis)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")             # NumPy warns about the one-element std it returns NaN for
            OB.observe_lsqplus(st, x)
        mn, mx, bound = EO.moment_reference(x, axis)
        assert mn.shape == (shape[axis],) and EO.moment_within(st.min_val, mn, bound) and EO.moment_within(st.max_val, mx, bound), shape
        assert np.isnan(mn).all() == (shape == (4, 1)) and (bound[~np.isnan(mn)] > 0).all()
    x = EO.moment_data(4096, 10.0, 0.1)
    st = OB.ObserverState(bit=8, symmetric=True)
    OB.observe_lsqplus(st, x)
    mn, mx, _ = EO.moment_reference(x)
    assert F32(st.min_val) == mn and F32(st.max_val) == mx


def test_moment_cases_reach_the_launch_shapes():
    ns = EO.MOMENT_NS
    assert {n % 4 for n in ns} == {0, 1, 2, 3} and min(ns) == 1                # every tail length
    assert max(n for n in ns) // 4 + 1 > 4 * EO.THREADS                        # more than one workgroup
    assert (EO.MOMENT_BIG_N // 4 + 1 + 1023) // 1024 > EO.MOMENT_MAX_BLOCKS and EO.MOMENT_BIG_N % 4 == 3
    seq = EO.moment_thread_sequences(np.arange(1, 20484, dtype=F32))
    assert seq.shape[0] % EO.THREADS == 0 and np.sort(seq[seq != 0]).tolist() == list(range(1, 20484))
    assert seq[:3, -1].tolist() == [20481.0, 20482.0, 20483.0]                # the tail: threads 0..2, after their float4s
    seq = EO.moment_thread_sequences(np.arange(1, 1028, dtype=F32), misaligned=True)
    assert seq[:, 0].tolist()[:3] == [1.0, 2.0, 3.0] and seq.shape == (256, 5) and seq[3, 4] == 0


def test_moment_bound_rejects_fp32_products_and_accepts_float64():
    """The bound is sharp.  The fp32-product arithmetic, emulated thread by thread as the launch deals the elements, misses it
    for every (mean, std) with |mean| >= 1 at some of the GPU test's sizes -- so that pair's GPU test fails on it -- and at
    n = 4096 by factors of 7 to 250 for (1, 0.001) and (+-100, 0.01).  (At n = 4096 a thread adds only 8 elements, and the
    two mildest pairs, (1, 0.02) and (10, 0.1), land at 3 to 5 and 2 to 3 ulp there: either side of the 4 ulp bound; they
    miss it at smaller and at misaligned sizes.)  The float64 form stays inside at every per-tensor case of the GPU test."""
    for k, (mean, std) in enumerate(EO.MOMENT_PAIRS):
        ratios = {}
        for n in EO.MOMENT_NS[1:]:
            for mis in (False, True):
                x = EO.moment_data(n, mean, std, k)
                mn, mx, bound = EO.moment_reference(x)
                old = EO.moment_emulation(x, "fp32-products", mis)
                ratios[(n, mis)] = max(abs(float(old[0]) - float(mn)), abs(float(old[1]) - float(mx))) / bound
                assert (ratios[(n, mis)] <= 1.0) == (EO.moment_within(old[0], mn, bound) and EO.moment_within(old[1], mx, bound))
        print((mean, std), "fp32-product error / bound:", {k_: round(v, 2) for k_, v in ratios.items()})
        if mean == 0:
            assert max(ratios.values()) <= 1.0
        else:
            assert max(ratios.values()) > 3.0, (mean, std)
            if (abs(mean), std) in ((1.0, 0.001), (100.0, 0.01)):
                assert min(ratios[(4096, False)], ratios[(4096, True)]) > 5.0, (mean, std)
    worst = 0.0
    for n in EO.MOMENT_NS + (EO.MOMENT_BIG_N,):
        for k, (mean, std) in enumerate(EO.MOMENT_PAIRS):
            x = EO.moment_data(n, mean, std, k)
            mn, mx, bound = EO.moment_reference(x)
            new = EO.moment_emulation(x, "f64-shifted")
            assert EO.moment_within(new[0], mn, bound) and EO.moment_within(new[1], mx, bound), (n, mean, std, new, mn, mx, bound)
            if n > 1:
                worst = max(worst, abs(float(new[0]) - float(mn)) / bound, abs(float(new[1]) - float(mx)) / bound)
    assert worst <= 0.25            # within one ulp: the bound leaves the float64 form a margin of four
    for c in EO.MOMENT_CONSTANTS:
        for n in EO.MOMENT_CONSTANT_NS:
            assert EO.moment_emulation(np.full(n, c, dtype=F32), "f64-shifted") == (F32(c), F32(c))


# ----------------------------------------------------------------------------------- 2. quantile

def test_quantile_helpers_are_the_oracle():
    """torch.histc (the reference's call) counts what the oracle's restatement counts, edges included; quantile_observe is
    oracle.observe_avg_quantile with that histogram."""
    for name in ("edges_pow2", "edges_13bit", "dense_4x9x256", "view_seq3", "flat7", "flat1", "all_zero"):
        sites, thresholds = EO.quantile_case(name)
        for thr in thresholds:
            st = OB.ObserverState(bit=6, symmetric=False)
            for it, s in enumerate(sites):
                x = s.observed()
                hist, mn, mx, max_range = EO.quantile_hist(x)
                if max_range > 0:
                    assert np.array_equal(hist, OB.torch_histc(np.abs(x), EO.HIST_BINS, 0.0, max_range)), (name, it)
                assert hist.sum() == x.size
                OB.observe_avg_quantile(st, s.view(s.mem), s.lengths, s.seq_pos, threshold=thr)
                want = EO.quantile_reference(name)[thr][it]
                assert OB_same(st.min_val, want[0]) and OB_same(st.max_val, want[1]), (name, thr, it)


def OB_same(a, b):
    return np.array_equal(EO.OB_bits(a), EO.OB_bits(b))


def test_quantile_cases_reach_the_launch_shapes():
    assert (1100003 // 4 + 1 + 1023) // 1024 > EO.HIST_MAX_BLOCKS > (262147 // 4 + 1 + 1023) // 1024 > 1
    for name in EO.QUANTILE_CASES:
        sites, thresholds = EO.quantile_case(name)
        assert len(sites) == 3
        for s in sites:
            x = s.observed()
            assert 0 < x.size < 2 ** 24 and np.isfinite(s.mem).all(), name
            if s.lengths is not None:
                g = s.geometry()
                assert (s.lengths >= 0).all() and (s.lengths <= g["tokens"]).all() and s.lengths[:g["batch"]].sum() > 0, name
    g = {n: EO.quantile_case(n)[0][0].geometry() for n in ("dense_4x9x256", "view_seq2", "view_seq3", "short_mask")}
    L = EO.quantile_case("dense_4x9x256")[0][0].lengths
    assert 0 in L and 9 in L and EO.vector_path(g["dense_4x9x256"])
    assert EO.vector_path(g["view_seq2"]) and g["view_seq2"]["feat_outer"] == 4
    assert not EO.vector_path(g["view_seq3"]) and g["view_seq3"]["stride_inner"] == 10 and g["view_seq3"]["stride_token"] == 1
    assert g["short_mask"]["batch"] == 3 < EO.quantile_case("short_mask")[0][0].mem.shape[0]
    # elements on edges: k * step, with 0 and hi itself; with hi a power of two every edge of torch.linspace is such a value
    for name in ("edges_pow2", "edges_13bit"):
        x = np.abs(EO.quantile_case(name)[0][0].observed())
        hi = x.max()
        k = x / F32(hi / F32(2048))
        assert np.array_equal(k, np.rint(k)) and 0.0 in x and k.max() == 2048 and np.unique(k).size > 1500
    x = np.abs(EO.quantile_case("edges_pow2")[0][0].observed())
    edges = np.array([OB.linspace_edge(i, 0.0, x.max(), 2049) for i in range(2049)], dtype=F32)
    assert np.isin(x, edges).all()
    hist = EO.quantile_hist(x)[0]
    assert hist[2047] == (x >= edges[2047]).sum() and hist[0] == (x < edges[1]).sum()          # the last bin is closed


def test_quantile_thresholds_land_in_every_wave_of_the_finaliser():
    sites, thresholds = EO.quantile_case("quarters")
    x = sites[0].observed()
    hist = EO.quantile_hist(x)[0]
    bins = [EO.quantile_bin(hist, x.size, t) for t in thresholds]
    assert [b // 512 for b in bins[:4]] == [0, 1, 2, 3] and bins[:4] == [100, 700, 1300, 1900]
    assert bins[4] == 2047 and bins[5] == EO.HIST_BINS            # threshold 1.0: the last bin; 1.5: no bin reaches it
    for s in sites[1:]:                                           # later batches: still one target per wave
        h = EO.quantile_hist(s.observed())[0]
        assert [EO.quantile_bin(h, s.observed().size, t) // 512 for t in thresholds[:4]] == [0, 1, 2, 3]
    # the all-zero tensor: the device counts nothing (hi == 0), no bin reaches the target, the clip is the range: 0
    assert EO.quantile_reference("all_zero")[0.9][2] == (F32(0), F32(0))


# ----------------------------------------------------------------------------------- 3. MSE grid

@pytest.mark.parametrize("name,kind", [("flat5", "sym"), ("flat5", "side"), ("flat5", "asym"), ("flat4099", "side"), ("view_seq3", "asym"),
                                       ("short_mask", "sym"), ("dense_3x5x260", "side")])
def test_grid_reference_is_the_oracle_search(name, kind):
    """Candidates in arrays + first minimum + update_chain == oracle.observe_mse, running and average."""
    bit, symmetric = EO.grid_scheme(kind)
    sites, side = EO.grid_sites(name, kind)
    refs = EO.grid_reference(name, kind)
    for average in (False, True):
        st = OB.ObserverState(bit=bit, symmetric=symmetric)
        st.one_side_dist = side
        chain = EO.update_chain([r["best_range"] for r in refs], average)
        for s, want in zip(sites, chain):
            OB.observe_mse(st, s.view(s.mem), s.lengths, s.seq_pos, average=average)
            assert OB_same(st.min_val, want[0]) and OB_same(st.max_val, want[1]), (name, kind, average)
    if side != "no":
        assert OB.one_side_dist(sites[0].observed()) == side


@pytest.mark.parametrize("shape", EO.ROW_SHAPES)
def test_rows_reference_is_the_oracle_search(shape):
    for kind in EO.GRID_KINDS:
        bit, symmetric = EO.grid_scheme(kind)
        w, side, refs = EO.rows_reference(shape, kind)
        st = OB.ObserverState(bit=bit, symmetric=symmetric, ch_axis=0)
        st.one_side_dist = side
        OB.observe_mse(st, w)
        assert OB_same(st.min_val, [r["best_range"][0] for r in refs]) and OB_same(st.max_val, [r["best_range"][1] for r in refs]), kind
    w = EO.rows_case(shape)
    assert (w[0] > 0).all() and (w[1] < 0).all() and all((r > 0).any() and (r < 0).any() for r in w[2:] if r.size > 1)


def test_grid_cases_reach_the_launch_shapes():
    for name in EO.GRID_CASES:
        for s in EO.grid_case(name):
            g = s.geometry()
            n = s.observed().size
            assert 0 < n < 2 ** 24 and np.isfinite(s.mem).all()
            assert n <= EO.GRID_2D_MAX_ELEMS or name in EO.GRID_1D_ONLY, (name, n)
            if g is None:
                continue
            assert (s.lengths >= 0).all() and (s.lengths <= g["tokens"]).all() and s.lengths[:g["batch"]].sum() > 0, name
            assert EO.pieces_path(g) == (name in EO.GRID_PIECES), name
            if EO.pieces_path(g):
                units = int(s.lengths[:g["batch"]].sum()) * g["feat_inner"] // EO.PIECE
                blocks = min(EO.GRID_ALL_MAX_BLOCKS, -(-g["batch"] * g["tokens"] // EO.GRID_ALL_WAVES))
                assert (units > blocks * EO.GRID_ALL_WAVES) == (name in EO.GRID_SECOND_TRIP), (name, units, blocks)
    geo = {n: EO.grid_case(n)[0].geometry() for n in EO.GRID_CASES}
    assert 0 in EO.grid_case("dense_4x8x768")[0].lengths[:1] and geo["dense_4x8x768"]["feat_inner"] // EO.PIECE == 3
    assert geo["slice_3x5x320"]["stride_token"] == 320 and geo["slice_3x5x320"]["feat_inner"] == 256
    assert geo["batch1025"]["batch"] > EO.GRID_ALL_MAX_BATCH and EO.vector_path(geo["batch1025"]) and 0 in EO.grid_case("batch1025")[0].lengths
    assert geo["dense_3x5x260"]["feat_inner"] % EO.PIECE and EO.vector_path(geo["dense_3x5x260"])
    assert geo["view_seq2"]["feat_outer"] > 1 and EO.vector_path(geo["view_seq2"])
    assert geo["view_seq3"]["stride_inner"] > 1 and not EO.vector_path(geo["view_seq3"])
    assert geo["short_mask"]["batch"] < EO.grid_case("short_mask")[0].mem.shape[0]
    assert (1100003 + 4 * 1024 - 1) // (4 * 1024) > EO.GRID_ALL_MAX_BLOCKS            # the flat form's second trip
    # tiny magnitudes: some pieces (waves) hold one, most do not; the float4 slot of a tiny element is shared by 64 lanes
    for s in EO.grid_case("tiny_values"):
        x = np.abs(s.mem).reshape(-1, EO.PIECE)
        tiny = ((x < EO.FAST_DIVIDEND_MIN) & (x > 0)).any(axis=1)
        assert 0 < tiny.sum() < len(tiny) and ((x >= EO.FAST_DIVIDEND_MIN) | (x == 0))[~tiny].all()


def test_grid_minima_are_separated():
    """The seeds: at most 1 unit in 8 has a second range within NEAR_MIN of the oracle's minimum (units whose device result
    is held to the near-minimum set only); the candidate count is what the scratch of the launch-per-32 form holds."""
    units = [(name, kind, it) for name, kind in EO.GRID_UNITS for it in range(2)]
    loose = [(name, kind, it) for name, kind, it in units if not EO.grid_reference(name, kind)[it]["separated"]]
    print("units", len(units), "not separated", loose)
    assert len(loose) * 8 <= len(units)
    for name, kind in EO.GRID_UNITS:
        for r in EO.grid_reference(name, kind):
            assert r["loss"].size == (1600 if kind == "asym" else 100) and np.isfinite(r["loss"]).all() and r["near"][r["best"]]
    rows = [r for shape in EO.ROW_SHAPES for kind in EO.GRID_KINDS for r in EO.rows_reference(shape, kind)[2]]
    loose_rows = sum(not r["separated"] for r in rows)
    print("rows", len(rows), "not separated", loose_rows)
    assert loose_rows * 8 <= len(rows)

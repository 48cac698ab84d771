"""The table recipes of tests/_multi_tables.py have the properties tests/test_gpu_multi_tables.py relies on: without them
the GPU file would pass while never reaching the global-memory bisection, a second grid-stride trip, a row longer than
one unrolled trip, an empty entry, or a special at the edge of a row.  CPU only."""
import numpy as np
import pytest

import _multi_tables as MT


def test_weight_tables_straddle_the_lds_limit_and_the_grid():
    lengths = [len(MT.weight_table(f"n{n}")["entries"]) for n in MT.WEIGHT_LENGTHS]
    assert lengths == [1, 2, 77, 1024, 1025, 1300]
    assert MT.LDS_WEIGHTS in lengths and MT.LDS_WEIGHTS + 1 in lengths and max(lengths) > MT.LDS_WEIGHTS + 1
    assert MT.WEIGHT_GRID_WAVES == 32768
    t = MT.weight_table("second_trip")
    assert t["total_rows"] == MT.WEIGHT_GRID_WAVES + 5 and all(e["inner"] == 4 for e in t["entries"])
    last = t["entries"][-1]
    assert last["rows"] > 5 and last["channels"] == last["rows"]          # the second trip's rows have parameters of their own
    for name in MT.WEIGHT_TABLES:
        t = MT.weight_table(name)
        assert np.array_equal(t["row_end"], np.cumsum([e["rows"] for e in t["entries"]]))
        assert t["total_rows"] <= MT.WEIGHT_GRID_WAVES or name == "second_trip"


@pytest.mark.parametrize("name", ["n77", "n1024", "n1025", "n1300"])
def test_weight_tables_mix_every_listed_shape(name):
    es = MT.weight_table(name)["entries"]
    assert {e["inner"] for e in es} == set(MT.WEIGHT_INNERS)
    # one float4 either side of the unrolled trip, and two trips
    assert {MT.WEIGHT_TRIP - 4, MT.WEIGHT_TRIP, MT.WEIGHT_TRIP + 4, 2 * MT.WEIGHT_TRIP + 4} <= {e["inner"] for e in es}
    assert {1, 2, 3, 64} <= {e["rows"] for e in es}
    assert {"per_row", "per_tensor", "wrap"} == {e["layout"] for e in es}
    for e in es:
        want = {"per_row": e["rows"], "per_tensor": 1, "wrap": e["rows"] // 3}[e["layout"]]
        assert e["channels"] == want and e["rows"] % e["channels"] == 0 and e["inner"] % 4 == 0
    assert any(e["layout"] == "wrap" and e["rows"] == 3 * e["channels"] and e["channels"] > 1 for e in es)
    # channels == 1 next to per-channel entries
    assert any(a["channels"] == 1 and b["channels"] > 1 for a, b in zip(es, es[1:]))
    assert {e["zp_type"] for e in es} == {MT.ZP_INT32, MT.ZP_FLOAT32}
    assert {e["mode"] for e in es} == {MT.FIXED, MT.LSQ, MT.LSQPLUS}
    assert all(e["grad_factor"] != 1.0 for e in es if e["mode"] != MT.FIXED)
    assert any(e["mode"] == MT.LSQPLUS and np.any(e["zp"] != np.rint(e["zp"])) for e in es)
    assert {e["bit"] for e in es} == {2, 4, 6, 8} and {e["symmetric"] for e in es} == {True, False}
    assert all(e["quant_max"] - e["quant_min"] == (1 << e["bit"]) - 1 for e in es)
    # rows of more than one trip at the ends of the table and on both sides of the LDS limit
    for i in {0, len(es) - 1, MT.LDS_WEIGHTS - 1, MT.LDS_WEIGHTS}:
        if i < len(es):
            assert es[i]["inner"] > MT.WEIGHT_TRIP and es[i]["rows"] > 3, i


def test_weight_tables_have_empty_and_one_row_entries():
    rows = [e["rows"] for e in MT.weight_table("zero_rows")["entries"]]
    assert rows[0] == 0 and rows[-1] == 0 and 0 in rows[2:-2] and 1 in rows
    assert any(a == 0 and b == 0 for a, b in zip(rows[1:], rows[2:-1]))           # two in a row in the middle
    assert MT.weight_table("all_zero_rows")["total_rows"] == 0
    for name in ("n77", "n1300"):
        assert 1 in [e["rows"] for e in MT.weight_table(name)["entries"]]


@pytest.mark.parametrize("name", [n for n in MT.WEIGHT_TABLES if n != "all_zero_rows"])
def test_weight_tables_plant_specials_at_the_edges(name):
    t = MT.weight_table(name)
    seen = set()
    for e in t["entries"]:
        if e["rows"] == 0:
            continue
        x = MT.weight_entry_x(t, e)
        for pos, (r, j) in enumerate(((0, 0), (0, -1), (-1, 0), (-1, -1))):
            kind = MT.classify_special(x[r, j], e["scale"][(r % e["rows"]) % e["channels"]])
            assert kind is not None, (name, e["index"], pos, x[r, j])
            seen.add((pos, kind))
    if len(t["entries"]) >= 77:        # every kind of special at every one of the four places
        assert seen == {(p, k) for p in range(4) for k in MT.SPECIAL_KINDS}
    # offsets: 16-byte aligned rows, outputs separated by guard words
    offs = [(e["y_off"], e["rows"] * e["inner"]) for e in t["entries"]]
    assert all(o % 4 == 0 for o, _ in offs) and all(e["x_off"] % 4 == 0 for e in t["entries"])
    assert all(o2 - (o1 + n1) == MT.GUARD for (o1, n1), (o2, _) in zip(offs, offs[1:]))
    assert MT.weight_guard_mask(t).sum() == MT.GUARD * (len(offs) + 1)


def test_weight_reference_is_the_oracle_per_tensor():
    """The table reference against the oracle's own per-tensor / per-channel functions on whole entries."""
    from oracle import fake_quant_oracle as FQ
    t, ref = MT.weight_table("n77"), MT.weight_reference("n77")
    checked = set()
    for e in t["entries"]:
        if e["mode"] != MT.FIXED or e["layout"] == "wrap":
            continue
        x, s, z = MT.weight_entry_x(t, e), t["scale"][e["p_off"]:e["p_off"] + e["channels"]], MT.weight_entry_zp(t, e)
        if e["channels"] == 1:
            _, y = FQ.fake_quantize_per_tensor_affine(x, s[0], z[0], e["quant_min"], e["quant_max"])
        else:
            _, y = FQ.fake_quantize_per_channel_affine(x, s, z, 0, e["quant_min"], e["quant_max"])
        assert np.array_equal(MT.bits(y).reshape(-1), ref[e["y_off"]:e["y_off"] + x.size]), e["index"]
        checked.add(e["channels"] == 1)
    assert checked == {True, False}
    assert (ref[MT.weight_guard_mask(t)] == MT.SENTINEL_BITS).all()


def test_site_tables_straddle_the_lds_limit_and_the_grid():
    counts = [len(MT.site_table(f"n{n}")["sites"]) for n in MT.SITE_COUNTS]
    assert counts == [1, 2, 96, 512, 513, 700]
    assert MT.LDS_SITES in counts and MT.LDS_SITES + 1 in counts
    assert MT.TOKEN_GRID_WAVES == 65536
    t = MT.site_table("second_trip")
    assert t["total_tokens"] > MT.TOKEN_GRID_WAVES and all(MT.site_features(s)[0] == 4 for s in t["sites"])
    assert t["tok_end"][-2] < MT.TOKEN_GRID_WAVES                        # the second trip ends inside the last site ...
    valid = MT.site_valid(t, t["sites"][-1]).reshape(-1)
    assert valid[MT.TOKEN_GRID_WAVES - t["tok_end"][-2]:].any()          # ... on tokens that must be written
    for name in MT.SITE_TABLES:
        t = MT.site_table(name)
        assert np.array_equal(t["tok_end"], np.cumsum([s["B"] * s["T"] for s in t["sites"]]))


@pytest.mark.parametrize("name", ["n96", "n512", "n513", "n700"])
def test_site_tables_mix_every_listed_layout(name):
    t = MT.site_table(name)
    ss = t["sites"]
    assert {s["kind"] for s in ss} == set(MT.SITE_KINDS)
    assert {s["mem_shape"][2] for s in ss if s["kind"] == "bth"} == set(MT.BTH_FEATURES)
    assert {MT.TOKEN_TRIP - 4, MT.TOKEN_TRIP, MT.TOKEN_TRIP + 4, 2 * MT.TOKEN_TRIP + 4} <= set(MT.BTH_FEATURES)
    for kind in ("bhtd", "bhdt"):
        f4 = {s["mem_shape"][2] * s["mem_shape"][3] // 4 for s in ss if s["kind"] == kind}
        assert {191, 192, 193} <= f4, (kind, f4)
        assert all(s["mem_shape"][3] % 4 == 0 and s["vec"] == 1 for s in ss if s["kind"] == kind)
    assert {MT.site_features(s)[0] for s in ss if not s["vec"]} >= {33, 1}
    for s in ss:
        v = MT.site_view(t["x"], s)
        stride_inner = v.strides[-1 if s["kind"] != "bhdt" else 2] // 4
        assert (stride_inner == 2) == (s["kind"] == "strided")
        assert (s["x_off"] % 4 != 0) == (s["kind"] == "unaligned")
        assert s["vec"] == int(s["kind"] in ("bth", "bhtd", "bhdt"))
    assert {s["length_kind"] for s in ss} == set(MT.LENGTH_KINDS)
    assert any(a["len_off"] is not None and a["len_off"] == b["len_off"] for a, b in zip(ss, ss[1:]))   # one vector, two sites
    for s in ss:
        L = MT.site_lengths(t, s)
        if s["length_kind"] == "zero":
            assert (L == 0).all()
        if s["length_kind"] == "full":
            assert (L >= s["T"]).all()
    assert any(s["length_kind"] == "ragged" and (MT.site_lengths(t, s) == 0).any() and MT.site_valid(t, s).any() for s in ss)
    assert {s["T"] % 4 for s in ss} == {0, 1, 3}
    planted = set().union(*(s["planted"] for s in ss))
    assert planted == {"nan_valid", "inf_valid", "zero_extremum", "special_padded"}
    for i in {0, len(ss) - 1, MT.LDS_SITES - 1, MT.LDS_SITES}:
        if i < len(ss):
            assert MT.site_features(ss[i])[0] > MT.TOKEN_TRIP and MT.site_valid(t, ss[i]).any(), i
    # outputs of consecutive sites lie 1-3 floats apart
    gaps = [b["out_off"] - (a["out_off"] + a["B"] * a["T"]) for a, b in zip(ss, ss[1:])]
    assert set(gaps) == {1, 2, 3} and ss[0]["out_off"] >= 1 and t["out_len"] > ss[-1]["out_off"] + ss[-1]["B"] * ss[-1]["T"]


@pytest.mark.parametrize("name", ["n96", "n700"])
def test_site_reference_poisons_one_token_and_ignores_padding(name):
    t = MT.site_table(name)
    mn, mx, written = MT.site_reference(name)
    assert (MT.bits(mn[~written]) == MT.SENTINEL_BITS).all() and (MT.bits(mx[~written]) == MT.SENTINEL_BITS).all()
    n_nan = n_inf = n_edge = 0
    for s in t["sites"]:
        sl = slice(s["out_off"], s["out_off"] + s["B"] * s["T"])
        valid = MT.site_valid(t, s).reshape(-1)
        tok = np.moveaxis(MT.site_view(t["x"], s), s["seq_pos"], 1).reshape(s["B"] * s["T"], -1)
        has_nan = np.isnan(tok).any(axis=1)
        assert np.array_equal(np.isnan(mn[sl]), has_nan & valid) and np.array_equal(np.isnan(mx[sl]), has_nan & valid)
        n_nan += int((has_nan & valid).sum())
        n_inf += int((np.isinf(mx[sl]) & valid).sum())
        ok = valid & ~has_nan
        if tok.shape[1] > 1:           # extrema at the first / last feature: no element may be skipped
            n_edge += int(((tok.argmax(axis=1) == tok.shape[1] - 1) & ok).sum()) + int(((tok.argmin(axis=1) == tok.shape[1] - 1) & ok).sum())
    assert n_nan >= 5 and n_inf >= 5 and n_edge >= 20


def test_final_tables():
    assert [q * b for q, b in MT.FINAL_SHAPES] == [1, 3, 3, 9, 40, 120]
    for n_q, n_b, wide in [(q, b, w) for q, b in MT.FINAL_SHAPES for w in (False, True)]:
        t = MT.final_table(n_q, n_b, wide)
        S = t["B"] * t["T"]
        assert (S >= MT.FINAL_WIDE_MIN) == wide and S % 4 == 0 and t["T"] >= 4
        assert t["stride"] > S and t["stride"] % 4 == 0 and t["tmin"].shape == (n_q, n_b, t["stride"])
        assert np.isnan(t["tmin"][..., S:]).all() and np.isinf(t["tmax"][..., S:]).all()
        assert np.isfinite(t["tmin"][..., :S]).all() and np.isfinite(t["tmax"][..., :S]).all()
        assert t["lengths"][-1, -1].sum() == 1
        if n_q * n_b > 1:
            assert t["lengths"][0, 0].sum() == 0
        if n_q > 1:
            assert not np.array_equal(t["lengths"][0], t["lengths"][1]) and set(t["flags"]) == {0, 1}
        for p in MT.FINAL_PERCENTILES:
            ref = MT.final_reference(n_q, n_b, p, wide).view(np.float32)
            empty = t["lengths"].sum(axis=2).T == 0
            assert (MT.bits(ref[empty]) == MT.SENTINEL_BITS).all() and np.isfinite(ref[~empty]).all()
            assert (ref[~empty][:, 0] <= ref[~empty][:, 1]).all()
    a, b = MT.final_reference(40, 3, 0.5), MT.final_reference(40, 3, 1.0)
    assert not np.array_equal(a, b)                                      # the percentile matters

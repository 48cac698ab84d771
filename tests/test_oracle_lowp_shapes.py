"""The tables, predictors and cases of tests/_lowp_shapes.py on the CPU: the host emulation of the in-dtype chain against plain
torch arithmetic on ALL 65536 input words (forward, and autograd for dx), the factorisation of the backward that the tables
rest on, the launchers' predictors reaching every loop form with the size tables as they stand, and the sentinels."""
import numpy as np
import pytest
import torch

import _lowp_chain as L
import _lowp_shapes as S

DP = [(dn, p) for dn in S.DTYPES for p in S.EVERY_WORD_PARAMS]
DP_IDS = [f"{dn}-{S.param_id(p)}" for dn, p in DP]


def _torch_chain(x_words, g_words, dt, s, zp, qmin, qmax):
    """README "Defaults": the reference's per-tensor call with Python-number parameters, in x's dtype, under autograd."""
    x = L.from_words(x_words, dt).requires_grad_(True)
    a = x / s
    xi = (a.round() - a).detach() + a + zp
    y = (torch.clamp(xi, qmin, qmax) - zp) * s
    assert y.dtype == dt
    y.backward(L.from_words(g_words, dt))
    return L.tensor_words(y), L.tensor_words(x.grad)


@pytest.mark.parametrize("dn,params", DP, ids=DP_IDS)
def test_emulation_equals_torch_on_every_word(dn, params):
    dt = L.DTYPES[dn]
    bit, sym, s, zp = params
    qmin, qmax = S.qrange(bit, sym)
    g = np.random.default_rng(65536 + bit).permutation(S.ALL_WORDS)           # every g word once, against an unrelated x word
    y, dx = _torch_chain(S.ALL_WORDS, g, dt, s, zp, qmin, qmax)
    np.testing.assert_array_equal(L.canon(L.chain_forward(S.ALL_WORDS, dt, s, zp, qmin, qmax), dt), L.canon(y, dt))
    np.testing.assert_array_equal(L.canon(L.chain_backward(S.ALL_WORDS, g, dt, s, zp, qmin, qmax), dt), L.canon(dx, dt))
    # the g table's own rows: every g word against the kept x word
    t = S.chain_tables(dn, params)
    _, dxk = _torch_chain(np.full(65536, t.kept, np.uint16), S.ALL_WORDS, dt, s, zp, qmin, qmax)
    np.testing.assert_array_equal(t.g, L.canon(dxk, dt))
    np.testing.assert_array_equal(t.y, L.canon(y, dt))


@pytest.mark.parametrize("dn,params", DP, ids=DP_IDS)
def test_backward_factorises(dn, params):
    """dx(x, g) = in_range[x] ? g_table[g] : zero_word on 2^20 seeded pairs."""
    dt = L.DTYPES[dn]
    bit, sym, s, zp = params
    t = S.chain_tables(dn, params)
    rng = np.random.default_rng(20 + bit)
    x = rng.integers(0, 65536, 1 << 20).astype(np.uint16)
    g = rng.integers(0, 65536, 1 << 20).astype(np.uint16)
    assert t.in_range[x].any() and not t.in_range[x].all()
    want = L.canon(L.chain_backward(x, g, dt, s, zp, t.qmin, t.qmax), dt)
    np.testing.assert_array_equal(S.expected_dx(t, x, g), want)


@pytest.mark.parametrize("dn", S.DTYPES)
def test_the_inner_rounding_of_round_ste_is_exact(dn):
    """rd(rint(a) - a) == rint(a) - a for every a of the dtype: the difference is a multiple of a's ulp no larger than a (or a
    itself below one half), so it has a's precision.  The chain's rounding of r - a therefore changes no word, and a kernel
    without it computes the same function -- no test of values can tell the two apart."""
    dt = L.DTYPES[dn]
    a = L.to_f32(S.ALL_WORDS, dt)
    with np.errstate(all="ignore"):
        d = np.rint(a) - a
    fin = np.isfinite(d)
    assert np.array_equal(L.to_f32(L.to_words(d[fin], dt), dt), d[fin])


# ------------------------------------------------------------------ predictors

def test_predictors_restate_the_launchers_rows():
    """Rows worked out by hand from lowp.hip: n -> (n_vec, grid, thread 0, last thread, tail) as (unrolled trips, remainder
    iterations)."""
    G = S.G
    assert G == 33_554_432
    chain = {2048: (256, 1, (0, 1), (0, 1), 0), 2057: (257, 1, (1, 0), (0, 1), 1), 4095: (511, 1, (1, 0), (0, 1), 7),
             4096: (512, 1, (1, 0), (1, 0), 0), 4104: (513, 2, (1, 0), (0, 1), 0), 8207: (1025, 3, (1, 0), (0, 1), 7),
             G: (4194304, 8192, (1, 0), (1, 0), 0), G + 13: (4194305, 8192, (1, 1), (1, 0), 5),
             5 * G // 2 + 25: (10485763, 8192, (3, 0), (2, 1), 1)}
    widen = {1029: (257, 1, (0, 2), (0, 1), 1), 3072: (768, 1, (0, 3), (0, 3), 0), 3079: (769, 1, (1, 0), (0, 3), 3),
             4096: (1024, 1, (1, 0), (1, 0), 0), 4100: (1025, 2, (0, 3), (0, 2), 0), G + 7: (8388609, 8192, (1, 1), (1, 0), 3),
             9 * G // 4 + 13: (18874371, 8192, (2, 2), (2, 1), 1)}
    for rows, predict in ((chain, S.predict_chain), (widen, S.predict_widen)):
        for n, (n_vec, grid, first, last, tail) in rows.items():
            p = predict(n)
            assert (p.n_vec, p.grid, p.stride, p.first, p.last, p.tail) == (n_vec, grid, 256 * grid, first, last, tail), n
    p = S.predict_backward(G + 13)             # no unroll on a grid sized for two granules a lane: two passes, one granule more
    assert (p.n_vec, p.grid, p.first, p.last, p.tail) == (4194305, 8192, (3, 0), (2, 0), 5)


def _reached(predict, sizes, aligns):
    out = {}
    for n in sizes:
        for offs in aligns:
            out[(n,) + tuple(offs)] = predict(n, *offs)
    return out


def _need(cases, what, cond):
    assert any(cond(p) for p in cases.values()), f"no size of the table reaches: {what} -- move the table with the launcher's constants"


def test_size_tables_reach_every_form():
    """A condition on the tables, not a measurement: if a constant of a launcher changes, this says which table to move."""
    only = lambda *pairs: (lambda p: p.pairs == set(pairs))                                   # noqa: E731
    has = lambda form: (lambda p: form in p.forms)                                            # noqa: E731
    chain = _reached(S.predict_chain, S.CHAIN_SIZES + list(S.CHAIN_CAPPED), [(0, 0)])
    _need(chain, "chain remainder only", only((0, 1)))
    _need(chain, "chain unrolled only", only((1, 0)))
    _need(chain, "chain unrolled for some threads, remainder for others", only((1, 0), (0, 1)))
    _need(chain, "chain remainder for some threads, nothing for others", only((0, 1), (0, 0)))
    _need(chain, "chain unrolled then remainder in one thread", has("unrolled then remainder"))
    _need(chain, "chain two or more unrolled trips", lambda p: any(t >= 2 for t, _ in p.pairs))
    _need(chain, "chain capped", has("capped"))
    widen = _reached(S.predict_widen, S.WIDEN_SIZES + list(S.WIDEN_CAPPED), [(0, 0)])
    _need(widen, "widen remainder only", lambda p: all(t == 0 for t, _ in p.pairs) and p.n_vec > 0)
    _need(widen, "widen unrolled only", only((1, 0)))
    _need(widen, "widen unrolled for some threads, remainder for others", lambda p: (1, 0) in p.pairs and (0, 3) in p.pairs)
    _need(widen, "widen unrolled then remainder in one thread", has("unrolled then remainder"))
    _need(widen, "widen two or more unrolled trips", lambda p: any(t >= 2 for t, _ in p.pairs))
    for k in (1, 2, 3):
        _need(widen, f"widen remainder ×{k} in every thread", only((0, k)))
        _need(widen, f"widen remainder ×{k}", has(f"remainder×{k}"))
    _need(widen, "widen two remainder iterations after the unrolled trips", lambda p: any(t and r == 2 for t, r in p.pairs))
    _need(widen, "widen capped", has("capped"))
    back = _reached(S.predict_backward, S.CHAIN_SIZES + list(S.BACKWARD_CAPPED), [(0, 0, 0)])
    for k in (1, 2, 3):
        _need(back, f"backward {k} passes", has(f"unrolled×{k}"))
    _need(back, "backward some threads idle", lambda p: (0, 0) in p.pairs and (1, 0) in p.pairs)
    _need(back, "backward capped", has("capped"))
    assert not any("remainder" in f for p in back.values() for f in p.forms)
    for name, cases, tails in (("chain", chain, (1, 7, 5)), ("backward", back, (1, 7, 5)), ("widen", widen, (1, 3))):
        for t in tails:
            _need(cases, f"{name} tail of {t}", lambda p, t=t: p.tail == t and "tail" in p.forms)
        _need(cases, f"{name} no tail", lambda p: p.n_vec > 0 and p.tail == 0 and "tail" not in p.forms)
        _need(cases, f"{name} a tail alone", lambda p: p.n_vec == 0 and p.tail > 0 and "elements only" not in p.forms)


def test_alignment_tables_take_the_paths_they_must():
    n = 4104
    for x, y in S.CHAIN_ALIGN:
        p = S.predict_chain(n, x, y)
        assert ("elements only" in p.forms) == bool(x or y) and (p.n_vec == 0) == bool(x or y)
    assert {a for a in S.CHAIN_ALIGN if sum(map(bool, a)) == 1} == {(2, 0), (0, 2)} and (2, 2) in S.CHAIN_ALIGN
    for offs in S.BACKWARD_ALIGN:
        p = S.predict_backward(n, *offs)
        assert ("elements only" in p.forms) == any(offs) and (p.n_vec == 0) == any(offs)
    assert {(2, 0, 0), (0, 2, 0), (0, 0, 2)} <= set(S.BACKWARD_ALIGN)
    want = {(0, 0): True, (2, 0): False, (8, 0): True, (0, 4): False, (0, 16): True}
    assert set(want) <= set(S.WIDEN_ALIGN)
    for (x, y), vector in want.items():
        p = S.predict_widen(n, x, y)
        assert ("elements only" not in p.forms) == vector and (p.n_vec == n // 4) == vector, (x, y)
    # the element path alone: one or more passes of the whole grid over the elements
    p = S.predict_chain(8207, 2, 0)
    assert p.grid == 3 and p.forms == {"elements only"} and p.pairs == {(0, 0)}


def test_exhaustive_launches_take_the_loops_they_are_for():
    assert S.predict_chain(65536).pairs == {(1, 0)} and S.predict_chain(65536).tail == 0       # every granule in an unrolled trip
    assert S.predict_chain(2048).pairs == {(0, 1)}                                             # ... in the remainder loop
    assert S.predict_chain(65536, 2, 0).forms == {"elements only"}
    assert S.predict_backward(65536).pairs == {(2, 0)} and S.predict_backward(65536, 2, 2, 2).forms == {"elements only"}
    assert S.predict_widen(65536).pairs == {(1, 0)} and S.predict_widen(2048).pairs == {(0, 2)}
    assert S.predict_widen(65536, 2, 0).forms == {"elements only"}


# ------------------------------------------------------------------ sentinels

@pytest.mark.parametrize("dn,params", DP, ids=DP_IDS)
def test_sentinel_is_finite_and_outside_the_tables(dn, params):
    dt = L.DTYPES[dn]
    t = S.chain_tables(dn, params)
    w = np.array([t.sentinel], np.uint16)
    assert np.isfinite(L.to_f32(w, dt)).all() and L.canon(w, dt)[0] == t.sentinel
    assert not (t.y == t.sentinel).any() and not (t.g == t.sentinel).any() and t.zero_word != t.sentinel
    assert all(np.isfinite(L.to_f32(w, d)).all() for d in L.DTYPES.values())           # finite read as either dtype


def test_no_single_sentinel_serves_every_parameter_set():
    """Why the sentinel is chosen per (dtype, parameter set): the tables of PARAMS hold every finite word between them."""
    for dn in S.DTYPES:
        used = np.zeros(65536, bool)
        for p in S.PARAMS:
            t = S.chain_tables(dn, p)
            used[t.y] = used[t.g] = True
        assert used[np.isfinite(L.to_f32(S.ALL_WORDS, L.DTYPES[dn]))].all()


def test_fp32_sentinel_is_a_marked_nan_no_table_holds():
    s = np.array([S.SENTINEL32], np.uint32)
    assert np.isnan(s.view(np.float32))[0] and S.SENTINEL32 != int(S.CANON_NAN32) and S.SENTINEL32 & 0xFFFF
    for dn in S.DTYPES:
        for W in S.WIDEN_MODES:
            w = S.widen_table(dn, W)
            assert w.dtype == np.uint32 and w.size == 65536 and not (w == S.SENTINEL32).any()
            assert len(np.unique(w)) >= 60, (dn, W.name)


def test_widen_repairs():
    rep = {W.name: S.repaired(W) for W in S.WIDEN_MODES}
    assert rep["sanitize_lsq_negative"] == (np.float32(0.0371), np.float32(128))
    assert rep["sanitize_lsq_below_eps"] == (np.float32(np.finfo(np.float32).eps), np.float32(17))
    assert rep["sanitize_lsqplus_zp_high"] == (np.float32(0.11), np.float32(63))
    assert rep["lsqplus"] == (np.float32(0.05), np.float32(3.25))

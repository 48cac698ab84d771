"""CPU checks of tests/_fake_quant_shapes.py: the oracle's words against plain float64 arithmetic on every input class the
GPU suite uses, the special inputs against the reference's chain, and the predictor's claim that the shape tables reach
every loop of every forward fake-quant kernel at the shipped constants."""
import itertools

import numpy as np
import pytest
import torch

import _fake_quant_shapes as S
from oracle import fake_quant_oracle as FQ

F32 = np.float32


@pytest.mark.parametrize("P", S.PARAM_SETS, ids=lambda P: P.name)
def test_oracle_words_satisfy_the_float64_anchor(P):
    x = S.normal_data(1 << 20, P, 11)
    q, y = S.expected(x, P)
    se, ze = S.effective(P)
    share, inside, rel = S.anchor(x, q, y, se, ze, P.qmin, P.qmax)
    print(P.name, "exempt share", share, "disagreements inside it", inside, "y error / 2^-24", rel * 2.0 ** 24)
    assert se > 0 and (P.mode == "lsqplus" or ze == np.rint(ze))


@pytest.mark.parametrize("P", (S.P_FIXED, S.P_LSQPLUS), ids=lambda P: P.name)
@pytest.mark.parametrize("ch_axis", (0, 1, 2))
def test_per_channel_oracle_words_satisfy_the_float64_anchor(P, ch_axis):
    shape = (24, 31, 130)
    x = S.normal_data(int(np.prod(shape)), P, 12).reshape(shape)
    s, z = S.channel_params(shape[ch_axis], P, 5)
    q, y = S.expected_channel(x, s, z, ch_axis, P)
    se, ze = FQ.lsq_effective(s, z, F32(P.g), P.mode)
    shp = [1, 1, 1]
    shp[ch_axis] = -1
    S.anchor(x, q, y, np.asarray(se).reshape(shp), np.asarray(ze).reshape(shp), P.qmin, P.qmax)


def test_anchor_refuses_wrong_words_and_inputs_it_would_have_to_exempt():
    P = S.P_FIXED
    x = S.normal_data(4096, P, 3)
    q, y = S.expected(x, P)
    se, ze = S.effective(P)
    inside = np.flatnonzero((q > P.qmin) & (q < P.qmax))
    q2 = q.copy()
    q2[inside[7]] += 1
    with pytest.raises(AssertionError):
        S.anchor(x, q2, y, se, ze, P.qmin, P.qmax)
    y2 = y.copy()
    k = np.flatnonzero(y != 0)[5]
    y2[k] = np.nextafter(np.nextafter(np.nextafter(y[k], F32(np.inf)), F32(np.inf)), F32(np.inf))
    with pytest.raises(AssertionError):
        S.anchor(x, q, y2, se, ze, P.qmin, P.qmax)
    ties = (np.arange(-6, 6, dtype=F32) + F32(0.5)) * F32(0.5)          # every element a tie: all would be exempt
    tq, ty = S.expected(ties, S.P_POW2)
    with pytest.raises(AssertionError):
        S.anchor(ties, tq, ty, *S.effective(S.P_POW2), S.P_POW2.qmin, S.P_POW2.qmax)


def test_specials_follow_the_reference_chain():
    P = S.P_POW2                                                        # scale 0.5, zero point 0, [-8, 7]
    sp = S.specials(P.scale)
    q, y = S.expected(sp, P)
    nan, inf, ninf, pz, nz, sub, nsub, big, nbig = range(9)
    # inf -> NaN through round_ste ((inf.round() - inf) + inf), NaN passes the clamp, an overflowing quotient is an inf
    for k in (nan, inf, ninf, big, nbig):
        assert np.isnan(q[k]) and np.isnan(y[k]), k
    with np.errstate(over="ignore"):
        assert np.isinf(sp[big] / F32(P.scale))
    # +-0 and +-subnormal: x_quant = the zero point, y = +0.0 (the reference dequantizes -0.0 to +0.0: test_sign_of_zero_vs_oracle)
    for k in (pz, nz, sub, nsub):
        assert q[k] == 0 and S.words(y[k:k + 1])[0] == 0, k
    # ties go to even: (k + 0.5) * 0.5 / 0.5 is exact in fp32 and in float64
    ks = np.array([0, 1, 2, -1, -2, -3, 6, 7], np.float64)
    want = np.clip(np.array([0, 2, 2, 0, -2, -2, 6, 8], np.float64), P.qmin, P.qmax)
    assert np.array_equal(sp[9:].astype(np.float64) / 0.5, ks + 0.5)
    assert np.array_equal(q[9:].astype(np.float64), want)
    assert np.array_equal(y[9:].astype(np.float64), want * 0.5)
    # with a zero point the sign of zero washes out the same way
    _, y0 = S.expected(np.array([-0.0, 0.0], F32), S.P_FIXED)
    se, ze = S.effective(S.P_FIXED)
    assert np.array_equal(S.words(y0), S.words((F32([ze, ze]) - ze) * se))


def test_sanitize_repair_is_applied_before_the_oracle():
    s, z = S.repaired(S.P_SANITIZE)
    assert s == F32(0.037) and z == F32(63.0)
    s, z = S.repaired(S.P_SANITIZE_LSQ)
    assert s == F32(0.11) and z == F32(29.0)                            # LSQ: the scale alone is repaired
    assert S.repaired(S.P_FIXED._replace(scale=1e-9, sanitize=True))[0] == S.LSQ_EPS
    x = S.normal_data(1000, S.P_SANITIZE, 1)
    q, y = S.expected(x, S.P_SANITIZE)
    q2, y2 = S.expected(x, S.P_SANITIZE._replace(scale=0.037, zp=63.0, sanitize=False))
    assert np.array_equal(S.words(q), S.words(q2)) and np.array_equal(S.words(y), S.words(y2))


def test_loop_formula_equals_walking_every_thread():
    for stride, unroll in itertools.product((8, 16, 24), (2, 4, 8)):
        for n in range(0, 3 * unroll * stride + 40):
            assert S.stream_loops(n, stride, unroll) == S.stream_loops_brute(n, stride, unroll), (n, stride, unroll)


def _strides(shape, view):
    t = torch.empty(shape)
    v = view(t)
    sizes, xs = [1] * (4 - v.dim()) + list(v.shape), [0] * (4 - v.dim()) + list(v.stride())
    ys = list(torch.empty(sizes).stride())
    return sizes, xs, ys, v.storage_offset()


def table_predictions():
    """(kernel, loops, reason, tag) of every table entry at the shipped constants."""
    out = []
    for n, why in S.DENSE_SMALL:
        for want_q in (False, True):
            k, loops = S.predict_per_tensor(n, want_q=want_q)
            out.append((k, loops, why if not want_q or why in ("tail", "rem") else "rem", ("dense", n, want_q)))
    out.append(S.predict_per_tensor(S.DENSE_LARGE) + ("body2", "dense large"))
    out.append(S.predict_per_tensor(S.DENSE_LARGE, want_q=True) + ("body", "dense large q"))
    for n, why in S.SCALAR:
        for want_q in (False, True):
            out.append(S.predict_per_tensor(n, aligned=False, want_q=want_q) + (why, ("scalar", n, want_q)))
    for n, why in S.GELU:
        out.append(S.predict_gelu(n) + (why, ("gelu", n)))
    for shape, slices, off, want_q, why in S.STRIDED_SCALAR:
        sizes, xs, ys, so = _strides(shape, lambda t: S.slice_view(t, slices))
        out.append(S.predict_strided(sizes, xs, ys, aligned=(so + off) % 4 == 0, want_q=want_q) + (why, ("strided scalar", shape)))
        assert out[-1][0].startswith("strided_scalar"), (shape, out[-1][0])
    for shape, how, why in S.STRIDED_VEC:
        sizes, xs, ys, so = _strides(shape, lambda t: S.strided_vec_view(t, how))
        out.append(S.predict_strided(sizes, xs, ys, aligned=so % 4 == 0) + (why, ("strided vec", shape, how)))
        assert out[-1][0] == "strided_vec", (shape, how, out[-1][0])
    geoms = list(itertools.product(S.HEAD_B, S.HEAD_T, S.HEAD_H, S.HEAD_D)) + [S.HEADSPLIT_LARGE]
    for B, T, h, d in geoms:
        sizes, xs, ys = [B, h, T, d], [T * h * d, d, h * d, 1], [h * T * d, T * d, d, 1]
        k, loops = S.predict_strided(sizes, xs, ys)
        out.append((k, loops, "body2" if (B, T, h, d) == S.HEADSPLIT_LARGE else "rem" if B * T * h * d // 4 <= 256 else "body",
                    ("headsplit", B, T, h, d)))
        assert k == "headsplit"
    for (B, T, h, d), n_sites in itertools.product(S.HEADSPLIT_MULTI, (1, 2, 3, 4)):
        out.append(S.predict_headsplit_multi(n_sites, B, T, h, d) + ("rem" if B * T * h * d // 4 <= 256 else "body", ("multi", B, T, h, d)))
    for itemsize, widths in S.ROWS_INNER_G.items():
        for ig, (outer, ch) in itertools.product(widths, S.ROWS_LAYOUTS):
            k, loops = S.predict_channel(outer, ch, ig * S.GRANULE[itemsize], itemsize)
            assert k == "channel_rows"
            out.append((k, loops, "row_body" if ig > (S.ROW_LOADS[itemsize] - 1) * S.WAVE else "row_rem", ("rows", itemsize, ig)))
    out.append(S.predict_channel(*S.ROWS_TRIP2) + ("row_trip2", "rows trip2"))
    for shape, ax, off, why in S.GENERIC:
        outer, ch, inner = int(np.prod(shape[:ax])), shape[ax], int(np.prod(shape[ax + 1:]))
        k, loops = S.predict_channel(outer, ch, inner, 4, aligned=off % 4 == 0)
        assert k == "channel_generic", shape
        out.append((k, loops, why, ("generic", shape)))
    return out


def test_tables_reach_every_loop_of_every_kernel():
    reached = {}
    for kernel, loops, why, tag in table_predictions():
        assert why in loops, (tag, why, loops)                # the entry reaches the loop it is listed for
        reached.setdefault(kernel, set()).update(loops)
    assert set(reached) == set(S.ALL_LOOPS)
    for kernel, need in S.ALL_LOOPS.items():
        assert need <= reached[kernel], (kernel, need - reached[kernel])


def test_write_q_body_needs_the_large_case_at_the_shipped_constants():
    """The return_quantized kernel unrolls 4 on a grid sized for 2: below the cap its body never runs, the large dense case
    is the smallest size class at which it does (and at which the y-only body runs a second trip)."""
    below = 4 * (3 * S.FQ_CAP * S.BLOCK)                      # tests/test_gpu_parity.py::test_full_size_properties' size
    assert "body" not in S.predict_per_tensor(below, want_q=True)[1]
    assert "body2" not in S.predict_per_tensor(below)[1]
    assert all("body" not in S.predict_per_tensor(n, want_q=True)[1] for n, _ in S.DENSE_SMALL)
    assert {"body", "rem", "rem2", "tail", "capped"} <= S.predict_per_tensor(S.DENSE_LARGE, want_q=True)[1]
    assert {"body2", "rem_after_body", "tail", "capped"} <= S.predict_per_tensor(S.DENSE_LARGE)[1]
    assert S.DENSE_LARGE < 26_000_000


def test_knob_sizes_reach_every_loop_at_every_knob_setting():
    for blocks, unroll in itertools.product((1, 2, 3), (2, 4, 8)):
        for want_q in (False, True):
            reached = set()
            for n4, tail in itertools.product(S.knob_sizes(blocks, unroll), (0, 3)):
                if 4 * n4 + tail:
                    reached |= S.predict_per_tensor(4 * n4 + tail, want_q=want_q, unroll=unroll, cap=blocks)[1]
            need = {"body", "rem", "rem_after_body", "tail", "capped"} | ({"body2"} if not want_q or unroll >= 4 else set())
            assert need <= reached, (blocks, unroll, want_q, need - reached)


def test_structural_positions_hold_the_specials():
    n, grid = 4 * (2 * 2 * 256 + 300) + 3, 2                  # two workgroups, unroll 2, a remainder and a tail
    pos = S.stream_positions(n, grid, 2)
    S_ = grid * S.BLOCK
    assert {0, n - 1, n - 2, n - 3, 4 * (2 * S_ - 1), 4 * (2 * S_), 4 * S_} <= pos
    x = S.per_tensor_input(n, S.P_FIXED, 1, grid, 2)
    assert np.isnan(x[0]) and not np.isfinite(x[sorted(pos)][:3]).any()
    assert len({w for w in S.words(x[sorted(pos)])}) >= S.specials(0.11).size - 1
    assert S.row_positions(5, 7) == {0, 6, 7, 13, 14, 20, 21, 27, 28, 34}

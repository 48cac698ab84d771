"""Integer linear layers on the GPU (csrc/linear_int.hip) at every K split, parameter mode, stride and grid stride, against the
int64 restatement of tests/_linear_int.py, WORD FOR WORD -- there is no tolerance anywhere in this file.  Its sibling
tests/test_gpu_linear_int.py covers the tile edges of M and N; this file the loops over K, the parameter paths and the
launch forms the sibling leaves out.

A. K splits (seeded normal data: every position differs), M 1 / 32 (rows kernel) / 33 (tile kernel), N 36 (two workgroups of
the rows kernel, the second with four channels; one channel tile of the tile kernel).  The rows kernel gives wave w the
128-byte chunks w, w + 4, ... of a row, a chunk in four sub-steps of 32 bytes whose halves belong to the lower and upper 32
lanes; the tile kernel steps 64 bytes through two LDS buffers; encode_row walks a row in trips of 4 lane groups (u = 0 .. 3)
of 64 float4 = 1024 elements.  What each K reaches:

    K      rows kernel (M <= 32)                              tile kernel (M = 33)                 encode_row
    128    waves 1-3 idle                                     two full steps
    144    wave 1 has 16 bytes: one sub-step, upper half zero three steps, the last a quarter
    176    wave 1: one sub-step and a half
    192                                                       three full steps (odd, a buffer reused)
    240    wave 1: three sub-steps and a half
    256                                                                                            lane group u = 0 full
    272                                                                                            u = 1 begins
    512    every wave one chunk
    528    ... then wave 0 a second, partial chunk            nine steps, the last a quarter
    768    waves 0, 1 two chunks, waves 2, 3 one              twelve steps                         three lane groups
    784                                                                                            the fourth group begins
    1008   waves 0-3 two chunks, wave 3's last of 112 bytes                                         four float4 short of one full trip
    1040   wave 0 a third chunk of 16 bytes                                                        a second trip of 4 float4
    2064                                                                                           two trips and a tail
    3072   six chunks per wave                                                                     three full trips
    4096   eight chunks per wave                                                                   four full trips

ops.weight_codes is checked on its own at the same K (codes, colsum, scale, zw), per channel, in all three modes.
B. Parameter modes: the input record in fixed / lsq / lsqplus with int32 and float32 zero points, two grad factors, the
weight in all three modes per channel; the scales are chosen so that a kernel that ignored the mode would write other words.
C. The in-launch repair (PARAM_SANITIZE) in activation_codes and in linear_int, and its absence without the flag.
D. Strided, copied and misaligned inputs, ranks 1 and 3, the scalar epilogue at N % 4 == 0 (a misaligned bias or out), empties.
E. The encoders' grid stride (more than 16384 rows) and every way the `bad` word and a no-code row come about."""
import functools
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import _linear_int as LI
from test_gpu_linear_int import PAD, SENTINEL, dev, operands, run, same_words

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]

MODE_ID = {name: i for i, name in enumerate(LI.MODES)}      # ops.PARAM_FIXED / _LSQ / _LSQPLUS
NO_ROW = -2 ** 31
N, NAN = LI.EDGE_N, float("nan")


def assert_words(got, want, skip_codes_of=()):
    """out, codes, rowsum word for word; the bytes of a row without codes are not specified."""
    keep = np.setdiff1d(np.arange(want[1].shape[0]), skip_codes_of)
    assert same_words(got[0], want[0]), "out"
    assert same_words(got[1][keep], want[1][keep]), "codes"
    assert same_words(got[2], want[2]), "rowsum"


# ---- A ------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def edge_reference(m, k):
    case = LI.edge_case(m, k)                            # computed once, not to be modified
    return case, LI.rule(*case)


@pytest.mark.parametrize("k", LI.EDGE_KS)
@pytest.mark.parametrize("m", LI.EDGE_MS)
def test_words_at_every_k_split(m, k):
    case, want = edge_reference(m, k)
    assert_words(run(case, dev, zp_int=(m + k // 16) % 2 == 0), want)


@pytest.mark.parametrize("k", LI.EDGE_KS)
def test_weight_codes_at_every_k_split(k):
    """ops.weight_codes alone, per channel: b, its sums, the effective scales and zw; the modes rotate (grad factor 0.3, raw
    LSQ+ zero points fractional)."""
    from outlier_suppression_amd import ops
    i = LI.EDGE_KS.index(k)
    mode = LI.MODES[i % 3]
    _, _, w, wq, _ = LI.make_case(2500 + i, 1, N, k, LI.QUANTS[(0, 1, 3)[(i // 3) % 3]], False)
    raw_zp = wq.zero_point + LI.F32(0.25 if mode == "lsqplus" else 0.0)
    s_eff, z_eff = LI.effective(wq.scale, raw_zp, mode, 0.3)
    assert np.all((z_eff == np.rint(z_eff)) & (z_eff >= wq.qmin) & (z_eff <= wq.qmax))
    b = LI.units(w, wq._replace(scale=s_eff, zero_point=z_eff)).astype(np.int64) - 128
    e = ops.weight_codes(torch.from_numpy(w).to(dev), torch.from_numpy(wq.scale).to(dev),
                         torch.from_numpy(raw_zp).to(dev).to(torch.float32 if mode == "lsqplus" or i % 2 else torch.int32), 0,
                         wq.qmin, wq.qmax, MODE_ID[mode], 0.3)
    assert same_words(e.codes.cpu().numpy(), (b & 0xFF).astype(np.uint8))
    assert same_words(e.colsum.cpu().numpy(), b.sum(1).astype(np.int32))
    assert same_words(e.scale.cpu().numpy(), s_eff)
    assert same_words(e.zw.cpu().numpy(), (z_eff.astype(np.int64) - wq.qmin - 128).astype(np.int32))
    assert e.bad.item() == 0


# ---- B ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("g_kind", LI.GRAD_FACTORS, ids=str)
@pytest.mark.parametrize("x_mode, x_zp_int", LI.X_MODES)
@pytest.mark.parametrize("m", (2, 33))
def test_parameter_modes(m, x_mode, x_zp_int, g_kind):
    """Expected words: the rule on LI.effective of the raw words.  LI.mode_reference asserts, before the GPU is asked, that the
    launch is good and that the rule on the raw words of either quantizer gives other words of out."""
    for w_mode in LI.W_MODES:
        raw, g, want = LI.mode_reference(m, x_mode, g_kind, w_mode)
        x_side = dict(zp_int=x_zp_int, x_mode=MODE_ID[x_mode], x_g=g)
        assert_words(run(raw, dev, w_mode=MODE_ID[w_mode], w_g=g, w_zp_int=w_mode == "fixed", **x_side), want)
        if w_mode == "lsqplus":                          # the same fractional zero points, taken as they are
            assert np.isnan(run(raw, dev, w_zp_int=False, **x_side)[0]).all()


# ---- C ------------------------------------------------------------------------------------------------------------------

def _left_in_memory(record, left, zp_int):
    scale, zp = (t.cpu().numpy() for t in record[:2])
    assert same_words(scale, left[0]), "scale"
    assert same_words(zp, left[1].astype(np.int32 if zp_int else np.float32)), "zero point"


@pytest.mark.parametrize("what", LI.REPAIRS)
@pytest.mark.parametrize("mode", ("lsq", "lsqplus"))
@pytest.mark.parametrize("m", (2, 33))
def test_the_repair_rides_in_both_launches(m, mode, what):
    """activation_codes alone repairs the raw words in memory (an int32 zero point is never touched) and encodes under the
    repaired ones; linear_int alone, given the raw words again, repairs the same way and multiplies under the repaired ones."""
    from outlier_suppression_amd import ops
    raw, g, zp_int, left, want = LI.repair_reference(m, mode, what)
    x, record, entry, bias = operands(raw, dev, zp_int, x_mode=MODE_ID[mode] | ops.PARAM_SANITIZE, x_g=g, w_zp_int=True)
    raw_words = [t.clone() for t in record[:2]]
    codes, rowsum = ops.activation_codes(x, record)
    _left_in_memory(record, left, zp_int)
    assert same_words(codes.cpu().numpy(), want[1]) and same_words(rowsum.cpu().numpy(), want[2])
    for t, r in zip(record[:2], raw_words):
        t.copy_(r)
    out = ops.linear_int(codes, rowsum, record, entry, bias)
    _left_in_memory(record, left, zp_int)
    assert same_words(out.cpu().numpy(), want[0])
    assert np.isnan(want[0]).all() == (mode == "lsq" and "zero point" in what)      # only an int32 zero point stays outside


@pytest.mark.parametrize("mode, what", [(mode, what) for mode in ("lsq", "lsqplus") for what in LI.REPAIRS]
                         + [("fixed", what) for what in LI.REPAIRS[2:]])
@pytest.mark.parametrize("m", (2, 33))
def test_without_the_flag_the_raw_words_stay(m, mode, what):
    """... and are what both launches compute with; a zero point outside the range, in fixed mode too: all of out is NaN."""
    from outlier_suppression_amd import ops
    raw, g, zp_int, left, want = LI.repair_reference(m, mode, what, sanitize=False)
    x, record, entry, bias = operands(raw, dev, zp_int, x_mode=MODE_ID[mode], x_g=g, w_zp_int=True)
    codes, rowsum = ops.activation_codes(x, record)
    out = ops.linear_int(codes, rowsum, record, entry, bias)
    _left_in_memory(record, (raw[1].scale, raw[1].zero_point), zp_int)
    no_codes = np.nonzero(want[2] == NO_ROW)[0]
    assert_words(tuple(t.cpu().numpy() for t in (out, codes, rowsum)), want, no_codes)
    assert np.isnan(want[0]).all() == ("zero point" in what)


@pytest.mark.parametrize("kind, mode", (("LSQFakeQuantize", "lsq"), ("LSQPlusFakeQuantize", "lsqplus")))
def test_the_helpers_state_what_the_modules_do(kind, mode):
    """LI.repaired and LI.effective against the learnable quantizers themselves (observer off): the parameters after a forward
    and the fake-quantised output, word for word."""
    from outlier_suppression_amd.quantization import Quantizer
    x, xq = LI.make_case(6000, 5, 4, 48, LI.MODE_QUANT, False)[:2]
    q = Quantizer(None, NS(quantizer=kind, observer="MinMaxObserver", bit=8, symmetric=False, ch_axis=-1)).to(dev)
    q.disable_observer()
    q.enable_fake_quant()
    zp_float = q.zero_point.dtype == torch.float32
    raw_s, raw_z = -xq.scale, LI.F32([xq.qmax + 3.5 if zp_float else xq.zero_point[0]])
    q.scale.data.copy_(torch.from_numpy(raw_s))
    q.zero_point.data.copy_(torch.from_numpy(raw_z))
    with torch.no_grad():
        y = q(torch.from_numpy(x).to(dev)).cpu().numpy()
    left = LI.repaired(raw_s, raw_z, mode, zp_float, xq.qmin, xq.qmax)
    assert same_words(q.scale.detach().cpu().numpy(), left[0]) and same_words(q.zero_point.detach().cpu().numpy().astype(np.float32), left[1])
    s, z = LI.effective(*left, mode, LI.grad_factor("site", *x.shape, xq.qmax))
    want = ((LI.units(x, xq._replace(scale=s, zero_point=z)).astype(np.float32) + LI.F32(xq.qmin) - z) * s).astype(np.float32)
    assert same_words(y, want)


# ---- D ------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def small_reference(m, k=80):
    case = LI.make_case(4000 + m, m, N, k, LI.QUANTS[0], True)       # per-channel scales, a bias; not to be modified
    return case, LI.rule(*case)


@pytest.mark.parametrize("layout", ("stride K + 16", "stride K + 2", "misaligned"))
@pytest.mark.parametrize("m", (2, 33))
def test_strided_copied_and_misaligned_inputs(m, layout):
    """A [:, :K] view of NaN-padded rows goes down ops.activation_codes' strided branch (row stride K + 16) or its copy branch
    (K + 2: rows not 16-byte aligned); a dense view 4 bytes off alignment is copied too.  No padding is read as data."""
    from outlier_suppression_amd import ops
    (case, want), k = small_reference(m), 80
    x, record, entry, bias = operands(case, dev)
    if layout == "misaligned":
        view = torch.full((m * k + 1,), NAN, device=dev)[1:].view(m, k)
        assert view.is_contiguous() and view.data_ptr() % 16 == 4
    else:
        pad = int(layout.split("+")[1])
        view = torch.full((m, k + pad), NAN, device=dev)[:, :k]
        assert view.stride(0) == k + pad and view.data_ptr() % 16 == 0
    view.copy_(x)
    codes, rowsum = ops.activation_codes(view, record)
    dense = ops.activation_codes(x, record)
    assert (rowsum.cpu().numpy() != NO_ROW).all() and codes.is_contiguous()
    assert all(same_words(a.cpu().numpy(), b.cpu().numpy()) for a, b in zip((codes, rowsum), dense))
    assert_words(tuple(t.cpu().numpy() for t in (ops.linear_int(codes, rowsum, record, entry, bias), codes, rowsum)), want)


def test_ranks_one_and_three():
    from outlier_suppression_amd import ops
    (x, xq, w, wq, bias), k = small_reference(6)[0], 80
    _, record, entry, bias_d = operands((x, xq, w, wq, bias), dev)
    for shape, rows in (((k,), x[:1]), ((2, 3, k), x)):
        want = LI.rule(rows, xq, w, wq, bias)
        codes, rowsum = ops.activation_codes(torch.from_numpy(rows.reshape(shape)).to(dev), record)
        out = ops.linear_int(codes, rowsum, record, entry, bias_d)
        assert (tuple(codes.shape), tuple(rowsum.shape), tuple(out.shape)) == (shape, shape[:-1], shape[:-1] + (N,))
        for got, ref in zip((out, codes, rowsum), want):
            assert same_words(got.cpu().numpy().reshape(ref.shape), ref)


@pytest.mark.parametrize("m", (2, 33))
def test_scalar_epilogue_at_a_multiple_of_four(m):
    """N = 36 with a bias, or an out, that is 4-byte but not 16-byte aligned: the scalar epilogue writes the words of the
    16-byte one, and nothing either side of out."""
    from outlier_suppression_amd import _hip, ops
    (case, want), k = small_reference(m), 80
    x, record, e, bias = operands(case, dev)
    off_bias = torch.zeros(N + 4, device=dev)[1:N + 1].copy_(bias)
    assert off_bias.data_ptr() % 16 == 4 and bias.data_ptr() % 16 == 0
    codes, rowsum = ops.activation_codes(x, record)
    assert same_words(ops.linear_int(codes, rowsum, record, e, bias).cpu().numpy(), want[0])
    assert same_words(ops.linear_int(codes, rowsum, record, e, off_bias).cpu().numpy(), want[0])
    scale, zp, qmin, qmax, mode, gf = record
    buf = torch.full((2 * PAD + 1 + m * N,), SENTINEL, device=dev)
    body = buf[PAD + 1:PAD + 1 + m * N]
    assert body.data_ptr() % 16 == 4
    _hip.check(_hip.load().osq_linear_int(codes.data_ptr(), rowsum.data_ptr(), e.codes.data_ptr(), e.colsum.data_ptr(), e.scale.data_ptr(),
                                          e.zw.data_ptr(), e.bad.data_ptr(), bias.data_ptr(), body.data_ptr(), m, N, k, scale.data_ptr(),
                                          zp.data_ptr(), ops._zp_type(zp), mode, gf, qmin, qmax, _hip.stream_ptr(dev)))
    got = buf.cpu().numpy()
    assert (got[:PAD + 1] == SENTINEL).all() and (got[-PAD:] == SENTINEL).all() and same_words(got[PAD + 1:-PAD].reshape(m, N), want[0])


def test_empty_operands():
    """No row, or no channel (per row and per tensor): empty tensors of the right shapes, and nothing that is launched fails."""
    from outlier_suppression_amd import ops
    (case, _), k = small_reference(2), 80
    x, record, entry, bias = operands(case, dev)
    codes, rowsum = ops.activation_codes(x[:0], record)
    out = ops.linear_int(codes, rowsum, record, entry, bias)
    assert [(tuple(t.shape), t.dtype) for t in (codes, rowsum, out)] == [((0, k), torch.uint8), ((0,), torch.int32), ((0, N), torch.float32)]
    codes, rowsum = ops.activation_codes(x, record)
    for ch_axis, count in ((0, 0), (-1, 1)):
        e = ops.weight_codes(torch.empty(0, k, device=dev), torch.ones(count, device=dev), torch.zeros(count, dtype=torch.int32, device=dev),
                             ch_axis, 0, 255)
        assert [tuple(t.shape) for t in e] == [(0, k), (0,), (0,), (0,), (1,)] and e.bad.item() == 0
        out = ops.linear_int(codes, rowsum, record, e, torch.empty(0, device=dev))
        assert tuple(out.shape) == (2, 0) and out.dtype == torch.float32
    torch.cuda.synchronize()


# ---- E ------------------------------------------------------------------------------------------------------------------

LONG = 4 * 2 * 2048 + 3        # rows past one grid stride of the encoders: 2 * kMaxBlocks workgroups of four waves, a wave per row


@functools.lru_cache(maxsize=None)
def long_reference(rows_of_x):
    case = LI.make_case(5000, LONG, 4, 16, LI.QUANTS[0], True) if rows_of_x else LI.make_case(5001, 1, LONG, 16, LI.QUANTS[0], False)
    return case, LI.rule(*case)


def test_grid_stride_over_the_rows_of_x():
    """Every row's codes, row sum and out; then a NaN in row 16386, which a workgroup meets in its second round: that row alone."""
    case, want = long_reference(True)
    assert_words(run(case, dev), want)
    x = case[0].copy()
    x[LONG - 1, 5] = np.nan
    want = LI.rule(x, *case[1:])
    got = run((x,) + case[1:], dev)
    assert got[2][LONG - 1] == NO_ROW and np.isnan(got[0][LONG - 1]).all() and not np.isnan(got[0][:LONG - 1]).any()
    assert_words(got, want, [LONG - 1])


def test_grid_stride_over_the_rows_of_w_and_the_bad_word():
    """Every weight row of N = 16387 (through out, and the entry on its own); one NaN element in the last row, or one zero
    point at qmax + 1 (an integer outside the range): bad == 1 and all of out NaN; a good weight afterwards: bad == 0."""
    from outlier_suppression_amd import ops
    (x, xq, w, wq, bias), want = long_reference(False)
    xd, record, entry, _ = operands((x, xq, w, wq, bias), dev)
    b = LI.units(w, wq).astype(np.int64) - 128
    assert same_words(entry.codes.cpu().numpy(), (b & 0xFF).astype(np.uint8)) and same_words(entry.colsum.cpu().numpy(), b.sum(1).astype(np.int32))
    assert same_words(entry.scale.cpu().numpy(), wq.scale) and entry.bad.item() == 0
    codes, rowsum = ops.activation_codes(xd, record)
    assert same_words(ops.linear_int(codes, rowsum, record, entry).cpu().numpy(), want[0])
    w_nan, zp_out = w.copy(), wq.zero_point.copy()
    w_nan[LONG - 1, 15], zp_out[LONG - 2] = np.nan, wq.qmax + 1
    for broken in ((x, xq, w_nan, wq, bias), (x, xq, w, wq._replace(zero_point=zp_out), bias)):
        assert np.isnan(LI.rule(*broken)[0]).all()
        e = operands(broken, dev)[2]
        assert e.bad.item() == 1 and np.isnan(ops.linear_int(codes, rowsum, record, e).cpu().numpy()).all()
    assert operands((x, xq, w, wq, bias), dev)[2].bad.item() == 0


@pytest.mark.parametrize("m", (2, 33))
def test_a_nan_in_the_second_trip(m):
    """The last element of a K = 1040 row, which encode_row's second trip holds: that row alone has no codes, in both product
    kernels."""
    x, *rest = LI.make_case(5100 + m, m, N, 1040, LI.QUANTS[3], True)
    x[m - 1, 1039] = np.nan
    want = LI.rule(x, *rest)
    got = run((x, *rest), dev)
    assert got[2][m - 1] == NO_ROW and np.isnan(got[0][m - 1]).all() and not np.isnan(got[0][:m - 1]).any()
    assert_words(got, want, [m - 1])

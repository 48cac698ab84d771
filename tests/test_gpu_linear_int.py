"""Integer linear layers on the GPU (csrc/linear_int.hip): ops.activation_codes / ops.weight_codes / ops.linear_int against the
int64 restatement of tests/_linear_int.py, WORD FOR WORD -- there is no tolerance anywhere in this file.

Shapes: M 1 / 31 / 32 (the rows kernel and its last size), 33 (the tile kernel's first), 127 / 128 / 129 (a wave's 64 rows and
the workgroup's 128, both sides), 257 (three row tiles); N 4 (one group of four channels), 127 / 128 / 129 (the channel tile and
the rows kernel's 32-channel workgroups, both sides; 127 and 129 take the scalar epilogue), 260 (three channel tiles, 16-byte
epilogue); K 16 / 48 (half steps), 64 (one step), 80 (a step and a quarter), 1024 (16 steps; two chunks per wave of the rows
kernel)."""
import functools

import numpy as np
import pytest
import torch

import _linear_int as LI

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]

MS, NS_, KS = (1, 31, 32, 33, 127, 128, 129, 257), (4, 127, 128, 129, 260), (16, 48, 64, 80, 1024)
SENTINEL, PAD, dev = -12345.0, 64, torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def reference(m, n, k):
    # operands and expected words of one shape: computed once, not to be modified; quantizers and bias rotate
    i = MS.index(m) * 7 + NS_.index(n) * 3 + KS.index(k)
    case = LI.make_case(1000 + i, m, n, k, LI.QUANTS[i % len(LI.QUANTS)], i % 2 == 0)
    return case, LI.rule(*case)


def operands(case, dev, zp_int=True, x_mode=0, x_g=1.0, w_mode=0, w_g=1.0, w_zp_int=None):
    """The launches' operands from a case whose parameters are the RAW words of both quantizers: under the default mode,
    PARAM_FIXED, they are the effective ones LI.rule takes; under another (x_mode may carry PARAM_SANITIZE) LI.effective_case
    says what the rule takes.  Zero points are int32 (zp_int / w_zp_int; the weight's follows the input's unless given) or
    float32."""
    from outlier_suppression_amd import ops
    x, xq, w, wq, bias = case
    (xs, xz), (ws, wz) = ((torch.from_numpy(q.scale).to(dev), torch.from_numpy(q.zero_point).to(dev).to(torch.int32 if as_int else torch.float32))
                          for q, as_int in ((xq, zp_int), (wq, zp_int if w_zp_int is None else w_zp_int)))
    entry = ops.weight_codes(torch.from_numpy(w).to(dev), ws, wz, 0 if ws.numel() > 1 else -1, wq.qmin, wq.qmax, w_mode, w_g)
    return (torch.from_numpy(x).to(dev), (xs, xz, xq.qmin, xq.qmax, x_mode, x_g), entry,
            None if bias is None else torch.from_numpy(bias).to(dev))


def run(case, dev, zp_int=True, **modes):
    from outlier_suppression_amd import ops
    x, record, entry, bias = operands(case, dev, zp_int, **modes)
    codes, rowsum = ops.activation_codes(x, record)
    return tuple(t.cpu().numpy() for t in (ops.linear_int(codes, rowsum, record, entry, bias), codes, rowsum))


def same_words(got, want):
    return (got.shape, got.dtype, got.tobytes()) == (want.shape, want.dtype, want.tobytes())


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", NS_)
@pytest.mark.parametrize("m", MS)
def test_words_at_every_tile_edge(m, n, k):
    case, want = reference(m, n, k)
    assert all(same_words(g, w) for g, w in zip(run(case, dev, zp_int=(m + n) % 2 == 0), want))


@pytest.mark.parametrize("m", (2, 33))
@pytest.mark.parametrize("mixed", (False, True))
def test_saturation_at_the_longest_k(m, mixed):
    """Every code 255, zero points 0, K = 16384: N = 255 * 255 * 16384 > 2**30.  Mixed: codes 0 / 255 alternate and the zero
    points sit at 255: a, b, zx and zw take both signs, the correction terms are large and cancel."""
    k, n = 16384, 8
    sign = np.where(np.arange(k) % 2 == 0, 1.0, -1.0).astype(np.float32) if mixed else np.ones(k, np.float32)
    x, w = np.tile(1e6 * sign, (m, 1)), np.tile(1e6 * np.roll(sign, int(mixed)), (n, 1))
    w[1::2] = 1e6 * sign
    zp = np.float32(255.0 if mixed else 0.0)
    case = (x, LI.Quant(np.full(1, 0.5, np.float32), np.full(1, zp), 0, 255), w, LI.Quant(np.full(n, 0.25, np.float32), np.full(n, zp), 0, 255), None)
    want = LI.rule(*case)[0]
    assert mixed or want[0, 0] == np.float32(255 * 255 * k) * np.float32(0.125)
    assert same_words(run(case, dev)[0], want)


@pytest.mark.parametrize("m", (2, 129))
def test_non_finite_row_and_a_fractional_zero_point(m):
    """A NaN and an infinity in one row: that row of out is NaN, its neighbours are the rule's words.  A zero point of the input
    or of one weight channel that is no integer: all of out is NaN.  In the rows kernel (M = 2) and the tile kernel."""
    x, xq, w, wq, bias = LI.make_case(5, m, 260, 80, LI.QUANTS[0], True)
    x[m - 2, 17], x[m - 2, 3] = np.nan, np.inf
    want = LI.rule(x, xq, w, wq, bias)
    out, _, rowsum = run((x, xq, w, wq, bias), dev)
    assert np.isnan(out[m - 2]).all() and not np.isnan(np.delete(out, m - 2, 0)).any()
    assert same_words(out, want[0]) and same_words(rowsum, want[2])
    for bad in ((x, xq._replace(zero_point=xq.zero_point + np.float32(0.5)), w, wq, bias),
                (x, xq, w, wq._replace(zero_point=wq.zero_point + np.float32(0.5) * (np.arange(260) == 200)), bias)):
        assert np.isnan(run(bad, dev, zp_int=False)[0]).all()


@pytest.mark.parametrize("m, n, k", ((1, 4, 16), (32, 129, 80), (33, 127, 48), (129, 260, 1024)))
def test_sentinel_and_canaries(m, n, k):
    """Through the C ABI on this test's buffers: every word of codes, rowsum and out is written, nothing either side is."""
    from outlier_suppression_amd import _hip, ops
    case, want = reference(m, n, k)
    x, (scale, zp, qmin, qmax, mode, gf), e, bias = operands(case, dev)
    out, codes, rowsum = (torch.full((2 * PAD + size,), fill, dtype=dt, device=dev) for size, fill, dt in
                          ((m * n, SENTINEL, torch.float32), (m * k, 0x5A, torch.uint8), (m, 77, torch.int32)))
    group = (scale.data_ptr(), zp.data_ptr(), ops._zp_type(zp), mode, gf, qmin, qmax, _hip.stream_ptr(dev))
    _hip.check(_hip.load().osq_activation_codes(x.data_ptr(), m, k, k, codes[PAD:].data_ptr(), rowsum[PAD:].data_ptr(), *group))
    _hip.check(_hip.load().osq_linear_int(codes[PAD:].data_ptr(), rowsum[PAD:].data_ptr(), e.codes.data_ptr(), e.colsum.data_ptr(), e.scale.data_ptr(),
                                  e.zw.data_ptr(), e.bad.data_ptr(), _hip.ptr(bias), out[PAD:].data_ptr(), m, n, k, *group))
    for buf, body, fill in ((out, want[0], SENTINEL), (codes, want[1], 0x5A), (rowsum, want[2], 77)):
        got = buf.cpu().numpy()
        assert (got[:PAD] == fill).all() and (got[-PAD:] == fill).all() and same_words(got[PAD:-PAD].reshape(body.shape), body)


def test_stream_capture_replays_the_same_words():
    from outlier_suppression_amd import ops
    case, want = reference(129, 260, 80)
    x, record, entry, bias = operands(case, dev)
    xd = torch.zeros_like(x)

    def step():
        return ops.linear_int(*ops.activation_codes(xd, record), record, entry, bias)
    step()                                               # the library is loaded and warm before the capture
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    xd.copy_(x)
    for _ in range(2):
        out.fill_(SENTINEL)
        graph.replay()
        assert same_words(out.cpu().numpy(), want[0])

"""The 16-bit-only kernels of csrc/lowp.hip on the device, through the C ABI with raw pointers: EVERY input word on every code
path (the in-dtype chain, its backward, the widening form in every parameter mode with OSQ_PARAM_SANITIZE), the per-channel
widening of fake_quant.hip, every loop edge and pointer alignment of tests/_lowp_shapes.py, and the capped grids.

Expected values are table lookups (tests/_lowp_shapes.py; tests/test_oracle_lowp_shapes.py pins the tables to plain torch
arithmetic on the CPU).  Outputs are pre-filled with a sentinel word no table holds and sit between guard bands that must
survive; buffers are compared whole, as words, NaN equal to NaN whatever its payload.  Equality is exact everywhere."""
import numpy as np
import pytest
import torch

import _lowp_chain as L
import _lowp_shapes as S

pytestmark = pytest.mark.gpu

DP = [(dn, p) for dn in S.DTYPES for p in S.EVERY_WORD_PARAMS]
DP_IDS = [f"{dn}-{S.param_id(p)}" for dn, p in DP]
DW = [(dn, W) for dn in S.DTYPES for W in S.WIDEN_MODES]
DW_IDS = [f"{dn}-{W.name}" for dn, W in DW]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from outlier_suppression_amd import _hip
    _hip.load()
    return torch.device("cuda:0")


def _lib():
    from outlier_suppression_amd import _hip
    return _hip, _hip.load()


def _code(dn):
    from outlier_suppression_amd import _hip
    return {"bf16": _hip.DTYPE_BF16, "f16": _hip.DTYPE_F16}[dn]


def _i16(word):
    return int(word) - 65536 if int(word) >= 32768 else int(word)


def _i32(word):
    return int(word) - (1 << 32) if int(word) >= (1 << 31) else int(word)


# ------------------------------------------------------------------ buffers

def place16(words, dev, off_bytes=0):
    """A device copy of uint16 words that starts off_bytes past a 16-byte boundary (room behind it, so that a vector load of the
    last granule stays inside the allocation wherever the copy starts)."""
    words = np.ascontiguousarray(words, dtype=np.uint16)
    assert off_bytes % 2 == 0 and 0 <= off_bytes < 16
    buf = torch.zeros(words.size + 16, dtype=torch.int16, device=dev)
    assert buf.data_ptr() % 16 == 0
    v = buf[off_bytes // 2:off_bytes // 2 + words.size]
    v.copy_(torch.from_numpy(words.view(np.int16)))
    return v


class Out:
    """n elements of `itemsize` bytes at byte offset off_bytes from a 16-byte boundary, payload and guard bands pre-filled with
    the sentinel word."""

    def __init__(self, n, dev, itemsize, sentinel, off_bytes=0):
        assert off_bytes % itemsize == 0 and S.GUARD * itemsize % 16 == 0
        self.n, self.start, self.sentinel = n, S.GUARD + off_bytes // itemsize, sentinel
        tdt, fill = (torch.int16, _i16(sentinel)) if itemsize == 2 else (torch.int32, _i32(sentinel))
        self.np_dt = np.uint16 if itemsize == 2 else np.uint32
        self.buf = torch.full((S.GUARD + n + S.GUARD + 16,), fill, dtype=tdt, device=dev)
        assert self.buf.data_ptr() % 16 == 0
        self.ptr = self.buf.data_ptr() + self.start * itemsize
        assert self.ptr % 16 == off_bytes % 16

    def words(self, tag):
        """Payload words; asserts that no word outside the payload changed."""
        w = self.buf.cpu().numpy().view(self.np_dt)
        assert (w[:self.start] == self.sentinel).all() and (w[self.start + self.n:] == self.sentinel).all(), \
            (tag, "a word outside the output changed")
        return w[self.start:self.start + self.n].copy()


def _canon32(w):
    """fp32 words with every NaN but the sentinel canonical."""
    w = w.copy()
    w[np.isnan(w.view(np.float32)) & (w != S.SENTINEL32)] = S.CANON_NAN32
    return w


def _same(got, want, tag, sentinel):
    if np.array_equal(got, want):
        return
    bad = np.flatnonzero(got != want)
    raise AssertionError((tag, "words differ", bad.size, "still the sentinel", int((got == sentinel).sum()), "first", bad[:8].tolist(),
                          [hex(int(v)) for v in got[bad[:4]]], [hex(int(v)) for v in want[bad[:4]]]))


class Params16:
    """(scale, zero_point) of a chain parameter set on the device: fp32 [1], and int32 [1] or -- a float zero point -- fp32 [1]."""

    def __init__(self, params, dev):
        from outlier_suppression_amd import ops
        _, _, s, zp = params
        self.scale = torch.tensor([s], dtype=torch.float32, device=dev)
        self.zp = torch.tensor([zp], dtype=torch.float32 if isinstance(zp, float) else torch.int32, device=dev)
        self.zp_type = ops._zp_type(self.zp)


# ------------------------------------------------------------------ launches (each twice: the same words both times)

def run_chain(dev, dn, xw, params, x_off=0, y_off=0, forms=None, tag=None):
    _hip, lib = _lib()
    t = S.chain_tables(dn, params)
    p = S.predict_chain(xw.size, x_off, y_off)
    assert forms is None or p.forms == forms, (tag, p.forms)
    x, P = place16(xw, dev, x_off), Params16(params, dev)
    runs = []
    for _ in range(2):
        y = Out(xw.size, dev, 2, t.sentinel, y_off)
        _hip.check(lib.osq_fake_quant_chain_lowp(_code(dn), x.data_ptr(), y.ptr, xw.size, P.scale.data_ptr(), P.zp.data_ptr(), P.zp_type,
                                                 t.qmin, t.qmax, _hip.stream_ptr(dev)), "fake_quant_chain_lowp")
        torch.cuda.synchronize()
        runs.append(L.canon(y.words(tag), L.DTYPES[dn]))
    _same(runs[0], t.y[xw], tag, t.sentinel)
    _same(runs[1], runs[0], (tag, "second launch"), t.sentinel)


def run_backward(dev, dn, xw, gw, params, x_off=0, g_off=0, dx_off=0, forms=None, tag=None):
    _hip, lib = _lib()
    t = S.chain_tables(dn, params)
    p = S.predict_backward(xw.size, x_off, g_off, dx_off)
    assert forms is None or p.forms == forms, (tag, p.forms)
    x, g, P = place16(xw, dev, x_off), place16(gw, dev, g_off), Params16(params, dev)
    runs = []
    for _ in range(2):
        dx = Out(xw.size, dev, 2, t.sentinel, dx_off)
        _hip.check(lib.osq_fake_quant_chain_backward_lowp(_code(dn), x.data_ptr(), g.data_ptr(), dx.ptr, xw.size, P.scale.data_ptr(),
                                                          P.zp.data_ptr(), P.zp_type, t.qmin, t.qmax, _hip.stream_ptr(dev)),
                   "fake_quant_chain_backward_lowp")
        torch.cuda.synchronize()
        runs.append(L.canon(dx.words(tag), L.DTYPES[dn]))
    _same(runs[0], S.expected_dx(t, xw, gw), tag, t.sentinel)
    _same(runs[1], runs[0], (tag, "second launch"), t.sentinel)


class ParamsW:
    """A widening parameter set on the device, and the check that a launch left (or repaired) its words as it must."""

    def __init__(self, W, dev):
        self.W = W
        self.scale = torch.tensor([W.scale], dtype=torch.float32, device=dev)
        self.zp = torch.tensor([W.zp], dtype=torch.float32 if W.zp_float else torch.int32, device=dev)
        self.zp_type = 1 if W.zp_float else 0
        self.mode = S.MODE_CODE[W.mode] | (S.SANITIZE if W.sanitize else 0)

    def check(self, tag):
        W = self.W
        s, z = S.repaired(W)                       # the parameters themselves without the flag
        assert np.array_equal(self.scale.cpu().numpy().view(np.uint32), np.array([s], np.float32).view(np.uint32)), (tag, "scale")
        want = np.array([z], np.float32) if W.zp_float else np.array([W.zp], np.int32)
        assert np.array_equal(self.zp.cpu().numpy().view(np.uint32), want.view(np.uint32)), (tag, "zero point")


def run_widen(dev, dn, xw, W, x_off=0, y_off=0, forms=None, tag=None):
    _hip, lib = _lib()
    p = S.predict_widen(xw.size, x_off, y_off)
    assert forms is None or p.forms == forms, (tag, p.forms)
    x = place16(xw, dev, x_off)
    runs = []
    for _ in range(2):
        P = ParamsW(W, dev)                        # the raw parameters again: the second launch repairs them itself
        y = Out(xw.size, dev, 4, S.SENTINEL32, y_off)
        _hip.check(lib.osq_fake_quant_per_tensor_widen(_code(dn), x.data_ptr(), y.ptr, xw.size, P.scale.data_ptr(), P.zp.data_ptr(),
                                                       P.zp_type, P.mode, float(W.g), W.qmin, W.qmax, _hip.stream_ptr(dev)),
                   "fake_quant_per_tensor_widen")
        torch.cuda.synchronize()
        runs.append(_canon32(y.words(tag)))
        P.check(tag)
    _same(runs[0], S.widen_table(dn, W)[xw], tag, S.SENTINEL32)
    _same(runs[1], runs[0], (tag, "second launch"), S.SENTINEL32)
    return runs[0]


# ------------------------------------------------------------------ every word, every code path

@pytest.mark.parametrize("dn,params", DP, ids=DP_IDS)
def test_chain_forward_every_word(dev, dn, params):
    run_chain(dev, dn, S.ALL_WORDS, params, forms={"unrolled×1"}, tag="unrolled")
    for k in range(32):
        run_chain(dev, dn, S.ALL_WORDS[2048 * k:2048 * (k + 1)], params, forms={"remainder×1"}, tag=("remainder", k))
    run_chain(dev, dn, S.ALL_WORDS, params, x_off=2, forms={"elements only"}, tag="elements")


def _g_probes(dn):
    """1.0, -2.5, +0.0, -0.0, a subnormal, inf, NaN as words of the dtype."""
    dt = L.DTYPES[dn]
    w = L.to_words(np.array([1.0, -2.5, 0.0, -0.0, np.inf, np.nan], np.float32), dt).tolist()
    sub = 0x0003                                               # three units of the smallest subnormal, in either dtype
    v = L.to_f32(np.array([sub], np.uint16), dt)[0]
    assert v > 0 and v < (2.0 ** -126 if dn == "bf16" else 2.0 ** -14)
    return w[:4] + [sub] + w[4:]


@pytest.mark.parametrize("dn,params", DP, ids=DP_IDS)
def test_chain_backward_every_word(dev, dn, params):
    t = S.chain_tables(dn, params)
    kept = np.full(65536, t.kept, np.uint16)
    for offs, forms in (((0, 0, 0), {"unrolled×2"}), ((2, 2, 2), {"elements only"})):
        run_backward(dev, dn, kept, S.ALL_WORDS, params, *offs, forms=forms, tag=("every g", offs))
        for gword in _g_probes(dn):
            run_backward(dev, dn, S.ALL_WORDS, np.full(65536, gword, np.uint16), params, *offs, forms=forms,
                         tag=("every x", hex(gword), offs))


@pytest.mark.parametrize("dn,W", DW, ids=DW_IDS)
def test_widen_every_word(dev, dn, W):
    from outlier_suppression_amd import ops
    dt = L.DTYPES[dn]
    got = run_widen(dev, dn, S.ALL_WORDS, W, forms={"unrolled×1"}, tag="unrolled")
    for k in range(32):
        run_widen(dev, dn, S.ALL_WORDS[2048 * k:2048 * (k + 1)], W, forms={"remainder×2"}, tag=("remainder", k))
    run_widen(dev, dn, S.ALL_WORDS, W, x_off=2, forms={"elements only"}, tag="elements")
    run_widen(dev, dn, S.ALL_WORDS, W, y_off=4, forms={"elements only"}, tag="elements, y off")
    # the fp32 kernel on x.float() and the package's own dispatch of a 16-bit x with [1] parameters: the same words, and the same
    # parameter words afterwards
    x = L.from_words(S.ALL_WORDS, dt, dev)
    Pf, Ph = ParamsW(W, dev), ParamsW(W, dev)
    yf = ops.fake_quant_per_tensor(x.float(), Pf.scale, Pf.zp, W.qmin, W.qmax, Pf.mode, W.g)
    yh = ops.fake_quant(x, Ph.scale, Ph.zp, -1, W.qmin, W.qmax, Ph.mode, W.g)
    assert yh.dtype == torch.float32
    torch.cuda.synchronize()
    _same(_canon32(yf.cpu().numpy().view(np.uint32)), got, "fp32 kernel on x.float()", S.SENTINEL32)
    _same(_canon32(yh.cpu().numpy().view(np.uint32)), got, "ops.fake_quant", S.SENTINEL32)
    Pf.check("fp32 kernel")
    Ph.check("ops.fake_quant")


@pytest.mark.parametrize("dn", S.DTYPES)
def test_per_channel_widening_every_word(dev, dn):
    """Granule<T>::widen in fake_quant.hip: the rows kernel ([8, 8192], ch_axis 0) and the generic one (the transposed view,
    ch_axis 1: inner 1) against the same call on x.float() and the oracle."""
    from outlier_suppression_amd import ops
    from oracle import fake_quant_oracle as FQ
    import _fake_quant_shapes as FS
    x = L.from_words(S.ALL_WORDS, L.DTYPES[dn], dev).view(8, 8192)
    rng = np.random.default_rng(8)
    sc = (0.0371 * rng.uniform(0.5, 2.0, 8)).astype(np.float32)
    zc = rng.integers(0, 256, 8).astype(np.int32)
    sd, zd = torch.from_numpy(sc).to(dev), torch.from_numpy(zc).to(dev)
    assert FS.predict_channel(1, 8, 8192, itemsize=2)[0] == "channel_rows" and FS.predict_channel(8192, 8, 1, itemsize=2)[0] == "channel_generic"
    _, want = FQ.fake_quantize_per_channel_affine(L.to_f32(S.ALL_WORDS, L.DTYPES[dn]).reshape(8, 8192), sc, zc, 0, 0, 255)
    for xv, ax, ref in ((x, 0, want), (x.t(), 1, want.T)):
        yh = ops.fake_quant_per_channel(xv, sd, zd, ax, 0, 255)
        yf = ops.fake_quant_per_channel(xv.float(), sd, zd, ax, 0, 255)
        assert yh.dtype == torch.float32 and yh.shape == xv.shape
        got = S.f32_words(yh.cpu().numpy())
        _same(got, S.f32_words(yf.cpu().numpy()), ("x.float()", ax), S.SENTINEL32)
        _same(got, S.f32_words(np.ascontiguousarray(ref)), ("oracle", ax), S.SENTINEL32)


# ------------------------------------------------------------------ loop edges and alignments

def _words(n, seed):
    return np.random.default_rng(seed).integers(0, 65536, n).astype(np.uint16)


@pytest.mark.parametrize("dn", S.DTYPES)
def test_chain_loop_edges_and_alignments(dev, dn):
    for n in S.CHAIN_SIZES:
        xw = _words(n, n)
        for params in S.EDGE_PARAMS:
            for x_off, y_off in S.CHAIN_ALIGN:
                run_chain(dev, dn, xw, params, x_off, y_off, tag=(n, S.param_id(params), x_off, y_off))


@pytest.mark.parametrize("dn", S.DTYPES)
def test_backward_loop_edges_and_alignments(dev, dn):
    for n in S.CHAIN_SIZES:
        xw, gw = _words(n, n), _words(n, 100000 + n)
        for params in S.EDGE_PARAMS:
            for offs in S.BACKWARD_ALIGN:
                run_backward(dev, dn, xw, gw, params, *offs, tag=(n, S.param_id(params), offs))


@pytest.mark.parametrize("dn", S.DTYPES)
def test_widen_loop_edges_and_alignments(dev, dn):
    for n in S.WIDEN_SIZES:
        xw = _words(n, n)
        for W in S.WIDEN_EDGE_MODES:
            for x_off, y_off in S.WIDEN_ALIGN:
                run_widen(dev, dn, xw, W, x_off, y_off, tag=(n, W.name, x_off, y_off))


# ------------------------------------------------------------------ capped grids: everything stays on the device

def _dev_table16(words, dev):
    return torch.from_numpy(np.ascontiguousarray(words, dtype=np.uint16).view(np.int16).copy()).to(dev)


def _index(t16):
    return t16.long() & 0xFFFF


def _draw(n, dev, seed):
    gen = torch.Generator(device=dev).manual_seed(seed)
    return torch.randint(-32768, 32768, (n,), dtype=torch.int16, device=dev, generator=gen)


def _guarded(n, dev, tdt, fill):
    buf = torch.full((S.GUARD + n + S.GUARD,), fill, dtype=tdt, device=dev)
    assert buf.data_ptr() % 16 == 0
    return buf, buf[S.GUARD:S.GUARD + n]


def _check_dev(buf, got, want, fill, tag):
    assert bool((buf[:S.GUARD] == fill).all()) and bool((buf[S.GUARD + got.numel():] == fill).all()), (tag, "a word outside the output changed")
    if not torch.equal(got, want):
        bad = torch.nonzero(got != want).reshape(-1)
        raise AssertionError((tag, "words differ", int(bad.numel()), "first", bad[:8].tolist(), got[bad[:4]].tolist(), want[bad[:4]].tolist()))


CAPPED_CHAIN = [("bf16", n) for n in S.CHAIN_CAPPED] + [("f16", S.CHAIN_CAPPED[0])]
CAPPED_BACKWARD = [("bf16", n) for n in S.BACKWARD_CAPPED] + [("f16", S.BACKWARD_CAPPED[0])]
CAPPED_WIDEN = [("bf16", n) for n in S.WIDEN_CAPPED] + [("f16", S.WIDEN_CAPPED[0])]


@pytest.mark.parametrize("dn,n", CAPPED_CHAIN)
def test_chain_capped_grid(dev, dn, n):
    _hip, lib = _lib()
    params = S.EDGE_PARAMS[0]
    t, P = S.chain_tables(dn, params), Params16(params, dev)
    assert "capped" in S.predict_chain(n).forms
    canon = _dev_table16(L.canon(S.ALL_WORDS, L.DTYPES[dn]), dev)
    x = _draw(n, dev, n % 1000)
    want = _dev_table16(t.y, dev)[_index(x)]
    first = None
    for _ in range(2):
        buf, y = _guarded(n, dev, torch.int16, _i16(t.sentinel))
        _hip.check(lib.osq_fake_quant_chain_lowp(_code(dn), x.data_ptr(), y.data_ptr(), n, P.scale.data_ptr(), P.zp.data_ptr(), P.zp_type,
                                                 t.qmin, t.qmax, _hip.stream_ptr(dev)), "fake_quant_chain_lowp")
        got = canon[_index(y)]
        _check_dev(buf, got, want, _i16(t.sentinel), (dn, n))
        assert first is None or torch.equal(got, first)
        first = got


@pytest.mark.parametrize("dn,n", CAPPED_BACKWARD)
def test_backward_capped_grid(dev, dn, n):
    _hip, lib = _lib()
    params = S.EDGE_PARAMS[0]
    t, P = S.chain_tables(dn, params), Params16(params, dev)
    p = S.predict_backward(n)
    assert "capped" in p.forms and p.first == (3, 0) and p.last == (2, 0) and p.tail
    canon = _dev_table16(L.canon(S.ALL_WORDS, L.DTYPES[dn]), dev)
    x, g = _draw(n, dev, 1), _draw(n, dev, 2)
    in_range = torch.from_numpy(t.in_range.copy()).to(dev)
    want = torch.where(in_range[_index(x)], _dev_table16(t.g, dev)[_index(g)], torch.tensor(_i16(t.zero_word), dtype=torch.int16, device=dev))
    first = None
    for _ in range(2):
        buf, dx = _guarded(n, dev, torch.int16, _i16(t.sentinel))
        _hip.check(lib.osq_fake_quant_chain_backward_lowp(_code(dn), x.data_ptr(), g.data_ptr(), dx.data_ptr(), n, P.scale.data_ptr(),
                                                          P.zp.data_ptr(), P.zp_type, t.qmin, t.qmax, _hip.stream_ptr(dev)),
                   "fake_quant_chain_backward_lowp")
        got = canon[_index(dx)]
        _check_dev(buf, got, want, _i16(t.sentinel), (dn, n))
        assert first is None or torch.equal(got, first)
        first = got


@pytest.mark.parametrize("dn,n", CAPPED_WIDEN)
def test_widen_capped_grid(dev, dn, n):
    _hip, lib = _lib()
    W = S.W_FIXED_I32
    assert "capped" in S.predict_widen(n).forms
    x = _draw(n, dev, n % 1000)
    table = torch.from_numpy(S.widen_table(dn, W).view(np.int32).copy()).to(dev)
    want = table[_index(x)]
    fill, nan = _i32(S.SENTINEL32), _i32(int(S.CANON_NAN32))
    first = None
    for _ in range(2):
        P = ParamsW(W, dev)
        buf, y = _guarded(n, dev, torch.int32, fill)
        _hip.check(lib.osq_fake_quant_per_tensor_widen(_code(dn), x.data_ptr(), y.data_ptr(), n, P.scale.data_ptr(), P.zp.data_ptr(),
                                                       P.zp_type, P.mode, float(W.g), W.qmin, W.qmax, _hip.stream_ptr(dev)),
                   "fake_quant_per_tensor_widen")
        got = torch.where(y.view(torch.float32).isnan() & (y != fill), torch.tensor(nan, dtype=torch.int32, device=dev), y)
        _check_dev(buf, got, want, fill, (dn, n))
        assert first is None or torch.equal(got, first)
        first = got
        P.check((dn, n))

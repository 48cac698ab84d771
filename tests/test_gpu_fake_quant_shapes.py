"""The forward fake-quant kernels of csrc/fake_quant.hip at every launch shape (tests/_fake_quant_shapes.py).

Every case checks three things: y (and x_quant) are WORD-equal to the oracle (oracle/fake_quant_oracle.py, NaNs canonical),
no word outside the output changed, and no word of the output was left unwritten -- the outputs sit between guard bands
pre-filled with a sentinel NaN, so the C ABI is called directly (ops allocates its own outputs).  Parameter sets: Fixed with
an int32 zero point, LSQ, LSQ+ with an fp32 zero point, and SANITIZE with a negative scale and a zero point out of range,
after which the written-back parameters are checked too.

The cases at the shipped constants run against the release library.  The test_knobs_* cases need the performance A/B knobs
as variables: they skip themselves unless the loaded library is the -DOSQ_TUNABLE build, and
tests/test_gpu_tunable_build.py runs them against libosq_hip_dbg.so in a child process."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import _fake_quant_shapes as S

pytestmark = pytest.mark.gpu
F32 = np.float32


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


class DevParams:
    """A parameter set on the device, and the check that the launch left (or repaired) it as it must."""

    def __init__(self, P, dev):
        self.P = P
        self.scale = torch.tensor([P.scale], dtype=torch.float32, device=dev)
        self.zp = torch.tensor([P.zp], dtype=torch.float32 if P.zp_float else torch.int32, device=dev)
        self.zp_type = S.ZP_FLOAT32 if P.zp_float else S.ZP_INT32
        self.mode = S.MODE_CODE[P.mode] | (S.SANITIZE if P.sanitize else 0)

    def args(self):
        P = self.P
        return (self.scale.data_ptr(), self.zp.data_ptr(), self.zp_type, self.mode, float(P.g), P.qmin, P.qmax)

    def check(self, tag):
        s, z = S.repaired(self.P)
        assert np.array_equal(S.words(self.scale.cpu().numpy()), S.words([s])), (tag, "scale after the launch")
        got = self.zp.cpu().numpy()
        assert got[0] == (z if self.P.zp_float else int(self.P.zp)) and not np.isnan(got[0]), (tag, "zero point after the launch", got)


def _place(a, dev, offset=0):
    """A device copy of the fp32 array `a` that starts `offset` bytes past a 16-byte boundary."""
    a = np.ascontiguousarray(a, dtype=F32)
    buf = torch.empty(a.size + 8, dtype=torch.float32, device=dev)
    v = buf[offset // 4:offset // 4 + a.size]
    v.copy_(torch.from_numpy(a.reshape(-1)))
    assert v.data_ptr() % 16 == offset
    return v.view(a.shape)


def _flat_positions(n, grid):
    s = grid * S.BLOCK
    return {0, 1, n - 1, 63, 64, 255, 256, s - 1, s, s + 1, n - 2}


def _pad4(vals, fill):
    vals = list(vals)
    return [fill] * (4 - len(vals)) + vals


def _i64x4(vals):
    return (ctypes.c_int64 * 4)(*vals)


def _dense_strides(sizes):
    out, acc = [], 1
    for s in reversed(sizes):
        out.append(acc)
        acc *= s
    return out[::-1]


# ------------------------------------------------------------------ launches

def run_per_tensor(dev, x_np, P, want_q, offset=0, tag=None, kernel=None, want=None):
    _hip, lib = _lib()
    n = x_np.size
    got_kernel = S.predict_per_tensor(n, aligned=offset == 0, want_q=want_q)[0]
    assert kernel is None or got_kernel == kernel, (tag, got_kernel)
    x = _place(x_np, dev, offset)
    y = S.Guarded(n, dev, offset)
    q = S.Guarded(n, dev, offset) if want_q else None
    dp = DevParams(P, dev)
    _hip.check(lib.osq_fake_quant_per_tensor(x.data_ptr(), y.ptr(), q.ptr() if q else None, n, *dp.args(), _hip.stream_ptr(dev)),
               "fake_quant_per_tensor")
    torch.cuda.synchronize()
    eq, ey = want if want is not None else S.expected(x_np, P)
    S.check_guarded(y, ey, (tag, P.name, "y"))
    if q:
        S.check_guarded(q, eq, (tag, P.name, "x_quant"))
    dp.check((tag, P.name))


def run_strided(dev, xv, logical, P, want_q, kernel, tag, headsplit=1, cap=S.FQ_CAP):
    """xv: a device view of at most 4 dims; logical: its values as a dense numpy array."""
    _hip, lib = _lib()
    sizes, xs = _pad4(xv.shape, 1), _pad4(xv.stride(), 0)
    ys = _dense_strides(sizes)
    n = int(np.prod(sizes))
    got_kernel = S.predict_strided(sizes, xs, ys, aligned=xv.data_ptr() % 16 == 0, want_q=want_q, headsplit=headsplit, cap=cap)[0]
    assert got_kernel == kernel, (tag, got_kernel)
    y = S.Guarded(n, dev)
    q = S.Guarded(n, dev) if want_q else None
    dp = DevParams(P, dev)
    _hip.check(lib.osq_fake_quant_per_tensor_strided(xv.data_ptr(), y.ptr(), q.ptr() if q else None, _i64x4(sizes), _i64x4(xs),
                                                     _i64x4(ys), *dp.args(), _hip.stream_ptr(dev)), "fake_quant_per_tensor_strided")
    torch.cuda.synchronize()
    eq, ey = S.expected(np.ascontiguousarray(logical, dtype=F32), P)
    S.check_guarded(y, ey, (tag, P.name, "y"))
    if q:
        S.check_guarded(q, eq, (tag, P.name, "x_quant"))
    dp.check((tag, P.name))
    return y


def headsplit_input(B, T, h, d, P, seed, grid=None):
    """[B, T, h, d] memory with the specials at the launch's structural positions and at the ends of every token's row."""
    n = B * T * h * d
    grid = grid or S.grid_for(n // 4, S.BLOCK * S.VEC_UNROLL, S.HEADSPLIT_CAP)
    x = S.normal_data(n, P, seed)
    S.plant(x, S.stream_positions(n, grid, S.VEC_UNROLL) | S.row_positions(B * T, h * d) | S.row_positions(B * T * h, d),
            S.repaired(P)[0])
    return x.reshape(B, T, h, d)


def run_headsplit(dev, B, T, h, d, P, seed, kernel="headsplit", headsplit=1, cap=S.FQ_CAP, grid=None):
    x_np = headsplit_input(B, T, h, d, P, seed, grid)
    x = _place(x_np, dev)
    # explicit strides: h = 1 or T = 1 must not let torch call the view contiguous
    xv = torch.as_strided(x, (B, h, T, d), (T * h * d, d, h * d, 1))
    return run_strided(dev, xv, x_np.transpose(0, 2, 1, 3), P, False, kernel, ("headsplit", B, T, h, d), headsplit, cap)


def run_multi(dev, geom, sets, seed, cap=S.FQ_CAP):
    """osq_fake_quant_headsplit_multi on len(sets) sites of one geometry; returns the payload words of every site."""
    _hip, lib = _lib()
    B, T, h, d = geom
    n = B * T * h * d
    grid = S.grid_for(n // 4, S.BLOCK * S.VEC_UNROLL, min(cap, S.HEADSPLIT_CAP) // len(sets) + 1)
    table = (_hip.HeadSplitSite * len(sets))()
    keep = []
    for i, P in enumerate(sets):
        x_np = headsplit_input(B, T, h, d, P, seed + i, grid)
        x, y, dp = _place(x_np, dev), S.Guarded(n, dev), DevParams(P, dev)
        keep.append((x_np, x, y, dp))
        e = table[i]
        e.x, e.y, e.scale, e.zero_point = x.data_ptr(), y.ptr(), dp.scale.data_ptr(), dp.zp.data_ptr()
        e.zp_type, e.mode, e.grad_factor, e.quant_min, e.quant_max = dp.zp_type, dp.mode, float(P.g), P.qmin, P.qmax
    _hip.check(lib.osq_fake_quant_headsplit_multi(table, len(sets), B, T, h, d, _hip.stream_ptr(dev)), "fake_quant_headsplit_multi")
    torch.cuda.synchronize()
    out = []
    for i, (x_np, _, y, dp) in enumerate(keep):
        tag = ("multi", geom, len(sets), i, dp.P.name)
        S.check_guarded(y, S.expected(np.ascontiguousarray(x_np.transpose(0, 2, 1, 3)), dp.P)[1], tag)
        dp.check(tag)
        out.append(y.report()[0])
    return out


def run_channel(dev, x_t, x_np, ch_axis, P, want_q, kernel, tag, offset=0):
    """x_t: contiguous device tensor (fp32 / bf16 / fp16); x_np: its values widened to fp32."""
    _hip, lib = _lib()
    code = {torch.float32: _hip.DTYPE_F32, torch.bfloat16: _hip.DTYPE_BF16, torch.float16: _hip.DTYPE_F16}[x_t.dtype]
    shape = x_np.shape
    outer, ch, inner = int(np.prod(shape[:ch_axis])), shape[ch_axis], int(np.prod(shape[ch_axis + 1:]))
    got_kernel = S.predict_channel(outer, ch, inner, x_t.element_size(), aligned=x_t.data_ptr() % 16 == 0 and offset == 0)[0]
    assert got_kernel == kernel, (tag, got_kernel)
    s, z = S.channel_params(ch, P, 77 + ch)
    s_t = torch.from_numpy(s).to(dev)
    z_t = torch.from_numpy(z if P.zp_float else z.astype(np.int32)).to(dev)
    y = S.Guarded(x_np.size, dev, offset)
    q = S.Guarded(x_np.size, dev, offset) if want_q else None
    _hip.check(lib.osq_fake_quant_per_channel(code, x_t.data_ptr(), y.ptr(), q.ptr() if q else None, outer, ch, inner,
                                              s_t.data_ptr(), z_t.data_ptr(), S.ZP_FLOAT32 if P.zp_float else S.ZP_INT32,
                                              S.MODE_CODE[P.mode], float(P.g), P.qmin, P.qmax, _hip.stream_ptr(dev)),
               "fake_quant_per_channel")
    torch.cuda.synchronize()
    eq, ey = S.expected_channel(x_np, s, z, ch_axis, P)
    S.check_guarded(y, ey, (tag, P.name, "y"))
    if q:
        S.check_guarded(q, eq, (tag, P.name, "x_quant"))
    assert np.array_equal(S.words(s_t.cpu().numpy()), S.words(s)), (tag, "per-channel scales changed")


def run_gelu(dev, x_np, P, tag):
    _hip, lib = _lib()
    n = x_np.size
    x = _place(x_np, dev)
    y = S.Guarded(n, dev)
    dp = DevParams(P, dev)
    _hip.check(lib.osq_gelu_fake_quant_per_tensor(x.data_ptr(), y.ptr(), n, *dp.args(), _hip.stream_ptr(dev)), "gelu_fake_quant_per_tensor")
    torch.cuda.synchronize()
    act = torch.nn.functional.gelu(x).cpu().numpy()             # the fused GELU is pinned bit-equal to it (test_gelu_fake_quant_fused)
    S.check_guarded(y, S.expected(act, P)[1], (tag, P.name))
    dp.check((tag, P.name))


# ------------------------------------------------------------------ at the shipped constants (release library)

@pytest.mark.parametrize("want_q", (False, True), ids=("y", "y+x_quant"))
@pytest.mark.parametrize("n", [n for n, _ in S.DENSE_SMALL])
def test_dense_vector_around_one_workgroups_trip(dev, n, want_q):
    grid = S.grid_for(n // 4, S.BLOCK * S.FQ_UNROLL, S.FQ_CAP)
    for k, P in enumerate(S.PARAM_SETS):
        x = S.per_tensor_input(n, P, 100 + k, grid, S.Q_UNROLL if want_q else S.FQ_UNROLL)
        run_per_tensor(dev, x, P, want_q, tag=("dense", n), kernel="dense_q" if want_q else "dense")


_large = {}


def _large_dense():
    if not _large:
        n = S.DENSE_LARGE
        x = S.normal_data(n, S.P_FIXED, 7)
        S.plant(x, S.stream_positions(n, S.FQ_CAP, S.FQ_UNROLL) | S.stream_positions(n, S.FQ_CAP, S.Q_UNROLL), 0.11)
        _large["x"] = x
    return _large["x"]


@pytest.mark.parametrize("want_q,P", ((False, S.P_SANITIZE), (True, S.P_FIXED)), ids=("y", "y+x_quant"))
def test_dense_vector_one_large_tensor(dev, want_q, P):
    """4 * (3 * 8192 * 256 + 300) + 3 elements: the smallest size class at which the return_quantized kernel's unrolled body
    with its write-through stores runs (its grid is sized for an unroll of 2, it unrolls 4), and at which the y-only kernel
    runs a second trip of its body.  The whole output is compared."""
    loops = S.predict_per_tensor(S.DENSE_LARGE, want_q=want_q)[1]
    assert ("body" in loops) if want_q else ("body2" in loops)
    run_per_tensor(dev, _large_dense(), P, want_q, tag="dense large", kernel="dense_q" if want_q else "dense")


@pytest.mark.parametrize("want_q", (False, True), ids=("y", "y+x_quant"))
@pytest.mark.parametrize("offset", S.SCALAR_OFFSETS)
def test_scalar_fallback_at_every_misalignment(dev, offset, want_q):
    for k, (n, _) in enumerate(S.SCALAR):
        grid = S.grid_for(n, S.BLOCK, S.MAX_BLOCKS)
        for P in ((S.MAIN_SETS[(k + offset // 4) % 4],) if n > 4096 else S.MAIN_SETS):
            x = S.plant(S.normal_data(n, P, 200 + k), _flat_positions(n, grid), S.repaired(P)[0])
            run_per_tensor(dev, x, P, want_q, offset, tag=("scalar", n, offset), kernel="scalar_q" if want_q else "scalar")


@pytest.mark.parametrize("case", range(len(S.STRIDED_SCALAR)))
def test_strided_scalar_views(dev, case):
    shape, slices, off, want_q, _ = S.STRIDED_SCALAR[case]
    for k, P in enumerate(S.MAIN_SETS[:2] if np.prod(shape) > 100000 else S.MAIN_SETS):
        base = S.normal_data(int(np.prod(shape)), P, 300 + case).reshape(shape)
        view = S.slice_view(base, slices)
        logical = view.copy()
        n = logical.size
        S.plant(logical, _flat_positions(n, S.grid_for(n, S.BLOCK, S.MAX_BLOCKS)) | S.row_positions(n // logical.shape[-1], logical.shape[-1]),
                S.repaired(P)[0])
        view[...] = logical
        xv = S.slice_view(_place(base, dev, 4 * off), slices)
        run_strided(dev, xv, logical, P, want_q, "strided_scalar_q" if want_q else "strided_scalar", ("strided scalar", case))


@pytest.mark.parametrize("case", range(len(S.STRIDED_VEC)))
def test_strided_vector_views_the_head_split_does_not_match(dev, case):
    shape, how, _ = S.STRIDED_VEC[case]
    n_base = int(np.prod(shape))
    for k, P in enumerate((S.P_FIXED,) if n_base > 1000000 else S.MAIN_SETS):
        base = S.normal_data(n_base, P, 400 + case)
        S.plant(base, S.row_positions(n_base // shape[-1], shape[-1]) | S.stream_positions(n_base, 1, 2), S.repaired(P)[0])
        base = base.reshape(shape)
        logical = S.strided_vec_view(torch.from_numpy(base), how).contiguous().numpy()
        xv = S.strided_vec_view(_place(base, dev), how)
        run_strided(dev, xv, logical, P, False, "strided_vec", ("strided vec", shape, how))


@pytest.mark.parametrize("d", S.HEAD_D)
def test_head_split_geometries(dev, d):
    for k, (h, T, B) in enumerate(itertools.product(S.HEAD_H, S.HEAD_T, S.HEAD_B)):
        run_headsplit(dev, B, T, h, d, S.MAIN_SETS[(k + d // 4) % 4], 500 + k)


def test_head_split_one_large_tensor(dev):
    B, T, h, d = S.HEADSPLIT_LARGE
    assert {"body2", "capped", "rem_after_body"} <= S.predict_strided([B, h, T, d], [T * h * d, d, h * d, 1], [h * T * d, T * d, d, 1])[1]
    run_headsplit(dev, B, T, h, d, S.P_LSQPLUS, 6)


@pytest.mark.parametrize("geom", [(1, 5, 3, 8), (3, 37, 12, 64), (2, 128, 16, 32), (1, 1, 1, 4), (3, 7, 1, 256)])
def test_key_layout_through_ops(dev, geom):
    """The [B, h, d, T] view of the key: ops.fake_quant_per_tensor quantises its transpose through the head split."""
    from outlier_suppression_amd import ops
    B, T, h, d = geom
    for P in S.MAIN_SETS:
        x_np = headsplit_input(B, T, h, d, P, 600)
        dp = DevParams(P, dev)
        key = _place(x_np, dev).permute(0, 2, 3, 1)
        y = ops.fake_quant_per_tensor(key, dp.scale, dp.zp, P.qmin, P.qmax, dp.mode, P.g)
        assert tuple(y.shape) == (B, h, d, T)
        want = S.expected(np.ascontiguousarray(x_np.transpose(0, 2, 3, 1)), P)[1]
        assert np.array_equal(S.words(y.contiguous().cpu().numpy()), S.words(want)), (geom, P.name)
        dp.check((geom, P.name))


_SITE_SETS = (S.P_SANITIZE, S.P_FIXED, S.P_LSQPLUS, S.P_LSQ)


@pytest.mark.parametrize("n_sites", (1, 2, 3, 4))
def test_head_split_of_several_sites(dev, n_sites):
    for geom in S.HEADSPLIT_MULTI:
        sets = _SITE_SETS[:n_sites]
        got = run_multi(dev, geom, sets, 700)
        B, T, h, d = geom
        grid = S.grid_for(B * T * h * d // 4, S.BLOCK * S.VEC_UNROLL, S.HEADSPLIT_CAP // n_sites + 1)
        for i, P in enumerate(sets):                  # every site equals its own single-site launch on the same input
            y = run_headsplit(dev, B, T, h, d, P, 700 + i, grid=grid)
            assert np.array_equal(y.report()[0], got[i]), (geom, n_sites, i)


def _rows_input(shape, ch_axis, P, seed, dtype):
    n = int(np.prod(shape))
    inner = int(np.prod(shape[ch_axis + 1:]))
    x = S.normal_data(n, P, seed)
    S.plant(x, S.row_positions(n // inner, inner) | {1, 2, 3, inner // 2}, P.scale)
    t = torch.from_numpy(x.reshape(shape)).to(dtype)
    return t, t.float().numpy()                       # the 16-bit inputs are widened exactly


@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16, torch.float16), ids=("fp32", "bf16", "fp16"))
def test_per_channel_rows(dev, dtype):
    itemsize = 4 if dtype == torch.float32 else 2
    k = 0
    for ig, (outer, ch) in itertools.product(S.ROWS_INNER_G[itemsize], S.ROWS_LAYOUTS):
        P = (S.P_FIXED, S.P_LSQ, S.P_LSQPLUS)[k % 3]
        k += 1
        shape, ax = ((ch, ig * S.GRANULE[itemsize]), 0) if outer == 1 else ((outer, ch, ig * S.GRANULE[itemsize]), 1)
        t, x_np = _rows_input(shape, ax, P, 800 + k, dtype)
        for want_q in ((False, True) if itemsize == 4 else (False,)):
            run_channel(dev, t.to(dev), x_np, ax, P, want_q, "channel_rows", ("rows", shape, str(dtype), want_q))


@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16), ids=("fp32", "bf16"))
def test_per_channel_rows_second_trip(dev, dtype):
    outer, ch, inner = S.ROWS_TRIP2
    assert "row_trip2" in S.predict_channel(outer, ch, inner, 4 if dtype == torch.float32 else 2)[1]
    t, x_np = _rows_input((ch, inner), 0, S.P_LSQPLUS, 850, dtype)
    run_channel(dev, t.to(dev), x_np, 0, S.P_LSQPLUS, dtype == torch.float32, "channel_rows", ("rows trip2", str(dtype)))


@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16, torch.float16), ids=("fp32", "bf16", "fp16"))
def test_per_channel_generic(dev, dtype):
    for k, (shape, ax, off, _) in enumerate(S.GENERIC):
        if off and dtype != torch.float32:
            continue                                 # the misaligned base is an fp32 case (any inner that is no granule is generic anyway)
        P = (S.P_FIXED, S.P_LSQ, S.P_LSQPLUS)[k % 3]
        t, x_np = _rows_input(shape, ax, P, 900 + k, dtype)
        x_t = _place(x_np, dev, 4 * off).view(shape) if off else t.to(dev)
        for want_q in ((False, True) if dtype == torch.float32 and np.prod(shape) < 100000 else (False,)):
            run_channel(dev, x_t, x_np, ax, P, want_q, "channel_generic", ("generic", shape, str(dtype), want_q))


@pytest.mark.parametrize("n", [n for n, _ in S.GELU])
def test_gelu_form_with_every_tail(dev, n):
    grid = S.grid_for(max(n // 4, 1), S.BLOCK * S.VEC_UNROLL, S.FQ_CAP)
    for k, P in enumerate(S.MAIN_SETS):
        x = S.per_tensor_input(n, P._replace(sigma=1.5), 1000 + k, grid, S.VEC_UNROLL)
        run_gelu(dev, x, P, ("gelu", n))


# ------------------------------------------------------------------ on the tunable library: the other instantiations

_DEFAULTS = (("fq_unroll", 2), ("fq_max_blocks", 8192), ("fq_nt", 5), ("stream_wt", 1), ("fq_headsplit", 1))


def _need_tunable():
    from outlier_suppression_amd import ops
    if not ops.tunable_build():
        pytest.skip("the fake-quant A/B knobs are compile-time constants in the release library; "
                    "tests/test_gpu_tunable_build.py runs this test against libosq_hip_dbg.so in a child process")
    return ops


def _restore(ops):
    for key, value in _DEFAULTS:
        ops.set_tuning(key, value)


def _knob_inputs(blocks, unroll):
    """(n, x) per size of knob_sizes x tails (0, 3): at most about 60 K elements each."""
    out = []
    for n4, tail in itertools.product(S.knob_sizes(blocks, unroll), (0, 3)):
        n = 4 * n4 + tail
        if n:
            assert n <= 62000
            pos = S.stream_positions(n, blocks, unroll) | S.stream_positions(n, blocks, S.Q_UNROLL) | S.stream_positions(n, blocks, 2)
            out.append((n, S.plant(S.normal_data(n, S.P_FIXED, n), pos, 0.11)))
    return out


@pytest.mark.parametrize("unroll", (2, 4, 8))
@pytest.mark.parametrize("blocks", (1, 2, 3))
def test_knobs_dense_instantiations(dev, blocks, unroll):
    """fq_max_blocks x fq_unroll x fq_nt: every instantiation of the dense kernel, y-only and return_quantized, gives the
    oracle's words at sizes around every trip of a grid of `blocks` workgroups."""
    ops = _need_tunable()
    inputs = _knob_inputs(blocks, unroll)
    wants = [S.expected(x, S.P_FIXED) for _, x in inputs]
    wants_s = [S.expected(x, S.P_SANITIZE) for _, x in inputs]
    try:
        ops.set_tuning("fq_max_blocks", blocks)
        ops.set_tuning("fq_unroll", unroll)
        for nt in range(6):
            ops.set_tuning("fq_nt", nt)
            for (n, x), want, want_s in zip(inputs, wants, wants_s):
                for want_q in (False, True):
                    P, w = ((S.P_FIXED, want), (S.P_SANITIZE, want_s))[(nt + want_q) % 2]
                    run_per_tensor(dev, x, P, want_q, tag=("knobs dense", blocks, unroll, nt, n, want_q), want=w)
    finally:
        _restore(ops)


def _geoms_for(n4s):
    """Head-split geometries of about n4 float4 each: d = 4, h = 1 gives any n4 exactly; d = 8, h = 3 rounds it up."""
    out = []
    for n4 in n4s:
        if n4:
            out.append((1, n4, 1, 4))
            out.append((1, -(-n4 // 6), 3, 8))
    return out


@pytest.mark.parametrize("blocks", (1, 2, 3))
def test_knobs_head_split_strided_vector_and_gelu(dev, blocks):
    """fq_max_blocks x fq_nt for the head split, the head split of 2 sites and the strided-vector kernel, and
    fq_max_blocks x stream_wt for the GELU form, at sizes around every trip of the capped grid (these kernels unroll 2)."""
    ops = _need_tunable()
    sizes = S.knob_sizes(blocks, 2)
    try:
        ops.set_tuning("fq_max_blocks", blocks)
        for nt in range(6):
            ops.set_tuning("fq_nt", nt)
            for k, geom in enumerate(_geoms_for(sizes)):
                B, T, h, d = geom
                P = S.MAIN_SETS[(k + nt) % 4]
                run_headsplit(dev, B, T, h, d, P, 1100 + k, cap=blocks, grid=blocks)
                run_multi(dev, geom, (S.P_SANITIZE, P), 1200 + k, cap=blocks)
        for k, n4 in enumerate(s for s in sizes if s):           # strided vector: every other float4 of a [1, 2 n4, 1, 4] buffer
            P = S.MAIN_SETS[k % 4]
            base = S.plant(S.normal_data(8 * n4, P, 1300 + k), S.stream_positions(8 * n4, 2 * blocks, 2), S.repaired(P)[0]).reshape(1, 2 * n4, 1, 4)
            run_strided(dev, _place(base, dev)[:, ::2], base[:, ::2], P, False, "strided_vec", ("knobs strided vec", blocks, n4), cap=blocks)
        for wt in (0, 1):
            ops.set_tuning("stream_wt", wt)
            for k, (n4, tail) in enumerate(itertools.product(sizes, (0, 3))):
                if 4 * n4 + tail:
                    P = S.MAIN_SETS[(k + wt) % 4]
                    x = S.per_tensor_input(4 * n4 + tail, P._replace(sigma=1.5), 1400 + k, blocks, 2)
                    run_gelu(dev, x, P, ("knobs gelu", blocks, wt, n4, tail))
    finally:
        _restore(ops)


def test_knobs_head_split_off_gives_the_same_words(dev):
    """fq_headsplit = 0: the head-split geometries run the strided-vector kernel and give the same words ("A/B; results are
    equal" of the knob's comment)."""
    ops = _need_tunable()
    geoms = [(B, T, h, d) for k, (d, h, T, B) in enumerate(itertools.product(S.HEAD_D, S.HEAD_H, S.HEAD_T, S.HEAD_B)) if k % 5 == 0]
    try:
        for k, (B, T, h, d) in enumerate(geoms):
            P = S.MAIN_SETS[k % 4]
            ops.set_tuning("fq_headsplit", 1)
            on = run_headsplit(dev, B, T, h, d, P, 1500 + k).report()[0]
            ops.set_tuning("fq_headsplit", 0)
            off = run_headsplit(dev, B, T, h, d, P, 1500 + k, kernel="strided_vec", headsplit=0).report()[0]
            assert np.array_equal(on, off), (B, T, h, d)
    finally:
        _restore(ops)

"""bf16 / fp16 inputs on the device: the in-dtype chain of FixedFakeQuantize per-tensor (forward and backward) against the
reference's words (tests/golden/lowp.npz) and the host emulation (tests/_lowp_chain.py); the rows that promote to fp32 and
every observer against the same call on x.float(); sizes, alignments, layouts; a deferred-observation block with a half
site.  16-bit results are compared as words, NaN equal to NaN whatever its payload."""
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import _lowp_chain as L

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DTYPES = sorted(L.DTYPES)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(HERE, "golden", "lowp.npz"))


def _qrange(bit, symmetric):
    return (-(1 << (bit - 1)), (1 << (bit - 1)) - 1) if symmetric else (0, (1 << bit) - 1)


def _same_words(a, b, dtype):
    np.testing.assert_array_equal(L.canon(a, dtype), L.canon(b, dtype))


def _same_f32(a, b):
    a = torch.as_tensor(a).detach().cpu().float().numpy().reshape(-1)
    b = torch.as_tensor(b).detach().cpu().float().numpy().reshape(-1)
    assert a.shape == b.shape
    nan = np.isnan(a)
    assert np.array_equal(nan, np.isnan(b))
    np.testing.assert_array_equal(a[~nan].view(np.uint32), b[~nan].view(np.uint32))


def _case(fx, ci):
    bit, sym, s, zp, fz = fx["chain_cases"][ci]
    zp = float(zp) if fz else int(zp)
    return (float(s), zp) + _qrange(int(bit), int(sym))


# ------------------------------------------------------------------ the in-dtype chain

@pytest.mark.parametrize("dn", DTYPES)
def test_chain_forward_backward_equal_reference(dev, fx, dn):
    from outlier_suppression_amd.quantization import util_quant as UQ
    dt = L.DTYPES[dn]
    xw, gw = fx[f"x_{dn}"], fx[f"gy_{dn}"]
    for ci in range(len(fx["chain_cases"])):
        s, zp, qmin, qmax = _case(fx, ci)
        x = L.from_words(xw, dt, dev).requires_grad_(True)
        y = UQ.fake_quantize_per_tensor_affine(x, s, zp, qmin, qmax)
        assert y.dtype == dt
        y.backward(L.from_words(gw, dt, dev))
        _same_words(L.tensor_words(y), fx[f"chain_{dn}_{ci}_y"], dt)
        _same_words(L.tensor_words(x.grad), fx[f"chain_{dn}_{ci}_dx"], dt)
        # 0-dim tensor parameters take the same form
        y0 = UQ.fake_quantize_per_tensor_affine(x.detach(), torch.tensor(s, device=dev),
                                                torch.tensor(zp, device=dev), qmin, qmax)
        assert y0.dtype == dt
        _same_words(L.tensor_words(y0), fx[f"chain_{dn}_{ci}_y"], dt)


@pytest.mark.parametrize("dn", DTYPES)
def test_promoted_rows_equal_reference(dev, fx, dn):
    from outlier_suppression_amd.quantization import util_quant as UQ
    dt = L.DTYPES[dn]
    x = L.from_words(fx[f"x_{dn}"], dt, dev)
    for ci in range(len(fx["chain_cases"])):
        s, zp, qmin, qmax = _case(fx, ci)
        zt = torch.tensor([zp], dtype=torch.float32 if isinstance(zp, float) else torch.int32, device=dev)
        y = UQ.fake_quantize_per_tensor_affine(x, torch.tensor([s], device=dev), zt, qmin, qmax)
        assert y.dtype == torch.float32
        _same_f32(y, fx[f"prom_{dn}_{ci}_y"])
    w = L.from_words(fx[f"chan_{dn}_x"], dt, dev)
    sc = torch.from_numpy(fx[f"chan_{dn}_scale"]).to(dev)
    zc = torch.from_numpy(fx[f"chan_{dn}_zp"]).to(dev)
    yc = UQ.fake_quantize_per_channel_affine(w, sc, zc, 0, 0, 255)
    assert yc.dtype == torch.float32
    _same_f32(yc, fx[f"chan_{dn}_y"])


@pytest.mark.parametrize("dn", DTYPES)
def test_learnable_rows_equal_reference_and_float_call(dev, fx, dn, sum_tier):
    from outlier_suppression_amd.quantization import util_quant as UQ
    dt = L.DTYPES[dn]
    xh = L.from_words(fx[f"lsq_{dn}_x"], dt, dev)
    gy = torch.from_numpy(fx[f"lsq_{dn}_gy"]).to(dev)
    fns = {("lsq", False): UQ.fake_quantize_learnable_per_tensor_affine_training,
           ("lsq", True): UQ.fake_quantize_learnable_per_channel_affine_training,
           ("lsqp", False): UQ.fake_quantize_learnableplus_per_tensor_affine_training,
           ("lsqp", True): UQ.fake_quantize_learnableplus_per_channel_affine_training}
    for (kind, per_ch), fn in fns.items():
        key = f"{kind}_{dn}_{'ch' if per_ch else 'pt'}"
        bit, sym = (4, True) if kind == "lsq" else (5, False)
        qmin, qmax = _qrange(bit, sym)
        gf = float(fx[key + "_gf"])
        runs = []
        for x0 in (xh, xh.float()):
            s = torch.from_numpy(fx[key + "_scale"]).to(dev).requires_grad_(True)
            z = torch.from_numpy(fx[key + "_zp"]).to(dev)
            if kind == "lsqp":
                z.requires_grad_(True)
            x = x0.clone().requires_grad_(True)
            args = (x, s, z, 0, qmin, qmax, gf) if per_ch else (x, s, z, qmin, qmax, gf)
            y = fn(*args)
            assert y.dtype == torch.float32
            y.backward(gy)
            runs.append((y, x.grad, s.grad, z.grad if kind == "lsqp" else None))
        (yh, dxh, dsh, dzh), (yf, dxf, dsf, dzf) = runs
        assert dxh.dtype == dt
        _same_f32(yh, yf)
        _same_f32(yh, fx[key + "_y"])
        _same_words(L.tensor_words(dxh), L.tensor_words(dxf.to(dt)), dt)
        _same_words(L.tensor_words(dxh), fx[key + "_dx"], dt)
        _same_f32(dsh, dsf)
        np.testing.assert_allclose(dsh.cpu().numpy(), fx[key + "_ds"], rtol=2e-5, atol=1e-7)
        if kind == "lsqp":
            _same_f32(dzh, dzf)
            np.testing.assert_allclose(dzh.cpu().numpy(), fx[key + "_dz"], rtol=2e-5, atol=1e-7)


def _quantizer(dev, quantizer, observer, bit=8, symmetric=False, ch_axis=-1, name="encoder.layer.0.x_post_act_fake_quantize"):
    from outlier_suppression_amd.quantization import Quantizer
    q = Quantizer(None, NS(quantizer=quantizer, observer=observer, bit=bit, symmetric=symmetric, ch_axis=ch_axis)).to(dev)
    q.observer.set_name(name + ".observer")
    if hasattr(q.observer, "set_percentile"):
        q.observer.set_percentile(0.95)
    return q


@pytest.mark.parametrize("dn", DTYPES)
def test_module_output_dtypes(dev, dn):
    dt = L.DTYPES[dn]
    gen = torch.Generator().manual_seed(5)
    x = (torch.randn(4, 16, 64, generator=gen) * 3).to(dt).to(dev)
    for quantizer, ch_axis, expect in (("FixedFakeQuantize", -1, dt), ("FixedFakeQuantize", 2, torch.float32),
                                       ("LSQFakeQuantize", -1, torch.float32), ("LSQPlusFakeQuantize", -1, torch.float32)):
        q = _quantizer(dev, quantizer, "MinMaxObserver", ch_axis=ch_axis)
        q.enable_observer()
        q.enable_fake_quant()
        y = q(x)
        assert y.dtype == expect, (quantizer, ch_axis, y.dtype)
        q.disable_observer()
        xr = x.clone().requires_grad_(True)
        y = q(xr)
        assert y.dtype == expect
        y.float().sum().backward()
        assert xr.grad.dtype == dt
        # the float call of the promoted rows: the same numbers
        qf = _quantizer(dev, quantizer, "MinMaxObserver", ch_axis=ch_axis)
        qf.load_state_dict(q.state_dict())
        qf.disable_observer()
        qf.enable_fake_quant()
        if expect == torch.float32:
            _same_f32(q(x), qf(x.float()))
        else:
            s, zp = float(q.scale.item()), int(q.zero_point.item())
            _same_words(L.tensor_words(q(x)), L.chain_forward(L.tensor_words(x), dt, s, zp, q.quant_min, q.quant_max), dt)


# ------------------------------------------------------------------ observers

OBSERVERS = ["MinMaxObserver", "AvgMinMaxObserver", "AvgPruneMinMaxObserver", "MSEFastObserver", "AvgMSEFastObserver",
             "AvgQuantileObserver", "MSEObserver", "AvgMSEObserver", "LSQPlusObserver"]


def _observer_batches(dn, dev, fx):
    dt = L.DTYPES[dn]
    xs1 = [L.from_words(w, dt, dev) for w in fx[f"obs_{dn}_x1"]]
    xs2 = [L.from_words(w, dt, dev) for w in fx[f"obs_{dn}_x2"]]
    lens = [torch.from_numpy(v).to(dev) for v in fx[f"obs_{dn}_lens"]]
    return xs1, xs2, lens


def _state(q):
    o = q.observer
    return [o.min_val.clone(), o.max_val.clone(), q.scale.clone(), q.zero_point.clone()]


@pytest.mark.parametrize("dn", DTYPES)
@pytest.mark.parametrize("name", OBSERVERS)
def test_observers_equal_float_observation(dev, fx, dn, name):
    xs1, xs2, lens = _observer_batches(dn, dev, fx)
    shape = list(xs1[0].shape)
    sites = ["flat", "tok1", "tok2"]
    if name == "MinMaxObserver":
        sites.append("chan")
    if name == "LSQPlusObserver":
        sites = ["flat", "chan"]
    for sym in ((True,) if name == "LSQPlusObserver" else (False, True)):
        for site in sites:
            ch_axis = 0 if site == "chan" else -1
            qh = _quantizer(dev, "FixedFakeQuantize", name, symmetric=sym, ch_axis=ch_axis)
            qf = _quantizer(dev, "FixedFakeQuantize", name, symmetric=sym, ch_axis=ch_axis)
            for q in (qh, qf):
                q.enable_observer()
            for b in range(3):
                for q, conv in ((qh, lambda t: t), (qf, lambda t: t.float())):
                    if site == "flat":
                        q(conv(xs1[b]))
                    elif site == "chan":
                        q(conv(xs1[b].reshape(-1, shape[-1]).t().contiguous()))
                    else:
                        sp = 1 if site == "tok1" else 2
                        q(conv(xs1[b] if sp == 1 else xs2[b]), lens[b], sp)
                for a, c in zip(_state(qh), _state(qf)):
                    _same_f32(a, c)
                key = f"obs_{dn}_{name}_{int(sym)}_{site}"
                if key in fx.files:   # the reference's own statistics and parameters after this batch
                    ref = fx[key][b]
                    st = _state(qh)
                    for k in range(4):
                        np.testing.assert_array_equal(st[k].float().cpu().numpy().reshape(-1), ref[k], err_msg=f"{key} {b} {k}")


# ------------------------------------------------------------------ sizes and layouts

def _fixed_params(dev, s=0.0371, zp=128):
    return torch.tensor([s], device=dev), torch.tensor([zp], dtype=torch.int32, device=dev)


def _check_chain(x, s, zp, qmin=0, qmax=255):
    from outlier_suppression_amd import ops
    dt = x.dtype
    sc, zt = torch.tensor([s], device=x.device), torch.tensor([zp], dtype=torch.int32, device=x.device)
    y = ops.fake_quant(x, sc, zt, -1, qmin, qmax, scalar_params=True)
    assert y.dtype == dt and y.shape == x.shape
    xw = L.tensor_words(x)
    _same_words(L.tensor_words(y), L.chain_forward(xw, dt, s, zp, qmin, qmax), dt)
    g = torch.randn(x.shape, generator=torch.Generator().manual_seed(x.numel())).to(dt).to(x.device)
    xr = x.detach().requires_grad_(True)
    dx = torch.autograd.grad(ops.fake_quant(xr, sc, zt, -1, qmin, qmax, scalar_params=True), xr, g)[0]
    _same_words(L.tensor_words(dx), L.chain_backward(xw, L.tensor_words(g), dt, s, zp, qmin, qmax), dt)
    # promoted rows and the flat observation against the fp32 kernels on x.float()
    for mode in (ops.PARAM_FIXED, ops.PARAM_LSQPLUS):
        zf = zt.float() if mode == ops.PARAM_LSQPLUS else zt
        _same_f32(ops.fake_quant(x, sc, zf, -1, qmin, qmax, mode, 0.01), ops.fake_quant(x.float(), sc, zf, -1, qmin, qmax, mode, 0.01))
    if x.numel():
        st = [torch.full((), v, device=x.device) for v in (float("inf"), float("-inf"), float("inf"), float("-inf"))]
        cur = torch.empty(4, device=x.device)
        ops.observe_flat(x, ops.UPDATE_RUNNING, 0, st[0], st[1], qmin, qmax, False, None, cur[:2])
        ops.observe_flat(x.float(), ops.UPDATE_RUNNING, 0, st[2], st[3], qmin, qmax, False, None, cur[2:])
        _same_f32(cur[:2], cur[2:])


@pytest.mark.parametrize("dn", DTYPES)
def test_sizes_alignment_layouts(dev, dn):
    dt = L.DTYPES[dn]
    gen = torch.Generator().manual_seed(11)
    for n in (0, 1, 7, 8, 9, 8 * 1000 + 3, (1 << 20) + 5):
        x = (torch.randn(n, generator=gen) * 4).to(dt).to(dev)
        _check_chain(x, 0.0371, 128)
    base = (torch.randn(8 * 999 + 1, generator=gen) * 4).to(dt).to(dev)
    _check_chain(base[1:], 0.05, 3)                                       # 2-byte offset: misaligned for 16-byte accesses
    t = (torch.randn(6, 10, 24, generator=gen) * 4).to(dt).to(dev)
    _check_chain(t.permute(2, 0, 1), 0.0371, 128)                         # dense, permuted
    _check_chain(t[:, ::2, :5], 0.0371, 128)                              # not dense: one contiguous copy first
    _check_chain((torch.randn(2, 3, 5, 16, generator=gen) * 4).to(dt).to(dev), 0.25, 7)
    _check_chain((torch.randn(2, 3, 4, 5, 8, generator=gen) * 4).to(dt).to(dev), 0.125, 100)
    # per-channel widening and per-channel / masked observation on views
    from outlier_suppression_amd import ops
    w = (torch.randn(48, 72, generator=gen) * 2).to(dt).to(dev)
    sc = torch.rand(48, generator=gen).to(dev) * 0.05 + 0.005
    zc = torch.randint(0, 256, (48,), generator=gen, dtype=torch.int32).to(dev)
    for ww, ax in ((w, 0), (w.t(), 1), (w[:, 1:], 0)):
        _same_f32(ops.fake_quant(ww, sc, zc, ax, 0, 255), ops.fake_quant(ww.float(), sc, zc, ax, 0, 255))
        # per-channel observation: (w, 0) takes the row kernel, the two views the generic one
        got = []
        for xx in (ww, ww.float()):
            st = [torch.full((48,), float("inf"), device=dev), torch.full((48,), float("-inf"), device=dev),
                  torch.empty(48, device=dev), torch.empty(48, dtype=torch.int32, device=dev)]
            ops.observe_channels(xx, ax, ops.UPDATE_RUNNING, 0, st[0], st[1], 0, 255, False, ops.QParamSink(st[2], st[3]))
            got.append(st)
        for h, f in zip(*got):
            _same_f32(h, f)
    a = (torch.randn(5, 9, 40, generator=gen) * 3).to(dt).to(dev)
    lens = torch.tensor([9, 3, 1, 7, 5], device=dev)
    for v, sp in ((a, 1), (a.permute(0, 2, 1), 2), (a[:, :, 1:], 1)):
        n = v.shape[0] * v.shape[sp]
        oh = (torch.empty(n, device=dev), torch.empty(n, device=dev))
        of = (torch.empty(n, device=dev), torch.empty(n, device=dev))
        ops.token_minmax(v, sp, lens, out=oh)
        ops.token_minmax(v.float(), sp, lens, out=of)
        valid = (torch.arange(v.shape[sp], device=dev)[None, :] < lens[:, None]).reshape(-1)
        _same_f32(oh[0][valid], of[0][valid])
        _same_f32(oh[1][valid], of[1][valid])
        # masked token observation behind one call: inner width 40 takes the 16-byte path for both element sizes, the
        # [:, :, 1:] view the generic one
        for prune in (False, True):
            got = []
            for xx in (v, v.float()):
                st = [torch.full((), float("inf"), device=dev), torch.full((), float("-inf"), device=dev),
                      torch.empty(2, device=dev), torch.empty(1, device=dev), torch.empty(1, device=dev)]
                ops.observe_tokens(xx, sp, lens, prune, 0.9, ops.UPDATE_AVERAGE, 0, st[0], st[1], 0, 255, False,
                                   ops.QParamSink(st[3], st[4]), st[2])
                got.append(st)
            for h, f in zip(*got):
                _same_f32(h, f)


@pytest.mark.parametrize("dn", ["bf16"])
def test_headline_shape_chain(dev, dn):
    dt = L.DTYPES[dn]
    gen = torch.Generator().manual_seed(3)
    x = (torch.randn(256, 128, 768, generator=gen) * 3).to(dt)
    x[..., 7] *= 30
    xd = x.to(dev)
    from outlier_suppression_amd import ops
    y = ops.fake_quant(xd, *_fixed_params(dev, 0.0413, 121), -1, 0, 255, scalar_params=True)
    _same_words(L.tensor_words(y), L.chain_forward(L.tensor_words(x), dt, 0.0413, 121, 0, 255), dt)


@pytest.mark.parametrize("dn", DTYPES)
def test_deferred_block_runs_half_sites_at_once(dev, dn):
    from outlier_suppression_amd.quantization.deferred import deferred_observation
    dt = L.DTYPES[dn]
    gen = torch.Generator().manual_seed(8)
    xs = [(torch.randn(4, 20, 64, generator=gen) * (i + 1)).to(dt).to(dev) for i in range(3)]
    lens = torch.tensor([20, 13, 1, 7], device=dev)
    qd = _quantizer(dev, "LSQPlusFakeQuantize", "AvgPruneMinMaxObserver")
    qr = _quantizer(dev, "LSQPlusFakeQuantize", "AvgPruneMinMaxObserver")
    for q in (qd, qr):
        q.enable_observer()
        q.disable_fake_quant()
    with deferred_observation() as sites:
        for x in xs:
            qd(x, lens, 1)
            assert not sites.sites          # a half site is never recorded: it ran at once
            sites.flush()
    for x in xs:
        qr(x.float(), lens, 1)
    for a, c in zip(_state(qd), _state(qr)):
        _same_f32(a, c)

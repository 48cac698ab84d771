#!/usr/bin/env python3
"""Golden vectors of bf16 / fp16 inputs (tests/golden/lowp.npz) by RUNNING THE REFERENCE on the CPU, one thread.

Imports the reference's ``quant_transformer.quantization`` unmodified with the same process-local shims as make_golden.py
(empty ``seaborn`` module, ``.cuda()`` = identity).  Outputs are DATA ONLY.  numpy has no bfloat16: every 16-bit tensor is
stored as its uint16 words (``t.view(torch.int16)``); fp32 results as float32.

  chain_*     util_quant.fake_quantize_per_tensor_affine with Python numbers (FixedFakeQuantize per-tensor): y and, for a
              16-bit upstream gradient, dx -- both in x.dtype
  prom_*      the same call with [1] tensors (fp32 result) -- equal to the call on x.float()
  chan_*      fake_quantize_per_channel_affine, [C] parameters (fp32 result)
  lsq_* / lsqp_*  learnable per-tensor and per-channel: y (fp32), dx words, ds, dzp for a random fp32 upstream gradient
  obs_*       MinMax / AvgMinMax / AvgPruneMinMax over three batches: (min_val, max_val, scale, zero_point) after each,
              flat, per-channel and masked at seq_pos 1 ([B, T, H]) and 2 ([B, h, T, d]) with ragged lengths
Re-run:  python tests/golden/make_golden_lowp.py
"""
import os
import sys
import types

import numpy as np
import torch

REF = os.environ.get("OSQ_REFERENCE", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))


def _import_reference():
    sys.modules.setdefault("seaborn", types.ModuleType("seaborn"))
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.nn.Module.cuda = lambda self, *a, **k: self
    sys.path.insert(0, REF)
    from quant_transformer.quantization import observer, util_quant
    return observer, util_quant


O, U = _import_reference()
torch.set_num_threads(1)

DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
# (bit, symmetric, scale, zero point): scales exactly representable and not; 0.25 gives exact .5 quotients; 0.01 makes
# fp16 x/s overflow for |x| > 655; float zero points as util_quant accepts them
CHAIN_CASES = [(8, False, 0.0371, 128), (8, True, 0.05, 0), (4, False, 0.25, 7), (4, True, 0.25, 0),
               (2, False, 0.5, 1), (6, False, 0.01, 30), (5, True, 0.125, 0), (8, False, 0.0371, 127.5),
               (3, False, 0.3, 2.25)]


def words(t):
    return t.detach().contiguous().view(torch.int16).numpy().view(np.uint16)


def qrange(bit, symmetric):
    return (-(1 << (bit - 1)), (1 << (bit - 1)) - 1) if symmetric else (0, (1 << bit) - 1)


def edge_values(dtype):
    fi = torch.finfo(dtype)
    sub = fi.tiny / 8                                        # a subnormal of this dtype
    vals = [0.0, -0.0, float("inf"), float("-inf"), float("nan"), fi.tiny, -fi.tiny, sub, -sub, fi.tiny / 2 ** (fi.bits - 9),
            fi.max, -fi.max, 60000.0, -60000.0, 700.0, -700.0]
    vals += [(k + 0.5) * 0.25 for k in range(-12, 12)]       # exact .5 quotients for s = 0.25
    vals += [(k + 0.5) * 0.125 for k in range(-8, 8)]
    return torch.tensor(vals, dtype=torch.float32).to(dtype)


def sample(gen, n, dtype):
    x = torch.randn(n, generator=gen) * 3.0
    x[: n // 8] *= 40.0                                      # outliers beyond the clip range
    x[n // 8: n // 4] *= 1e-3                                # values that round to zero
    return torch.cat([edge_values(dtype), x.to(dtype)])


def main():
    g = torch.Generator().manual_seed(2026)
    out = {}
    for dn, dt in DTYPES.items():
        x = sample(g, 4000, dt)
        gy = (torch.randn(x.numel(), generator=g) * 2.0).to(dt)
        out[f"x_{dn}"] = words(x)
        out[f"gy_{dn}"] = words(gy)
        for ci, (bit, sym, s, zp) in enumerate(CHAIN_CASES):
            qmin, qmax = qrange(bit, sym)
            xr = x.clone().requires_grad_(True)
            y = U.fake_quantize_per_tensor_affine(xr, s, zp, qmin, qmax)
            assert y.dtype == dt
            y.backward(gy)
            out[f"chain_{dn}_{ci}_y"] = words(y)
            out[f"chain_{dn}_{ci}_dx"] = words(xr.grad)
            # [1] tensor parameters: promoted to fp32
            zpt = torch.tensor([zp], dtype=torch.float32 if isinstance(zp, float) else torch.int32)
            yp = U.fake_quantize_per_tensor_affine(x, torch.tensor([s], dtype=torch.float32), zpt, qmin, qmax)
            assert yp.dtype == torch.float32
            out[f"prom_{dn}_{ci}_y"] = yp.numpy()
        out["chain_cases"] = np.array([[b, int(sm), s, float(z), int(isinstance(z, float))] for b, sm, s, z in CHAIN_CASES],
                                      dtype=np.float64)

        # per-channel Fixed: [C, K] weight, [C] parameters
        C, K = 24, 40
        w = (torch.randn(C, K, generator=g) * torch.linspace(0.1, 4.0, C)[:, None]).to(dt)
        w[0, :5] = edge_values(dt)[:5]
        sc = (torch.rand(C, generator=g) * 0.05 + 0.005)
        zc = torch.randint(0, 256, (C,), generator=g, dtype=torch.int32)
        out[f"chan_{dn}_x"] = words(w)
        out[f"chan_{dn}_scale"] = sc.numpy()
        out[f"chan_{dn}_zp"] = zc.numpy()
        yc = U.fake_quantize_per_channel_affine(w, sc, zc, 0, 0, 255)
        assert yc.dtype == torch.float32
        out[f"chan_{dn}_y"] = yc.numpy()

        # learnable rows: per-tensor [B, T, H] and per-channel [C, K]
        xl = (torch.randn(10, 300, generator=g) * 3.0).to(dt)      # finite: ds / dzp are sums over every element
        xl[0, :4] = torch.tensor([0.0, -0.0, torch.finfo(dt).tiny / 8, 700.0]).to(dt)
        gl = torch.randn(10, 300, generator=g)
        out[f"lsq_{dn}_x"] = words(xl)
        out[f"lsq_{dn}_gy"] = gl.numpy()
        for kind in ("lsq", "lsqp"):
            for per_ch in (False, True):
                bit, sym = (4, True) if kind == "lsq" else (5, False)
                qmin, qmax = qrange(bit, sym)
                n_par = 10 if per_ch else 1
                s = (torch.rand(n_par, generator=g) * 0.2 + 0.05).requires_grad_(True)
                if kind == "lsq":
                    z = torch.zeros(n_par, dtype=torch.int32)
                else:
                    z = (torch.rand(n_par, generator=g) * 10.0 + 3.0).requires_grad_(True)
                gf = 1.0 / (xl.numel() / (10 if per_ch else 1) * qmax) ** 0.5
                xr = xl.clone().requires_grad_(True)
                if kind == "lsq":
                    y = (U.fake_quantize_learnable_per_channel_affine_training(xr, s, z, 0, qmin, qmax, gf) if per_ch else
                         U.fake_quantize_learnable_per_tensor_affine_training(xr, s, z, qmin, qmax, gf))
                else:
                    y = (U.fake_quantize_learnableplus_per_channel_affine_training(xr, s, z, 0, qmin, qmax, gf) if per_ch else
                         U.fake_quantize_learnableplus_per_tensor_affine_training(xr, s, z, qmin, qmax, gf))
                assert y.dtype == torch.float32 and not torch.isnan(y).any()
                y.backward(gl)
                key = f"{kind}_{dn}_{'ch' if per_ch else 'pt'}"
                out[key + "_scale"] = s.detach().numpy()
                out[key + "_zp"] = z.detach().numpy()
                out[key + "_gf"] = np.float64(gf)
                out[key + "_y"] = y.detach().numpy()
                out[key + "_dx"] = words(xr.grad)
                out[key + "_ds"] = s.grad.numpy()
                if kind == "lsqp":
                    out[key + "_dz"] = z.grad.numpy()

        # observers over three batches
        B, T, H, heads, hd = 4, 20, 64, 4, 16
        obs_x = {1: [], 2: []}
        lens = []
        for b in range(3):
            a = torch.randn(B, T, H, generator=g)
            a[..., 3] *= 30.0
            obs_x[1].append(a.to(dt))
            obs_x[2].append((torch.randn(B, heads, T, hd, generator=g) * 2.0).to(dt))
            lens.append(torch.tensor([T, 13, 1, 7][: B], dtype=torch.int64).roll(b))
        for sp in (1, 2):
            out[f"obs_{dn}_x{sp}"] = np.stack([words(t) for t in obs_x[sp]])
        out[f"obs_{dn}_lens"] = np.stack([t.numpy() for t in lens])
        for name in ("MinMaxObserver", "AvgMinMaxObserver", "AvgPruneMinMaxObserver"):
            for sym in (False, True):
                for site in ("flat", "tok1", "tok2", "chan"):
                    if site == "chan" and name != "MinMaxObserver":
                        continue
                    ob = getattr(O, name)(bit=8, symmetric=sym, ch_axis=0 if site == "chan" else -1)
                    ob.set_name("encoder.layer.0.output.LayerNorm.post_act_fake_quantize.observer")
                    ob.set_percentile(0.95)
                    rows = []
                    for b in range(3):
                        if site == "flat":
                            ob(obs_x[1][b])
                        elif site == "chan":
                            ob(obs_x[1][b].reshape(B * T, H).t().contiguous())
                        else:
                            sp = 1 if site == "tok1" else 2
                            ob(obs_x[sp][b], observation_mask=lens[b], seq_pos=sp)
                        sc, zp = ob.calculate_qparams(ob.min_val, ob.max_val)
                        rows.append(np.stack([ob.min_val.reshape(-1).numpy(), ob.max_val.reshape(-1).numpy(),
                                              sc.reshape(-1).numpy(), zp.reshape(-1).to(torch.float32).numpy()]))
                    out[f"obs_{dn}_{name}_{int(sym)}_{site}"] = np.stack(rows).astype(np.float32)
    path = os.path.join(OUT, "lowp.npz")
    np.savez_compressed(path, **{k: np.asarray(v) for k, v in out.items()})
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

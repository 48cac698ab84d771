#!/usr/bin/env python3
"""Golden vectors of tests/test_oracle_vs_reference_live.py: the REFERENCE's own functions and observer classes run on the
seeded random cases of tests/_reference_live_cases.py, their results stored in tests/golden/reference_live.npz, and the
`quant:` section of every config.yaml under the reference's exp/ in tests/golden/reference_quant_sections.json.

Needs the reference tree (OSQ_REFERENCE; imported read-only, CPU, one thread; two process-local shims: an empty
``seaborn`` module, an identity ``Tensor.cuda``).  Outputs are DATA ONLY:

    python tests/golden/make_golden_reference_live.py
"""
import glob
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("OSQ_REFERENCE", os.path.join(os.path.dirname(ROOT), "reference"))    # default: checked out beside this repository
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _reference_live_cases as C    # noqa: E402


def main():
    sys.modules.setdefault("seaborn", types.ModuleType("seaborn"))
    torch.Tensor.cuda = lambda self, *a, **k: self
    sys.path.insert(0, REF)
    from quant_transformer.quantization import observer as O, util_quant as U
    torch.set_num_threads(1)
    out = {}

    for c in C.fake_quant_cases():
        t = c["trial"]
        out[f"fq/{t}/y"] = U.fake_quantize_per_tensor_affine(c["x"], c["scale"], c["zp"], c["qmin"], c["qmax"]).numpy()
        if "s" in c:
            out[f"fq/{t}/y_channel"] = U.fake_quantize_per_channel_affine(c["x"], c["s"], c["z"], 0, c["qmin"], c["qmax"]).numpy()

    for c in C.observer_cases():
        t = c["trial"]
        ob = getattr(O, c["cls_name"])(bit=c["bit"], symmetric=c["sym"], ch_axis=-1)
        ob.set_name(c["name"])
        if c["cls_name"] == "AvgPruneMinMaxObserver":
            ob.set_percentile(c["pct"])
        for it, (x, L, sp) in enumerate(c["batches"]):
            if c["masked"]:
                ob(x, L, sp)
            elif c["cls_name"] == "AvgPruneMinMaxObserver":
                ob(x, None, sp)
            else:
                ob(x)
            s, z = ob.calculate_qparams(ob.min_val, ob.max_val)
            out[f"obs/{t}/{it}/min_val"] = ob.min_val.numpy()
            out[f"obs/{t}/{it}/max_val"] = ob.max_val.numpy()
            out[f"obs/{t}/{it}/scale"] = s.numpy()
            out[f"obs/{t}/{it}/zero_point"] = z.numpy()

    for c in C.lsqplus_cases():
        t = c["trial"]
        x, scale, zp = (c[k].clone().requires_grad_(True) for k in ("x", "scale", "zp"))
        y = U.fake_quantize_learnableplus_per_tensor_affine_training(x, scale, zp, c["qmin"], c["qmax"], c["g"])
        y.backward(c["gy"])
        out[f"lsqplus/{t}/y"] = y.detach().numpy()
        out[f"lsqplus/{t}/dx"] = x.grad.numpy()
        out[f"lsqplus/{t}/dscale"] = scale.grad.numpy()
        out[f"lsqplus/{t}/dzero_point"] = zp.grad.numpy()

    weights, acts, one_sided = C.msefast_cases()
    for cols, bit, w in weights:
        ob = O.MSEFastObserver(bit=bit, symmetric=True, ch_axis=0)
        ob(w)
        out[f"msefast/weights/{cols}/min_val"], out[f"msefast/weights/{cols}/max_val"] = ob.min_val.numpy(), ob.max_val.numpy()
    for j, (sym, shape, x) in enumerate(acts):
        ob = O.AvgMSEFastObserver(bit=6, symmetric=sym, ch_axis=-1)
        for it in range(2):
            ob(x * (it + 1))
            out[f"msefast/acts/{j}/{it}/min_val"], out[f"msefast/acts/{j}/{it}/max_val"] = ob.min_val.numpy(), ob.max_val.numpy()
    for avg, side, xs in one_sided:
        ob = (O.AvgMSEFastObserver if avg else O.MSEFastObserver)(bit=6, symmetric=False, ch_axis=-1)
        for it, x in enumerate(xs):
            ob(x)
            key = f"msefast/one_sided/{int(avg)}/{side}/{it}"
            out[key + "/min_val"], out[key + "/max_val"] = ob.min_val.numpy(), ob.max_val.numpy()

    scales, zps = [], []
    for sym in (False, True):
        ob = O.AvgMSEFastObserver(bit=8, symmetric=sym, ch_axis=-1)
        for _, _, mn, mx in (c for c in C.mixed_dtype_cases() if c[0] == sym):
            s, z = ob.calculate_qparams(torch.tensor(mn), torch.tensor(mx))
            scales.append(s.numpy().reshape(()))
            zps.append(float(z))
    out["mixed/scale_is_f64"] = np.array([s.dtype == np.float64 for s in scales])
    out["mixed/scale"] = np.array([float(s) for s in scales], dtype=np.float64)
    out["mixed/zero_point"] = np.array(zps, dtype=np.float64)

    np.savez_compressed(os.path.join(HERE, "reference_live.npz"), **out)

    import yaml
    exp = os.path.join(REF, "exp")
    sections = {os.path.relpath(f, exp).replace(os.sep, "/"): yaml.safe_load(open(f))["quant"]
                for f in sorted(glob.glob(os.path.join(exp, "**", "config.yaml"), recursive=True))}
    with open(os.path.join(HERE, "reference_quant_sections.json"), "w") as f:
        json.dump(sections, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(out)} arrays, {len(sections)} quant sections")


if __name__ == "__main__":
    main()

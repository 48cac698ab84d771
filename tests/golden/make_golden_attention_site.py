#!/usr/bin/env python3
"""Golden vectors of the ATTENTION-PROBABILITIES SITE of a quantized block, made by running the reference's eager lines
(quant_transformer/model/quant_bert.py:169-185: ``scores / sqrt(d) + mask``; quant_bart.py:232-256: ``(w.view(B,h,T,S) +
mask).view(B*h,T,S)``; then ``softmax(dim=-1)`` and the attention_probs quantizer) with the reference's own quantization
package on the CPU, one thread, for each case of tests/_attention_site.py:

    observer pass   (observer on, fake-quant off):  probs = quantizer(softmax(pre(scores) + mask), lengths, 2)  -> probs, scale, zero_point, min / max
    quantized pass  (observer off, fake-quant on):  the same                                                     -> the integer tensor x_quant

Stored per case: the un-quantised probabilities of a slice (sample 0, head 0, 64 queries; fp32), the integer tensor of
sample 0, heads 0-3 (uint8) and the histogram of the integer values over ALL entries, scale / zero_point / observer
statistics, checksums of the re-drawn inputs (about 0.2 MB in all).  The inputs are not stored
(tests/_attention_site.py re-draws them).  Outputs are DATA ONLY.  Runs in the build container (needs the reference):
    python tests/golden/make_golden_attention_site.py
"""
import os
import sys
import types

import numpy as np
import torch

REF = os.environ.get("OSQ_REFERENCE", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
from _attention_site import CASES, OBSERVER_NAME, PROBS_SLICE, XQ_SLICE, attention_site_inputs, checksum, scaling  # noqa: E402


class Cfg(dict):
    __getattr__ = dict.__getitem__


def main():
    sys.modules.setdefault("seaborn", types.ModuleType("seaborn"))
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.nn.Module.cuda = lambda self, *a, **k: self
    sys.path.insert(0, REF)
    from quant_transformer.quantization.quantized_module import Quantizer
    torch.set_num_threads(1)
    out = {}
    for name, kind, shape, d, quantizer, observer, pct, bit, seed in CASES:
        scores, mask, L = attention_site_inputs(seed, kind, shape, d)
        b, h, t, s = shape
        cfg = Cfg(quantizer=quantizer, observer=observer, bit=bit, symmetric=False, ch_axis=-1)
        q = Quantizer(None, cfg).eval()
        q.observer.set_name(OBSERVER_NAME)
        if pct is not None:
            q.observer.set_percentile(pct)

        def site():
            if kind == "bert":                                       # quant_bert.py:169-185
                v = scores / scaling(kind, d)
                v = v + mask
                return q(torch.nn.functional.softmax(v, dim=-1), L, 2)
            w = scores.view(b * h, t, s)                             # quant_bart.py:232-256
            w = (w.view(b, h, t, s) + mask).view(b * h, t, s)
            return q(torch.nn.functional.softmax(w, dim=-1), L, 2).view(b, h, t, s)
        with torch.no_grad():
            q.enable_observer()
            q.disable_fake_quant()
            p_obs = site()
            q.disable_observer()
            q.enable_fake_quant()
            p_q = site()
        scale, zp = q.scale.detach().reshape(-1), q.zero_point.detach().reshape(-1).float()
        xq = torch.round(p_q / scale + torch.round(zp))
        assert float(xq.min()) >= q.quant_min and float(xq.max()) <= q.quant_max
        assert torch.equal((xq - torch.round(zp)) * scale, p_q)     # util_quant.py:15, exact reconstruction
        out[name + "_probs"] = p_obs[PROBS_SLICE].numpy()
        out[name + "_xq"] = xq[XQ_SLICE].numpy().astype(np.uint8)
        out[name + "_xq_hist"] = np.bincount(xq.numpy().astype(np.int64).reshape(-1), minlength=q.quant_max + 1)
        out[name + "_scale"], out[name + "_zp"] = scale.numpy(), zp.numpy()
        out[name + "_min"] = np.asarray(q.observer.min_val.numpy(), dtype=np.float32).reshape(-1)
        out[name + "_max"] = np.asarray(q.observer.max_val.numpy(), dtype=np.float32).reshape(-1)
        out[name + "_sums"] = np.array([checksum(scores), checksum(mask.contiguous()), int(L.sum())], dtype=np.int64)
        print(name, "scale", float(scale), "zp", float(zp), "min", out[name + "_min"], "max", out[name + "_max"], flush=True)
    path = os.path.join(OUT, "attention_site.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Forward + backward of the GELU and attention-probabilities sites under autograd, the eager chain against the one-launch
pair (util_layernorm.FUSE_BACKWARD; the softmax site with FUSE_SOFTMAX on in both forms' switch, which only the fused form can
use under autograd), and one learn_scale step of BERT-base (random weights, W6A6 LSQ+ activation quantizers) at 32 x 128
and 32 x 384.

Per figure: microseconds (sites) / milliseconds (step) from HIP events around a window of about a quarter second that ends in a
synchronise, all forms in one process, alternating, 7 rounds; printed as median [min .. max].  A difference inside the eager form's own range is reported
as such.
    python tools/site_backward_ab.py [--out profiles/site_backward_ab.txt] [--no-model]
"""
import argparse
import os
import statistics
import sys
from types import SimpleNamespace as NS

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from outlier_suppression_amd import _hip, util_layernorm as UL  # noqa: E402
from outlier_suppression_amd.quantization import Quantizer  # noqa: E402

A_Q = NS(quantizer="LSQPlusFakeQuantize", observer="MinMaxObserver", bit=6, symmetric=False, ch_axis=-1)
ROUNDS = 7


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / n


WINDOW_US = 250e3         # a timed window: long enough that the clock and the scheduler do not show in it


def alternate(forms):
    """{name: [us per call] * ROUNDS}: every form warmed up first, the calls per window then sized from the first form
    to about WINDOW_US, then the forms in turn within each round.  What the sites did is left in UL.site_backward for
    report() to print: a fused form that fell back to the eager lines must not pass as one."""
    res = {name: [] for name in forms}
    UL.site_backward.reset()
    for fn in forms.values():
        timed(fn, 3)
    n = max(3, int(WINDOW_US / timed(next(iter(forms.values())), 3)))      # sized once everything is warm
    for _ in range(ROUNDS):
        for name, fn in forms.items():
            res[name].append(timed(fn, n))
    return res


def _site_calls():
    took = UL.site_backward
    return f"gelu {took.gelu}, softmax {took.softmax}, eager {took.eager}"


def report(label, res, unit=1.0, suffix="us", calls=_site_calls):
    med = {k: statistics.median(v) for k, v in res.items()}
    text = "   ".join(f"{k} {med[k] / unit:9.2f} [{min(v) / unit:.2f} .. {max(v) / unit:.2f}] {suffix}" for k, v in res.items())
    lo, hi = min(res["eager"]), max(res["eager"])
    verdict = "inside eager's own range" if lo <= med["fused"] <= hi else f"x{med['eager'] / med['fused']:.2f}"
    return f"{label:44s} {text}   fused vs eager: {verdict}   (site calls: {calls()})"


def quantizer(dev, x):
    q = Quantizer(None, A_Q).to(dev)
    q.enable_observer()
    with torch.no_grad():
        q(x)
    q.disable_observer()
    q.enable_fake_quant()
    return q


def site_forms(run):
    def form(fused):
        def fn():
            UL.FUSE_BACKWARD = fused
            run()
        return fn
    return {"eager": form(False), "fused": form(True)}


def sites(dev, lines):
    g = torch.Generator().manual_seed(0)
    x = torch.randn(32, 128, 3072, generator=g).to(dev).requires_grad_(True)
    gy = torch.randn(32, 128, 3072, generator=g).to(dev)
    q = quantizer(dev, F.gelu(x.detach()))

    def gelu():
        y = UL.activation_fake_quant(F.gelu, q, x)
        torch.autograd.grad(y, [x, q.scale, q.zero_point], gy)
    lines.append(report("GELU site fwd+bwd [32,128,3072]", alternate(site_forms(gelu))))
    print(lines[-1], flush=True)
    del x, gy
    for shape in ((32, 12, 128, 128), (32, 12, 384, 384)):
        b, h, t, s = shape
        sc = (torch.randn(*shape, generator=g) * 16.0).to(dev).requires_grad_(True)
        gp = torch.randn(*shape, generator=g).to(dev)
        lengths = torch.randint(s // 2, s + 1, (b,), generator=g)
        mask = ((torch.arange(s)[None, :] >= lengths[:, None]).float() * -10000.0)[:, None, None, :].to(dev)
        qs = quantizer(dev, torch.softmax(sc.detach() * 0.125 + mask, -1))

        def probs():
            p = UL.attention_probs_fake_quant(qs, sc, mask, alpha=0.125)
            torch.autograd.grad(p, [sc, qs.scale, qs.zero_point], gp)
        lines.append(report(f"attention-probabilities site fwd+bwd {list(shape)}", alternate(site_forms(probs))))
        print(lines[-1], flush=True)
        del sc, gp
        torch.cuda.empty_cache()


def _site_switches(fused):
    UL.FUSE_BACKWARD = UL.FUSE_SOFTMAX = fused


def learn_scale_step(dev, lines, seq, switch=_site_switches, calls=_site_calls):
    """``switch(fused)`` sets the switches of a form, ``calls()`` words what the sites did (tools/layernorm_backward_ab.py
    times its own switch through this function)."""
    from transformers import BertConfig, BertForSequenceClassification
    from outlier_suppression_amd import token_wise_clipping as TWC
    from outlier_suppression_amd.quant_model import quantize_model
    from outlier_suppression_amd.quantization import disable_all
    from outlier_suppression_amd.quantization.state import set_observer_name
    torch.manual_seed(0)
    cfg = BertConfig(num_labels=2, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    fp = BertForSequenceClassification(cfg).eval().to(dev)
    g = torch.Generator().manual_seed(1)
    lengths = torch.randint(seq // 2, seq + 1, (32,), generator=g)
    mask = (torch.arange(seq)[None, :] < lengths[:, None]).long()
    ids = torch.randint(1, cfg.vocab_size, (32, seq), generator=g) * mask
    batch = {"input_ids": ids.to(dev), "attention_mask": mask.to(dev), "token_type_ids": torch.zeros_like(ids).to(dev)}
    with torch.no_grad():
        target = fp(**batch)[0].detach()
    w_q = NS(quantizer="FixedFakeQuantize", observer="MinMaxObserver", bit=6, symmetric=True, ch_axis=0)
    a_q = NS(quantizer="LSQPlusFakeQuantize", observer="AvgPruneMinMaxObserver", bit=6, symmetric=False, ch_axis=-1)
    model = quantize_model(fp, w_q, a_q).to(dev)
    disable_all(model)
    set_observer_name(model)
    TWC.set_ratio(model, 1.0)
    TWC.calibrate(model, [batch])
    disable_all(model)
    quantizers = [q for _, q in TWC._act_quantizers(model)]
    for q in quantizers:
        q.enable_fake_quant()
        q.disable_observer()
    params = [p for q in quantizers for p in (q.scale, q.zero_point)]

    def step(fused):
        def fn():
            switch(fused)
            for p in params:
                p.grad = None
            TWC.batch_loss(model(**batch), batch, target, "glue").backward()
        return fn
    with TWC._only_these_learn(model, params):
        res = alternate({"eager": step(False), "fused": step(True)})
    lines.append(report(f"learn_scale step, BERT-base 32 x {seq} (forward + backward)", res, 1000.0, "ms", calls))
    print(lines[-1], flush=True)
    del model, fp
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-model", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    _hip.load()          # loading applies the environment's switches: before this tool sets its own
    lines = [f"# sites under autograd, eager chain vs one launch forward + one launch backward ({torch.cuda.get_device_name(dev)})",
             f"# HIP events around a window of ~{WINDOW_US / 1e3:.0f} ms ending in a synchronise; median [min .. max] of {ROUNDS} alternating rounds, one process"]
    saved = (UL.FUSE_BACKWARD, UL.FUSE_SOFTMAX)
    try:
        UL.FUSE_SOFTMAX = True
        sites(dev, lines)
        UL.FUSE_SOFTMAX = saved[1]
        if not args.no_model:
            for seq in (128, 384):
                learn_scale_step(dev, lines, seq)
    finally:
        UL.FUSE_BACKWARD, UL.FUSE_SOFTMAX = saved
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

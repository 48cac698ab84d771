#!/usr/bin/env python3
"""The attention-probabilities site (util_layernorm.attention_probs_fake_quant) eager against one launch
(util_layernorm.FUSE_SOFTMAX), in the two states the site meets:

  quantising    the probs quantizer fake-quantises (LSQ+, 6 bit, observer off): eager = add + softmax + fake-quant, one
                launch = the whole site;
  softmax-only  no quantizer work in the site (observer passes hand the probabilities on): eager = add + softmax, one
                launch = add + softmax.

Shapes: BERT-base at SQuAD length [32,12,384,384] (BERT mask, alpha = 1/8), at GLUE length [32,12,128,128], and a BART-large
self-attention [8*16, 512, 512] with the causal + padding mask.  Per call: microseconds from HIP events around 50 calls
(launch gaps included), median of 5 alternating rounds; for the one-launch form also the kernel's own time (the timing
hook of osq_time_next_launch, median of 20).  Also printed: max |one launch - eager| and the integer entries that differ.
    python tools/attention_site_ab.py [--out profiles/attention_site_ab.txt]
"""
import argparse
import ctypes
import os
import statistics
import sys
from types import SimpleNamespace as NS

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from outlier_suppression_amd import _hip, util_layernorm as UL  # noqa: E402
from outlier_suppression_amd.quantization import Quantizer  # noqa: E402

SHAPES = (
    ("bert [32,12,384,384]", "bert", (32, 12, 384, 384)),
    ("bert [32,12,128,128]", "bert", (32, 12, 128, 128)),
    ("bart-large [8*16,512,512]", "bart", (8, 16, 512, 512)),
)


def inputs(kind, shape, dev):
    b, h, t, s = shape
    g = torch.Generator().manual_seed(0)
    scores = (torch.randn(*shape, generator=g) * 16.0).to(dev)
    lengths = torch.randint(s // 2, s + 1, (b,), generator=g)
    valid = (torch.arange(s)[None, :] < lengths[:, None]).float()
    if kind == "bert":
        mask = (1.0 - valid[:, None, None, :]) * -10000.0
    else:
        pad = (1.0 - valid[:, None, None, :].expand(b, 1, t, s)).contiguous()
        pad = pad.masked_fill(pad.bool(), torch.finfo(torch.float32).min)
        causal = torch.full((t, s), float("-inf")).triu(1)
        mask = pad + causal
        scores = scores.view(b * h, t, s) / 8.0
    return scores, mask.to(dev), lengths.to(dev)


def site(q, kind, heads, scores, mask, L):
    if kind == "bert":
        return UL.attention_probs_fake_quant(q, scores, mask, alpha=0.125, observation_mask=L)
    return UL.attention_probs_fake_quant(q, scores, mask, dropout=(0.1, False), observation_mask=L, heads=heads)


def timed(fn, n=50):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / n


def kernel_us(fn, n=20):
    lib = _hip.load()
    a, b = ctypes.c_void_p(), ctypes.c_void_p()
    _hip.check(lib.osq_timing_events_create(ctypes.byref(a), ctypes.byref(b)), "timing_events_create")
    out = []
    for _ in range(n):
        _hip.check(lib.osq_time_next_launch(_hip.TIME_ATTENTION_SOFTMAX, a, b), "time_next_launch")
        fn()
        us = ctypes.c_float()
        _hip.check(lib.osq_timing_elapsed_us(a, b, ctypes.byref(us)), "timing_elapsed_us")
        out.append(us.value)
    lib.osq_timing_events_destroy(a, b)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = [f"# attention-probabilities site, eager vs one launch ({torch.cuda.get_device_name(dev)})",
             "# us per call: HIP events around 50 calls, median of 5 alternating rounds; kernel = the one-launch kernel's own time"]
    old = UL.FUSE_SOFTMAX
    for label, kind, shape in SHAPES:
        scores, mask, L = inputs(kind, shape, dev)
        nbytes = scores.numel() * 4
        q = Quantizer(None, NS(quantizer="LSQPlusFakeQuantize", observer="MinMaxObserver", bit=6, symmetric=False, ch_axis=-1)).to(dev)
        q.observer.set_name("attention_probs_post_act_fake_quantize.observer")
        with torch.no_grad():
            UL.FUSE_SOFTMAX = False
            q.enable_observer()
            site(q, kind, shape[1], scores, mask, L)
            q.disable_observer()
            q.enable_fake_quant()
            for state, qq in (("quantising", q), ("softmax-only", None)):
                res = {False: [], True: []}
                outs = {}
                for fused in (False, True):
                    UL.FUSE_SOFTMAX = fused
                    outs[fused] = site(qq, kind, shape[1], scores, mask, L)
                    timed(lambda: site(qq, kind, shape[1], scores, mask, L), 5)
                for _ in range(5):
                    for fused in (False, True):
                        UL.FUSE_SOFTMAX = fused
                        res[fused].append(timed(lambda: site(qq, kind, shape[1], scores, mask, L)))
                UL.FUSE_SOFTMAX = True
                k_us = kernel_us(lambda: site(qq, kind, shape[1], scores, mask, L))
                eager, one = statistics.median(res[False]), statistics.median(res[True])
                diff = (outs[True] - outs[False]).abs()
                extra = ""
                if qq is not None:
                    steps = torch.round(diff / q.scale.detach())
                    extra = f", integer entries differing {int((steps != 0).sum())} of {diff.numel()}"
                lines.append(f"{label:28s} {state:13s} eager {eager:8.1f} us   one launch {one:8.1f} us "
                             f"(kernel {k_us:7.1f} us, {2 * nbytes / k_us / 1e6:5.2f} TB/s of scores read + probs written)   "
                             f"x{eager / one:4.2f}   max |diff| {float(diff.max()):.2e}{extra}")
                print(lines[-1], flush=True)
        del scores, mask
        torch.cuda.empty_cache()
    UL.FUSE_SOFTMAX = old
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

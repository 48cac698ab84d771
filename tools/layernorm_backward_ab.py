#!/usr/bin/env python3
"""Forward + backward of the LayerNorm site under autograd -- residual, LayerNorm, affine pair, output fake-quant -- the eager
chain against the one-launch pair (util_layernorm.FUSE_LAYERNORM_BACKWARD), with and without gamma, at [32,128,768],
[32,384,768] and [32,512,1024]; and one learn_scale step of BERT-base (random weights, W6A6 LSQ+ activation quantizers) at
32 x 128 and 32 x 384 with the switch off and on.  Timing, alternation and the report's form are tools/site_backward_ab.py's:
median [min .. max] of 7 rounds in one process; a difference inside the eager form's own range is reported as such.
    python tools/layernorm_backward_ab.py [--out profiles/layernorm_backward_ab.txt] [--no-model]
"""
import argparse
import os
import sys

import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import site_backward_ab as AB  # noqa: E402
from site_backward_ab import UL, _hip  # noqa: E402


def calls():
    took = UL.layernorm_backward
    return f"layernorm fused {took.fused}, eager {took.eager}"


def alternate(forms):
    UL.layernorm_backward.reset()
    return AB.alternate(forms)


def switch(fused):
    UL.FUSE_LAYERNORM_BACKWARD = fused


def sites(dev, lines):
    g = torch.Generator().manual_seed(0)
    for shape in ((32, 128, 768), (32, 384, 768), (32, 512, 1024)):
        width = shape[-1]
        x = torch.randn(*shape, generator=g).to(dev).requires_grad_(True)
        h = (torch.randn(*shape, generator=g) * 0.5).to(dev).requires_grad_(True)
        gy = torch.randn(*shape, generator=g).to(dev)
        org = nn.LayerNorm(width).to(dev)
        org.weight.data.uniform_(0.5, 1.5, generator=None)
        ln = UL.QuantizedLayerNorm(org, None, AB.A_Q).to(dev).requires_grad_(False)
        ln.layernorm_post_act_fake_quantize = AB.quantizer(dev, org(x.detach() + h.detach()))
        q = ln.layernorm_post_act_fake_quantize
        for with_gamma in (False, True):
            res = UL.GammaResidual()
            if with_gamma:
                res.set_gamma(torch.rand(width, generator=g).to(dev) + 0.5)
                res.requires_grad_(False)

            def run():
                y = UL.residual_layernorm(res, ln, x, h)
                torch.autograd.grad(y, [x, h, q.scale, q.zero_point], gy)

            def form(fused):
                def fn():
                    switch(fused)
                    run()
                return fn
            label = f"LayerNorm site fwd+bwd {list(shape)}{' gamma' if with_gamma else ''}"
            lines.append(AB.report(label, alternate({"eager": form(False), "fused": form(True)}), calls=calls))
            print(lines[-1], flush=True)
        del x, h, gy
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-model", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    _hip.load()          # loading applies the environment's switches: before this tool sets its own
    lines = [f"# the LayerNorm site under autograd, eager chain vs one launch forward + one launch backward ({torch.cuda.get_device_name(dev)})",
             f"# HIP events around a window of ~{AB.WINDOW_US / 1e3:.0f} ms ending in a synchronise; median [min .. max] of {AB.ROUNDS} alternating rounds, one process"]
    saved = UL.FUSE_LAYERNORM_BACKWARD
    try:
        sites(dev, lines)
        if not args.no_model:
            for seq in (128, 384):
                UL.layernorm_backward.reset()
                AB.learn_scale_step(dev, lines, seq, switch, calls)
    finally:
        UL.FUSE_LAYERNORM_BACKWARD = saved
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

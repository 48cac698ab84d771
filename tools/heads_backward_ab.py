#!/usr/bin/env python3
"""Forward + backward of the query / key / value head-split sites and of the context site under autograd, the eager lines
against the one-launch pair (util_layernorm.FUSE_HEADS_BACKWARD), the transposed-key site alone against its dense form (what
the LDS transpose costs), and one learn_scale step of BERT-base (random weights, W6A6 LSQ+ activation quantizers) at 32 x 128
and 32 x 384 with the other autograd switches as they are.

The three-site block is BERT's: the key's output is used as k^T, so its gradient arrives as the transposed view.  Figures as in
tools/site_backward_ab.py: HIP events around a window of about a quarter second, all forms in one process, alternating, 7
rounds, median [min .. max]; a difference inside the eager form's own range is reported as such.
    python tools/heads_backward_ab.py [--out profiles/heads_backward_ab.txt] [--no-model]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from site_backward_ab import ROUNDS, WINDOW_US, alternate, learn_scale_step, quantizer, report  # noqa: E402
from outlier_suppression_amd import _hip, util_layernorm as UL  # noqa: E402

SHAPES = ((32, 128, 768, 12), (32, 384, 768, 12), (32, 512, 1024, 16))


def _calls():
    took = UL.heads_backward
    return f"split {took.split}, merge {took.merge}, eager {took.eager}"


def _switch(fused):
    UL.FUSE_HEADS_BACKWARD = fused


def _forms(run):
    def form(fused):
        def fn():
            _switch(fused)
            run()
        return fn
    return {"eager": form(False), "fused": form(True)}


def _measure(label, forms, lines, **kw):
    UL.heads_backward.reset()
    lines.append(report(label, alternate(forms), calls=_calls, **kw))
    print(lines[-1], flush=True)


def sites(dev, lines):
    g = torch.Generator().manual_seed(0)
    for b, t, width, h in SHAPES:
        d = width // h
        xs = [torch.randn(b, t, width, generator=g).to(dev).requires_grad_(True) for _ in range(3)]
        gq, gkt, gv = (torch.randn(*s, generator=g).to(dev) for s in ((b, h, t, d), (b, h, d, t), (b, h, t, d)))
        qs = [quantizer(dev, x.detach()) for x in xs]
        params = [p for q in qs for p in (q.scale, q.zero_point)]
        heads = lambda x: x.view(b, t, h, d).permute(0, 2, 1, 3)      # noqa: E731

        def block():            # model/quant_bert.py: the three sites, the key's output used transposed
            fused = UL.qkv_heads_fake_quant(qs, xs, h)
            if fused is not None:
                outs = [fused[0], fused[1].transpose(-1, -2), fused[2]]
            else:
                outs = [qs[0](heads(xs[0]), None, 2), qs[1](heads(xs[1]).transpose(-1, -2), None, 3), qs[2](heads(xs[2]), None, 2)]
            torch.autograd.grad(outs, xs + params, [gq, gkt, gv])
        _measure(f"q / k / v sites fwd+bwd [{b},{t},{width}] h={h}", _forms(block), lines)

        ctx = torch.randn(b, h, t, d, generator=g).to(dev).requires_grad_(True)
        gm = torch.randn(b, t, width, generator=g).to(dev)

        def context():
            y = UL.merge_heads_fake_quant(qs[0], ctx)
            torch.autograd.grad(y, [ctx, qs[0].scale, qs[0].zero_point], gm)
        _measure(f"context site fwd+bwd [{b},{h},{t},{d}]", _forms(context), lines)

        def key(grad):
            def fn():
                y = UL.split_heads_fake_quant(qs[1], xs[1], h)
                torch.autograd.grad(y, [xs[1], qs[1].scale, qs[1].zero_point], grad)
            return fn
        _switch(True)
        UL.heads_backward.reset()
        res = alternate({"dense": key(gq), "transposed": key(gkt.transpose(-1, -2))})
        med = {k: statistics.median(v) for k, v in res.items()}
        text = "   ".join(f"{k} {med[k]:9.2f} [{min(v):.2f} .. {max(v):.2f}] us" for k, v in res.items())
        inside = min(res["dense"]) <= med["transposed"] <= max(res["dense"])
        verdict = "inside the dense form's own range" if inside else f"x{med['transposed'] / med['dense']:.2f} the dense form"
        lines.append(f"{f'key site fwd+bwd, one launch each [{b},{t},{width}] h={h}':44s} {text}   transposed gradient: {verdict}   (site calls: {_calls()})")
        print(lines[-1], flush=True)
        del xs, gq, gkt, gv, ctx, gm
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-model", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    _hip.load()          # loading applies the environment's switches: before this tool sets its own
    lines = [f"# head-split sites under autograd, eager lines vs one launch forward + one launch backward ({torch.cuda.get_device_name(dev)})",
             f"# HIP events around a window of ~{WINDOW_US / 1e3:.0f} ms ending in a synchronise; median [min .. max] of {ROUNDS} alternating rounds, one process"]
    saved = UL.FUSE_HEADS_BACKWARD
    try:
        sites(dev, lines)
        if not args.no_model:
            for seq in (128, 384):
                UL.heads_backward.reset()
                learn_scale_step(dev, lines, seq, switch=_switch, calls=_calls)
    finally:
        UL.FUSE_HEADS_BACKWARD = saved
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

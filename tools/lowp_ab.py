#!/usr/bin/env python3
"""bf16 / fp16 kernels against the fp32 ones at [256,128,768] and [32,128,3072] (profiles/lowp_ab.txt).

Times with device events, after a warm-up, the median of --reps repetitions of --iters back-to-back calls:
  * the in-dtype chain (FixedFakeQuantize per-tensor, osq_fake_quant_chain_lowp), bf16 and fp16;
  * the widening LSQ+ forward (fp32 result, osq_fake_quant_per_tensor_widen);
  * the flat observe (osq_observe_flat on 2-byte data) and the masked token-path observe (token extrema + the fp32 finaliser);
  * the per-channel observe and the per-channel widening forward of a [3072, 768] weight, ch_axis = 0;
  * the same calls on fp32 data through the existing kernels;
  * ".float() -> fp32 kernel -> .to(dtype)": a cost baseline only (it is NOT bit-equal to the reference's chain).
Bytes moved are computed from the shapes (compulsory HBM traffic of one call); share = bytes / time / 8 TB/s.
Run:  python tools/lowp_ab.py [--iters 50] [--reps 5]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from outlier_suppression_amd import ops  # noqa: E402

PEAK = 8.0e12


def timed(fn, iters, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    runs = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        runs.append(a.elapsed_time(b) * 1e3 / iters)
    runs.sort()
    return runs[len(runs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    rows = []

    def add(shape, name, dtype, fn, nbytes):
        us = timed(fn, args.iters, args.reps)
        rows.append({"shape": list(shape), "call": name, "dtype": dtype, "us": round(us, 2), "MB": round(nbytes / 1e6, 1),
                     "TB_s": round(nbytes / us / 1e6, 2), "share_8TBs": round(nbytes / us / 1e6 / 8.0, 3)})

    for shape in ((256, 128, 768), (32, 128, 3072)):
        B, T, H = shape
        n = B * T * H
        x32 = (torch.randn(shape, generator=gen) * 3).to(dev)
        x32[..., 5] *= 30
        lens = torch.randint(T // 2, T + 1, (B,), generator=gen).to(dev)
        valid = float(lens.sum().item()) / (B * T)
        s = torch.tensor([0.0413], device=dev)
        zi = torch.tensor([121], dtype=torch.int32, device=dev)
        zf = torch.tensor([121.3], device=dev)
        mn, mx = torch.full((), float("inf"), device=dev), torch.full((), float("-inf"), device=dev)
        sink = ops.QParamSink(torch.ones(1, device=dev), torch.zeros(1, device=dev))

        add(shape, "fake_quant fixed (fp32 kernel)", "fp32", lambda: ops.fake_quant_per_tensor(x32, s, zi, 0, 255), 8 * n)
        add(shape, "fake_quant lsq+ (fp32 kernel)", "fp32",
            lambda: ops.fake_quant_per_tensor(x32, s, zf, 0, 255, ops.PARAM_LSQPLUS, 0.01), 8 * n)
        add(shape, "observe flat (fp32 kernel)", "fp32", lambda: ops.observe_flat(x32, ops.UPDATE_AVERAGE, 0, mn, mx, 0, 255, False, sink), 4 * n)
        add(shape, "observe tokens (fp32 kernels)", "fp32",
            lambda: ops.observe_tokens(x32, 1, lens, True, 0.99, ops.UPDATE_AVERAGE, 0, mn, mx, 0, 255, False, sink), 4 * n * valid)
        for dn, dt in (("bf16", torch.bfloat16), ("f16", torch.float16)):
            xh = x32.to(dt)
            add(shape, "chain (in-dtype)", dn, lambda: ops.fake_quant_chain_lowp(xh, s, zi, 0, 255), 4 * n)
            add(shape, "widen lsq+ (fp32 out)", dn, lambda: ops.fake_quant_per_tensor_widen(xh, s, zf, 0, 255, ops.PARAM_LSQPLUS, 0.01), 6 * n)
            add(shape, "observe flat", dn, lambda: ops.observe_flat(xh, ops.UPDATE_AVERAGE, 0, mn, mx, 0, 255, False, sink), 2 * n)
            add(shape, "observe tokens", dn,
                lambda: ops.observe_tokens(xh, 1, lens, True, 0.99, ops.UPDATE_AVERAGE, 0, mn, mx, 0, 255, False, sink),
                2 * n * valid)
            add(shape, "baseline .float()->fp32 kernel->.to() (not bit-equal)", dn,
                lambda: ops.fake_quant_per_tensor(xh.float(), s, zi, 0, 255).to(dt), 20 * n)
        del x32
    shape = (3072, 768)
    w32 = torch.randn(shape, generator=gen).to(dev) * 0.05
    cs = torch.full((shape[0],), 0.0007, device=dev)
    cz = torch.zeros(shape[0], dtype=torch.int32, device=dev)
    cmn, cmx = torch.full((shape[0],), float("inf"), device=dev), torch.full((shape[0],), float("-inf"), device=dev)
    n = w32.numel()
    add(shape, "observe channels (fp32 kernel)", "fp32",
        lambda: ops.observe_channels(w32, 0, ops.UPDATE_RUNNING, 0, cmn, cmx, -128, 127, True), 4 * n)
    add(shape, "fake_quant per-channel (fp32 kernel)", "fp32", lambda: ops.fake_quant_per_channel(w32, cs, cz, 0, -128, 127), 8 * n)
    for dn, dt in (("bf16", torch.bfloat16), ("f16", torch.float16)):
        wh = w32.to(dt)
        add(shape, "observe channels", dn, lambda: ops.observe_channels(wh, 0, ops.UPDATE_RUNNING, 0, cmn, cmx, -128, 127, True), 2 * n)
        add(shape, "widen per-channel (fp32 out)", dn, lambda: ops.fake_quant_per_channel(wh, cs, cz, 0, -128, 127), 6 * n)
    for r in rows:
        print(json.dumps(r))


if __name__ == "__main__":
    main()

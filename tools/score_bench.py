"""A/B of teacher-forced scoring (csrc/token_logprob.hip): ops.lm_loss / losses.FusedLmLoss / model.score() against the torch
lines they stand beside, in one process, every form timed in turn within each of the --reps rounds.

On fp32 logits [32*62, 50265] and [32*128, 50265] (random normal, 5 % of the labels ignored):
    the loss without autograd      F.cross_entropy under no_grad          against ops.lm_loss into preallocated outputs
    the loss and its backward      F.cross_entropy(...).backward()        against FusedLmLoss.apply(...).backward()
    torch.cuda.max_memory_allocated above what is held before the call, of both, for both forms
A time is the median of --reps windows of --inner calls each, a device synchronisation at either end, with [min, max]; the
baseline's own spread stands beside every ratio.  For the forward alone the time of ONE read of the logits at the copy rate
measured on MI355X (6.29 TB/s) is printed beside it.

Then, on a random-init BART-large shape (d_model 1024, 12 + 12 layers, vocab 50265, W6A6 in the plain quantising state), batch
--batch, source 512, targets of 62 tokens: score(num_candidates=6) -- the encoder once per input -- against score() of the six
times repeated inputs.  --no-model skips it.

--share measures only this, on that model and shape: score(num_candidates=6) unshared against share_cross_kv=True -- the
cross-attention keys / values projected, quantized and attended once per input -- under each of: every one-launch attention
switch off, FUSE_SOFTMAX, FUSE_ATTENTION_INT, FUSE_ATTENTION; every form timed in turn in one process, with the peak memory
above the inputs and the largest difference of a token log-probability between the two forms (reported, not asserted:
rocBLAS may pick another kernel for the projections of B * S rows than of B * 6 * S).

    python tools/score_bench.py [--reps 7] [--out profiles/token_logprob_ab.txt]
    python tools/score_bench.py --share [--reps 7] [--out profiles/score_share_ab.txt]
"""
import argparse
import os
import statistics
import sys
import time

import torch
from torch.nn import functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

COPY_RATE = 6.29e12          # bytes / s, float4 copy on MI355X (README)
VOCAB = 50265


def timed(forms, reps, inner):
    """{name: [ms per call] * reps}: every form in turn within each round, two warm-up rounds first."""
    times = {name: [] for name in forms}
    for r in range(reps + 2):
        for name, fn in forms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(inner):
                fn()
            torch.cuda.synchronize()
            if r >= 2:
                times[name].append((time.perf_counter() - t0) * 1e3 / inner)
    return times


def say(ts):
    return f"{statistics.median(ts):9.4f} ms [{min(ts):.4f}, {max(ts):.4f}]"


def peak_above(fn):
    """Bytes the call allocates at its peak above what is held before it."""
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - held


def compare(emit, times, base, new):
    b, n = times[base], times[new]
    mb, mn = statistics.median(b), statistics.median(n)
    spread = (max(b) - min(b)) / mb
    gain = (mb - mn) / mb
    verdict = "exceeds" if abs(gain) > spread else "does NOT exceed"
    emit(f"    {base:<34} {say(b)}")
    emit(f"    {new:<34} {say(n)}")
    emit(f"    ratio {mb / mn:.2f}x; the difference ({gain * 100:+.1f} % of the baseline) {verdict} the baseline's own spread "
         f"({spread * 100:.1f} % of its median)")


def loss_forms(emit, rows, reps, inner):
    from outlier_suppression_amd import ops
    from outlier_suppression_amd.model.losses import FusedLmLoss
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(rows)
    logits = torch.randn((rows, VOCAB), generator=g, device=dev) * 3
    labels = torch.randint(0, VOCAB, (rows,), generator=g, device=dev)
    labels[torch.rand(rows, generator=g, device=dev) < 0.05] = -100
    out = (torch.empty((), device=dev), torch.empty(rows, device=dev), torch.empty(rows, device=dev),
           torch.empty(2, dtype=torch.int64, device=dev))
    leaf = logits.clone().requires_grad_(True)

    def ce():
        with torch.no_grad():
            return F.cross_entropy(logits, labels)

    def fused():
        return ops.lm_loss(logits, labels, out=out)[0]

    def ce_backward():
        leaf.grad = None
        F.cross_entropy(leaf, labels).backward()

    def fused_backward():
        leaf.grad = None
        FusedLmLoss.apply(leaf, labels, -100)[0].backward()

    want, got = float(ce()), float(fused())
    ce_backward()
    grad = leaf.grad.clone()
    fused_backward()
    emit(f"logits [{rows}, {VOCAB}] fp32, {logits.numel() * 4 / 1e6:.0f} MB; one read at 6.29 TB/s: "
         f"{logits.numel() * 4 / COPY_RATE * 1e3:.4f} ms")
    emit(f"    loss: F.cross_entropy {want:.7f}, ops.lm_loss {got:.7f}; max |dlogits difference| "
         f"{float((leaf.grad - grad).abs().max()):.3g} (largest |dlogits| {float(grad.abs().max()):.3g})")
    del grad
    leaf.grad = None
    times = timed({"F.cross_entropy, no grad": ce, "ops.lm_loss": fused, "F.cross_entropy + backward": ce_backward,
                   "FusedLmLoss + backward": fused_backward}, reps, inner)
    emit("  forward, autograd off")
    compare(emit, times, "F.cross_entropy, no grad", "ops.lm_loss")
    read = logits.numel() * 4 / COPY_RATE * 1e3
    emit(f"    ops.lm_loss is {statistics.median(times['ops.lm_loss']) / read:.2f}x the time of one read of the logits at 6.29 TB/s")
    emit("  forward + backward through autograd")
    compare(emit, times, "F.cross_entropy + backward", "FusedLmLoss + backward")
    emit("  torch.cuda.max_memory_allocated above what is held before the call (the gradient's own "
         f"{logits.numel() * 4 / 1e6:.0f} MB included in the backward forms)")
    for name, fn in (("F.cross_entropy, no grad", ce), ("ops.lm_loss", fused), ("F.cross_entropy + backward", ce_backward),
                     ("FusedLmLoss + backward", fused_backward)):
        leaf.grad = None
        emit(f"    {name:<34} {peak_above(fn) / 1e6:10.1f} MB")
    emit("")


def score_forms(emit, batch, reps):
    from decode_bench import build
    n, steps = 6, 62
    q, ids, mask = build(batch, 512, 12)
    dev = ids.device
    labels = torch.randint(3, VOCAB, (batch * n, steps), device=dev)
    rep_ids, rep_mask = ids.repeat_interleave(n, 0), mask.repeat_interleave(n, 0)

    def grouped():
        return q.score(ids, labels, attention_mask=mask, num_candidates=n)

    def repeated():
        return q.score(rep_ids, labels, attention_mask=rep_mask)

    a, b = grouped(), repeated()
    emit(f"score() on the BART-large shape, W6A6: {batch} inputs of 512 tokens, {n} candidates of {steps} tokens each "
         f"({batch * n * steps} rows of logits)")
    emit(f"    max |token log-prob difference| between the two forms {float((a[0] - b[0]).abs().max()):.3g}")
    times = timed({"score(), inputs repeated 6 times": repeated, "score(num_candidates=6)": grouped}, reps, 1)
    compare(emit, times, "score(), inputs repeated 6 times", "score(num_candidates=6)")
    emit("")


SHARE_SWITCHES = ("all switches off", "FUSE_SOFTMAX", "FUSE_ATTENTION_INT", "FUSE_ATTENTION")


def share_forms(emit, batch, reps):
    from decode_bench import build
    from outlier_suppression_amd import util_layernorm as UL
    n, steps = 6, 62
    q, ids, mask = build(batch, 512, 12)
    labels = torch.randint(3, VOCAB, (batch * n, steps), device=ids.device)
    names = ("FUSE_SOFTMAX", "FUSE_ATTENTION_INT", "FUSE_ATTENTION")
    old = {name: getattr(UL, name) for name in names}

    def form(switch, share):
        def run():
            for name in names:
                setattr(UL, name, name == switch)
            return q.score(ids, labels, attention_mask=mask, num_candidates=n, share_cross_kv=share)
        return run
    emit(f"score(num_candidates={n}) on the BART-large shape, W6A6: {batch} inputs of 512 tokens, {n} candidates of {steps} "
         f"tokens each; unshared (the encoder states repeated {n} times) against share_cross_kv=True")
    forms = {}
    for switch in SHARE_SWITCHES:
        forms[f"{switch}, unshared"], forms[f"{switch}, shared"] = form(switch, False), form(switch, True)
    try:
        for switch in SHARE_SWITCHES:
            a, b = forms[f"{switch}, unshared"](), forms[f"{switch}, shared"]()
            info = q.last_share_cross_kv
            emit(f"  {switch}: {info}; largest |token log-prob difference| shared - unshared "
                 f"{float((a[0] - b[0]).abs().max()):.3g} (largest |token log-prob| {float(a[0].abs().max()):.3g})")
            del a, b
        times = timed(forms, reps, 1)
        for switch in SHARE_SWITCHES:
            emit(f"  {switch}")
            compare(emit, times, f"{switch}, unshared", f"{switch}, shared")
            for name in (f"{switch}, unshared", f"{switch}, shared"):
                emit(f"    {name:<34} peak memory above the inputs {peak_above(forms[name]) / 1e6:10.1f} MB")
    finally:
        for name, value in old.items():
            setattr(UL, name, value)
    emit("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--share", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "score_bench.py measures on a GPU"
    lines = []

    def emit(line):
        print(line, flush=True)
        lines.append(line)
    if args.share:
        emit(f"tools/score_bench.py --share on {torch.cuda.get_device_name(0)}: medians of {args.reps} calls [min, max], every "
             "form in turn within each round")
        emit("")
        share_forms(emit, args.batch, args.reps)
    else:
        emit(f"tools/score_bench.py on {torch.cuda.get_device_name(0)}: medians of {args.reps} windows of {args.inner} calls "
             "[min, max], every form in turn within each round")
        emit("")
        for rows in (32 * 62, 32 * 128):
            loss_forms(emit, rows, args.reps, args.inner)
        if not args.no_model:
            score_forms(emit, args.batch, args.reps)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

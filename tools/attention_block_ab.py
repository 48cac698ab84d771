#!/usr/bin/env python3
"""A/B of the attention block over a whole sequence (csrc/attention_block.hip, csrc/attention_int.hip): the eager sequence,
the eager sequence with the one-launch probabilities site (util_layernorm.FUSE_SOFTMAX), the one-launch block in fp32
(util_layernorm.FUSE_ATTENTION) and the one-launch block on integer codes (util_layernorm.FUSE_ATTENTION_INT), in
one process, every form timed in turn within each of the --reps rounds; a time is the median of the rounds with [min, max],
a device synchronisation at either end of a round's --inner calls.  Before a block is timed the outputs of its four forms
are asserted within one quantization step of each other, and the number of codes that differ is printed.

  the block alone   from the fake-quantised q / k / v [B, h, T | S, d] to the quantised merged context [B, T, h * d], what
                    QuantizedBartAttention._attend runs before its output projection (W6A6 LSQ+ quantizers in the plain
                    quantising state; BERT shapes with the padding mask [B, 1, 1, S], the decoder's self-attention with the
                    causal mask [B, 1, T, S]): [B, h, T, S, d] = [32,12,128,128,64], [32,12,384,384,64], BART-large's encoder
                    [32,16,512,512,64], its decoder's self- [192,16,62,62,64] and cross-attention [192,16,62,512,64], and its
                    encoder at 1024 tokens [8,16,1024,1024,64];
  the shared row    (--shared runs it alone) both one-launch kernels on the cross-attention of score(num_candidates=6):
                    [32 x 6, 16, 62, 512, 64] with ``group=6`` -- 6 x 62 query rows over ONE copy of each input's keys and
                    values -- against [192, 16, 62, 512, 64] on the repeated copies; the outputs are asserted word-equal;
  models            (--no-models skips them) a random-init BERT-base forward at 32 x 128 and 32 x 384; on the random-init
                    BART-large shape of tools/decode_bench.py the encoder pass at 32 x 512, score(num_candidates=6) and
                    generate(max_length=62, num_beams=6).

    python tools/attention_block_ab.py [--reps 7] [--out profiles/attention_block_ab.txt]
"""
import argparse
import copy
import os
import statistics
import sys
import time
from types import SimpleNamespace as NS

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

FORMS = (("eager", False, False, False), ("FUSE_SOFTMAX", True, False, False), ("FUSE_ATTENTION", False, True, False),
         ("FUSE_ATTENTION_INT", False, False, True))
INT = "FUSE_ATTENTION_INT"
BLOCKS = (("bert-base 32x128", (32, 12, 128, 128, 64), "pad"), ("bert-base 32x384", (32, 12, 384, 384, 64), "pad"),
          ("bart-large encoder", (32, 16, 512, 512, 64), "pad"), ("bart-large decoder self", (192, 16, 62, 62, 64), "causal"),
          ("bart-large decoder cross", (192, 16, 62, 512, 64), "pad"), ("bart-large encoder 8x1024", (8, 16, 1024, 1024, 64), "pad"))
A_Q = NS(quantizer="LSQPlusFakeQuantize", observer="AvgMinMaxObserver", bit=6, symmetric=False, ch_axis=-1)
W_Q = NS(quantizer="FixedFakeQuantize", observer="MinMaxObserver", bit=6, symmetric=True, ch_axis=0)


def set_form(softmax, attention, attention_int=False):
    from outlier_suppression_amd import util_layernorm as UL
    UL.FUSE_SOFTMAX, UL.FUSE_ATTENTION, UL.FUSE_ATTENTION_INT = softmax, attention, attention_int


def timed(fn, reps, inner):
    """{form: [ms per call] * reps}: every form in turn within each round, two warm-up rounds first."""
    times = {name: [] for name, *_ in FORMS}
    for r in range(reps + 2):
        for name, *switches in FORMS:
            set_form(*switches)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(inner):
                fn()
            torch.cuda.synchronize()
            if r >= 2:
                times[name].append((time.perf_counter() - t0) * 1e3 / inner)
    set_form(False, False)
    return times


def report(emit, times):
    base = times["eager"]
    mb = statistics.median(base)
    spread = (max(base) - min(base)) / mb
    for name, *_ in FORMS:
        ts = times[name]
        m = statistics.median(ts)
        line = f"    {name:<18} {m:9.4f} ms [{min(ts):.4f}, {max(ts):.4f}]"
        if name != "eager":
            gain = (mb - m) / mb
            line += (f"   {mb / m:5.2f}x eager; the difference ({gain * 100:+.1f} %) "
                     f"{'exceeds' if abs(gain) > spread else 'does NOT exceed'} eager's own spread ({spread * 100:.1f} %)")
        emit(line)
    # the integer form against the other two switches, each difference held to that baseline's own spread
    m = statistics.median(times[INT])
    for name in ("FUSE_SOFTMAX", "FUSE_ATTENTION"):
        ts = times[name]
        mo = statistics.median(ts)
        gain, spread = (mo - m) / mo, (max(ts) - min(ts)) / mo
        emit(f"    {INT} {'wins against' if m < mo else 'LOSES to'} {name}: {mo / m:5.2f}x; the difference ({gain * 100:+.1f} %) "
             f"{'exceeds' if abs(gain) > spread else 'does NOT exceed'} {name}'s own spread ({spread * 100:.1f} %)")


def outputs(fn):
    outs = {}
    for name, *switches in FORMS:
        set_form(*switches)
        with torch.no_grad():
            outs[name] = fn()
    set_form(False, False)
    return outs


def block_forms(emit, label, shape, mask_kind, reps, inner):
    from outlier_suppression_amd import util_layernorm as UL
    from outlier_suppression_amd.quantization import Quantizer
    b, h, t, s, d = shape
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(t * 1000 + s)
    q = torch.randn((b, h, t, d), generator=g, device=dev) * (d ** -0.5 * 2.0)
    k, v = (torch.randn((b, h, s, d), generator=g, device=dev) for _ in range(2))
    lengths = torch.randint(s // 2, s + 1, (b,), generator=g, device=dev)
    mask = torch.zeros((b, 1, 1, s), device=dev).masked_fill(torch.arange(s, device=dev)[None, None, None] >= lengths[:, None, None, None],
                                                             torch.finfo(torch.float32).min)
    if mask_kind == "causal":
        mask = torch.full((t, s), torch.finfo(torch.float32).min, device=dev).triu(1)[None, None].expand(b, 1, t, s).contiguous()
    probs_q, ctx_q, q_q, k_q, v_q = (Quantizer(None, A_Q).to(dev) for _ in range(5))
    with torch.no_grad():                                # q / k / v as their sites hand them on: fake-quantised
        for qz in (q_q, k_q, v_q):
            qz.enable_observer()
            qz.disable_fake_quant()
        q_q(q), k_q(k), v_q(v)
        for qz in (q_q, k_q, v_q):
            qz.disable_observer()
            qz.enable_fake_quant()
        q, k, v = q_q(q), k_q(k), v_q(v)

    def block():
        out = UL.attention_int_block_fake_quant(q_q, k_q, v_q, probs_q, ctx_q, q, k, v, mask, dropout=(0.0, False))
        if out is not None:
            return out
        out = UL.attention_block_fake_quant(probs_q, ctx_q, q, k, v, mask, dropout=(0.0, False))
        if out is not None:
            return out
        w = torch.bmm(q.view(b * h, t, d), k.view(b * h, s, d).transpose(1, 2))
        probs = UL.attention_probs_fake_quant(probs_q, w, mask, dropout=(0.0, False), seq_pos=2, heads=h)
        return UL.merge_heads_fake_quant(ctx_q, torch.bmm(probs, v.view(b * h, s, d)).view(b, h, t, d))
    with torch.no_grad():
        for qz in (probs_q, ctx_q):                      # one observer pass, then the plain quantising state
            qz.enable_observer()
            qz.disable_fake_quant()
        block()
        for qz in (probs_q, ctx_q):
            qz.disable_observer()
            qz.enable_fake_quant()
        outs = outputs(block)
        step = float(ctx_q.scale.abs().max())
        emit(f"{label}: [B, h, T, S, d] = {list(shape)}, {mask_kind} mask; scores {b * h * t * s * 4 / 1e6:.0f} MB, "
             f"{4 * b * h * t * s * d / 1e9:.1f} GFLOP")
        for name in ("FUSE_SOFTMAX", "FUSE_ATTENTION", INT):
            diff = (outs[name] - outs["eager"]).abs()
            assert float(diff.max()) <= step * (1 + 1e-3), (name, float(diff.max()), step)
            emit(f"    {name} vs eager: {int((diff > 0.5 * step).sum())} of {diff.numel()} context codes differ (by one step)")
        report(emit, timed(block, reps, inner))
    emit("")


def shared_block(emit, reps, inner):
    """The cross-attention of score(num_candidates=6) on the BART-large shape in both one-launch kernels, grouped against
    unshared, every form timed in turn within each round."""
    from outlier_suppression_amd import _hip, util_layernorm as UL
    from outlier_suppression_amd.quantization import Quantizer
    b, n, h, t, s, d = 32, 6, 16, 62, 512, 64
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(t * 1000 + s)
    q = torch.randn((b * n, h, t, d), generator=g, device=dev) * (d ** -0.5 * 2.0)
    k, v = (torch.randn((b, h, s, d), generator=g, device=dev) for _ in range(2))
    lengths = torch.randint(s // 2, s + 1, (b,), generator=g, device=dev)
    mask = torch.zeros((b, 1, 1, s), device=dev).masked_fill(torch.arange(s, device=dev)[None, None, None] >= lengths[:, None, None, None],
                                                             torch.finfo(torch.float32).min)
    probs_q, ctx_q, q_q, k_q, v_q = (Quantizer(None, A_Q).to(dev) for _ in range(5))
    _hip.load()                                          # the first load applies the environment's tier, the switches included
    set_form(False, True, True)
    with torch.no_grad():
        for qz in (q_q, k_q, v_q):
            qz.enable_observer()
            qz.disable_fake_quant()
        q_q(q), k_q(k), v_q(v)
        for qz in (q_q, k_q, v_q):
            qz.disable_observer()
            qz.enable_fake_quant()
        q, k, v = q_q(q), k_q(k), v_q(v)
        kr, vr, mr = (x.repeat_interleave(n, dim=0) for x in (k, v, mask))
        for qz in (probs_q, ctx_q):                      # one observer pass through the eager lines, then the plain state
            qz.enable_observer()
            qz.disable_fake_quant()
        w = torch.bmm(q.view(b * n * h, t, d), kr.view(b * n * h, s, d).transpose(1, 2))
        probs = UL.attention_probs_fake_quant(probs_q, w, mr, dropout=(0.0, False), seq_pos=2, heads=h)
        UL.merge_heads_fake_quant(ctx_q, torch.bmm(probs, vr.view(b * n * h, s, d)).view(b * n, h, t, d))
        del w, probs
        for qz in (probs_q, ctx_q):
            qz.disable_observer()
            qz.enable_fake_quant()
        forms = {
            "FUSE_ATTENTION_INT unshared": lambda: UL.attention_int_block_fake_quant(q_q, k_q, v_q, probs_q, ctx_q, q, kr, vr, mr, dropout=(0.0, False)),
            "FUSE_ATTENTION_INT group=6": lambda: UL.attention_int_block_fake_quant(q_q, k_q, v_q, probs_q, ctx_q, q, k, v, mask, dropout=(0.0, False), group=n),
            "FUSE_ATTENTION unshared": lambda: UL.attention_block_fake_quant(probs_q, ctx_q, q, kr, vr, mr, dropout=(0.0, False)),
            "FUSE_ATTENTION group=6": lambda: UL.attention_block_fake_quant(probs_q, ctx_q, q, k, v, mask, dropout=(0.0, False), group=n),
        }
        outs = {name: fn() for name, fn in forms.items()}
        for name, out in outs.items():                   # a form that did not launch is an error here, with its reason
            if out is None:
                grouped = name.endswith("group=6")
                why = UL.attention_int_refusal(q_q, k_q, v_q, probs_q, ctx_q, q, k if grouped else kr, v if grouped else vr,
                                               mask if grouped else mr, (0.0, False), n if grouped else 1)
                raise RuntimeError(f"{name} did not launch (the integer form's own objection: {why}; last library error: "
                                   f"{_hip.load().osq_last_error().decode()!r})")
        emit(f"bart-large decoder cross, shared: [B x G, h, T, S, d] = [{b} x {n}, {h}, {t}, {s}, {d}] with group={n} against "
             f"[{b * n}, {h}, {t}, {s}, {d}] unshared, pad mask")
        for kernel in ("FUSE_ATTENTION_INT", "FUSE_ATTENTION"):
            same = torch.equal(outs[f"{kernel} group=6"].view(torch.int32), outs[f"{kernel} unshared"].view(torch.int32))
            assert same, kernel
            emit(f"    {kernel}: the grouped launch's context is word-equal to the unshared launch's")
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
    set_form(False, False)
    for kernel in ("FUSE_ATTENTION_INT", "FUSE_ATTENTION"):
        base, new = times[f"{kernel} unshared"], times[f"{kernel} group=6"]
        mb, mn = statistics.median(base), statistics.median(new)
        gain, spread = (mb - mn) / mb, (max(base) - min(base)) / mb
        emit(f"    {kernel + ' unshared':<30} {mb:9.4f} ms [{min(base):.4f}, {max(base):.4f}]")
        emit(f"    {kernel + ' group=6':<30} {mn:9.4f} ms [{min(new):.4f}, {max(new):.4f}]   {mb / mn:5.2f}x unshared; the difference "
             f"({gain * 100:+.1f} %) {'exceeds' if abs(gain) > spread else 'does NOT exceed'} the unshared form's own spread "
             f"({spread * 100:.1f} %)")
    emit("")


def model_forms(emit, label, fn, reps, inner):
    """A model call in the four forms.  A random-init W6A6 model carries a code that flips in one block through every
    later layer, so its outputs are not held to a bar here (tests/test_gpu_attention_block_model.py holds calibrated models
    to the project's bars): they must be finite, and how far they lie apart is printed."""
    outs = outputs(fn)
    for name in ("FUSE_SOFTMAX", "FUSE_ATTENTION", INT):
        a, e = outs[name], outs["eager"]
        if a.dtype.is_floating_point:
            assert bool(torch.isfinite(a).all()), (label, name)
            diff = (a - e).abs()
            emit(f"{label}: {name} vs eager max |difference| {float(diff.max()):.3g} (largest |eager| {float(e.abs().max()):.3g}), "
                 f"{float((diff > 1e-3).float().mean()) * 100:.2f} % of the entries differ by more than 1e-3")
        else:
            same = a.shape == e.shape and bool((a == e).all())
            emit(f"{label}: {name} vs eager tokens {'equal' if same else 'DIFFER'}")
    with torch.no_grad():
        report(emit, timed(fn, reps, inner))
    emit("")


def bert_base(batch, length):
    from transformers import BertConfig, BertForSequenceClassification
    from outlier_suppression_amd.quant_model import quantize_model
    from outlier_suppression_amd.quantization import disable_all, enable_calibration_woquantization, enable_quantization
    torch.manual_seed(0)
    dev = torch.device("cuda:0")
    fp = BertForSequenceClassification(BertConfig(hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)).eval()
    q = quantize_model(copy.deepcopy(fp), W_Q, A_Q).to(dev).eval()
    ids = torch.randint(3, 30000, (batch, length), device=dev)
    mask = torch.ones_like(ids)
    mask[1::2, length - length // 4:] = 0
    enable_calibration_woquantization(q)
    with torch.no_grad():
        q(input_ids=ids[:2], attention_mask=mask[:2], token_type_ids=torch.zeros_like(ids[:2]))
    disable_all(q)
    enable_quantization(q)
    return q, ids, mask


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--no-models", action="store_true")
    ap.add_argument("--shared", action="store_true", help="the shared row alone")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "attention_block_ab.py measures on a GPU"
    lines = []

    def emit(line):
        print(line, flush=True)
        lines.append(line)
    emit(f"tools/attention_block_ab.py on {torch.cuda.get_device_name(0)}: medians of {args.reps} rounds of --inner calls "
         "[min, max], every form in turn within each round")
    emit("")
    for label, shape, mask_kind in () if args.shared else BLOCKS:
        block_forms(emit, label, shape, mask_kind, args.reps, args.inner)
        torch.cuda.empty_cache()
    shared_block(emit, args.reps, args.inner)
    torch.cuda.empty_cache()
    if not args.no_models and not args.shared:
        for length in (128, 384):
            q, ids, mask = bert_base(32, length)
            tt = torch.zeros_like(ids)
            model_forms(emit, f"BERT-base forward 32 x {length}, W6A6",
                        lambda: q(input_ids=ids, attention_mask=mask, token_type_ids=tt)[0], args.reps, 2)
            del q
            torch.cuda.empty_cache()
        from decode_bench import build
        q, ids, mask = build(32, 512, 12)
        model_forms(emit, "BART-large shape, encoder pass 32 x 512", lambda: q.get_encoder()(ids, attention_mask=mask),
                    args.reps, 1)
        labels = torch.randint(3, 50265, (32 * 6, 62), device=ids.device)
        model_forms(emit, "BART-large shape, score(num_candidates=6), 62 tokens",
                    lambda: q.score(ids, labels, attention_mask=mask, num_candidates=6)[0], args.reps, 1)
        model_forms(emit, "BART-large shape, generate(max_length=62, num_beams=6)",
                    lambda: q.generate(ids, attention_mask=mask, max_length=62, num_beams=6), args.reps, 1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""A/B of the integer linear layers (csrc/linear_int.hip, util_layernorm.FUSE_LINEAR_INT) against ``F.linear`` on the
fake-quantised weight, in one process, both forms timed in turn within each of the --reps rounds; a time is the median of the
rounds with [min, max], a device synchronisation at either end of a round's --inner calls.  A difference counts only where it
exceeds the baseline's own range.

  layers   F.linear(x, w_fq, bias) against ops.activation_codes + ops.linear_int on the same operands (W6A6: per-channel 6-bit
           weights, a per-tensor 6-bit producer).  BERT-base at M = 32 x 128 and 32 x 384: 768 -> 768, query / key / value
           together (three products, ONE encode), 768 -> 3072, 3072 -> 768; BART-large at M = 32 x 512: 1024 -> 4096 and
           4096 -> 1024; one decoding step of 192 rows, 1024 -> 1024 and 1024 -> 4096; the pooler's 32 rows 768 -> 768.
           Before a layer is timed the two outputs are held to 2**-14 of the largest |output| (fp32 GEMM rounding at K = 4096).
  models   (--no-models skips them) the calls tools/attention_block_ab.py reports: a random-init BERT-base forward at 32 x 128
           and 32 x 384, the BART-large encoder pass at 32 x 512 and score(num_candidates=6).

  w4       (--w4: these rows alone) a weight quantizer of 16 codes: ops.linear_int on the packed entry, ops.weight_codes(bits=4),
           against the SAME call on the 8-bit entry of the same weight -- the baseline is the 8-bit form -- one activation_codes
           output shared by both and made outside the timed calls.  The two outputs are held word-equal first.  The rows kernel:
           BART's lm_head at 1 and 32 rows, the pooler, 1024 -> 4096 at 32 rows; the tile kernel: 768 -> 3072 at 4096 rows,
           4096 -> 1024 at 16384, 1024 -> 1024 at 192.

  ffn      (--ffn: these rows alone) a feed-forward block's integer launches from fc1's activation codes on (made outside the
           timed calls): the chain ops.linear_int -> ops.gelu_fake_quant_per_tensor -> ops.activation_codes -> ops.linear_int
           against ops.linear_int_codes -> ops.linear_int on the same operands, 8-bit and packed weights; the two results are
           held word-equal first.  Then BERT-base at 32 x 128 and the BART-large encoder pass with linear_int.FUSE_FFN off and
           on (FFN_MAX_ROWS lifted: the path at every M), both under set_fast_linear_int(True).  The baseline is the chain.

    python tools/linear_int_ab.py [--reps 7] [--out profiles/linear_int_ab.txt]
    python tools/linear_int_ab.py --ffn --inner 20 --out profiles/linear_int_codes_ab.txt
    python tools/linear_int_ab.py --w4 --inner 100 --out profiles/linear_int_w4_ab.txt
"""
import argparse
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

LAYERS = (("bert-base 32x128", 32 * 128, ((768, 768, 1), (768, 768, 3), (768, 3072, 1), (3072, 768, 1))),
          ("bert-base 32x384", 32 * 384, ((768, 768, 1), (768, 768, 3), (768, 3072, 1), (3072, 768, 1))),
          ("bart-large 32x512", 32 * 512, ((1024, 4096, 1), (4096, 1024, 1))),
          ("bart-large decoding step", 192, ((1024, 1024, 1), (1024, 4096, 1))),
          ("bert-base pooler", 32, ((768, 768, 1),)))


W4_LAYERS = ((1, 1024, 50265), (32, 1024, 50265), (32, 768, 768), (32, 1024, 4096), (4096, 768, 3072), (16384, 4096, 1024),
             (192, 1024, 1024))


def timed(forms, reps, inner):
    times = {name: [] for name in forms}
    for r in range(reps + 2):                            # two warm-up rounds
        for name, fn in forms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(inner):
                fn()
            torch.cuda.synchronize()
            if r >= 2:
                times[name].append((time.perf_counter() - t0) * 1e3 / inner)
    return times


def report(emit, times, base="F.linear", new="linear_int"):
    tb, tn = times[base], times[new]
    mb, mn = statistics.median(tb), statistics.median(tn)
    gain, spread = (mb - mn) / mb, (max(tb) - min(tb)) / mb
    emit(f"    {base:<12} {mb:9.4f} ms [{min(tb):.4f}, {max(tb):.4f}]")
    emit(f"    {new:<12} {mn:9.4f} ms [{min(tn):.4f}, {max(tn):.4f}]   {mb / mn:5.2f}x {base}: "
         f"{'a win' if mn < mb else 'a LOSS'}; the difference ({gain * 100:+.1f} %) "
         f"{'exceeds' if abs(gain) > spread else 'does NOT exceed'} {base}'s own range ({spread * 100:.1f} %)")


def layer(emit, m, k, n, count, reps, inner):
    from outlier_suppression_amd import ops
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(m + k + n)
    s_x = torch.tensor([0.05], device=dev)
    zp_x = torch.tensor([31], dtype=torch.int32, device=dev)
    record = (s_x, zp_x, 0, 63, ops.PARAM_FIXED, 1.0)
    x = ops.fake_quant_per_tensor(torch.randn((m, k), generator=g, device=dev), s_x, zp_x, 0, 63)
    ws = [torch.randn((n, k), generator=g, device=dev) * 0.03 for _ in range(count)]
    scales = [w.abs().amax(1) / 31 for w in ws]
    zps = torch.zeros(n, dtype=torch.int32, device=dev)
    biases = [torch.randn(n, generator=g, device=dev) for _ in range(count)]
    w_fq = [ops.fake_quant_per_channel(w, s, zps, 0, -32, 31) for w, s in zip(ws, scales)]
    entries = [ops.weight_codes(w, s, zps, 0, -32, 31) for w, s in zip(ws, scales)]

    def eager():
        return [F.linear(x, w, b) for w, b in zip(w_fq, biases)]

    def integer():
        codes, rowsum = ops.activation_codes(x, record)
        return [ops.linear_int(codes, rowsum, record, e, b) for e, b in zip(entries, biases)]
    for a, e in zip(integer(), eager()):
        tol = 2.0 ** -14 * float(e.abs().max())
        assert float((a - e).abs().max()) <= tol, (float((a - e).abs().max()), tol)
    emit(f"  [{m}, {k}] -> {n}" + (f", {count} products of one input" if count > 1 else ""))
    report(emit, timed({"F.linear": eager, "linear_int": integer}, reps, inner))


def layer_w4(emit, m, k, n, reps, inner):
    from outlier_suppression_amd import ops
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(m + k + n)
    s_x = torch.tensor([0.05], device=dev)
    zp_x = torch.tensor([127], dtype=torch.int32, device=dev)
    record = (s_x, zp_x, 0, 255, ops.PARAM_FIXED, 1.0)
    w = torch.randn((n, k), generator=g, device=dev) * 0.03
    scale, zps = w.abs().amax(1) / 7, torch.zeros(n, dtype=torch.int32, device=dev)
    bias = torch.randn(n, generator=g, device=dev)
    codes, rowsum = ops.activation_codes(torch.randn((m, k), generator=g, device=dev), record)
    entries = {bits: ops.weight_codes(w, scale, zps, 0, -8, 7, bits=bits) for bits in (8, 4)}
    forms = {"linear_int": lambda: ops.linear_int(codes, rowsum, record, entries[8], bias),
             "linear_int_w4": lambda: ops.linear_int(codes, rowsum, record, entries[4], bias)}
    assert torch.equal(forms["linear_int"](), forms["linear_int_w4"]()) and tuple(entries[4].codes.shape) == (n, k // 2)
    emit(f"  [{m}, {k}] -> {n}: {entries[8].codes.numel()} and {entries[4].codes.numel()} weight bytes, the same words")
    report(emit, timed(forms, reps, inner), "linear_int", "linear_int_w4")


FFN_LAYERS = ((4096, 768, 3072), (16384, 1024, 4096), (192, 1024, 4096), (32, 1024, 4096), (1, 1024, 4096))


def layer_ffn(emit, m, h, f, bits, reps, inner):
    """[m, h] -> f -> h: W8A8, or W4A8 on packed entries."""
    from outlier_suppression_amd import ops
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(m + h + f)
    zp = torch.tensor([127], dtype=torch.int32, device=dev)
    record = (torch.tensor([0.05], device=dev), zp, 0, 255, ops.PARAM_FIXED, 1.0)
    mid = (torch.tensor([0.02], device=dev), torch.tensor([9], dtype=torch.int32, device=dev), 0, 255, ops.PARAM_FIXED, 1.0)
    top = 2 ** (bits - 1) - 1
    entries, biases = [], []
    for n, k in ((f, h), (h, f)):
        w = torch.randn((n, k), generator=g, device=dev) * 0.03
        entries.append(ops.weight_codes(w, w.abs().amax(1) / top, torch.zeros(n, dtype=torch.int32, device=dev), 0, -top - 1, top, bits=bits))
        biases.append(torch.randn(n, generator=g, device=dev))
    codes, rowsum = ops.activation_codes(torch.randn((m, h), generator=g, device=dev), record)

    def chain():
        y = ops.gelu_fake_quant_per_tensor(ops.linear_int(codes, rowsum, record, entries[0], biases[0]), *mid)
        return ops.linear_int(*ops.activation_codes(y, mid), mid, entries[1], biases[1])

    def fused():
        return ops.linear_int(*ops.linear_int_codes(codes, rowsum, record, entries[0], biases[0], mid), mid, entries[1], biases[1])
    want = chain()
    assert torch.equal(fused(), want) and bool(torch.isfinite(want).all())
    emit(f"  [{m}, {h}] -> {f} -> {h}, W{bits}A8: the same words")
    report(emit, timed({"chain": chain, "ffn": fused}, reps, inner), "chain", "ffn")


def model_ffn(emit, label, fn, reps, inner):
    import outlier_suppression_amd as osq
    from outlier_suppression_amd import util_layernorm as UL
    from outlier_suppression_amd.quantization import linear_int

    def form(on):
        def call():
            linear_int.FUSE_FFN = on
            with torch.no_grad():
                return fn()
        return call
    old = linear_int.FUSE_FFN, linear_int.FFN_MAX_ROWS
    linear_int.FFN_MAX_ROWS = None                       # the path at every M: what ffn's routing by rows is decided from
    osq.set_fast_linear_int(True)
    UL.linear_int.reset()
    on = form(True)()
    emit(f"{label}: {UL.linear_int}; the same words: {bool(torch.equal(on, form(False)()))}")
    report(emit, timed({"chain": form(False), "ffn": form(True)}, reps, inner), "chain", "ffn")
    osq.set_fast_linear_int(False)
    linear_int.FUSE_FFN, linear_int.FFN_MAX_ROWS = old
    emit("")


def model(emit, label, fn, reps, inner):
    import outlier_suppression_amd as osq
    from outlier_suppression_amd import util_layernorm as UL

    def form(on):
        def call():
            osq.set_fast_linear_int(on)
            with torch.no_grad():
                return fn()
        return call
    UL.linear_int.reset()
    on, off = form(True)(), form(False)()
    emit(f"{label}: {UL.linear_int}; max |difference| {float((on - off).abs().max()):.3g} (largest |F.linear form| "
         f"{float(off.abs().max()):.3g})")
    assert bool(torch.isfinite(on).all())
    report(emit, timed({"F.linear": form(False), "linear_int": form(True)}, reps, inner))
    osq.set_fast_linear_int(False)
    emit("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--no-models", action="store_true")
    ap.add_argument("--w4", action="store_true", help="the packed 4-bit weight rows alone")
    ap.add_argument("--ffn", action="store_true", help="the feed-forward rows alone: fc1 writing fc2's codes against the chain")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "linear_int_ab.py measures on a GPU"
    lines = []

    def emit(line):
        print(line, flush=True)
        lines.append(line)
    emit(f"tools/linear_int_ab.py on {torch.cuda.get_device_name(0)}: medians of {args.reps} rounds of --inner calls [min, max], "
         "both forms in turn within each round" + ("" if args.w4 or args.ffn else "; linear_int includes its activation_codes launch"))
    emit("")
    if args.w4:
        emit("packed 4-bit weights against the 8-bit entry of the same weight (W4A8), ops.linear_int alone, "
             f"{args.inner} calls to a round")
        for m, k, n in W4_LAYERS:
            layer_w4(emit, m, k, n, args.reps, args.inner)
            torch.cuda.empty_cache()
    if args.ffn:
        emit(f"fc1 writing fc2's codes (ops.linear_int_codes) against the chain of launches it replaces, {args.inner} calls to a round")
        for m, h, f in FFN_LAYERS:
            for bits in (8, 4):
                layer_ffn(emit, m, h, f, bits, args.reps, args.inner)
            torch.cuda.empty_cache()
        emit("")
        if not args.no_models:
            from attention_block_ab import bert_base
            q, ids, mask = bert_base(32, 128)
            tt = torch.zeros_like(ids)
            model_ffn(emit, "BERT-base forward 32 x 128, W6A6", lambda: q(input_ids=ids, attention_mask=mask, token_type_ids=tt)[0], args.reps, 2)
            del q
            torch.cuda.empty_cache()
            from decode_bench import build
            q, ids, mask = build(32, 512, 12)
            model_ffn(emit, "BART-large shape, encoder pass 32 x 512", lambda: q.get_encoder()(ids, attention_mask=mask)[0], args.reps, 1)
    for label, m, shapes in ((), LAYERS)[not (args.w4 or args.ffn)]:
        emit(f"{label}: M = {m}")
        for k, n, count in shapes:
            layer(emit, m, k, n, count, args.reps, args.inner)
        emit("")
        torch.cuda.empty_cache()
    if not args.no_models and not args.w4 and not args.ffn:
        from attention_block_ab import bert_base
        for length in (128, 384):
            q, ids, mask = bert_base(32, length)
            tt = torch.zeros_like(ids)
            model(emit, f"BERT-base forward 32 x {length}, W6A6", lambda: q(input_ids=ids, attention_mask=mask, token_type_ids=tt)[0],
                  args.reps, 2)
            del q
            torch.cuda.empty_cache()
        from decode_bench import build
        q, ids, mask = build(32, 512, 12)
        model(emit, "BART-large shape, encoder pass 32 x 512", lambda: q.get_encoder()(ids, attention_mask=mask), args.reps, 1)
        labels = torch.randint(3, 50265, (32 * 6, 62), device=ids.device)
        model(emit, "BART-large shape, score(num_candidates=6), 62 tokens",
              lambda: q.score(ids, labels, attention_mask=mask, num_candidates=6)[0], args.reps, 1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

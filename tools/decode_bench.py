"""Decoder-step A/B of incremental decoding: the one-launch q/k/v + KV-cache append (util_layernorm.FUSE_KV_APPEND) against
the eager form (quantizer, head split, index_select, torch.cat).

BART-large shape, random init (d_model 1024, 12 + 12 layers, 16 heads, vocab 50265), W6A6 in the plain quantising state,
batch 32 x 6 beams, source 512.  Times one decoder step (all 12 layers + lm_head, a beam reorder pending as in beam
search) at past length S = 1, 31, 62, median and spread of --reps runs, and the whole generate(max_length=62, num_beams=6).
--profile-steps N only runs N cached decode steps (for ``rocprofv3 --kernel-trace --stats``: launches per step).
--fast-decode-attention: the A/B is instead the one-launch attention of a decoding step (util_layernorm.
FUSE_DECODE_ATTENTION, csrc/decode_attention.hip) off against on, the one-launch append on in both; with --profile-steps the
profiled steps run with the switch on.
--cache-codes: the A/B is the KV cache held as integer codes (util_layernorm.CACHE_CODES, csrc/kv_codes.hip) against the
fp32 cache, the one-launch append and the one-launch attention on in both; the cache of a timed step is filled token by
token, as generate() fills it (a first step of several tokens would demote the self-attention tensors of a coded cache),
and ``cache.nbytes()`` is reported both ways; with --profile-steps the profiled steps run with codes on.

    python tools/decode_bench.py [--reps 7] [--out profiles/decode_step_ab.txt]
    python tools/decode_bench.py --fast-decode-attention [--out profiles/decode_attention_ab.txt]
    python tools/decode_bench.py --cache-codes [--out profiles/kv_codes_ab.txt]
"""
import argparse
import copy
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build(batch, src_len, layers):
    from types import SimpleNamespace as NS
    from transformers import BartConfig, BartForConditionalGeneration
    from outlier_suppression_amd import util_layernorm as UL
    from outlier_suppression_amd.quant_model import quantize_model
    from outlier_suppression_amd.quantization import disable_all, enable_calibration_woquantization, enable_quantization
    torch.manual_seed(0)
    cfg = BartConfig(vocab_size=50265, d_model=1024, encoder_layers=layers, decoder_layers=layers, encoder_attention_heads=16,
                     decoder_attention_heads=16, encoder_ffn_dim=4096, decoder_ffn_dim=4096, max_position_embeddings=1024,
                     dropout=0.0, attention_dropout=0.0, activation_dropout=0.0)
    fp = BartForConditionalGeneration(cfg).eval()
    w = NS(quantizer="FixedFakeQuantize", observer="MinMaxObserver", bit=6, symmetric=True, ch_axis=0)
    a = NS(quantizer="LSQPlusFakeQuantize", observer="AvgMinMaxObserver", bit=6, symmetric=False, ch_axis=-1)
    dev = torch.device("cuda:0")
    q = quantize_model(copy.deepcopy(fp), w, a).to(dev).eval()
    del fp
    ids = torch.randint(3, 50265, (batch, src_len), device=dev)
    mask = torch.ones_like(ids)
    enable_calibration_woquantization(q)
    with torch.no_grad():
        q(ids[:2, :64], mask[:2, :64], decoder_input_ids=ids[:2, :8])
    disable_all(q)
    enable_quantization(q)
    assert UL.FUSE_KV_APPEND
    return q, ids, mask


def step_times(q, ids, mask, beams, past, reps, fused, attention=False, codes=None):
    """Median / min / max (ms) of one decoder step at past length `past` with a pending beam reorder, and the bytes the
    cache holds.  ``codes`` None: the cache filled by one call of `past` tokens; False / True: an fp32 / coded cache filled
    token by token."""
    from outlier_suppression_amd import util_layernorm as UL
    UL.FUSE_KV_APPEND = fused
    UL.FUSE_DECODE_ATTENTION = attention
    UL.CACHE_CODES = bool(codes)
    dev = ids.device
    bb = ids.shape[0] * beams
    try:
        with torch.no_grad():
            enc = q.get_encoder()(ids, attention_mask=mask).repeat_interleave(beams, 0)
            m = mask.repeat_interleave(beams, 0)
            tok = torch.randint(3, 50265, (bb, past + 1), device=dev)
            if codes is None:
                _, cache, _ = q(attention_mask=m, decoder_input_ids=tok[:, :past], encoder_outputs=(enc,), use_cache=True)
            else:
                cache = None
                for t in range(past):
                    _, cache, _ = q(attention_mask=m, decoder_input_ids=tok[:, t:t + 1], encoder_outputs=(enc,),
                                    past_key_values=cache, use_cache=True)
                assert bool(cache.coded()) is codes and not cache.demoted()
            perm = torch.randperm(bb, device=dev)
            lens = list(cache._len)
            times = []
            for r in range(reps + 2):
                cache._len = list(lens)
                cache.reorder(perm)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                q(attention_mask=m, decoder_input_ids=tok[:, past:past + 1], encoder_outputs=(enc,), past_key_values=cache,
                  use_cache=True)
                torch.cuda.synchronize()
                if r >= 2:
                    times.append((time.perf_counter() - t0) * 1e3)
            held = cache.nbytes()
            if codes:
                assert not cache.demoted() and cache.rejected() == 0
    finally:
        UL.FUSE_KV_APPEND = True
        UL.FUSE_DECODE_ATTENTION = False
        UL.CACHE_CODES = False
    times.sort()
    return times[len(times) // 2], times[0], times[-1], held


def generate_time(q, ids, mask, fused, attention=False, codes=None):
    from outlier_suppression_amd import util_layernorm as UL
    UL.FUSE_KV_APPEND = fused
    UL.FUSE_DECODE_ATTENTION = attention
    codes = bool(codes)
    try:
        with torch.no_grad():
            q.generate(ids[:2], attention_mask=mask[:2], max_length=4, num_beams=6, min_length=4, cache_codes=codes)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = q.generate(ids, attention_mask=mask, max_length=62, num_beams=6, min_length=62, cache_codes=codes)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, tuple(out.shape)
    finally:
        UL.FUSE_KV_APPEND = True
        UL.FUSE_DECODE_ATTENTION = False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--beams", type=int, default=6)
    ap.add_argument("--src", type=int, default=512)
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--profile-steps", type=int, default=0)
    ap.add_argument("--fast-decode-attention", action="store_true")
    ap.add_argument("--cache-codes", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    q, ids, mask = build(args.batch, args.src, args.layers)
    if args.profile_steps:
        from outlier_suppression_amd import util_layernorm as UL
        UL.FUSE_DECODE_ATTENTION = args.fast_decode_attention
        with torch.no_grad():
            q.generate(ids, attention_mask=mask, max_length=args.profile_steps + 1, num_beams=args.beams,
                       min_length=args.profile_steps + 1, cache_codes=args.cache_codes)
        torch.cuda.synchronize()
        return
    lines = [f"decoder step, BART-large shape (random init, {args.layers}+{args.layers} layers), W6A6 LSQ+ plain quantising, "
             f"batch {args.batch} x {args.beams} beams, source {args.src}; a beam reorder pending before every step; "
             f"{args.reps} runs each, ms: median [min, max]"]
    # (label, FUSE_KV_APPEND, FUSE_DECODE_ATTENTION, cache codes) of the two forms compared
    if args.cache_codes:
        forms = [("cache codes", True, True, True), ("cache fp32", True, True, False)]
        lines[0] += "; the q / k / v + append launch and the one-launch attention on in both; caches filled token by token"
    elif args.fast_decode_attention:
        forms = [("attention one-launch", True, True, None), ("attention eager", True, False, None)]
        lines[0] += "; the q / k / v + append launch on in both"
    else:
        forms = [("one-launch", True, False, None), ("eager", False, False, None)]
    for past in (1, 31, 62):
        row, held = [], []
        for label, fused, attention, codes in forms:
            med, lo, hi, nbytes = step_times(q, ids, mask, args.beams, past, args.reps, fused, attention, codes)
            row.append(f"{label} {med:.3f} [{lo:.3f}, {hi:.3f}]")
            held.append(f"{label} {nbytes}")
        lines.append(f"S = {past:2d}: " + "   ".join(row))
        if args.cache_codes:
            lines.append(f"        cache.nbytes() after the step: " + "   ".join(held))
    for label, fused, attention, codes in forms:
        secs, shape = generate_time(q, ids, mask, fused, attention, codes)
        lines.append(f"generate(max_length=62, num_beams=6, min_length=62) {label}: {secs:.2f} s, output {shape}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

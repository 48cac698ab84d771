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
--graph: the A/B is a captured graph of the step, replayed (model/graph_decode.py, generate(graph=True)), against the step
issued launch by launch -- with the default switches (the step as it was before graphs existed) and with the one-launch
attention on (the very launches the graph holds) -- for the fp32 and the coded cache; every form is timed in turn within
each of the --reps rounds, in one process; capture + instantiate time is reported apart.
--beam-select: the A/B is what beam search does with a step's logits -- log-softmax, the logits processors, the score add and
the top-k (generation._select_continuations) -- as the torch lines against ops.beam_select (csrc/beam_select.hip): those
steps alone on [batch * beams, 50265] logits at length 31 with min_length active, no_repeat_ngram_size 0 and 3; then the whole
generate() with the switch off and on, issued and with graph=True; and, once, the encoder pass alone.  Every form is timed
in turn within each of the --reps rounds, in one process.
--beam-advance: the A/B is the bookkeeping of a beam step after the selection (generation._advance_beams_torch) as the torch
lines against ops.beam_advance (csrc/beam_advance.hip): that step alone on the state and the top_lp / top_idx recorded at
length 31 of a generate() call; then generate(graph=True, beam_select=True) and the same issued launch by launch, with the
switch off and on.  Every form is timed in turn within each of the --reps rounds, in one process.
--beam-graph: the A/B is the whole beam step as one captured graph (generate(beam_graph=True); model/graph_decode.py,
BeamStepGraphs) against generate(graph=True, beam_select=True, beam_advance=True), where the selection and the bookkeeping
are issued between the replays: the whole call with no_repeat_ngram_size 0 and 3, the fp32 and the coded cache; every form
is timed in turn within each of the --reps rounds, in one process; capture + instantiate time is reported apart.
--greedy-advance: the A/B is greedy decoding with everything after the model step as one kernel call (ops.greedy_advance,
csrc/greedy_advance.hip; generate(greedy_advance=True)) and with the whole step as one captured graph
(generate(greedy_graph=True); graph_decode.GreedyStepGraph) against generate(graph=True), the best greedy form before them:
generate(num_beams=1, max_length=62, min_length=62) at batch 32 with no_repeat_ngram_size 0 and 3, the three forms with graphs
and the same three issued launch by launch (the one-launch attention on, so that every form computes the same words; asked
with graph=False, greedy_graph decodes as without it); then the bookkeeping alone -- the torch lines of generation._greedy
against the kernel call, each with its read of the stopping word -- on [32, 50265] logits at length 31.  The tokens of all
forms are asserted equal before a time is printed; every form is timed in turn within each of the --reps rounds, in one process.

    python tools/decode_bench.py [--reps 7] [--out profiles/decode_step_ab.txt]
    python tools/decode_bench.py --fast-decode-attention [--out profiles/decode_attention_ab.txt]
    python tools/decode_bench.py --cache-codes [--out profiles/kv_codes_ab.txt]
    python tools/decode_bench.py --graph [--out profiles/graph_decode_ab.txt]
    python tools/decode_bench.py --beam-select [--out profiles/beam_select_ab.txt]
    python tools/decode_bench.py --beam-advance [--out profiles/beam_advance_ab.txt]
    python tools/decode_bench.py --beam-graph [--out profiles/beam_graph_ab.txt]
    python tools/decode_bench.py --greedy-advance [--out profiles/greedy_advance_ab.txt]

--sample-advance: the A/B is seeded sampling (sample()) with everything after the model step as one kernel call
(ops.sample_advance, csrc/sample_advance.hip; sample(sample_advance=True)) and with the whole step as one captured graph
(sample(sample_graph=True); graph_decode.SampleStepGraph) against the torch lines of model/sampling.py, for top_k 50 with
top_p 0.95 and for the whole vocabulary, the tokens asserted equal between the forms first; then the selection alone against
transformers' own lines (warpers, softmax, torch.multinomial) and against sampling.select_torch.

    python tools/decode_bench.py --sample-advance [--out profiles/sample_advance_ab.txt]

--sample-nucleus: the same comparison for top_k=0, top_p=0.9 -- a nucleus over the whole vocabulary, which goes to
ops.sample_nucleus (csrc/sample_nucleus.hip) under sample(sample_nucleus=True) and to the torch lines without it:

    python tools/decode_bench.py --sample-nucleus [--out profiles/sample_nucleus_ab.txt]

--share-cross-kv: the A/B is beam search over ONE copy of the cross-attention keys / values per batch row
(generate(share_cross_kv=True); QuantizedBartCache(cross_group=beams); ops.decode_attention_shared,
csrc/decode_attention.hip) against one copy per beam, for the fp32 and the coded cache: the cross-attention launch alone
(device events around 50 launches); one decoder step as a replayed graph at S = 1 / 31 / 62; generate(graph=True,
beam_select=True, beam_advance=True); ``cache.nbytes()`` of both forms; and the largest logit difference over 12
teacher-forced steps.  Every form is timed in turn within each of the --reps rounds, in one process.

    python tools/decode_bench.py --share-cross-kv [--out profiles/share_cross_kv_ab.txt]

--sample-group: the A/B is sample(num_samples=--beams, sample_graph=True) over ONE copy of the cross-attention keys / values per
input (share_cross_kv=True) against one copy per sequence -- what a hand-repeated batch costs --, for top_k=50 / top_p=0.95 and
for the nucleus top_k=0 / top_p=0.9, with the fp32 and the coded cache; ``cache.nbytes()`` of both forms; and the step kernels
alone at [batch * beams, 50265] with and without ``logprobs``.  Every form is timed in turn within each of the --reps rounds.

    python tools/decode_bench.py --sample-group [--out profiles/sample_group_ab.txt]
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


def _stats(times):
    times = sorted(times)
    return f"{times[len(times) // 2]:.3f} [{times[0]:.3f}, {times[-1]:.3f}]"


# (label, FUSE_DECODE_ATTENTION, cache codes, graph) of the forms --graph compares
GRAPH_FORMS = [("issued, default switches, fp32 cache", False, False, False),
               ("issued, one-launch attention, fp32 cache", True, False, False),
               ("graph, fp32 cache", True, False, True),
               ("issued, one-launch attention, coded cache", True, True, False),
               ("graph, coded cache", True, True, True)]


def graph_step_ab(q, ids, mask, beams, past, reps):
    """One decoder step at past length ``past`` with a beam reorder pending, every form of GRAPH_FORMS timed in turn in each
    round.  Returns {label: [ms]} and {label: seconds of capture + instantiate}."""
    from outlier_suppression_amd import util_layernorm as UL
    from outlier_suppression_amd.model.graph_decode import GraphDecoder
    from outlier_suppression_amd.model.quant_bart import QuantizedBartCache
    dev = ids.device
    bb = ids.shape[0] * beams
    layers = len(q.model.decoder.layers)
    runs, capture, caches = {}, {}, {}
    with torch.no_grad():
        enc = q.get_encoder()(ids, attention_mask=mask).repeat_interleave(beams, 0)
        m = mask.repeat_interleave(beams, 0)
        tok = torch.randint(3, 50265, (bb, past + 1), device=dev)
        perm = torch.randperm(bb, device=dev)
        last = tok[:, past:past + 1]
        for label, attention, codes, graph in GRAPH_FORMS:
            UL.FUSE_DECODE_ATTENTION = attention
            cache = caches[label] = QuantizedBartCache(layers, capacity=past + 1, codes=codes)
            for t in range(past):
                q(attention_mask=m, decoder_input_ids=tok[:, t:t + 1], encoder_outputs=(enc,), past_key_values=cache, use_cache=True)
            lens = list(cache._len)
            decoder = GraphDecoder(q, enc, m, cache) if graph else None

            def run(cache=cache, decoder=decoder, attention=attention, lens=lens):
                UL.FUSE_DECODE_ATTENTION = attention
                cache._len = list(lens)
                if decoder is not None:
                    cache._pos.fill_(past)
                cache.reorder(perm)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if decoder is not None:
                    decoder.step(last)
                else:
                    q(attention_mask=m, decoder_input_ids=last, encoder_outputs=(enc,), past_key_values=cache, use_cache=True)
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3
            for _ in range(4):                      # lead-in: a graph form issues one step and captures its two graphs here
                run()
            if decoder is not None:
                assert decoder.info.captured == 2, decoder.info
                capture[label] = decoder.info.capture_seconds
            runs[label] = (run, [])
        for _ in range(reps):
            for label, (run, times) in runs.items():
                times.append(run())
        for label, cache in caches.items():
            assert cache.rejected() == 0 and bool(cache.coded()) is ("coded" in label) and not cache.demoted()
    UL.FUSE_DECODE_ATTENTION = False
    return {label: times for label, (run, times) in runs.items()}, capture


def graph_generate_ab(q, ids, mask, reps):
    from outlier_suppression_amd import util_layernorm as UL
    times = {label: [] for label, *_ in GRAPH_FORMS}
    capture = {}
    kw = dict(attention_mask=mask, max_length=62, num_beams=6, min_length=62)
    try:
        with torch.no_grad():
            for r in range(reps + 1):
                for label, attention, codes, graph in GRAPH_FORMS:
                    UL.FUSE_DECODE_ATTENTION = attention
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    q.generate(ids, cache_codes=codes, graph=graph, **kw)
                    torch.cuda.synchronize()
                    if r:                           # the first round warms every form up
                        times[label].append(time.perf_counter() - t0)
                        if graph:
                            assert q.last_decode_graph.captured == 2, q.last_decode_graph
                            capture.setdefault(label, []).append(q.last_decode_graph.capture_seconds)
    finally:
        UL.FUSE_DECODE_ATTENTION = False
    return times, capture


def graph_ab(q, ids, mask, args):
    lines = [f"decoder step as a captured graph, BART-large shape (random init, {args.layers}+{args.layers} layers), W6A6 LSQ+ plain "
             f"quantising, batch {args.batch} x {args.beams} beams, source {args.src}; a beam reorder pending before every step (the "
             f"graph forms replay their A->B / B->A graphs alternately); caches filled token by token; every form timed in turn in each "
             f"of {args.reps} rounds, one process; median [min, max]"]
    print(lines[0], flush=True)
    for past in (1, 31, 62):
        times, capture = graph_step_ab(q, ids, mask, args.beams, past, args.reps)
        lines.append(f"S = {past:2d}, one step, ms:")
        lines += [f"    {label:45s} {_stats(t)}" for label, t in times.items()]
        lines += [f"    capture + instantiate of the two graphs, {label}: {secs * 1e3:.0f} ms (not in the step times)"
                  for label, secs in capture.items()]
        print("\n".join(lines[-len(times) - len(capture) - 1:]), flush=True)         # as it comes: a run of minutes
    times, capture = graph_generate_ab(q, ids, mask, args.reps)
    lines.append("generate(max_length=62, num_beams=6, min_length=62), s, wall time of the call (a graph form: capture included):")
    lines += [f"    {label:45s} {_stats(t)}" for label, t in times.items()]
    lines += [f"    of which capture + instantiate, {label}: {_stats(t)}" for label, t in capture.items()]
    print("\n".join(lines[-len(times) - len(capture) - 1:]), flush=True)
    return lines


def _timed(fn, unit=1e3):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * unit, out


def beam_select_ab(q, ids, mask, args):
    from outlier_suppression_amd.model import generation
    dev = ids.device
    bsz, nb, vocab, cur, max_length = args.batch, args.beams, q.config.vocab_size, 31, 62
    keep = 2 * nb                                   # one eos id: generation._beam_search's keep
    lines = [f"a beam step's continuations (log-softmax, logits processors, score add, top-{keep}), the torch lines of "
             f"generation._select_continuations against ops.beam_select; logits [{bsz * nb}, {vocab}] fp32 (randn * 4), "
             f"{bsz} x {nb} beams, length {cur}, min_length {max_length} active (one eos id banned), token history over 40 ids; "
             f"every form timed in turn in each of {args.reps} rounds, one process; median [min, max]"]
    print(lines[0], flush=True)
    g = torch.Generator().manual_seed(0)
    logits = (torch.randn(bsz * nb, vocab, generator=g) * 4).to(dev)
    running = torch.randn(bsz, nb, generator=g).to(dev)
    flat = torch.randint(3, 43, (bsz * nb, cur), generator=g).to(dev)
    eos = torch.tensor([q.config.eos_token_id], device=dev)
    with torch.no_grad():
        forms = {}
        for ngram in (0, 3):
            procs = generation._processors(max_length, eos, ngram, None, None, max_length, dev)
            plan = generation._BeamSelectPlan(procs, dev, nb, vocab, keep, max_length)
            assert plan.reason is None, plan.reason
            for label, p in (("torch lines", None), ("ops.beam_select", plan)):
                forms[f"no_repeat_ngram_size {ngram}, {label}"] = (
                    lambda procs=procs, p=p: generation._select_continuations(logits, flat, running, procs, bsz, nb, vocab, keep, p))
        times = {label: [] for label in forms}
        outs = {}
        for r in range(args.reps + 3):              # three lead-in rounds
            for label, fn in forms.items():
                ms, outs[label] = _timed(fn)
                if r >= 3:
                    times[label].append(ms)
        lines.append("steps a-c alone, ms:")
        lines += [f"    {label:45s} {_stats(t)}" for label, t in times.items()]
        for ngram in (0, 3):
            a, b = outs[f"no_repeat_ngram_size {ngram}, torch lines"], outs[f"no_repeat_ngram_size {ngram}, ops.beam_select"]
            lines.append(f"    no_repeat_ngram_size {ngram}: indices equal: {bool(torch.equal(a[1], b[1]))}, "
                         f"max |value difference| {float((a[0] - b[0]).abs().max()):.3g}")
        print("\n".join(lines[1:]), flush=True)

        enc_ms = sorted(_timed(lambda: q.get_encoder()(ids, attention_mask=mask))[0] for _ in range(args.reps + 1))[:-1]
        lines.append(f"encoder pass alone ({bsz} x {args.src}), ms: {_stats(enc_ms)}")
        print(lines[-1], flush=True)

        gen = [(f"no_repeat_ngram_size {ngram}, {'graph' if graph else 'issued'}, beam_select {'on' if on else 'off'}", ngram, graph, on)
               for ngram in (0, 3) for graph in (False, True) for on in (False, True)]
        times = {label: [] for label, *_ in gen}
        tokens, selected = {}, {}
        for r in range(args.reps + 1):              # the first round warms every form up
            for label, ngram, graph, on in gen:
                secs, tokens[label] = _timed(lambda: q.generate(ids, attention_mask=mask, max_length=max_length, num_beams=nb,
                                                                min_length=max_length, no_repeat_ngram_size=ngram,
                                                                graph=graph, beam_select=on), 1.0)
                info = q.last_beam_select
                selected[label] = (info.selected, info.eager)
                if r:
                    times[label].append(secs)
        lines.append(f"generate(max_length={max_length}, num_beams={nb}, min_length={max_length}), s, wall time of the call "
                     "(a graph form: capture included); (steps through the kernel, steps through torch):")
        lines += [f"    {label:55s} {_stats(t)}   {selected[label]}" for label, t in times.items()]
        for label, ngram, graph, on in gen:
            if on:
                off = label.replace("beam_select on", "beam_select off")
                same = tokens[label].shape == tokens[off].shape and bool(torch.equal(tokens[label], tokens[off]))
                lines.append(f"    {label}: tokens equal to beam_select off: {same}")
        print("\n".join(lines[-len(gen) - len(gen) // 2 - 1:]), flush=True)
    return lines


def beam_advance_ab(q, ids, mask, args):
    from outlier_suppression_amd import ops
    from outlier_suppression_amd.model import generation
    dev = ids.device
    bsz, nb, vocab, at, max_length = args.batch, args.beams, q.config.vocab_size, 31, 62
    keep = 2 * nb                                   # one eos id: generation._beam_search's keep
    lines = [f"a beam step's bookkeeping after the selection (finished continuations, the {nb} beams that go on, the merge "
             f"into the finished set, cache rows, early-stop heuristic, go_on), the torch lines of "
             f"generation._advance_beams_torch against ops.beam_advance; {bsz} x {nb} beams, top-{keep}, max_length "
             f"{max_length}, the state and top_lp / top_idx recorded at length {at} of generate(min_length={max_length}); every "
             f"form timed in turn in each of {args.reps} rounds, one process; median [min, max]"]
    print(lines[0], flush=True)
    recorded = {}
    real = generation._advance_beams_torch

    def recording(state, top_lp, top_idx, cur, *rest, **kw):
        if cur == at:
            recorded["args"] = (state, top_lp.clone(), top_idx.clone(), cur) + tuple(rest[:-2])   # without reorder, prompt
        return real(state, top_lp, top_idx, cur, *rest, **kw)
    generation._advance_beams_torch = recording
    try:
        with torch.no_grad():
            q.generate(ids, attention_mask=mask, max_length=at + 2, num_beams=nb, min_length=max_length, beam_select=True)
    finally:
        generation._advance_beams_torch = real
    state, top_lp, top_idx, cur, _, eos, top_mask, offsets, _, length_penalty, early_stopping = recorded["args"]
    # the state as the max_length-62 call holds it: token rows of 62 positions
    wide = {}
    for name in generation._BeamState.FIELDS:
        t = getattr(state, name)
        if t.dim() == 3:
            t = torch.cat((t, t[:, :, -1:].expand(-1, -1, max_length - t.shape[2])), dim=2).contiguous()
        wide[name] = t
    state = generation._BeamState(**wide)
    now, spare = state.paired()
    eos_ids = eos.to(torch.int64).reshape(-1).contiguous()
    best_len = (max_length - 1) if (early_stopping == "never" and length_penalty > 0.0) else cur
    len_div, best_div = cur ** length_penalty, best_len ** length_penalty
    with torch.no_grad():
        def torch_lines():
            new, beam_idx, go_on = real(state, top_lp, top_idx, cur, vocab, eos, top_mask, offsets, max_length, length_penalty,
                                        early_stopping)
            return new, beam_idx, bool(go_on)

        def kernel():
            ops.beam_advance(top_lp, top_idx, now, spare, cur, vocab, eos_ids, early_stopping, len_div, best_div,
                             generation._ADVANCE_RECIPROCAL)
            return spare, spare.beam_idx, bool(int(spare.go_on))
        forms = {"torch lines (with the read of go_on)": torch_lines, "ops.beam_advance (with the read of go_on)": kernel}
        times = {label: [] for label in forms}
        outs = {}
        for r in range(args.reps + 3):              # three lead-in rounds
            for label, fn in forms.items():
                ms, outs[label] = _timed(fn)
                if r >= 3:
                    times[label].append(ms)
        lines.append("the bookkeeping alone, ms:")
        lines += [f"    {label:45s} {_stats(t)}" for label, t in times.items()]
        (a, a_idx, a_go), (b, b_idx, b_go) = outs.values()
        same = all(torch.equal(getattr(a, n).reshape(-1), getattr(b, n).reshape(-1))
                   for n in ("running", "running_scores", "scores", "done", "improvable"))
        lines.append(f"    running, running_scores, scores, done, improvable, beam_idx and go_on equal: "
                     f"{bool(same and torch.equal(a_idx, b_idx) and a_go == b_go)}")
        print("\n".join(lines[1:]), flush=True)

        gen = [(f"{'graph' if graph else 'issued'}, beam_advance {'on' if on else 'off'}", graph, on)
               for graph in (True, False) for on in (False, True)]
        times = {label: [] for label, *_ in gen}
        tokens, advanced = {}, {}
        for r in range(args.reps + 1):              # the first round warms every form up
            for label, graph, on in gen:
                secs, tokens[label] = _timed(lambda: q.generate(ids, attention_mask=mask, max_length=max_length, num_beams=nb,
                                                                min_length=max_length, graph=graph, beam_select=True,
                                                                beam_advance=on), 1.0)
                info = q.last_beam_advance
                advanced[label] = (info.advanced, info.eager)
                if r:
                    times[label].append(secs)
        lines.append(f"generate(max_length={max_length}, num_beams={nb}, min_length={max_length}, beam_select=True), s, wall time "
                     "of the call (a graph form: capture included); (steps through the kernel, steps through torch):")
        lines += [f"    {label:35s} {_stats(t)}   {advanced[label]}" for label, t in times.items()]
        for label, graph, on in gen:
            if on:
                off = label.replace("beam_advance on", "beam_advance off")
                same = tokens[label].shape == tokens[off].shape and bool(torch.equal(tokens[label], tokens[off]))
                lines.append(f"    {label}: tokens equal to beam_advance off: {same}")
        print("\n".join(lines[-len(gen) - len(gen) // 2 - 1:]), flush=True)
    return lines


def beam_graph_ab(q, ids, mask, args):
    bsz, nb, max_length = args.batch, args.beams, 62
    parent = dict(graph=True, beam_select=True, beam_advance=True)
    lines = [f"a whole beam step as one captured graph -- token copy, model step, ops.beam_select_at, ops.beam_advance_at, the "
             f"cache's row index -- generate(beam_graph=True) against generate(graph=True, beam_select=True, beam_advance=True); "
             f"{bsz} x {nb} beams, source {args.src}, max_length = min_length = {max_length} (BART's forced eos on: the last step is "
             f"issued launch by launch); every form timed in turn in each of {args.reps} rounds, one process; median [min, max]"]
    print(lines[0], flush=True)
    m = q
    gen = [(f"no_repeat_ngram_size {ngram}, {'coded' if codes else 'fp32'} cache, {'beam_graph' if whole else 'graph + select + advance'}",
            ngram, codes, whole) for ngram in (0, 3) for codes in (False, True) for whole in (False, True)]
    times = {label: [] for label, *_ in gen}
    capture = {label: [] for label, *_ in gen}
    tokens, did = {}, {}
    with torch.no_grad():
        for r in range(args.reps + 1):              # the first round warms every form up
            for label, ngram, codes, whole in gen:
                kw = dict(beam_graph=True) if whole else parent
                secs, tokens[label] = _timed(lambda: m.generate(ids, attention_mask=mask, max_length=max_length, num_beams=nb,
                                                                min_length=max_length, no_repeat_ngram_size=ngram,
                                                                cache_codes=codes, **kw), 1.0)
                info = m.last_beam_graph
                assert (info.reason is None) == whole, info
                did[label] = (m.last_decode_graph.captured, m.last_decode_graph.replays, info.issued)
                if r:
                    times[label].append(secs)
                    capture[label].append(m.last_decode_graph.capture_seconds)
    lines.append(f"generate(max_length={max_length}, num_beams={nb}, min_length={max_length}), s, wall time of the call (capture "
                 "included); (graphs captured, replays, steps issued launch by launch):")
    lines += [f"    {label:70s} {_stats(t)}   {did[label]}" for label, t in times.items()]
    lines.append("of which capture + instantiate, s:")
    lines += [f"    {label:70s} {_stats(t)}" for label, t in capture.items()]
    for label, ngram, codes, whole in gen:
        if whole:
            off = label.replace("beam_graph", "graph + select + advance")
            same = tokens[label].shape == tokens[off].shape and bool(torch.equal(tokens[label], tokens[off]))
            a, b = sorted(times[off]), sorted(times[label])
            gain = a[len(a) // 2] - b[len(b) // 2]
            spread = a[-1] - a[0]
            lines.append(f"    {label}: tokens equal to graph + select + advance: {same}; median gain {gain * 1e3:.1f} ms "
                         f"({gain / (max_length - 1) * 1e3:.3f} ms per token), the parent form's own spread {spread * 1e3:.1f} ms")
    print("\n".join(lines[1:]), flush=True)
    return lines


# (label, generate()'s switches) of the forms --greedy-advance compares; the first is the baseline of its group
GREEDY_FORMS = [("graph", dict(graph=True)),
                ("graph + greedy_advance", dict(graph=True, greedy_advance=True)),
                ("greedy_graph", dict(greedy_graph=True)),
                ("issued", dict(graph=False)),
                ("issued + greedy_advance", dict(graph=False, greedy_advance=True)),
                ("issued, greedy_graph asked (falls back)", dict(graph=False, greedy_graph=True))]


def greedy_advance_ab(q, ids, mask, args):
    from outlier_suppression_amd import ops, util_layernorm as UL
    from outlier_suppression_amd.model import generation
    dev = ids.device
    bsz, vocab, at, max_length = args.batch, q.config.vocab_size, 31, 62
    lines = [f"greedy decoding: everything after the model step as one kernel call (ops.greedy_advance) and the whole step as one "
             f"captured graph (greedy_graph) against generate(graph=True); BART-large shape, batch {bsz}, source {args.src}, "
             f"generate(num_beams=1, max_length={max_length}, min_length={max_length}) (BART's forced eos on the last step); the "
             f"one-launch attention on in the issued forms as in the graphs; every form timed in turn in each of {args.reps} "
             f"rounds, one process; median [min, max]"]
    print(lines[0], flush=True)
    old = UL.FUSE_DECODE_ATTENTION
    UL.FUSE_DECODE_ATTENTION = True                 # the issued forms run the launches the graphs hold: the same words
    try:
        with torch.no_grad():
            for ngram in (0, 3):
                kw = dict(num_beams=1, max_length=max_length, min_length=max_length, no_repeat_ngram_size=ngram)
                times = {label: [] for label, _ in GREEDY_FORMS}
                tokens, did = {}, {}
                for r in range(args.reps + 1):      # the first round warms every form up
                    for label, switches in GREEDY_FORMS:
                        secs, tokens[label] = _timed(lambda: q.generate(ids, attention_mask=mask, **kw, **switches), 1.0)
                        did[label] = (q.last_greedy_advance.advanced, q.last_greedy_advance.eager, q.last_decode_graph.captured,
                                      q.last_decode_graph.replays, q.last_greedy_graph.captured)
                        if r:
                            times[label].append(secs)
                first = tokens[GREEDY_FORMS[0][0]]
                for label, t in tokens.items():     # before a time is printed
                    assert t.shape == first.shape and bool(torch.equal(t, first)), f"{label}: tokens differ from graph=True"
                assert did["greedy_graph"][4] == 1 and did["graph + greedy_advance"][:2] == (max_length - 1, 0), did
                block = [f"no_repeat_ngram_size {ngram}: tokens {tuple(first.shape)} equal in all {len(tokens)} forms; s, wall time "
                         "of the call (a graph form: capture included); (steps through the kernel, through torch, graphs "
                         "captured, replays, whole-step graphs):"]
                block += [f"    {label:42s} {_stats(t)}   {did[label]}" for label, t in times.items()]
                for group in (GREEDY_FORMS[:3], GREEDY_FORMS[3:5]):
                    base = sorted(times[group[0][0]])
                    spread = base[-1] - base[0]
                    for label, _ in group[1:]:
                        mine = sorted(times[label])
                        gain = base[len(base) // 2] - mine[len(mine) // 2]
                        block.append(f"    {label} against {group[0][0]}: median gain {gain * 1e3:.1f} ms "
                                     f"({gain / (max_length - 1) * 1e3:.3f} ms per token, {gain / base[len(base) // 2] * 100:.1f} %), "
                                     f"the baseline's own spread {spread * 1e3:.1f} ms: "
                                     f"{'above' if gain > spread else 'within'} it")
                print("\n".join(block), flush=True)
                lines += block

            # the bookkeeping alone at length `at`: min_length active, one eos id, every row unfinished
            g = torch.Generator(device="cpu").manual_seed(3)
            logits = (torch.randn(bsz, vocab, generator=g) * 4).to(dev)
            history = torch.randint(3, 40, (bsz, at), generator=g).to(dev)
            eos = torch.tensor([2], device=dev)
            lines.append(f"the greedy bookkeeping alone (with the read of the stopping word), logits [{bsz}, {vocab}] fp32 (randn * 4), "
                         f"history of {at} tokens, min_length {max_length} active, one eos id, ms:")
            for ngram in (0, 3):
                procs = generation._processors(max_length, eos, ngram, None, 2, max_length, dev)
                plan = generation._GreedyPlan(procs, dev, vocab, max_length, eos, 1)
                assert plan.reason is None, plan.reason
                bufs = ops.GreedyBuffers(bsz, max_length, dev, vocab)
                bufs.seq[:, :at] = history

                def torch_lines():
                    seq, unfinished = history, torch.ones(bsz, dtype=torch.long, device=dev)
                    nxt = torch.argmax(procs(seq, logits), dim=-1)
                    nxt = nxt * unfinished + 1 * (1 - unfinished)
                    seq = torch.cat([seq, nxt[:, None]], dim=-1)
                    unfinished = unfinished & ~torch.isin(nxt, eos)
                    return nxt, bool(unfinished.max() == 0)

                def kernel():
                    bufs.unfinished.fill_(1)
                    ops.greedy_advance(logits, bufs, at, plan.ngram, plan.ban, plan.forced(at), plan.eos, plan.pad)
                    return bufs.next_tokens, not int(bufs.go_on)
                forms = {"torch lines": torch_lines, "ops.greedy_advance": kernel}
                times = {label: [] for label in forms}
                outs = {}
                for r in range(args.reps + 3):      # three lead-in rounds
                    for label, fn in forms.items():
                        ms, outs[label] = _timed(fn)
                        if r >= 3:
                            times[label].append(ms)
                (a, a_stop), (b, b_stop) = outs.values()
                assert bool(torch.equal(a, b)) and a_stop == b_stop, "the kernel's tokens differ from the torch lines'"
                lines += [f"    no_repeat_ngram_size {ngram}, {label:20s} {_stats(t)}" for label, t in times.items()]
            print("\n".join(lines[-5:]), flush=True)
    finally:
        UL.FUSE_DECODE_ATTENTION = old
    return lines


# (label, sample()'s switches) of the forms --sample-advance compares; the first is the baseline of its group
SAMPLE_FORMS = [("graph", dict(graph=True)),
                ("graph + sample_advance", dict(graph=True, sample_advance=True)),
                ("sample_graph", dict(sample_graph=True)),
                ("issued", dict(graph=False)),
                ("issued + sample_advance", dict(graph=False, sample_advance=True))]


def sample_advance_ab(q, ids, mask, args):
    from transformers.generation.logits_process import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    from outlier_suppression_amd import ops, util_layernorm as UL
    from outlier_suppression_amd.model import generation, sampling
    dev = ids.device
    bsz, vocab, at, max_length, seed = args.batch, q.config.vocab_size, 31, 62, 20261019
    draws = (("top_k 50, top_p 0.95, temperature 0.8", dict(top_k=50, top_p=0.95, temperature=0.8)),
             ("the whole vocabulary, temperature 0.8", dict(top_k=0, top_p=1.0, temperature=0.8)))
    lines = [f"seeded sampling: everything after the model step as one kernel call (ops.sample_advance) and the whole step as one "
             f"captured graph (sample_graph) against the torch lines (model/sampling.py); BART-large shape, batch {bsz}, source "
             f"{args.src}, sample(max_length={max_length}, min_length={max_length}, seed={seed}) (BART's forced eos on the last "
             f"step); the one-launch attention on in the issued forms as in the graphs; every form timed in turn in each of "
             f"{args.reps} rounds, one process; median [min, max]"]
    print(lines[0], flush=True)
    old = UL.FUSE_DECODE_ATTENTION
    UL.FUSE_DECODE_ATTENTION = True                 # the issued forms run the launches the graphs hold: the same words
    try:
        with torch.no_grad():
            for name, draw in draws:
                kw = dict(max_length=max_length, min_length=max_length, seed=seed, **draw)
                times = {label: [] for label, _ in SAMPLE_FORMS}
                tokens, did = {}, {}
                for r in range(args.reps + 1):      # the first round warms every form up
                    for label, switches in SAMPLE_FORMS:
                        secs, tokens[label] = _timed(lambda: q.sample(ids, attention_mask=mask, **kw, **switches), 1.0)
                        did[label] = (q.last_sample_advance.advanced, q.last_sample_advance.eager, q.last_decode_graph.captured,
                                      q.last_decode_graph.replays, q.last_sample_graph.captured)
                        if r:
                            times[label].append(secs)
                first = tokens[SAMPLE_FORMS[0][0]]
                assert did["sample_graph"][4] == 1 and did["graph + sample_advance"][:2] == (max_length - 1, 0), did
                families = [[label for label in tokens if (did[label][0] > 0) == kernel] for kernel in (False, True)]
                for family in families:             # before a time is printed
                    for label in family:
                        assert bool(torch.equal(tokens[label], tokens[family[0]])), f"{label}: tokens differ from {family[0]}"
                parted = (tokens[families[0][0]] != tokens[families[1][0]]).any(dim=0).nonzero()
                # with top_k the intervals of the running sums are wide and the two families must agree; over the whole
                # vocabulary of a near-flat distribution an interval is about W / vocab, the size of the fp32 sums' own band
                assert draw["top_k"] == 0 or parted.numel() == 0, f"{name}: the kernel's tokens part from the torch lines'"
                agree = (f"equal in all {len(tokens)} forms" if parted.numel() == 0 else
                         f"equal among the {len(families[0])} torch forms and among the {len(families[1])} kernel forms; the two "
                         f"part at position {int(parted[0])} (the fp32 sums run in another order and an interval here is about "
                         f"W / {vocab}: a draw within rounding of a boundary)")
                block = [f"{name}: tokens {tuple(first.shape)} {agree}; s, wall time of the call (a graph "
                         "form: capture included); (steps through the kernel, through torch, graphs captured, replays, "
                         "whole-step graphs):"]
                block += [f"    {label:42s} {_stats(t)}   {did[label]}" for label, t in times.items()]
                for group in (SAMPLE_FORMS[:3], SAMPLE_FORMS[3:5]):
                    base = sorted(times[group[0][0]])
                    spread = base[-1] - base[0]
                    for label, _ in group[1:]:
                        mine = sorted(times[label])
                        gain = base[len(base) // 2] - mine[len(mine) // 2]
                        block.append(f"    {label} against {group[0][0]}: median gain {gain * 1e3:.1f} ms "
                                     f"({gain / (max_length - 1) * 1e3:.3f} ms per token, {gain / base[len(base) // 2] * 100:.1f} %), "
                                     f"the baseline's own spread {spread * 1e3:.1f} ms: "
                                     f"{'above' if gain > spread else 'within'} it")
                print("\n".join(block), flush=True)
                lines += block

            # the selection alone at length `at`: min_length active, one eos id, every row unfinished
            g = torch.Generator(device="cpu").manual_seed(3)
            logits = (torch.randn(bsz, vocab, generator=g) * 4).to(dev)
            history = torch.randint(3, 40, (bsz, at), generator=g).to(dev)
            eos = torch.tensor([2], device=dev)
            procs = generation._processors(max_length, eos, 0, None, 2, max_length, dev)
            plan = generation._GreedyPlan(procs, dev, vocab, max_length, eos, 1)
            assert plan.reason is None, plan.reason
            lines.append(f"the selection alone (with the read of the stopping word), logits [{bsz}, {vocab}] fp32 (randn * 4), history "
                         f"of {at} tokens, min_length {max_length} active, one eos id, ms; transformers' lines: its temperature / "
                         "top-k / top-p warpers, softmax and torch.multinomial (another random stream: its tokens are not compared):")
            for name, draw in draws:
                bufs = ops.SampleBuffers(bsz, max_length, dev, vocab, draw["top_k"])
                bufs.seq[:, :at] = history
                warpers = [TemperatureLogitsWarper(draw["temperature"])]
                if draw["top_k"]:
                    warpers.append(TopKLogitsWarper(draw["top_k"]))
                if draw["top_p"] < 1.0:
                    warpers.append(TopPLogitsWarper(draw["top_p"]))

                def finish(nxt):
                    unfinished = torch.ones(bsz, dtype=torch.long, device=dev)
                    nxt = nxt * unfinished + 1 * (1 - unfinished)
                    torch.cat([history, nxt[:, None]], dim=-1)
                    unfinished = unfinished & ~torch.isin(nxt, eos)
                    return nxt, bool(unfinished.max() == 0)

                def transformers_lines():
                    scores = procs(history, logits)
                    for w in warpers:
                        scores = w(history, scores)
                    return finish(torch.multinomial(torch.softmax(scores, dim=-1), num_samples=1).squeeze(1))

                def torch_lines():
                    u = sampling.uniforms(seed, bsz, at)
                    return finish(sampling.select_torch(procs(history, logits), u, **draw))

                def kernel():
                    bufs.unfinished.fill_(1)
                    ops.sample_advance(logits, bufs, at, seed, ngram=plan.ngram, ban_ids=plan.ban, forced=plan.forced(at),
                                       eos_ids=plan.eos, pad=plan.pad, **draw)
                    return bufs.next_tokens, not int(bufs.go_on)
                forms = {"transformers' lines": transformers_lines, "sampling.select_torch": torch_lines, "ops.sample_advance": kernel}
                times = {label: [] for label in forms}
                outs = {}
                for r in range(args.reps + 3):      # three lead-in rounds
                    for label, fn in forms.items():
                        ms, outs[label] = _timed(fn)
                        if r >= 3:
                            times[label].append(ms)
                (a, a_stop), (b, b_stop) = outs["sampling.select_torch"], outs["ops.sample_advance"]
                assert bool(torch.equal(a, b)) and a_stop == b_stop, "the kernel's tokens differ from the torch lines'"
                lines += [f"    {name}, {label:24s} {_stats(t)}" for label, t in times.items()]
            print("\n".join(lines[-7:]), flush=True)
    finally:
        UL.FUSE_DECODE_ATTENTION = old
    return lines


# (label, sample()'s switches) of the forms --sample-nucleus compares; the first is the baseline of its group (the switch
# off: the torch lines, what sample() did with top_k=0, top_p<1 before ops.sample_nucleus)
NUCLEUS_FORMS = [("graph", dict(graph=True)),
                 ("graph + sample_advance + sample_nucleus", dict(graph=True, sample_advance=True, sample_nucleus=True)),
                 ("sample_graph + sample_nucleus", dict(sample_graph=True, sample_nucleus=True)),
                 ("issued", dict(graph=False)),
                 ("issued + sample_advance + sample_nucleus", dict(graph=False, sample_advance=True, sample_nucleus=True))]


def sample_nucleus_ab(q, ids, mask, args):
    from transformers.generation.logits_process import TemperatureLogitsWarper, TopPLogitsWarper
    from outlier_suppression_amd import ops, util_layernorm as UL
    from outlier_suppression_amd.model import generation, sampling
    dev = ids.device
    bsz, vocab, at, max_length, seed = args.batch, q.config.vocab_size, 31, 62, 20261020
    draw = dict(top_k=0, top_p=0.9, temperature=1.0)
    lines = [f"a nucleus over the whole vocabulary (top_k=0, top_p={draw['top_p']}): everything after the model step as one kernel "
             f"call (ops.sample_nucleus, sample(sample_nucleus=True)) and the whole step as one captured graph against the torch "
             f"lines (model/sampling.py: a stable sort of the row), which the switch off runs; BART-large shape, batch {bsz}, "
             f"source {args.src}, sample(max_length={max_length}, min_length={max_length}, seed={seed}) (BART's forced eos on the "
             f"last step); the one-launch attention on in the issued forms as in the graphs; every form timed in turn in each of "
             f"{args.reps} rounds, one process; median [min, max]"]
    print(lines[0], flush=True)
    old = UL.FUSE_DECODE_ATTENTION
    UL.FUSE_DECODE_ATTENTION = True                 # the issued forms run the launches the graphs hold: the same words
    try:
        with torch.no_grad():
            kw = dict(max_length=max_length, min_length=max_length, seed=seed, **draw)
            times = {label: [] for label, _ in NUCLEUS_FORMS}
            tokens, did = {}, {}
            for r in range(args.reps + 1):          # the first round warms every form up
                for label, switches in NUCLEUS_FORMS:
                    secs, tokens[label] = _timed(lambda: q.sample(ids, attention_mask=mask, **kw, **switches), 1.0)
                    did[label] = (q.last_sample_advance.advanced, q.last_sample_advance.eager, q.last_decode_graph.captured,
                                  q.last_decode_graph.replays, q.last_sample_graph.captured)
                    if r:
                        times[label].append(secs)
            first = tokens[NUCLEUS_FORMS[0][0]]
            assert did["sample_graph + sample_nucleus"][4] == 1, did
            assert did["graph + sample_advance + sample_nucleus"][:2] == (max_length - 1, 0), did
            assert did["graph"][:2] == (0, max_length - 1), did
            families = [[label for label in tokens if (did[label][0] > 0) == kernel] for kernel in (False, True)]
            for family in families:                 # before a time is printed
                for label in family:
                    assert bool(torch.equal(tokens[label], tokens[family[0]])), f"{label}: tokens differ from {family[0]}"
            parted = (tokens[families[0][0]] != tokens[families[1][0]]).any(dim=0).nonzero()
            agree = (f"equal in all {len(tokens)} forms" if parted.numel() == 0 else
                     f"equal among the {len(families[0])} torch forms and among the {len(families[1])} kernel forms; the two "
                     f"part at position {int(parted[0])} (the fp32 sums run in another order: a draw within rounding of a "
                     f"boundary)")
            block = [f"tokens {tuple(first.shape)} {agree}; s, wall time of the call (a graph form: capture included); (steps "
                     "through the kernel, through torch, graphs captured, replays, whole-step graphs):"]
            block += [f"    {label:42s} {_stats(t)}   {did[label]}" for label, t in times.items()]
            for group in (NUCLEUS_FORMS[:3], NUCLEUS_FORMS[3:5]):
                base = sorted(times[group[0][0]])
                spread = base[-1] - base[0]
                for label, _ in group[1:]:
                    mine = sorted(times[label])
                    gain = base[len(base) // 2] - mine[len(mine) // 2]
                    block.append(f"    {label} against {group[0][0]}: median gain {gain * 1e3:.1f} ms "
                                 f"({gain / (max_length - 1) * 1e3:.3f} ms per token, {gain / base[len(base) // 2] * 100:.1f} %), "
                                 f"the baseline's own spread {spread * 1e3:.1f} ms: "
                                 f"{'above' if gain > spread else 'within'} it")
            print("\n".join(block), flush=True)
            lines += block

            # the selection alone at length `at`: min_length active, one eos id, every row unfinished
            g = torch.Generator(device="cpu").manual_seed(3)
            logits = (torch.randn(bsz, vocab, generator=g) * 4).to(dev)
            history = torch.randint(3, 40, (bsz, at), generator=g).to(dev)
            eos = torch.tensor([2], device=dev)
            procs = generation._processors(max_length, eos, 0, None, 2, max_length, dev)
            plan = generation._GreedyPlan(procs, dev, vocab, max_length, eos, 1)
            assert plan.reason is None, plan.reason
            bufs = ops.SampleBuffers(bsz, max_length, dev, vocab, 0, nucleus=True)
            bufs.seq[:, :at] = history
            warpers = [TemperatureLogitsWarper(draw["temperature"]), TopPLogitsWarper(draw["top_p"])]

            def finish(nxt):
                unfinished = torch.ones(bsz, dtype=torch.long, device=dev)
                nxt = nxt * unfinished + 1 * (1 - unfinished)
                torch.cat([history, nxt[:, None]], dim=-1)
                unfinished = unfinished & ~torch.isin(nxt, eos)
                return nxt, bool(unfinished.max() == 0)

            def transformers_lines():
                scores = procs(history, logits)
                for w in warpers:
                    scores = w(history, scores)
                return finish(torch.multinomial(torch.softmax(scores, dim=-1), num_samples=1).squeeze(1))

            def torch_lines():
                u = sampling.uniforms(seed, bsz, at)
                return finish(sampling.select_torch(procs(history, logits), u, **draw))

            def kernel():
                bufs.unfinished.fill_(1)
                ops.sample_nucleus(logits, bufs, at, seed, draw["temperature"], draw["top_p"], ngram=plan.ngram, ban_ids=plan.ban,
                                   forced=plan.forced(at), eos_ids=plan.eos, pad=plan.pad)
                return bufs.next_tokens, not int(bufs.go_on)
            forms = {"transformers' lines": transformers_lines, "sampling.select_torch": torch_lines, "ops.sample_nucleus": kernel}
            times = {label: [] for label in forms}
            outs = {}
            for r in range(args.reps + 3):          # three lead-in rounds
                for label, fn in forms.items():
                    ms, outs[label] = _timed(fn)
                    if r >= 3:
                        times[label].append(ms)
            (a, a_stop), (b, b_stop) = outs["sampling.select_torch"], outs["ops.sample_nucleus"]
            same = int((a == b).sum())
            assert a_stop == b_stop and same >= bsz - 1, "the kernel's tokens differ from the torch lines'"
            lines.append(f"the selection alone (with the read of the stopping word), logits [{bsz}, {vocab}] fp32 (randn * 4), history "
                         f"of {at} tokens, min_length {max_length} active, one eos id, ms; {same} of {bsz} tokens equal between "
                         "sampling.select_torch and ops.sample_nucleus; transformers' lines: its temperature / top-p warpers, "
                         "softmax and torch.multinomial (another random stream: its tokens are not compared):")
            lines += [f"    {label:24s} {_stats(t)}" for label, t in times.items()]
            print("\n".join(lines[-4:]), flush=True)
    finally:
        UL.FUSE_DECODE_ATTENTION = old
    return lines


# (label, cache codes, share_cross_kv) of the forms --share-cross-kv compares: the baseline of each pair first
SHARE_FORMS = [("fp32 cache, one copy per beam", False, False), ("fp32 cache, shared", False, True),
               ("coded cache, one copy per beam", True, False), ("coded cache, shared", True, True)]


def share_launch_ab(q, ids, beams, reps, launches=50):
    """The cross-attention launch of one layer alone at the model's shape: ops.decode_attention_fake_quant / _codes on K / V
    of batch * beams rows against ops.decode_attention_shared on batch rows.  {label: [us per launch]}."""
    from outlier_suppression_amd import ops
    dev = ids.device
    attn = q.model.decoder.layers[0].encoder_attn
    b, s, h, d = ids.shape[0], ids.shape[1], attn.num_heads, attn.head_dim
    query = torch.randn(b * beams, h, 1, d, device=dev) * d ** -0.5
    mask = torch.zeros(b, 1, 1, s, device=dev)
    quant = lambda scale, zp: (torch.tensor([scale], device=dev), torch.tensor([zp], dtype=torch.int32, device=dev), 0, 63, ops.PARAM_FIXED, 1.0)  # noqa: E731
    pq, cq = quant(1.0 / 63, 0), quant(0.05, 31)
    rejected = torch.zeros(1, dtype=torch.int32, device=dev)
    rec = (torch.tensor([0.06], device=dev), torch.tensor([31.0], device=dev), 0)
    runs = {}
    for label, codes, share in SHARE_FORMS:
        rows = b if share else b * beams
        if codes:
            k, v = (torch.randint(0, 64, (rows, h, s, d), device=dev).to(torch.uint8) for _ in range(2))
        else:
            k, v = (torch.randn(rows, h, s, d, device=dev) for _ in range(2))
        m = mask if share else mask.repeat_interleave(beams, 0)
        if share:
            fn = lambda k=k, v=v, m=m, codes=codes: ops.decode_attention_shared(  # noqa: E731
                query, k, v, m, pq, cq, beams, codes=(rec, rec, rejected) if codes else None)
        elif codes:
            fn = lambda k=k, v=v, m=m: ops.decode_attention_codes(query, k, v, m, pq, cq, rec, rec, rejected)  # noqa: E731
        else:
            fn = lambda k=k, v=v, m=m: ops.decode_attention_fake_quant(query, k, v, m, pq, cq)  # noqa: E731
        assert fn() is not None, label
        runs[label] = (fn, [])
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for r in range(reps + 1):
        for label, (fn, times) in runs.items():
            torch.cuda.synchronize()
            start.record()
            for _ in range(launches):
                fn()
            stop.record()
            torch.cuda.synchronize()
            if r:                                   # the first round warms every form up
                times.append(start.elapsed_time(stop) * 1e3 / launches)
    return {label: times for label, (fn, times) in runs.items()}


def share_step_ab(q, ids, mask, beams, past, reps):
    """One decoder step at past length ``past`` as a replayed graph with a beam reorder pending, every form of SHARE_FORMS
    timed in turn in each round.  Returns {label: [ms]} and {label: cache.nbytes()}."""
    from outlier_suppression_amd.model.graph_decode import GraphDecoder
    from outlier_suppression_amd.model.quant_bart import QuantizedBartCache
    dev = ids.device
    bb = ids.shape[0] * beams
    layers = len(q.model.decoder.layers)
    runs, held = {}, {}
    with torch.no_grad():
        enc1 = q.get_encoder()(ids, attention_mask=mask)
        tok = torch.randint(3, 50265, (bb, past + 1), device=dev)
        perm = (torch.arange(bb, device=dev).view(-1, beams)[:, torch.randperm(beams, device=dev)]).reshape(-1)   # beams stay in their row
        last = tok[:, past:past + 1]
        for label, codes, share in SHARE_FORMS:
            enc, m = (enc1, mask) if share else (enc1.repeat_interleave(beams, 0), mask.repeat_interleave(beams, 0))
            cache = QuantizedBartCache(layers, capacity=past + 1, codes=codes, cross_group=beams if share else 1)
            cache.cross_one_launch = share
            for t in range(past):
                q(attention_mask=m, decoder_input_ids=tok[:, t:t + 1], encoder_outputs=(enc,), past_key_values=cache, use_cache=True)
            lens = list(cache._len)
            decoder = GraphDecoder(q, enc, m, cache)

            def run(cache=cache, decoder=decoder, lens=lens):
                cache._len = list(lens)
                cache._pos.fill_(past)
                cache.reorder(perm)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                decoder.step(last)
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3
            for _ in range(4):                      # lead-in: one issued step, the two graphs captured
                run()
            assert decoder.info.captured == 2, decoder.info
            runs[label] = (run, [])
            held[label] = cache.nbytes()
            assert cache.rejected() == 0 and bool(cache.coded()) is codes and not cache.demoted()
            assert cache._cross[0][0].shape[0] == (ids.shape[0] if share else bb)
        for _ in range(reps):
            for label, (run, times) in runs.items():
                times.append(run())
    return {label: times for label, (run, times) in runs.items()}, held


def share_logits_ab(q, ids, mask, beams, steps=12, rows=4):
    """max |logit difference| over ``steps`` teacher-forced steps on the first ``rows`` inputs, shared against unshared, the
    one-launch attention on in both, and how many stored cross-attention words of layer 0 differ between the two caches (the
    shared form projects K / V on ``rows`` rows, the unshared one on ``rows * beams``): {"fp32": (d, words, of), "codes": ...}."""
    from outlier_suppression_amd import util_layernorm as UL
    from outlier_suppression_amd.model.quant_bart import QuantizedBartCache
    layers = len(q.model.decoder.layers)
    ids, mask = ids[:rows], mask[:rows]
    out = {}
    UL.FUSE_DECODE_ATTENTION = True
    try:
        with torch.no_grad():
            enc1 = q.get_encoder()(ids, attention_mask=mask)
            tok = torch.randint(3, 50265, (rows * beams, steps), device=ids.device)
            for name, codes in (("fp32", False), ("codes", True)):
                logits, held = [], []
                for share in (False, True):
                    enc, m = (enc1, mask) if share else (enc1.repeat_interleave(beams, 0), mask.repeat_interleave(beams, 0))
                    cache = QuantizedBartCache(layers, capacity=steps, codes=codes, cross_group=beams if share else 1)
                    logits.append(torch.stack([q(attention_mask=m, decoder_input_ids=tok[:, t:t + 1], encoder_outputs=(enc,),
                                                 past_key_values=cache, use_cache=True)[0][:, -1] for t in range(steps)], 1))
                    held.append(torch.cat([cache[0][2], cache[0][3]]))
                out[name] = ((logits[0] - logits[1]).abs().max().item(), int((held[0] != held[1]).sum()), held[0].numel())
    finally:
        UL.FUSE_DECODE_ATTENTION = False
    return out


def share_cross_kv_ab(q, ids, mask, args):
    lines = [f"cross-attention keys / values shared among the beams of a row, BART-large shape (random init, {args.layers}+{args.layers} "
             f"layers), W6A6 LSQ+ plain quantising, batch {args.batch} x {args.beams} beams, source {args.src}; every form timed in "
             f"turn in each of {args.reps} rounds, one process; median [min, max]"]
    print(lines[0], flush=True)

    def emit(new):
        lines.extend(new)
        print("\n".join(new), flush=True)
    times = share_launch_ab(q, ids, args.beams, args.reps)
    emit(["the cross-attention launch of one layer alone, us per launch (device events around 50 launches):"]
         + [f"    {label:34s} {_stats(t)}" for label, t in times.items()])
    held = {}
    for past in (1, 31, 62):
        times, held = share_step_ab(q, ids, mask, args.beams, past, args.reps)
        emit([f"S = {past:2d}, one decoder step as a replayed graph, a beam reorder pending, ms:"]
             + [f"    {label:34s} {_stats(t)}" for label, t in times.items()])
    attn = q.model.decoder.layers[0].encoder_attn
    for fmt, size in (("fp32", 4), ("coded", 1)):
        cross = 2 * args.layers * args.batch * args.beams * attn.num_heads * args.src * attn.head_dim * size
        a, b = held[f"{fmt} cache, one copy per beam"], held[f"{fmt} cache, shared"]
        emit([f"cache.nbytes() at capacity 63, {fmt} cache: one copy per beam {a}, shared {b}; the difference {a - b} is the cross "
              f"tensors' {cross} B * ({args.beams} - 1) / {args.beams} = {cross // args.beams * (args.beams - 1)}"])
        assert a - b == cross // args.beams * (args.beams - 1), (a, b, cross)
    gen = {label: [] for label, *_ in SHARE_FORMS}
    tokens, did = {}, {}
    kw = dict(attention_mask=mask, max_length=62, num_beams=args.beams, min_length=62, graph=True, beam_select=True, beam_advance=True)
    from outlier_suppression_amd import util_layernorm as UL
    UL.FUSE_DECODE_ATTENTION = True                 # the first step, issued by the model, computes the replayed steps' words in every form
    try:
        with torch.no_grad():
            for r in range(args.reps + 1):
                for label, codes, share in SHARE_FORMS:
                    secs, out = _timed(lambda: q.generate(ids, cache_codes=codes, share_cross_kv=share, **kw), unit=1.0)
                    tokens[label], did[label] = out, repr(q.last_share_cross_kv)
                    assert (q.last_share_cross_kv.reason is None) is share and q.last_decode_graph.reason is None, (label, did[label])
                    if r:                           # the first round warms every form up
                        gen[label].append(secs)
    finally:
        UL.FUSE_DECODE_ATTENTION = False
    emit([f"generate(max_length=62, num_beams={args.beams}, min_length=62, graph=True, beam_select=True, beam_advance=True), the "
          f"one-launch attention on for the first step too, s, wall time of the call (capture included):"]
         + [f"    {label:34s} {_stats(t)}   {did[label]}" for label, t in gen.items()])
    for fmt in ("fp32", "coded"):
        a, b = tokens[f"{fmt} cache, one copy per beam"], tokens[f"{fmt} cache, shared"]
        same = a.shape == b.shape and bool(torch.equal(a, b))
        emit([f"    tokens, {fmt} cache, shared against one copy per beam: " + ("equal" if same else
              f"DIFFER in {int((a != b).sum()) if a.shape == b.shape else 'shape'} of {a.numel()} positions")])
    for rows in sorted({min(4, args.batch), args.batch}):
        d = share_logits_ab(q, ids, mask, args.beams, rows=rows)
        emit([f"{rows} x {args.beams} rows, 12 teacher-forced steps, shared against one copy per beam, the one-launch attention on in "
              f"both: max |logit difference| fp32 cache {d['fp32'][0]:.3g}, coded cache {d['codes'][0]:.3g}"
              + (" -- 0: every word is the same" if d["fp32"][0] == 0 and d["codes"][0] == 0 else "")
              + f"; stored cross K / V words of layer 0 that differ (K / V projected on {rows} rows against {rows * args.beams}): "
              f"fp32 cache {d['fp32'][1]} of {d['fp32'][2]}, coded cache {d['codes'][1]} of {d['codes'][2]}"])
    return lines


def sample_group_step_ab(rows, group, reps, dev, launches=50):
    """The step kernels alone on [rows, 50265] logits, us per call (device events around ``launches`` calls), with and without
    ``logprobs``: {label: [us]}."""
    from outlier_suppression_amd import ops
    vocab, max_length = 50265, 62
    logits = torch.randn((rows, vocab), device=dev) * 3
    forms = [("sample_advance, top_k=50 top_p=0.95", ops.sample_advance, dict(top_k=50, top_p=0.95)),
             ("sample_nucleus, top_p=0.9", ops.sample_nucleus, dict(top_p=0.9))]
    calls = {}
    for label, fn, draw in forms:
        for lp in (False, True):
            bufs = ops.SampleBuffers(rows, max_length, dev, vocab, top_k=draw.get("top_k", 0), nucleus=True, logprobs=lp)
            calls[f"{label}, group {group}" + (", logprobs" if lp else "")] = (
                lambda fn=fn, bufs=bufs, draw=draw: fn(logits, bufs, 7, 12345, 1.0, **draw, group=group, logprobs=bufs.logprobs))
    times = {label: [] for label in calls}
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for r in range(reps + 1):
        for label, call in calls.items():
            call()
            start.record()
            for _ in range(launches):
                call()
            stop.record()
            torch.cuda.synchronize()
            if r:                                   # the first round warms every form up
                times[label].append(start.elapsed_time(stop) * 1e3 / launches)
    return times


def sample_group_ab(q, ids, mask, args):
    from outlier_suppression_amd import util_layernorm as UL
    from outlier_suppression_amd.model import quant_bart
    n = args.beams
    lines = [f"sample(num_samples={n}) with the cross-attention keys / values held once per input, BART-large shape (random init, "
             f"{args.layers}+{args.layers} layers), W6A6 LSQ+ plain quantising, {args.batch} inputs x {n} samples, source {args.src}; "
             f"every form timed in turn in each of {args.reps} rounds, one process; median [min, max]"]
    print(lines[0], flush=True)

    def emit(new):
        lines.extend(new)
        print("\n".join(new), flush=True)
    draws = [("top_k=50, top_p=0.95", dict(top_k=50, top_p=0.95)), ("top_k=0, top_p=0.9 (sample_nucleus)", dict(top_k=0, top_p=0.9, sample_nucleus=True))]
    forms = [(f"{d}, {fmt} cache, {'shared' if share else 'one copy per sequence'}", kw, codes, share)
             for d, kw in draws for fmt, codes in (("fp32", False), ("coded", True)) for share in (False, True)]
    made = []

    class Recorded(quant_bart.QuantizedBartCache):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            del made[:]
            made.append(self)
    plain_cache, quant_bart.QuantizedBartCache = quant_bart.QuantizedBartCache, Recorded
    gen = {label: [] for label, *_ in forms}
    tokens, did, held = {}, {}, {}
    kw = dict(attention_mask=mask, max_length=62, min_length=62, seed=2 ** 40 + 3, num_samples=n, sample_graph=True)
    UL.FUSE_DECODE_ATTENTION = True                 # the first step, issued by the model, computes the replayed steps' words in every form
    try:
        with torch.no_grad():
            for r in range(args.reps + 1):
                for label, draw, codes, share in forms:
                    secs, out = _timed(lambda: q.sample(ids, cache_codes=codes, share_cross_kv=share, **draw, **kw), unit=1.0)
                    tokens[label], did[label], held[label] = out, repr(q.last_share_cross_kv), made[0].nbytes()
                    assert (q.last_share_cross_kv.reason is None) is share and q.last_sample_graph.reason is None, (label, did[label])
                    if r:                           # the first round warms every form up
                        gen[label].append(secs)
            del made[:]
            lp_times = {}
            for label, draw, codes, share in forms[1:4:2]:          # the shared forms of the first draw, with the log-probabilities
                for want in (False, True):
                    for r in range(args.reps + 1):
                        secs, _ = _timed(lambda: q.sample(ids, cache_codes=codes, share_cross_kv=share, return_logprobs=want,
                                                          **draw, **kw), unit=1.0)
                        if r:
                            lp_times.setdefault(label + (", return_logprobs" if want else ""), []).append(secs)
            del made[:]
    finally:
        UL.FUSE_DECODE_ATTENTION = False
        quant_bart.QuantizedBartCache = plain_cache
    emit([f"sample(max_length=62, min_length=62, num_samples={n}, sample_graph=True), the one-launch attention on for the first step "
          f"too, s, wall time of the call (encoder and capture included):"]
         + [f"    {label:72s} {_stats(t)}   {did[label]}" for label, t in gen.items()])
    for (a, *_), (b, *_) in zip(forms[0::2], forms[1::2]):
        ta, tb = sorted(gen[a])[len(gen[a]) // 2], sorted(gen[b])[len(gen[b]) // 2]
        same = tokens[a].shape == tokens[b].shape and bool(torch.equal(tokens[a], tokens[b]))
        outside = min(gen[a]) > max(gen[b]) or max(gen[a]) < min(gen[b])
        emit([f"    {b}: {100 * (ta - tb) / ta:.1f} % below the unshared call's time ("
              + ("outside" if outside else "INSIDE") + " the baseline's own range); tokens " + ("equal" if same else "DIFFER")
              + f"; cache.nbytes() {held[a]} -> {held[b]}"])
    emit(["the same shared calls with and without return_logprobs, s:"] + [f"    {label:88s} {_stats(t)}" for label, t in lp_times.items()])
    times = sample_group_step_ab(args.batch * n, n, args.reps, ids.device)
    emit([f"the step kernels alone at [{args.batch * n}, 50265], us per call (device events around 50 calls):"]
         + [f"    {label:60s} {_stats(t)}" for label, t in times.items()])
    for label in list(times)[0::2]:
        a, b = times[label], times[label + ", logprobs"]
        ma, mb = sorted(a)[len(a) // 2], sorted(b)[len(b) // 2]
        emit([f"    {label}: logprobs {mb - ma:+.3f} us, " + ("inside" if min(a) <= mb <= max(a) else "OUTSIDE") + " the baseline's own range"])
    return lines


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
    ap.add_argument("--graph", action="store_true")
    ap.add_argument("--beam-select", action="store_true")
    ap.add_argument("--beam-advance", action="store_true")
    ap.add_argument("--beam-graph", action="store_true")
    ap.add_argument("--greedy-advance", action="store_true")
    ap.add_argument("--sample-advance", action="store_true")
    ap.add_argument("--sample-nucleus", action="store_true")
    ap.add_argument("--share-cross-kv", action="store_true")
    ap.add_argument("--sample-group", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    q, ids, mask = build(args.batch, args.src, args.layers)
    if args.sample_group:
        text = "\n".join(sample_group_ab(q, ids, mask, args))
        if args.out:
            with open(args.out, "w") as f:
                f.write(text + "\n")
        return
    if args.share_cross_kv:
        text = "\n".join(share_cross_kv_ab(q, ids, mask, args))
        if args.out:
            with open(args.out, "w") as f:
                f.write(text + "\n")
        return
    if args.sample_nucleus:
        text = "\n".join(sample_nucleus_ab(q, ids, mask, args))
        if args.out:
            with open(args.out, "w") as f:
                f.write(text + "\n")
        return
    if args.sample_advance:
        text = "\n".join(sample_advance_ab(q, ids, mask, args))
        if args.out:
            with open(args.out, "w") as f:
                f.write(text + "\n")
        return
    if args.greedy_advance:
        text = "\n".join(greedy_advance_ab(q, ids, mask, args))
        if args.out:
            with open(args.out, "w") as f:
                f.write(text + "\n")
        return
    if args.beam_graph:
        text = "\n".join(beam_graph_ab(q, ids, mask, args))
        if args.out:
            with open(args.out, "w") as f:
                f.write(text + "\n")
        return
    if args.beam_advance:
        text = "\n".join(beam_advance_ab(q, ids, mask, args))
        if args.out:
            with open(args.out, "w") as f:
                f.write(text + "\n")
        return
    if args.beam_select:
        text = "\n".join(beam_select_ab(q, ids, mask, args))
        if args.out:
            with open(args.out, "w") as f:
                f.write(text + "\n")
        return
    if args.graph and not args.profile_steps:
        text = "\n".join(graph_ab(q, ids, mask, args))
        if args.out:
            with open(args.out, "w") as f:
                f.write(text + "\n")
        return
    if args.profile_steps:
        from outlier_suppression_amd import util_layernorm as UL
        UL.FUSE_DECODE_ATTENTION = args.fast_decode_attention
        with torch.no_grad():
            q.generate(ids, attention_mask=mask, max_length=args.profile_steps + 1, num_beams=args.beams,
                       min_length=args.profile_steps + 1, cache_codes=args.cache_codes, graph=args.graph)
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

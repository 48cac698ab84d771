"""generate() for the quantized BART wrapper: greedy and beam search over a KV cache.

The package's own loop, not transformers' GenerationMixin (whose cache contract does not fit the reference's tuples).
It follows transformers' greedy decoding and its vectorised beam search step for step, so that with the quantizers
disabled the tokens equal ``BartForConditionalGeneration.generate`` on the FP model.  The logits processors a BART
configuration turns on -- no_repeat_ngram_size, min_length, forced_bos_token_id, forced_eos_token_id -- are
transformers' own, applied in transformers' order.  Not covered: sampling (generate() refuses it; ``sample()``, below, is
the package's own), return_dict_in_generate, streaming.

Each step feeds the last token with the cache (quant_bart.QuantizedBartCache: the step's k / v are fake-quantized and
appended in one launch, a beam reorder rides in the next append); ``use_cache=False`` re-runs the whole prefix instead.
``graph=True`` (or the package switch, set_graph_decode) replays a captured graph of the step from the third step on
(model/graph_decode.py); ``model.last_decode_graph`` tells what happened.  ``beam_select=True`` (set_beam_select) hands a beam
step's log-softmax, banned tokens, score add and top-k to one kernel call (ops.beam_select) where the step's processors are
the no-repeat-ngram and min-length ones; ``model.last_beam_select`` tells how many steps took it.  ``beam_advance=True``
(set_beam_advance) hands the bookkeeping after the selection -- which continuations finished, the beams that go on, the merge
into the finished set, the early-stop heuristic -- to one kernel call (ops.beam_advance) on two alternating sets of state
buffers; ``model.last_beam_advance`` tells how many steps took it.  ``beam_graph=True`` (set_beam_graph) asks for all three
and captures the whole step -- token copy, model, selection, bookkeeping, the cache's row index -- into one graph per
direction of the alternating buffers (graph_decode.BeamStepGraphs): a token costs the host one replay and one read of the
stopping word; ``model.last_beam_graph`` tells what happened.  ``share_cross_kv=True`` (set_share_cross_kv) keeps the encoder
states and their mask at one row per input instead of one per beam: the cache holds the cross-attention keys / values once
per batch row (QuantizedBartCache, ``cross_group``) and a step's cross-attention serves all beams of a row from one pass over
them (ops.decode_attention_shared), launch by launch or inside any of the graphs above; ``model.last_share_cross_kv`` tells
what happened.

Greedy decoding has the same two steps off the host.  ``greedy_advance=True`` (set_greedy_advance) hands everything after the
model step -- the banned tokens of the logits processors, the arg-max, the pad / eos arithmetic, the new token into the
sequence, the stopping word -- to one kernel call (ops.greedy_advance) on one set of state buffers (ops.GreedyBuffers): the
model is fed the kernel's next_tokens and the host reads go_on once per token; ``model.last_greedy_advance`` tells how many
steps took it.  The tokens are those of the torch lines with no tolerance: the kernel's order is torch.argmax's.
``greedy_graph=True`` (set_greedy_graph) asks for ``graph`` and ``greedy_advance`` and captures the whole step -- token copy,
model, ops.greedy_advance_at -- into one graph (graph_decode.GreedyStepGraph), forced tokens included: a token costs the host
one replay and one read of the stopping word; ``model.last_greedy_graph`` tells what happened.

Sampling is ``sample()``, an entry point of its own (generate() promises transformers' tokens, a sampler with its own random
stream cannot): the greedy loop with a seeded draw in the place of the arg-max (model/sampling.py), ``sample_advance=True``
and ``sample_graph=True`` as the two greedy switches (ops.sample_advance, graph_decode.SampleStepGraph).
``num_samples=n`` draws n sequences per input from one run of the encoder -- sequence j of input b at the Philox counter
(b, length, j, 0) -- and, with ``share_cross_kv``, over one copy of the cross-attention keys / values per input;
``return_logprobs=True`` returns the log of the probability with which each token was drawn beside the tokens.

The host layer is written once.  Both entry points start from _call_setup (settings, processors, encoder pass, the share
decision, the cache) and take their ``graph`` switch through _graph_stepper; every ``model.last_*`` record is a
graph_decode.Outcome, made by ``Outcome.asked`` from the call's argument and the package switch; the processors are read by
_read_processors and the device by graph_decode._device_why_not, for every kernel plan alike; graph_decode.why_not and each
plan are computed at most once per call (_once) and handed on; _greedy and _sample_eager are one loop, _eager_loop.
"""
import functools
from types import SimpleNamespace

import torch
from torch import nn

from . import graph_decode
from .. import util_layernorm
from .graph_decode import Outcome, _device_why_not

_once = functools.lru_cache(maxsize=None)        # on a lambda without arguments: what a call asks once and hands on

_DEFAULTS = {"max_length": 20, "min_length": 0, "num_beams": 1, "no_repeat_ngram_size": 0, "forced_bos_token_id": None,
             "forced_eos_token_id": None, "length_penalty": 1.0, "early_stopping": False, "num_return_sequences": 1,
             "pad_token_id": None, "eos_token_id": None, "decoder_start_token_id": None, "bos_token_id": None}
_NOT_COVERED = ("do_sample", "return_dict_in_generate", "streamer", "output_scores", "num_beam_groups", "top_k", "top_p",
                "temperature")


def _setting(model, name, given):
    """The explicit argument, else the wrapped model's generation_config, else its config, else transformers' default."""
    if given is not None:
        return given
    for src in (getattr(model, "generation_config", None), model.config):
        v = getattr(src, name, None) if src is not None else None
        if v is not None:
            return v
    return _DEFAULTS[name]


def _processors(min_length, eos, no_repeat, forced_bos, forced_eos, max_length, device):
    from transformers.generation.logits_process import (ForcedBOSTokenLogitsProcessor, ForcedEOSTokenLogitsProcessor,
                                                        LogitsProcessorList, MinLengthLogitsProcessor,
                                                        NoRepeatNGramLogitsProcessor)
    procs = LogitsProcessorList()                # transformers' _get_logits_processor order
    if no_repeat and no_repeat > 0:
        procs.append(NoRepeatNGramLogitsProcessor(no_repeat))
    if min_length and min_length > 0 and eos is not None:
        procs.append(MinLengthLogitsProcessor(min_length, eos, device=device))
    if forced_bos is not None:
        procs.append(ForcedBOSTokenLogitsProcessor(forced_bos))
    if forced_eos is not None:
        procs.append(ForcedEOSTokenLogitsProcessor(max_length, forced_eos, device=device))
    return procs


def _step_logits(model, seq, enc, attention_mask, cache, stepper=None):
    """Logits of the last position: the last token through the cache (``stepper``: by a captured graph where it can), or
    the whole prefix without one."""
    if stepper is not None:
        return stepper.logits(seq, enc, attention_mask, cache)
    if cache is None:
        return model(decoder_input_ids=seq, encoder_outputs=(enc,), attention_mask=attention_mask)[0][:, -1, :]
    logits, cache_out, _ = model(decoder_input_ids=seq[:, -1:], encoder_outputs=(enc,), attention_mask=attention_mask,
                                 past_key_values=cache, use_cache=True)
    assert cache_out is cache
    return logits[:, -1, :]


class BeamSelectInfo(Outcome):
    """What a generate() call did with its beam steps' continuations: ``selected`` steps through ops.beam_select, ``eager``
    steps through the torch lines, and, when none was selected, the ``reason``."""
    COUNTERS = ("selected", "eager")


def _not_restated(proc):
    return f"a logits processor the kernel does not restate ({type(proc).__name__})"


def _read_processors(procs, device):
    """One walk over a call's logits processors for the kernels that restate them (_BeamSelectPlan, _GreedyPlan).  Yields, in
    the list's order: ("ngram", size); ("min_length", (min_length, the ids it bans: int64 on ``device``)); ("forced_bos",
    processor); ("forced_eos", processor) -- what a forced token needs is the plan's to judge -- and, as its last item,
    ("reason", text) at what no kernel restates: another class, a second n-gram or min-length processor, above 16 ids."""
    from transformers.generation.logits_process import (ForcedBOSTokenLogitsProcessor, ForcedEOSTokenLogitsProcessor,
                                                        MinLengthLogitsProcessor, NoRepeatNGramLogitsProcessor)
    kinds = {NoRepeatNGramLogitsProcessor: "ngram", MinLengthLogitsProcessor: "min_length",
             ForcedBOSTokenLogitsProcessor: "forced_bos", ForcedEOSTokenLogitsProcessor: "forced_eos"}
    seen = set()
    for proc in procs:
        kind = kinds.get(type(proc))
        if kind is None or (kind in seen and kind in ("ngram", "min_length")):
            yield "reason", _not_restated(proc)
            return
        seen.add(kind)
        if kind == "ngram":
            yield kind, int(proc.ngram_size)
        elif kind == "min_length":
            ban = proc.eos_token_id.to(device=device, dtype=torch.int64).reshape(-1).contiguous()
            yield kind, (int(proc.min_length), ban)
            if ban.numel() > 16:
                yield "reason", "more than 16 eos ids"
                return
        else:
            yield kind, proc


class _BeamSelectPlan:
    """What ops.beam_select needs from the processor list, read once per call: the n-gram size, min_length with its eos ids
    on the device, and the steps on which a forced token fires (those take the torch lines)."""

    def __init__(self, procs, device, nb, vocab, keep, max_length):
        self.ngram, self.min_length, self.eos, self.forced_at = 0, 0, None, set()
        self.reason = _device_why_not(device)
        if self.reason is None and (keep > vocab or keep > 64 or nb > 64 or max_length > 4096):
            self.reason = "the kernel takes keep <= min(vocab, 64), num_beams <= 64 and max_length <= 4096"
        for kind, value in () if self.reason is not None else _read_processors(procs, device):
            if kind == "ngram":
                self.ngram = value
            elif kind == "min_length":
                self.min_length, self.eos = value
            elif kind == "forced_bos":
                self.forced_at.add(1)
            elif kind == "forced_eos":
                self.forced_at.add(int(value.max_length) - 1)
            else:
                self.reason = value

    def takes(self, cur, logits):
        return self.reason is None and cur not in self.forced_at and logits.is_cuda and logits.dtype == torch.float32


def _select_continuations(logits, flat, running_scores, procs, bsz, nb, vocab, keep, plan=None, info=None):
    """Steps a-c of a beam step: the log-probabilities of the [bsz * nb, vocab] logits, the logits processors on the token
    history ``flat`` [bsz * nb, cur], the running beam scores, and the top ``keep`` continuations of every batch row over
    all its beams: (top_lp [bsz, keep], top_idx [bsz, keep], the flat index beam * vocab + token).  The torch lines, or,
    where ``plan`` takes the step, one call of ops.beam_select."""
    if plan is not None and plan.takes(flat.shape[1], logits):
        from .. import ops
        cur = flat.shape[1]
        if info is not None:
            info.selected += 1
        return ops.beam_select(logits, running_scores, keep, flat, cur, plan.ngram, plan.eos if cur < plan.min_length else None)
    if info is not None:
        info.eager += 1
    log_probs = procs(flat, nn.functional.log_softmax(logits, dim=-1))
    log_probs = (log_probs.view(bsz, nb, vocab) + running_scores[:, :, None]).view(bsz, nb * vocab)
    # c. top-K continuations over all beams
    return torch.topk(log_probs, k=keep)


class ShareCrossKvInfo(Outcome):
    """What a generate() call did with ``share_cross_kv``: ``shared`` beam steps over one copy of the cross-attention keys /
    values per batch row, ``eager`` beam steps over one copy per beam, and, when none was shared, the ``reason``.  Of a
    score() call the two count decoder LAYERS: those whose cross-attention ran on one copy per input, and on expanded rows."""
    COUNTERS = ("shared", "eager")


SHARE_MAX_SOURCE = 1024            # kMaxKv<8> of csrc/decode_attention.hip: the score rows of 8 queries in LDS
SHARE_MAX_BEAMS = 64               # kDecMaxGroup


def _share_why_not(model, device, use_cache, nb, source_len):
    """None when a generate() call can hold the cross-attention keys / values once per batch row, else the reason it
    decodes as without ``share_cross_kv``.  Everything here is known before the first step."""
    if nb == 1:
        return "one beam per batch row (num_beams == 1): there is nothing to share"
    if nb > SHARE_MAX_BEAMS:
        return f"num_beams above {SHARE_MAX_BEAMS}"
    if not use_cache:
        return "use_cache=False: there is no cache"
    reason = _device_why_not(device)
    if reason is not None:
        return reason
    decoder = model.model.decoder
    if _dropout_active(decoder):
        return "dropout is active"
    if source_len > SHARE_MAX_SOURCE:
        return f"the source is longer than {SHARE_MAX_SOURCE}"
    for i, layer in enumerate(decoder.layers):
        attn = layer.encoder_attn
        lpr = attn.head_dim // 4
        if attn.head_dim % 4 or lpr > 64 or lpr & (lpr - 1) or attn.embed_dim != attn.num_heads * attn.head_dim:
            return f"the shared cross-attention does not take head_dim {attn.head_dim}"
        reason = _cross_site_why_not(i, attn)
        if reason is not None:
            return reason
    return None


def _dropout_active(decoder):
    return decoder.training and any(p > 0 for layer in decoder.layers for p in (layer.dropout, layer.encoder_attn.dropout))


def _cross_site_why_not(i, attn):
    """The cross-attention quantizer of decoder layer ``i`` that is not in its plain quantising state, as a reason, or None."""
    for site in ("query", "key", "value", "attention_probs", "context"):
        if not graph_decode._plain(getattr(attn, site + "_post_act_fake_quantize")):
            return f"a cross-attention quantizer is not in the plain quantising state (decoder layer {i}, {site})"
    return None


def score_share_why_not(model, device, n):
    """None when a score() call of ``n`` candidates per input can run every decoder layer's cross-attention on one copy of
    the keys / values per input, else the reason it expands the encoder states as without ``share_cross_kv``.  Everything
    here is known before the decoder runs; lengths and head sizes are no reason: a layer whose launch does not take them
    runs on expanded rows, with the same words."""
    if n == 1:
        return "one candidate per input (num_candidates == 1): there is nothing to share"
    reason = _device_why_not(device)
    if reason is not None:
        return reason
    decoder = model.model.decoder
    if _dropout_active(decoder):
        return "dropout is active"
    for i, layer in enumerate(decoder.layers):
        reason = _cross_site_why_not(i, layer.encoder_attn)
        if reason is not None:
            return reason
    return None


class BeamAdvanceInfo(Outcome):
    """What a generate() call did with its beam steps' bookkeeping: ``advanced`` steps through ops.beam_advance, ``eager``
    steps through the torch lines, and, when none was advanced, the ``reason``."""
    COUNTERS = ("advanced", "eager")


# How ops.beam_advance divides by length ** length_penalty: as torch's GPU kernel divides by a host scalar, a multiplication
# by float32(1 / div) with the reciprocal taken in double (tests/test_gpu_beam_advance.py compares the words with the torch
# lines on the GPU under this flag).
_ADVANCE_RECIPROCAL = True


class _BeamState:
    """The tensors a beam search carries from step to step.  ``buffers``: for the kernel path (``paired``), the two sets of
    buffers a step alternates between -- ops.beam_advance reads one and writes the other."""
    FIELDS = ("running", "running_scores", "finished", "scores", "finished_len", "done", "improvable")

    def __init__(self, running, running_scores, finished, scores, finished_len, done, improvable):
        self.running, self.running_scores, self.finished, self.scores = running, running_scores, finished, scores
        self.finished_len, self.done, self.improvable = finished_len, done, improvable
        self.buffers = None

    @classmethod
    def start(cls, bsz, nb, max_length, start, fill, dev):
        running = torch.full((bsz, nb, max_length), fill, dtype=torch.long, device=dev)
        running[:, :, 0] = start
        finished = running.clone()
        running_scores = torch.zeros((bsz, nb), dtype=torch.float, device=dev)
        running_scores[:, 1:] = -1e9
        scores = torch.full((bsz, nb), -1e9, dtype=torch.float, device=dev)
        done = torch.zeros((bsz, nb), dtype=torch.bool, device=dev)
        improvable = torch.ones((bsz, 1), dtype=torch.bool, device=dev)
        finished_len = torch.zeros((bsz, nb), dtype=torch.long, device=dev)      # generated tokens of each finished beam
        return cls(running, running_scores, finished, scores, finished_len, done, improvable)

    def paired(self):
        """This state in the first of two ops.BeamBuffers: (the current set, the one the next step writes)."""
        from ..ops import BeamBuffers
        bsz, nb, max_length = self.running.shape
        self.buffers = [BeamBuffers(bsz, nb, max_length, self.running.device) for _ in range(2)]
        for name in self.FIELDS:
            getattr(self.buffers[0], name).copy_(getattr(self, name))
        return self.buffers


def _advance_why_not(device, nb, keep, max_length, eos):
    """None when ops.beam_advance takes the steps of this call, else the reason the torch lines run."""
    reason = _device_why_not(device)
    if reason is not None:
        return reason
    if keep > 64 or nb > 64 or not 2 <= max_length <= 4096:
        return "the kernel takes keep <= 64, num_beams <= 64 and max_length in [2, 4096]"
    if eos is not None and eos.numel() > 16:
        return "more than 16 eos ids"
    return None


def _advance_beams_torch(state, top_lp, top_idx, cur, vocab, eos, top_mask, offsets, max_length, length_penalty, early_stopping,
                         reorder=None, prompt=1):
    """Steps c'-g of a beam step at length ``cur`` and the early-stop heuristic, as torch lines: from the top ``keep``
    continuations (top_lp, top_idx [bsz, keep]) and the ``state`` to (the new state, beam_idx [bsz * nb] -- the cache rows
    of the kept beams --, go_on, a 0-dim bool tensor).  ``reorder(beam_idx)`` is called at step g, where the cache follows
    the kept beams."""
    running, running_scores, finished, scores = state.running, state.running_scores, state.finished, state.scores
    finished_len, done, improvable = state.finished_len, state.done, state.improvable
    bsz, nb = running_scores.shape
    keep = top_lp.shape[1]
    dev = top_lp.device
    beam = top_idx // vocab
    top_seq = _gather(running, beam)
    top_seq[:, :, cur] = top_idx % vocab
    rows = beam + offsets
    # d. which of them finished
    hits = torch.full((bsz, keep), cur + 1 >= max_length, dtype=torch.bool, device=dev)
    if eos is not None:
        hits = hits | torch.isin(top_seq[:, :, cur], eos)
    # e. the best num_beams unfinished continue
    top_running_lp = top_lp + hits.to(torch.float32) * -1.0e9
    nxt = torch.topk(top_running_lp, k=nb)[1]
    running = _gather(top_seq, nxt)
    running_scores = _gather(top_running_lp, nxt)
    beam_idx = _gather(rows, nxt).view(-1)
    # f. merge newly finished ones into the finished set
    just = hits & top_mask[None, :]
    cand = top_lp / ((cur + 1 - prompt) ** length_penalty)
    full = torch.all(done, axis=-1, keepdims=True) & (early_stopping is True)
    cand += full.to(torch.float32) * -1.0e9
    cand += (~improvable).to(torch.float32) * -1.0e9
    cand += (~just) * -1.0e9
    merged = torch.topk(torch.cat((scores, cand), dim=1), k=nb)[1]
    finished = _gather(torch.cat((finished, top_seq), dim=1), merged)
    scores = _gather(torch.cat((scores, cand), dim=1), merged)
    finished_len = _gather(torch.cat((finished_len, torch.full_like(top_idx, cur + 1 - prompt)), dim=1), merged)
    done = _gather(torch.cat((done, just), dim=1), merged)
    # g. next iteration: the cache follows the kept beams
    if reorder is not None:
        reorder(beam_idx)
    cur += 1
    # early-stop heuristic and stopping condition (transformers' _check_early_stop_heuristic / _has_unfinished)
    best_len = (max_length - prompt) if (early_stopping == "never" and length_penalty > 0.0) else (cur - prompt)
    best_running = running_scores[:, :1] / (best_len ** length_penalty)
    worst_done = torch.where(done, torch.min(scores, dim=1, keepdim=True)[0], -1.0e9)
    improvable = improvable & torch.any(best_running > worst_done, dim=-1, keepdim=True)
    go_on = torch.any(improvable) & ~(torch.all(done) & (early_stopping is True)) & ~torch.all(hits)
    return _BeamState(running, running_scores, finished, scores, finished_len, done, improvable), beam_idx, go_on


def generate(model, input_ids, attention_mask=None, max_length=None, num_beams=None, use_cache=True, cache_codes=None,
             graph=None, beam_select=None, beam_advance=None, beam_graph=None, greedy_advance=None, greedy_graph=None,
             share_cross_kv=None, **kwargs):
    if kwargs.pop("synced_gpus", False):      # Seq2SeqTrainer's predict_with_generate passes synced_gpus=False
        raise NotImplementedError("generate(): synced_gpus=True is not supported")
    for name in _NOT_COVERED:
        if kwargs.get(name):
            raise NotImplementedError(f"generate(): {name} is not supported (greedy and beam search only)")
    unknown = set(kwargs) - set(_DEFAULTS) - set(_NOT_COVERED)
    if unknown:
        raise TypeError(f"generate(): unexpected arguments {sorted(unknown)}")
    num_beams = _setting(model, "num_beams", num_beams)
    s = _call_setup(model, input_ids, attention_mask, max_length, kwargs, use_cache, cache_codes, share_cross_kv, num_beams)
    get, max_length, start, pad, eos_t, procs = s.get, s.max_length, s.start, s.pad, s.eos_t, s.procs
    enc, attention_mask, share, cache = s.enc, s.attention_mask, s.share, s.cache
    n_return = get("num_return_sequences")
    vocab, keep = model.config.vocab_size, _beam_keep(eos_t, num_beams)
    # what more than one of the switches below asks: answered on first need, once
    graph_why = _once(lambda: graph_decode.why_not(model, enc.device, use_cache, max_length))
    beam_plan = _once(lambda: _BeamSelectPlan(procs, enc.device, num_beams, vocab, keep, max_length))
    greedy_plan = _once(lambda: _GreedyPlan(procs, enc.device, vocab, max_length, eos_t, pad))
    # a whole beam step as one captured graph: it implies the three switches below for this call, where nothing -- known
    # before the first step -- stands against it (one of them passed as False, greedy decoding, a reason one of them would
    # give); else the call decodes as without it
    whole = model.last_beam_graph = graph_decode.BeamGraphInfo.asked(beam_graph, "BEAM_GRAPH")
    if whole.reason is None:
        whole.reason = (_passed_false(graph=graph, beam_select=beam_select, beam_advance=beam_advance)
                        or ("greedy decoding has no beam step (beam_select at one beam is not argmax of the raw logits under ties)"
                            if num_beams == 1 else None)
                        or graph_why() or beam_plan().reason or _advance_why_not(enc.device, num_beams, keep, max_length, eos_t))
        if whole.reason is None:
            graph = beam_select = beam_advance = True
    # a whole greedy step as one captured graph: likewise, for the two switches it implies
    gwhole = model.last_greedy_graph = graph_decode.GreedyGraphInfo.asked(greedy_graph, "GREEDY_GRAPH")
    if gwhole.reason is None:
        gwhole.reason = (_passed_false(graph=graph, greedy_advance=greedy_advance)
                         or ("beam search has no greedy step" if num_beams != 1 else None) or graph_why() or greedy_plan().reason)
        if gwhole.reason is None:
            graph = greedy_advance = True
    stepper, _ = _graph_stepper(model, graph, graph_why)
    select = model.last_beam_select = BeamSelectInfo.asked(beam_select, "BEAM_SELECT")
    advance = model.last_beam_advance = BeamAdvanceInfo.asked(beam_advance, "BEAM_ADVANCE")
    greedy = model.last_greedy_advance = GreedyAdvanceInfo.asked(greedy_advance, "GREEDY_ADVANCE")
    if num_beams != 1 and greedy.reason is None:
        greedy.reason = "beam search has no greedy step"
    if num_beams == 1:
        if select.reason is None:
            select.reason = "greedy decoding selects no beams"
        if advance.reason is None:
            advance.reason = "greedy decoding advances no beams"
        if n_return != 1:
            raise ValueError("greedy decoding returns one sequence per input (num_return_sequences must be 1)")
        if greedy.reason is None:
            greedy.reason = greedy_plan().reason
        if greedy.reason is None:
            return _checked(cache, _greedy_advanced(model, enc, attention_mask, start, greedy_plan(), max_length, cache, stepper,
                                                    greedy, gwhole if gwhole.reason is None else None))
        return _checked(cache, _greedy(model, enc, attention_mask, start, pad, eos_t, procs, max_length, cache, stepper, greedy))
    if n_return > num_beams:
        raise ValueError("num_return_sequences must not exceed num_beams")
    return _checked(cache, _beam_search(model, enc, attention_mask, start, pad, eos_t, procs, max_length, num_beams, n_return,
                                        get("length_penalty"), get("early_stopping"), cache, stepper, select,
                                        advance, whole if whole.reason is None else None, share,
                                        beam_plan() if select.reason is None else None))


def _call_setup(model, input_ids, attention_mask, max_length, kwargs, use_cache, cache_codes, share_cross_kv, group):
    """What generate() and sample() both start from: the settings (``get``, max_length, start, pad, eos_t), the logits
    processors, the default mask and the encoder pass, the share decision for ``group`` decoder rows per input -- decided
    once, here, and set on ``model.last_share_cross_kv`` -- and the cache with its ``cross_group`` and ``cross_one_launch``."""
    from .quant_bart import QuantizedBartCache
    s = SimpleNamespace()
    s.get = get = lambda name, given=None: _setting(model, name, kwargs.get(name, given))  # noqa: E731
    s.max_length = get("max_length", max_length)
    s.pad, s.start = get("pad_token_id"), get("decoder_start_token_id")
    if s.start is None:
        s.start = get("bos_token_id")
    eos = get("eos_token_id")
    s.eos_t = None if eos is None else torch.tensor(eos if isinstance(eos, (list, tuple)) else [eos], device=input_ids.device)
    s.procs = _processors(get("min_length"), s.eos_t, get("no_repeat_ngram_size"), get("forced_bos_token_id"),
                          get("forced_eos_token_id"), s.max_length, input_ids.device)
    s.attention_mask = torch.ones_like(input_ids) if attention_mask is None else attention_mask
    s.enc = model.get_encoder()(input_ids, attention_mask=s.attention_mask)
    codes = util_layernorm.CACHE_CODES if cache_codes is None else bool(cache_codes)
    s.share = model.last_share_cross_kv = ShareCrossKvInfo.asked(share_cross_kv, "SHARE_CROSS_KV")
    if s.share.reason is None:
        s.share.reason = _share_why_not(model, s.enc.device, use_cache, group, s.enc.shape[1])
    s.cache = None
    if use_cache:
        s.cache = QuantizedBartCache(len(model.model.decoder.layers), capacity=s.max_length, codes=codes,
                                     cross_group=group if s.share.reason is None else 1)
        s.cache.cross_one_launch = s.share.reason is None
    return s


def _graph_stepper(model, graph, why_not):
    """The ``graph`` switch of a call: (stepper, info) -- a graph_decode.GenerateStepper where a captured decoding step is
    asked for and ``why_not()`` has no objection, else None and the steps are issued as ever -- with ``info`` set on
    ``model.last_decode_graph``."""
    info = model.last_decode_graph = graph_decode.DecodeGraphInfo.asked(graph, "GRAPH_DECODE")
    if info.reason is None:
        info.reason = why_not()
    return (graph_decode.GenerateStepper(model, info) if info.reason is None else None), info


def _passed_false(**given):
    """The reason a whole-step switch does not hold when one of the switches it implies was passed as False, else None."""
    for name, value in given.items():
        if value is not None and not value:
            return f"{name}=False was passed"
    return None


def _beam_keep(eos, nb):
    """How many continuations of a batch row a beam step keeps: room for every beam to end on each eos id and go on."""
    return max(2, 1 + (eos.shape[0] if eos is not None else 0)) * nb


def _checked(cache, tokens):
    """After the last step on a cache of integer codes: one read of its counter (a host sync).  A cache that holds elements
    without a code has produced NaN, not tokens."""
    if cache is not None and cache.codes:
        bad = cache.rejected()
        if bad:
            raise RuntimeError(f"generate(): the KV cache holds {bad} elements without an integer code (x_quant is NaN or not "
                               "an integer: a NaN / infinite key or value, a non-integer zero point, or quantizer parameters "
                               "rewritten during decoding); decode with cache_codes=False")
    return tokens


def _eager_loop(model, enc, attention_mask, start, pad, eos, procs, max_length, cache, stepper, advance, pick, rows=None,
                logprobs=False):
    """Decoding by the torch lines, one token per row and step: ``pick(scores, cur)`` gives the next tokens [rows] from the
    processed scores at history length ``cur`` and, with ``logprobs``, their log-probabilities (0 for a finished row, and at
    column 0); returns the sequences, with ``logprobs`` (sequences, logprobs)."""
    b = enc.shape[0] if rows is None else rows
    seq = torch.full((b, 1), start, dtype=torch.long, device=enc.device)
    lps = torch.zeros((b, 1), dtype=torch.float32, device=enc.device) if logprobs else None
    unfinished = torch.ones(b, dtype=torch.long, device=enc.device)
    while seq.shape[1] < max_length:
        scores = procs(seq, _step_logits(model, seq, enc, attention_mask, cache, stepper).to(torch.float32))
        nxt, lp = pick(scores, seq.shape[1])
        if lps is not None:
            if eos is not None:
                lp = torch.where(unfinished.bool(), lp, torch.zeros_like(lp))
            lps = torch.cat([lps, lp[:, None]], dim=-1)
        if eos is not None:
            nxt = nxt * unfinished + pad * (1 - unfinished)
        seq = torch.cat([seq, nxt[:, None]], dim=-1)
        if advance is not None:
            advance.eager += 1
        if eos is not None:
            unfinished = unfinished & ~torch.isin(nxt, eos)
            if unfinished.max() == 0:
                break
    return seq if lps is None else (seq, lps)


def _greedy(model, enc, attention_mask, start, pad, eos, procs, max_length, cache, stepper=None, advance=None):
    return _eager_loop(model, enc, attention_mask, start, pad, eos, procs, max_length, cache, stepper, advance,
                       lambda scores, cur: (torch.argmax(scores, dim=-1), None))


class GreedyAdvanceInfo(Outcome):
    """What a generate() call did with its greedy steps: ``advanced`` steps through ops.greedy_advance, ``eager`` steps
    through the torch lines, and, when none was advanced, the ``reason``."""
    COUNTERS = ("advanced", "eager")


class _GreedyPlan:
    """What ops.greedy_advance needs from a call's settings, read once: the n-gram size, min_length with its eos ids on the
    device, the forced tokens, the eos ids and the pad -- or the ``reason`` the torch lines run instead."""

    def __init__(self, procs, device, vocab, max_length, eos, pad):
        self.ngram, self.min_length, self.ban, self.forced_bos, self.forced_eos = 0, 0, None, None, None
        self.eos = None if eos is None else eos.to(device=device, dtype=torch.int64).reshape(-1).contiguous()
        self.pad = 0 if pad is None else int(pad)
        self.max_length = max_length
        self.reason = _device_why_not(device)
        if self.reason is None and not 2 <= max_length <= 4096:
            self.reason = "the kernel takes max_length in [2, 4096]"
        elif self.reason is None and self.eos is not None:
            if self.eos.numel() > 16:
                self.reason = "more than 16 eos ids"
            elif pad is None:
                self.reason = "pad_token_id is missing and an eos is set"
            elif not 0 <= self.pad < vocab:
                self.reason = "pad_token_id is outside the vocabulary"
        for kind, value in () if self.reason is not None else _read_processors(procs, device):
            if kind == "ngram":
                self.ngram = value
            elif kind == "min_length":
                self.min_length, self.ban = value
            elif kind == "forced_bos" and self.forced_bos is None:
                self.forced_bos = int(value.bos_token_id)
            elif (kind == "forced_eos" and self.forced_eos is None and value.eos_token_id.numel() == 1
                  and int(value.max_length) == max_length):
                self.forced_eos = int(value.eos_token_id.reshape(-1)[0])
            else:                                    # the reader's reason, or a forced token this kernel does not take
                self.reason = value if kind == "reason" else _not_restated(value)
                break
        if self.reason is None and any(t is not None and not 0 <= t < vocab for t in (self.forced_bos, self.forced_eos)):
            self.reason = "a forced token is outside the vocabulary"

    def forced(self, cur):
        """The token the processors force at history length ``cur`` (the later processor wins), or None."""
        if self.forced_eos is not None and cur == self.max_length - 1:
            return self.forced_eos
        return self.forced_bos if cur == 1 else None


def _greedy_advanced(model, enc, attention_mask, start, plan, max_length, cache, stepper, advance, whole=None, draw=None):
    """The loop of _greedy with everything after the model step as one call of ops.greedy_advance: the sequence, the
    unfinished flags and the next tokens live in an ops.GreedyBuffers, the model is fed the kernel's next_tokens (without a
    cache: the sequence so far, a view), and the go_on word is read once per token (the one host sync of the torch lines).
    ``draw`` (sample(): dict(seed, temperature, top_k, top_p)): the same loop on ops.sample_advance and an ops.SampleBuffers;
    with ``nucleus`` set in it (top_k == 0 with top_p < 1 under sample_nucleus) on ops.sample_nucleus.  Its ``group`` (n
    sequences per input: the loop runs enc.shape[0] * n rows where the cache shares the cross-attention keys / values, else
    ``enc`` came expanded) and ``logprobs`` (the steps fill the buffers' logprobs; returns (sequences, logprobs)) go to the step.

    ``whole`` (a graph_decode.GreedyGraphInfo; generate(greedy_graph=True)): from the third step on a step is one replay of
    a captured graph that holds all of the above (graph_decode.GreedyStepGraph), a step on which a forced token fires
    included: the kernel takes the forced token itself."""
    from .. import ops
    if draw is None:
        bufs = ops.GreedyBuffers(enc.shape[0], max_length, enc.device, model.config.vocab_size)
    else:
        bufs = ops.SampleBuffers(draw.get("rows", enc.shape[0]), max_length, enc.device, model.config.vocab_size, draw["top_k"],
                                 nucleus=bool(draw.get("nucleus")), logprobs=bool(draw.get("logprobs")))
        grouped = dict(group=draw.get("group", 1), logprobs=bufs.logprobs)
    bufs.seq[:, 0] = start
    cur = 1
    captured = None
    while True:
        if whole is not None and captured is None and cur == 3:
            if stepper is None or stepper.decoder is None:          # the cache the first step left does not fit
                whole.reason, whole = stepper.info.reason if stepper is not None else "no captured step", None
            else:
                captured = (graph_decode.GreedyStepGraph(stepper.decoder, whole, bufs, plan) if draw is None else
                            graph_decode.SampleStepGraph(stepper.decoder, whole, bufs, plan, draw))
        if captured is not None:
            captured.step()
        else:
            tokens = bufs.seq[:, :cur] if cache is None or cur == 1 else bufs.next_tokens.view(-1, 1)
            logits = _step_logits(model, tokens, enc, attention_mask, cache, stepper).to(torch.float32)
            if draw is None:
                ops.greedy_advance(logits, bufs, cur, plan.ngram, plan.ban if cur < plan.min_length else None, plan.forced(cur),
                                   plan.eos, plan.pad)
            elif draw.get("nucleus"):
                ops.sample_nucleus(logits, bufs, cur, draw["seed"], draw["temperature"], draw["top_p"], plan.ngram,
                                   plan.ban if cur < plan.min_length else None, plan.forced(cur), plan.eos, plan.pad, **grouped)
            else:
                ops.sample_advance(logits, bufs, cur, draw["seed"], draw["temperature"], draw["top_k"], draw["top_p"], plan.ngram,
                                   plan.ban if cur < plan.min_length else None, plan.forced(cur), plan.eos, plan.pad, **grouped)
        cur += 1
        advance.advanced += 1
        go_on = int(bufs.go_on)
        if go_on < 0:
            raise RuntimeError(f"{'generate' if draw is None else 'sample'}(): a captured {'greedy' if draw is None else 'sampling'} "
                               f"step met the position {cur - 1}, outside [1, {max_length})")
        if not go_on:
            break
    if whole is not None and whole.captured == 0:
        whole.reason = "the search ended before a step could be captured"
    if draw is not None and draw.get("logprobs"):
        return bufs.seq[:, :cur], bufs.logprobs[:, :cur]
    return bufs.seq[:, :cur]


class SampleAdvanceInfo(GreedyAdvanceInfo):
    """What a sample() call did with its steps: ``advanced`` steps through ops.sample_advance, ``eager`` steps through the
    torch lines (sampling.select_torch), and, when none was advanced, the ``reason``."""


NUCLEUS_MAX_VOCAB = 51200          # kSnMaxVocab of csrc/sample_nucleus.hip: what one workgroup holds in registers


def _sample_why_not(plan, top_k, top_p, nucleus=False, vocab=0):
    """None when ops.sample_advance takes the steps of this call, else the reason the torch lines run: those of _GreedyPlan
    and the two forms the kernel does not have.  ``nucleus`` (sample_nucleus): top_k == 0 with top_p < 1 is
    ops.sample_nucleus's, for a vocabulary it holds."""
    if plan.reason is not None:
        return plan.reason
    if top_k == 0 and top_p < 1.0 and nucleus:
        return f"vocab above {NUCLEUS_MAX_VOCAB}" if vocab > NUCLEUS_MAX_VOCAB else None
    if top_k == 0 and top_p < 1.0:
        return "top_p below 1 without top_k"
    if top_k > 64:
        return "top_k above 64"
    return None


def _sample_eager(model, enc, attention_mask, start, pad, eos, procs, max_length, cache, stepper, advance, draw):
    """_greedy with the arg-max replaced by sampling.select_torch on the host's uniforms of (seed, input, sequence, length).
    ``draw`` with ``logprobs``: returns (sequences, logprobs), sampling.token_logprob of every drawn token (a forced token
    is a row's one survivor: 0), 0 for a finished row."""
    from . import sampling
    group, b, logprobs = draw.get("group", 1), draw.get("rows", enc.shape[0]), bool(draw.get("logprobs"))
    knobs = (draw["temperature"], draw["top_k"], draw["top_p"])

    def pick(scores, cur):
        u = sampling.uniforms(draw["seed"], b // group, cur, group) if group > 1 else sampling.uniforms(draw["seed"], b, cur)
        nxt = sampling.select_torch(scores, u, *knobs)
        return nxt, sampling.token_logprob(scores, nxt, *knobs) if logprobs else None
    return _eager_loop(model, enc, attention_mask, start, pad, eos, procs, max_length, cache, stepper, advance, pick, b, logprobs)


def sample(model, input_ids, attention_mask=None, max_length=None, seed=None, temperature=1.0, top_k=50, top_p=1.0,
           use_cache=True, cache_codes=None, graph=None, sample_advance=None, sample_graph=None, sample_nucleus=None,
           share_cross_kv=None, num_samples=1, return_logprobs=False, **kwargs):
    """Seeded sampling over a KV cache: generate()'s greedy loop with a draw in the place of the arg-max (model/sampling.py;
    the rule is osq_sample_advance's, include/osq_hip.h).  The tokens are a function of the inputs and ``seed`` alone -- the
    package's own random stream, not torch.multinomial's, so they are not transformers' tokens: hence an entry point of its
    own beside generate(), which keeps refusing ``do_sample``.  ``seed=None`` draws a 63-bit seed from torch's default CPU
    generator (torch.manual_seed makes the call reproducible).  ``top_k=0`` keeps every token, ``top_p=1.0`` cuts nothing.

    Settings, logits processors, cache and ``graph`` as in greedy generate().  ``sample_advance=True`` (set_sample_advance)
    hands everything after the model step to one kernel call (ops.sample_advance); ``model.last_sample_advance`` tells how
    many steps took it.  ``sample_graph=True`` (set_sample_graph) asks for ``graph`` and ``sample_advance`` and captures the
    whole step -- token copy, model, ops.sample_advance_at -- into one graph (graph_decode.SampleStepGraph);
    ``model.last_sample_graph`` tells what happened.  ``sample_nucleus=True`` (set_sample_nucleus): under either switch,
    ``top_k=0`` with ``top_p<1`` goes to ops.sample_nucleus(_at) instead of falling back to the torch lines.

    ``num_samples=n`` draws n sequences per input: [B * n, L], the rows of an input adjacent (b * n + j).  Sequence j of
    input b draws at the Philox counter (b, length, j, 0), so a sequence depends on (seed, b, j) and the input alone, not on
    n or the batch; the encoder runs once, on B rows.  ``share_cross_kv=True`` (set_share_cross_kv) then keeps the encoder
    states at B rows and the cross-attention keys / values once per input (QuantizedBartCache(cross_group=n),
    ops.decode_attention_shared), where _share_why_not has no objection (n <= 64, a cache, a source of at most 1024, ...);
    else they are expanded and ``model.last_share_cross_kv.reason`` says why.  ``return_logprobs=True`` returns (sequences,
    logprobs): fp32 [B * n, L], the log of the probability with which each token was drawn from its kept survivors
    (include/osq_hip.h, "seeded sampling"); 0 at column 0, on forced steps and after an eos."""
    import math
    if kwargs.pop("synced_gpus", False):
        raise NotImplementedError("sample(): synced_gpus=True is not supported")
    if kwargs.pop("num_beams", 1) not in (None, 1):
        raise ValueError("sample(): beam sampling is not supported (num_beams must be 1)")
    if kwargs.pop("num_return_sequences", 1) not in (None, 1):
        raise ValueError("sample(): num_return_sequences must be 1 -- several sequences per input are num_samples=n")
    n = int(num_samples)
    if n < 1:
        raise ValueError("sample(): num_samples must be at least 1")
    kwargs.pop("do_sample", None)
    unknown = set(kwargs) - set(_DEFAULTS)
    if unknown:
        raise TypeError(f"sample(): unexpected arguments {sorted(unknown)}")
    temperature, top_k, top_p = float(temperature), int(top_k), float(top_p)
    if not (temperature > 0.0 and math.isfinite(temperature)):
        raise ValueError("sample(): temperature must be positive and finite")
    if top_k < 0 or not 0.0 < top_p <= 1.0:
        raise ValueError("sample(): top_k must not be negative and top_p must lie in (0, 1]")
    if seed is None:
        seed = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64))
    draw = {"seed": int(seed) & 0xFFFFFFFFFFFFFFFF, "temperature": temperature, "top_k": top_k, "top_p": top_p}
    s = _call_setup(model, input_ids, attention_mask, max_length, kwargs, use_cache, cache_codes, share_cross_kv, n)
    max_length, start, pad, eos_t, procs = s.max_length, s.start, s.pad, s.eos_t, s.procs
    enc, attention_mask, share, cache = s.enc, s.attention_mask, s.share, s.cache
    if n > 1 or return_logprobs:
        draw.update(group=n, rows=enc.shape[0] * n, logprobs=bool(return_logprobs))
    if n > 1 and share.reason is not None:
        enc = enc.repeat_interleave(n, dim=0)
        attention_mask = attention_mask.repeat_interleave(n, dim=0)
    plan = _GreedyPlan(procs, enc.device, model.config.vocab_size, max_length, eos_t, pad)
    nucleus = bool(util_layernorm.SAMPLE_NUCLEUS if sample_nucleus is None else sample_nucleus)
    draw["nucleus"] = nucleus and top_k == 0 and top_p < 1.0
    graph_why = _once(lambda: graph_decode.why_not(model, enc.device, use_cache, max_length))
    kernel_why = _sample_why_not(plan, top_k, top_p, nucleus, model.config.vocab_size)
    # a whole step as one captured graph: it implies the two switches below for this call, where nothing stands against it
    whole = model.last_sample_graph = graph_decode.SampleGraphInfo.asked(sample_graph, "SAMPLE_GRAPH")
    if whole.reason is None:
        whole.reason = _passed_false(graph=graph, sample_advance=sample_advance) or graph_why() or kernel_why
        if whole.reason is None:
            graph = sample_advance = True
    stepper, _ = _graph_stepper(model, graph, graph_why)
    advance = model.last_sample_advance = SampleAdvanceInfo.asked(sample_advance, "SAMPLE_ADVANCE")
    if advance.reason is None:
        advance.reason = kernel_why
    if advance.reason is None:
        out = _greedy_advanced(model, enc, attention_mask, start, plan, max_length, cache, stepper, advance,
                               whole if whole.reason is None else None, draw)
    else:
        out = _sample_eager(model, enc, attention_mask, start, pad, eos_t, procs, max_length, cache, stepper, advance, draw)
    if n > 1:                                        # every step went over one copy per input, or over one per sequence
        steps = advance.advanced + advance.eager
        share.shared, share.eager = (steps, 0) if share.reason is None else (0, steps)
    return _checked(cache, out)


def _gather(t, idx):
    """t[b, idx[b, k], ...] for a [B, N, ...] tensor and a [B, K] index."""
    while idx.dim() < t.dim():
        idx = idx.unsqueeze(-1)
    return torch.gather(t, 1, idx.expand(*idx.shape[:2], *t.shape[2:]))


def _beam_search(model, enc, attention_mask, start, pad, eos, procs, max_length, nb, n_return, length_penalty,
                 early_stopping, cache, stepper=None, select=None, advance=None, whole=None, share=None, plan=None):
    """transformers' vectorised beam search (GenerationMixin._beam_search, 5.x) with the prompt of one start token.
    ``share`` (a ShareCrossKvInfo without a reason): the encoder states and their mask stay at one row per input -- the cache
    was built with ``cross_group=nb`` and the cross-attention reads one copy of its keys / values per batch row.  ``plan``:
    the call's _BeamSelectPlan where generate() has built it; None: it is built here, where ``select`` asks for one."""
    dev = enc.device
    bsz = enc.shape[0]
    if share is not None and share.reason is not None:
        share = None
    if share is None:
        enc = enc.repeat_interleave(nb, dim=0)
        attention_mask = attention_mask.repeat_interleave(nb, dim=0)
    vocab = model.config.vocab_size
    prompt = cur = 1
    keep = _beam_keep(eos, nb)
    top_mask = torch.cat((torch.ones(nb, dtype=torch.bool), torch.zeros(keep - nb, dtype=torch.bool))).to(dev)
    fill = (pad if pad else int(eos[0])) if eos is not None else -1
    state = _BeamState.start(bsz, nb, max_length, start, fill, dev)
    offsets = torch.arange(bsz, device=dev).view(-1, 1) * nb
    if select is None or select.reason is not None:
        plan = None
    else:
        plan = _BeamSelectPlan(procs, dev, nb, vocab, keep, max_length) if plan is None else plan
        select.reason = plan.reason
    if advance is not None and advance.reason is None:
        advance.reason = _advance_why_not(dev, nb, keep, max_length, eos)
    if whole is not None and (select.reason or advance.reason):      # generate() asked the same questions before the first step
        whole.reason, whole = select.reason or advance.reason, None
    if advance is not None and advance.reason is None:
        return _beam_search_advanced(model, enc, attention_mask, eos, procs, max_length, nb, n_return, length_penalty,
                                     early_stopping, cache, stepper, select, advance, state, plan, vocab, keep, whole, share)
    def reorder(beam_idx):
        nonlocal cache
        if cache is not None:
            cache = model._reorder_cache(cache, beam_idx)
    while True:
        flat = state.running[:, :, :cur].reshape(bsz * nb, cur)
        logits = _step_logits(model, flat, enc, attention_mask, cache, stepper).to(torch.float32)
        top_lp, top_idx = _select_continuations(logits, flat, state.running_scores, procs, bsz, nb, vocab, keep, plan, select)
        state, _, go_on = _advance_beams_torch(state, top_lp, top_idx, cur, vocab, eos, top_mask, offsets, max_length,
                                               length_penalty, early_stopping, reorder, prompt)
        cur += 1
        if advance is not None:
            advance.eager += 1
        _count_share(model, share)
        if not bool(go_on):
            break
    return _beam_result(state, select, n_return, prompt)


def _count_share(model, share):
    """One beam step went by: over shared cross-attention keys / values (``share``), or over one copy per beam."""
    if share is not None:
        share.shared += 1
    elif getattr(model, "last_share_cross_kv", None) is not None:
        model.last_share_cross_kv.eager += 1


def _beam_search_advanced(model, enc, attention_mask, eos, procs, max_length, nb, n_return, length_penalty, early_stopping,
                          cache, stepper, select, advance, state, plan, vocab, keep, whole=None, share=None):
    """The loop of _beam_search with the bookkeeping of every step as one call of ops.beam_advance: the state lives in two
    sets of buffers, a step reads one and writes the other.  The token history goes to the selection as a row-strided view
    of ``running``, the model is fed the kernel's next_tokens, the cache follows its beam_idx, and the go_on word is read
    once per step (the one host sync of the torch lines).

    ``whole`` (a graph_decode.BeamGraphInfo; generate(beam_graph=True)): from the third step on a step is one replay of a
    captured graph that holds all of the above (graph_decode.BeamStepGraphs) -- but a step on which a forced token fires,
    which is issued launch by launch on the capture stream and takes the lines below."""
    from .. import ops
    bsz = state.running.shape[0]
    prompt = cur = 1
    now, spare = sets = state.paired()
    eos_ids = None if eos is None else eos.to(torch.int64).reshape(-1).contiguous()
    graphs = None
    while True:
        if whole is not None and graphs is None and cur == prompt + 2:
            if stepper is None or stepper.decoder is None:          # the cache the first step left does not fit
                whole.reason, whole = stepper.info.reason if stepper is not None else "no captured step", None
            else:
                graphs = graph_decode.BeamStepGraphs(stepper.decoder, whole, sets, plan, keep, vocab, eos_ids, early_stopping,
                                                     length_penalty, _ADVANCE_RECIPROCAL)
        if graphs is not None and cur not in plan.forced_at:
            now, spare = graphs.step(0 if now is sets[0] else 1), now
            cur += 1
            select.selected += 1
            advance.advanced += 1
            _count_share(model, share)
            go_on = int(now.go_on)
            if go_on < 0:
                raise RuntimeError(f"generate(): a captured beam step met the position {cur - 1}, outside [1, {max_length})")
            if not go_on:
                break
            continue
        flat = now.running.view(bsz * nb, max_length)[:, :cur]
        tokens = flat if cache is None or cur == prompt else now.next_tokens.view(-1, 1)
        if graphs is not None:
            logits = stepper.decoder.issue(tokens, attention_mask).to(torch.float32)
            whole.issued += 1
        else:
            logits = _step_logits(model, tokens, enc, attention_mask, cache, stepper).to(torch.float32)
        top_lp, top_idx = _select_continuations(logits, flat, now.running_scores, procs, bsz, nb, vocab, keep, plan, select)
        best_len = (max_length - prompt) if (early_stopping == "never" and length_penalty > 0.0) else (cur + 1 - prompt)
        ops.beam_advance(top_lp, top_idx, now, spare, cur, vocab, eos_ids, early_stopping,
                         (cur + 1 - prompt) ** length_penalty, best_len ** length_penalty, _ADVANCE_RECIPROCAL)
        now, spare = spare, now
        if cache is not None:
            cache = model._reorder_cache(cache, now.beam_idx)
        cur += 1
        advance.advanced += 1
        _count_share(model, share)
        if not int(now.go_on):
            break
    if whole is not None and whole.captured == 0:
        whole.reason = "the search ended before a step could be captured"
    return _beam_result(now, select, n_return, prompt)


def _beam_result(state, select, n_return, prompt):
    bsz, _, max_length = state.finished.shape
    if select is not None and select.reason is None and select.selected == 0:
        select.reason = "a forced token fired on every step"
    seqs = state.finished[:, :n_return].reshape(bsz * n_return, max_length)
    length = prompt + int(state.finished_len[:, :n_return].max())
    return seqs[:, :length]

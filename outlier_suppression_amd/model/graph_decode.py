"""A cached BART decoding step as a captured graph, replayed once per token.

A step over the KV cache is several hundred small launches, and the host issuing them is what bounds it (DESIGN.md,
section 4).  Capturing the step into a hipGraph and replaying it takes the host out -- once nothing the host knows about
the position is baked into a launch.  So the cache goes into device-position mode (quant_bart.QuantizedBartCache): the past
length lives in one device int32, the append and the self-attention read it in their launches
(ops.fake_quant_kv_append_at / _codes_at, ops.decode_attention_at), the position embedding is indexed by a tensor derived
from it, and the decoder advances it after its last layer.  A captured step is then: position embedding, every layer, the
LM head, the position increment -- a single chain on one stream.

    step 0        eager: it computes the cross-attention keys / values and allocates the cache
    step 1        eager on the capture stream, the cache now in device-position mode: per-stream workspaces come to exist
    step 2, ...   captured on first need, replayed from then on

Which graph a step needs goes by what the step does to the cache: appending in place (greedy decoding: one graph), or, with
a beam reorder pending, copying the kept prefix from the current buffers into their partners through the row index, A -> B
or B -> A (beam search: two graphs, replayed alternately).  Inputs are static buffers filled before a replay: the last token,
the cache's row index (QuantizedBartCache.reorder) and the encoder mask; the logits are the graph's own output tensor, valid
until its next replay.  Beam bookkeeping and logits processors stay outside these graphs.  The graphs live as long as the
GraphDecoder: one generate() call.

A whole beam-search step (BeamStepGraphs; generate(beam_graph=True)) goes one further: the selection and the bookkeeping
read the position from the same device word -- after the decoder's increment it is the step's length ``cur`` -- through
ops.beam_select_at / ops.beam_advance_at, so the captured chain is: the copy of the current beam set's next_tokens into the
token buffer, the model step, the selection on the graph's own logits, the bookkeeping from the current set of state
buffers into the other, the copy of the new beam_idx into the cache's row index.  Two graphs again, cache A -> B with beam
set 0 -> 1 and the reverse; per token the host does the cache's bookkeeping, one replay and one read of go_on.  A step on
which a forced token fires is issued launch by launch on the capture stream (GraphDecoder.issue), as step 1 is.

A whole greedy step (GreedyStepGraph; generate(greedy_graph=True)) is the same idea with no beam state: the copy of the
search's next_tokens into the token buffer, the model step, and ops.greedy_advance_at on the graph's own logits with the
cache's position word -- bans, arg-max, pad / eos, the new token into the sequence, go_on.  One graph, keyed as the in-place
graph above; the kernel takes a forced token itself at its position, so no step is issued launch by launch.

The words are those of issuing the same steps one by one with the one-launch attention on (util_layernorm.
FUSE_DECODE_ATTENTION): a captured step always uses it, cross-attention included, whatever the switch says.

All three kinds of step look their graph up, capture it or replay it through one method, GraphDecoder.replay: they differ in
the key, in the chain they issue while capturing, and in the records that count.  Those records -- and generation.py's -- are
subclasses of Outcome, below; _device_why_not is the device / autograd pair of reasons that every kernel path of decoding
starts from.
"""
import time

import torch

from .. import util_layernorm as _UL
from ..quantization.fake_quant import QuantizeBase


class Outcome:
    """What a call did with one of its switches, as ``model.last_*`` holds it: the integer ``COUNTERS`` a subclass names,
    its ``SECONDS`` (floats that stay out of the repr), and, when the call decoded as without the switch, the ``reason``."""
    COUNTERS, SECONDS = (), ()

    def __init__(self, reason=None):
        for name in self.COUNTERS:
            setattr(self, name, 0)
        for name in self.SECONDS:
            setattr(self, name, 0.0)
        self.reason = reason

    def __repr__(self):
        counts = "".join(f"{name}={getattr(self, name)}, " for name in self.COUNTERS)
        return f"{type(self).__name__}({counts}reason={self.reason!r})"

    @classmethod
    def asked(cls, given, flag):
        """The record of a call that was passed ``given`` for a switch whose package-wide value is util_layernorm's
        ``flag``, read now: without a reason where either asks for it, else "not asked for"."""
        return cls(None if (getattr(_UL, flag) if given is None else given) else "not asked for")


class DecodeGraphInfo(Outcome):
    """What a generate() call did with its decoding steps: ``captured`` graphs, ``replays`` of them, and, when no step was
    captured, the ``reason``.  ``capture_seconds``: host time spent capturing and instantiating, the device idle."""
    COUNTERS, SECONDS = ("captured", "replays"), ("capture_seconds",)


def _plain(q):
    return q.fake_quant_enabled == 1 and q.observer_enabled != 1 and q.ch_axis == -1 and q.scale.is_cuda


def _device_why_not(device, between=None):
    """The reason none of the decoding kernels runs for tensors on ``device`` under the present autograd mode, or None.
    ``between``: a caller's own reason that ranks after the device and before autograd."""
    if device.type != "cuda":
        return "the tensors are on the CPU"
    if between is not None:
        return between
    return "autograd is on" if torch.is_grad_enabled() else None


def why_not(model, device, use_cache=True, max_length=None):
    """None when a decoding step of ``model`` can be captured, else the reason it cannot (generate() then decodes as it
    always did).  Everything here is known before the first step."""
    reason = _device_why_not(device, None if use_cache else "use_cache=False: there is no cached step")
    if reason is not None:
        return reason
    if not _UL.FUSE_KV_APPEND:
        return "the one-launch KV append is off (util_layernorm.FUSE_KV_APPEND)"
    decoder = model.model.decoder
    if max_length is None or not 2 <= max_length <= 4096:
        return "the one-launch attention takes lengths up to 4096"
    if decoder.training:
        rates = [decoder.dropout] + [p for layer in decoder.layers
                                     for p in (layer.dropout, layer.activation_dropout, layer.self_attn.dropout,
                                               layer.encoder_attn.dropout)]
        if any(p > 0 for p in rates):
            return "dropout is active"
    for name, m in list(decoder.named_modules()) + list(model.lm_head.named_modules()):
        if isinstance(m, QuantizeBase) and m.observer_enabled == 1:
            return f"an observer is enabled ({name})"
    for i, layer in enumerate(decoder.layers):
        for attn, sites in ((layer.self_attn, ("query", "key", "value", "attention_probs", "context")),
                            (layer.encoder_attn, ("query", "attention_probs", "context"))):
            lpr = attn.head_dim // 4
            if attn.head_dim % 4 or lpr > 64 or lpr & (lpr - 1) or attn.embed_dim != attn.num_heads * attn.head_dim:
                return f"the one-launch append and attention do not take head_dim {attn.head_dim}"
            for site in sites:
                if not _plain(getattr(attn, site + "_post_act_fake_quantize")):
                    return f"a quantizer is not in the plain quantising state (decoder layer {i}, {site})"
    return None


def _cache_fits(cache):
    """After the first step: the reason the cache it left cannot go into device-position mode, or None."""
    for i in range(len(cache)):
        k, v, cross = cache._k[i], cache._v[i], cache._cross[i]
        if k is None or cross is None:
            return f"decoder layer {i} holds no keys / values after the first step"
        if k.dim() != 4 or not (k.is_contiguous() and v.is_contiguous()) or k.shape[2] != cache.capacity or k.shape != v.shape:
            return f"decoder layer {i} took the eager append: its cache is no [B, h, capacity, d] buffer"
        if k.dtype != v.dtype:
            return f"decoder layer {i} holds keys and values in different formats"
        if cross[0].dtype != cross[1].dtype:
            return f"decoder layer {i} holds its cross-attention keys and values in different formats"
    return None


class GraphDecoder:
    """The decoding steps after the first, for one encoder batch and one cache: ``step(tokens)`` returns the logits
    [B, vocab] of the next position, by a captured graph from the third step on.  ``enc`` / ``attention_mask`` are the
    encoder states and mask the steps attend to: beam-expanded, or -- over a cache that holds the cross-attention keys / values
    once per batch row (``cross_group``) -- one row per input; ``cache`` is the QuantizedBartCache the first step left."""

    def __init__(self, model, enc, attention_mask, cache, info=None):
        self.model, self.cache = model, cache
        self.info = DecodeGraphInfo() if info is None else info
        self.enc = enc
        self.mask, self._mask_given = attention_mask.clone(), attention_mask
        self.tokens = torch.zeros((enc.shape[0] * cache.cross_group, 1), dtype=torch.long, device=enc.device)
        self.stream = torch.cuda.Stream(device=enc.device)
        self.graphs = {}
        self.warm = False
        cache.enter_device_position()

    def _issue(self):
        """One step's launches, as the model issues them; the one-launch attention on for the cross-attention as well."""
        old = _UL.FUSE_DECODE_ATTENTION
        _UL.FUSE_DECODE_ATTENTION = True
        try:
            logits, cache, _ = self.model(decoder_input_ids=self.tokens, encoder_outputs=(self.enc,), attention_mask=self.mask,
                                          past_key_values=self.cache, use_cache=True)
        finally:
            _UL.FUSE_DECODE_ATTENTION = old
        assert cache is self.cache
        return logits[:, -1, :]

    def check_room(self):
        cache = self.cache
        if not cache.positioned():
            raise RuntimeError("GraphDecoder: the cache left device-position mode (it was read with a reorder pending)")
        if cache.get_seq_length() + 1 > cache.capacity:
            raise RuntimeError(f"GraphDecoder: the cache is full ({cache.capacity} positions)")

    def _feed(self, tokens, attention_mask):
        self.check_room()
        self.tokens.copy_(tokens)
        if attention_mask is not None and attention_mask is not self._mask_given:      # another mask than the one held
            self.mask.copy_(attention_mask)
            self._mask_given = attention_mask

    def _issued(self):
        """The step issued launch by launch on the capture stream, not captured; the current stream waits for it."""
        current = torch.cuda.current_stream(self.enc.device)
        self.stream.wait_stream(current)
        with torch.cuda.stream(self.stream):
            logits = self._issue()
        current.wait_stream(self.stream)
        logits.record_stream(current)
        return logits

    def issue(self, tokens, attention_mask=None):
        """A step that is not to be captured (a forced token fires on it): its logits, issued as the second step is."""
        self._feed(tokens, attention_mask)
        self.warm = True
        return self._issued()

    def step(self, tokens, attention_mask=None):
        cache = self.cache
        self._feed(tokens, attention_mask)
        if not self.warm:
            # issued, not captured: whatever a stream allocates on first use (workspaces) exists before a capture on it
            self.warm = True
            return self._issued()
        # the graph this step needs: in place, or moving from the current buffers into their partners
        return self.replay(self.graphs, (cache.reorder_pending(), cache._k[0].data_ptr()), self._issue, (self.info,))

    def replay(self, graphs, key, chain, infos, reorders=False):
        """One step by a replay of ``graphs[key]``: the one capture-or-replay path of the model step and of the whole
        steps below.  A missing graph is captured first -- ``chain()`` issues the step's launches on the capturing stream
        and returns its logits -- which does the host side of the step as well: the cache's counters move as the model
        and the chain run, recorded, not executed.  On a later replay nothing of that runs, so the host side is done
        here: ``cache.stepped()`` and, where the chain ``reorders``, ``cache.reorder_carried()``.  Every record of
        ``infos`` counts the capture, its seconds and the replay.  Returns the graph's logits tensor."""
        entry = graphs.get(key)
        if entry is None:
            t0 = time.perf_counter()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=self.stream):
                logits = chain()
            entry = graphs[key] = (graph, logits)
            seconds = time.perf_counter() - t0
            for info in infos:
                info.captured += 1
                info.capture_seconds += seconds
        else:
            self.cache.stepped()
            if reorders:
                self.cache.reorder_carried()
        entry[0].replay()
        for info in infos:
            info.replays += 1
        return entry[1]


class BeamGraphInfo(Outcome):
    """What a generate() call did with ``beam_graph``: ``captured`` whole-step graphs, ``replays`` of them, steps ``issued``
    launch by launch because a forced token fired on them, and, when the call decoded as without the switch, the
    ``reason``.  ``capture_seconds``: host time spent capturing and instantiating."""
    COUNTERS, SECONDS = ("captured", "replays", "issued"), ("capture_seconds",)


class BeamStepGraphs:
    """Whole beam-search steps of one generate() call as captured graphs, over a warm GraphDecoder and the two
    ops.BeamBuffers ``sets`` of the search.  ``step(which)`` advances from ``sets[which]`` into the other set -- token copy,
    model step, selection, bookkeeping, the cache's row index -- by one replay; the caller reads the new set's go_on."""

    def __init__(self, decoder, info, sets, plan, keep, vocab, eos_ids, early_stopping, length_penalty, reciprocal):
        from .. import ops
        self.decoder, self.info, self.sets, self.plan = decoder, info, sets, plan
        self.keep, self.vocab, self.eos_ids, self.early_stopping, self.reciprocal = keep, vocab, eos_ids, early_stopping, reciprocal
        bsz, nb, self.max_length = sets[0].running.shape
        dev = sets[0].running.device
        self.top_lp = torch.empty((bsz, keep), dtype=torch.float32, device=dev)
        self.top_idx = torch.empty((bsz, keep), dtype=torch.int64, device=dev)
        self.workspace = torch.empty(ops.beam_select_workspace_bytes(bsz, nb, vocab, keep), dtype=torch.uint8, device=dev)
        # the divisors of every step, from the search's own Python expressions: a launch reads its step's words
        self.len_table, self.best_table = ops.beam_div_tables(self.max_length, length_penalty, early_stopping, reciprocal, dev)
        self.graphs = {}

    def _chain(self, now, spare):
        """One step's launches, in order, on the current (capturing) stream."""
        from .. import ops
        decoder, cache, plan = self.decoder, self.decoder.cache, self.plan
        decoder.tokens.copy_(now.next_tokens.view(-1, 1))
        logits = decoder._issue().to(torch.float32)
        cur = cache.position()                      # after the decoder's increment: the length of the history, this step's cur
        rows = now.running.shape[0] * now.running.shape[1]
        ops.beam_select_at(logits, now.running_scores, self.keep, cur, 0, self.max_length,
                           seq=now.running.view(rows, self.max_length), ngram=plan.ngram, ban_ids=plan.eos,
                           ban_below=plan.min_length, top_lp=self.top_lp, top_idx=self.top_idx, workspace=self.workspace)
        ops.beam_advance_at(self.top_lp, self.top_idx, now, spare, cur, 0, self.vocab, self.len_table, self.best_table,
                            self.eos_ids, self.early_stopping, self.reciprocal)
        cache.reorder(spare.beam_idx)               # the copy into the static row index; pending, on the host side
        return logits

    def step(self, which):
        decoder, cache = self.decoder, self.decoder.cache
        decoder.check_room()
        now, spare = self.sets[which], self.sets[1 - which]
        decoder.replay(self.graphs, (which, cache.reorder_pending(), cache._k[0].data_ptr()),
                       lambda: self._chain(now, spare), (self.info, decoder.info), reorders=True)
        return spare


class GreedyGraphInfo(Outcome):
    """What a generate() call did with ``greedy_graph``: ``captured`` whole-step graphs, ``replays`` of them, and, when the
    call decoded as without the switch, the ``reason``.  ``capture_seconds``: host time spent capturing and instantiating."""
    COUNTERS, SECONDS = ("captured", "replays"), ("capture_seconds",)


class GreedyStepGraph:
    """Whole greedy steps of one generate() call as a captured graph, over a warm GraphDecoder, the ops.GreedyBuffers
    ``buffers`` of the search and its ``plan`` (generation._GreedyPlan).  ``step()`` takes one step in place -- token copy,
    model step, bans, arg-max, pad / eos, the new token into buffers.seq -- by one replay; the caller reads buffers.go_on."""

    def __init__(self, decoder, info, buffers, plan):
        self.decoder, self.info, self.buffers, self.plan = decoder, info, buffers, plan
        self.graphs = {}

    def _chain(self):
        """One step's launches, in order, on the current (capturing) stream."""
        from .. import ops
        decoder, bufs, plan = self.decoder, self.buffers, self.plan
        decoder.tokens.copy_(bufs.next_tokens.view(-1, 1))
        logits = decoder._issue().to(torch.float32)
        cur = decoder.cache.position()              # after the decoder's increment: the length of the history, this step's cur
        self._advance(ops, logits, cur, dict(ngram=plan.ngram, ban_ids=plan.ban, ban_below=plan.min_length,
                                             forced_bos=plan.forced_bos, forced_eos=plan.forced_eos, eos_ids=plan.eos, pad=plan.pad))
        return logits

    def _advance(self, ops, logits, cur, settings):
        ops.greedy_advance_at(logits, self.buffers, cur, 0, **settings)

    def step(self):
        decoder, cache = self.decoder, self.decoder.cache
        decoder.check_room()
        decoder.replay(self.graphs, (cache.reorder_pending(), cache._k[0].data_ptr()), self._chain, (self.info, decoder.info))


class SampleGraphInfo(GreedyGraphInfo):
    """What a sample() call did with ``sample_graph``: as GreedyGraphInfo."""


class SampleStepGraph(GreedyStepGraph):
    """Whole sampling steps of one sample() call as a captured graph: GreedyStepGraph over an ops.SampleBuffers, with
    ops.sample_advance_at in the place of the arg-max -- ops.sample_nucleus_at where ``draw`` has ``nucleus`` set (top_k == 0
    with top_p < 1 under sample_nucleus).  ``draw``: dict(seed, temperature, top_k, top_p), kernel arguments and constant for
    the call; the generator is keyed by (seed, input, sequence, position) and has no state, so one graph serves every step.
    ``draw["group"]`` sequences per input and the buffers' ``logprobs`` go to the step as they are."""

    def __init__(self, decoder, info, buffers, plan, draw):
        super().__init__(decoder, info, buffers, plan)
        self.draw = draw

    def _advance(self, ops, logits, cur, settings):
        settings = dict(settings, group=self.draw.get("group", 1), logprobs=self.buffers.logprobs)
        if self.draw.get("nucleus"):
            ops.sample_nucleus_at(logits, self.buffers, cur, self.draw["seed"], 0, self.draw["temperature"], self.draw["top_p"],
                                  **settings)
            return
        ops.sample_advance_at(logits, self.buffers, cur, self.draw["seed"], 0, self.draw["temperature"], self.draw["top_k"],
                              self.draw["top_p"], **settings)


class GenerateStepper:
    """generate()'s steps with ``graph=True``: the first through the model, the rest through a GraphDecoder -- or all of
    them through the model when a step cannot be captured (``info.reason`` says why)."""

    def __init__(self, model, info):
        self.model, self.info, self.decoder = model, info, None

    def logits(self, seq, enc, attention_mask, cache):
        if self.decoder is not None:
            return self.decoder.step(seq[:, -1:], attention_mask)
        logits, cache_out, _ = self.model(decoder_input_ids=seq[:, -1:], encoder_outputs=(enc,), attention_mask=attention_mask,
                                          past_key_values=cache, use_cache=True)
        assert cache_out is cache
        if self.info.reason is None and seq.shape[1] == 1:
            self.info.reason = _cache_fits(cache)
            if self.info.reason is None:
                self.decoder = GraphDecoder(self.model, enc, attention_mask, cache, self.info)
        return logits[:, -1, :]

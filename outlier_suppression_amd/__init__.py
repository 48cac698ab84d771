"""MI355X-native fake-quant / observer hot path of Outlier Suppression.

``outlier_suppression_amd.quantization`` mirrors the reference's
``quant_transformer.quantization`` import surface (same class and function names,
constructor arguments, buffers and state-dict keys); underneath, every reduction and
every scale-clip-round-dequant pass is a hand-written gfx950 HIP kernel reached
through the C ABI in ``include/osq_hip.h``.  There is no CPU path.
"""
__version__ = "0.1.0"


def _env_on(name, environ=None):
    """What an on / off environment variable asks for: unset, empty or "0" -> False, anything else -> True."""
    import os
    return (os.environ if environ is None else environ).get(name, "") not in ("", "0")


def set_strict(on=True, simd_width=8, backward=None, _lib=None):
    """Which rounding of the path's two whole-tensor sums is returned: the REFERENCE's own order, or the correctly rounded sum.

    Two numbers of the path are sums over a whole activation: the loss of a per-tensor MSEFast search
    (`.pow(2).mean()`, quantization/observer.py:420-432) and the LSQ / LSQ+ parameter gradients (autograd's `sum_to_size`,
    quantization/util_quant.py:29-67).  The reference adds them with torch.sum on the CPU, whose order (ATen's
    cascade_sum) depends on the host's SIMD width and -- beyond 32768 elements -- on its thread count.  The order this
    package can pin is torch's on a ONE-thread host with ``simd_width`` fp32 lanes per vector (8: x86 torch; float64 sums
    use half as many), at any length (csrc/aten_order.h).  Note what that target is: the upstream reference hard-codes
    `.cuda()` on this path (observer.py:81,95,425), so no upstream run ever had this order -- it is the order of the
    reference's code run on a CPU with torch.set_num_threads(1), which is what the golden fixtures are
    (tests/golden/make_golden*.py); a multi-threaded CPU run differs from it beyond 32768 elements.

    ``on`` -- the MSEFast losses.  ON by default: min_val / max_val / scale / zero_point of every MSEFast observer equal
    that reference run bit for bit, and it is also the FASTER form of an observer pass (the searches of a forward run as
    rounds, quantization/deferred.py: BASELINE configs[3] 0.47-0.50 s against 2.2 s since round 6).  A lone search pays one launch per
    evaluation (15-24 us against 6-9 for the resident order-free form).  Per-channel (row) searches follow the
    reference's order in either mode.

    ``backward`` -- scale.grad / zero_point.grad of the learnable quantizers (default: follows ``on`` when set_strict is
    called; OFF in the package's default tier since round 5).  ON: bit-equal to the reference's one-thread autograd run
    (tests/test_gpu_strict_order.py; per-channel weights with ch_axis = 0 and rows of up to 3072 columns included).  OFF:
    float64 accumulation rounded once -- within 2e-5 of autograd's fp32 sums, 1.3x faster (53 against 68 us on
    [256,128,768]); BASELINE.json asks 1e-5 on the dequantised tensor and names no bar for gradients.

    Default tier when the library loads: ``set_strict(True, backward=False)``.  OSQ_STRICT=1: everything in the
    reference's order; OSQ_STRICT=0: everything order-free; OSQ_STRICT_SIMD=16 for a 16-lane reference host.
    ``reset_tier()`` returns to what the environment says."""
    from . import ops
    if simd_width not in (8, 16):
        raise ValueError("simd_width must be 8 or 16")
    backward = on if backward is None else backward
    ops.set_tuning("mse_sum_order", simd_width if on else 0, _lib)
    ops.set_tuning("bwd_sum_order", simd_width if backward else 0, _lib)


def set_fast(on=True):
    """The one-launch LayerNorm site (util_layernorm.FUSE_LAYERNORM; default ON since round 5 -- see there for how it
    compares with torch-ROCm's LayerNorm against the reference's CPU run).  ``set_fast(False)`` keeps the eager sequence."""
    from . import util_layernorm
    util_layernorm.FUSE_LAYERNORM = bool(on)


def set_fast_softmax(on=True):
    """The one-launch attention-probabilities site (util_layernorm.FUSE_SOFTMAX: mask + softmax + fake-quant; default
    OFF -- see there for how it compares with the eager sequence).  OSQ_FAST_SOFTMAX=1 turns it on at load."""
    from . import util_layernorm
    util_layernorm.FUSE_SOFTMAX = bool(on)


def set_fast_decode_attention(on=True):
    """The one-launch attention of a cached decoding step (util_layernorm.FUSE_DECODE_ATTENTION: scores, mask, softmax,
    probabilities quantizer, context, context quantizer over the KV cache; default OFF -- tolerance-equal to the eager
    sequence, not bit-equal).  OSQ_FAST_DECODE_ATTENTION=1 turns it on at load."""
    from . import util_layernorm
    util_layernorm.FUSE_DECODE_ATTENTION = bool(on)


def set_fast_attention(on=True):
    """The one-launch attention over whole sequences (util_layernorm.FUSE_ATTENTION: both products, scaling, mask, softmax,
    probabilities quantizer, merge heads and context quantizer of a BERT / RoBERTa / BART attention block with more than one
    query token, csrc/attention_block.hip; default OFF -- tolerance-equal to the eager sequence, not bit-equal).
    OSQ_FAST_ATTENTION=1 turns it on at load."""
    from . import util_layernorm
    util_layernorm.FUSE_ATTENTION = bool(on)


def set_fast_attention_int(on=True):
    """The one-launch attention over whole sequences on the quantizers' integer codes (util_layernorm.FUSE_ATTENTION_INT:
    the block of set_fast_attention with both products exact on the bf16 matrix instruction, S up to 16384,
    csrc/attention_int.hip; needs per-tensor q / k / v / probabilities quantizers of at most 256 codes; tried before the
    fp32 form when both are on; default OFF -- tolerance-equal to the eager sequence, not bit-equal).
    OSQ_FAST_ATTENTION_INT=1 turns it on at load."""
    from . import util_layernorm
    util_layernorm.FUSE_ATTENTION_INT = bool(on)


def set_cache_codes(on=True):
    """New KV caches of incremental decoding hold integer codes, one byte per element, instead of fp32 words
    (util_layernorm.CACHE_CODES; model/quant_bart.py, QuantizedBartCache; default OFF).  What is read back from the cache,
    and what attention computes over it, are the same words.  OSQ_CACHE_CODES=1 turns it on at load.  Independent of
    set_fast_decode_attention."""
    from . import util_layernorm
    util_layernorm.CACHE_CODES = bool(on)


def set_graph_decode(on=True):
    """generate() captures a cached decoding step into a hipGraph and replays it instead of issuing its launches one by one
    (util_layernorm.GRAPH_DECODE; model/graph_decode.py; default OFF).  A captured step uses the one-launch attention
    whatever set_fast_decode_attention says; a step that cannot be captured is decoded as before.  OSQ_GRAPH_DECODE=1 turns
    it on at load; ``generate(..., graph=True)`` asks for one call."""
    from . import util_layernorm
    util_layernorm.GRAPH_DECODE = bool(on)


def set_beam_select(on=True):
    """generate()'s beam search selects a step's continuations with ops.beam_select -- log-softmax, the no-repeat-ngram and
    min-length bans, the running scores and the top-k in one kernel call (util_layernorm.BEAM_SELECT; csrc/beam_select.hip;
    default OFF) -- instead of the torch lines; a step it cannot take runs those.  OSQ_BEAM_SELECT=1 turns it on at load;
    ``generate(..., beam_select=True)`` asks for one call."""
    from . import util_layernorm
    util_layernorm.BEAM_SELECT = bool(on)


def set_beam_advance(on=True):
    """generate()'s beam search advances its beams with ops.beam_advance -- the finished continuations, the beams that go on,
    the merge into the finished set, the cache rows, the early-stop heuristic and the stopping word in one kernel call on two
    alternating sets of state buffers (util_layernorm.BEAM_ADVANCE; csrc/beam_advance.hip; default OFF) -- instead of the
    torch lines; a call it cannot take runs those.  OSQ_BEAM_ADVANCE=1 turns it on at load;
    ``generate(..., beam_advance=True)`` asks for one call."""
    from . import util_layernorm
    util_layernorm.BEAM_ADVANCE = bool(on)


def set_beam_graph(on=True):
    """generate()'s beam search captures a whole step -- the token copy, the model step, ops.beam_select_at,
    ops.beam_advance_at and the copy of the cache's row index -- into one hipGraph per direction of the alternating buffers
    and replays it: per token the host issues one replay and reads one word (util_layernorm.BEAM_GRAPH;
    model/graph_decode.py, BeamStepGraphs; default OFF).  For its call it implies set_graph_decode, set_beam_select and
    set_beam_advance; a call it cannot take -- one of those says why, one of them is passed as False, greedy decoding --
    decodes as without it (``model.last_beam_graph.reason``).  OSQ_BEAM_GRAPH=1 turns it on at load;
    ``generate(..., beam_graph=True)`` asks for one call."""
    from . import util_layernorm
    util_layernorm.BEAM_GRAPH = bool(on)


def set_greedy_advance(on=True):
    """generate()'s greedy decoding takes a step with ops.greedy_advance -- the banned tokens of the logits processors, the
    arg-max in torch.argmax's order, the pad / eos arithmetic, the new token into the sequence and the stopping word in one
    kernel call on one set of state buffers (util_layernorm.GREEDY_ADVANCE; csrc/greedy_advance.hip; default OFF) -- instead
    of the torch lines; a call it cannot take runs those (``model.last_greedy_advance.reason``).  OSQ_GREEDY_ADVANCE=1 turns
    it on at load; ``generate(..., greedy_advance=True)`` asks for one call."""
    from . import util_layernorm
    util_layernorm.GREEDY_ADVANCE = bool(on)


def set_greedy_graph(on=True):
    """generate()'s greedy decoding captures a whole step -- the token copy, the model step and ops.greedy_advance_at -- into
    one hipGraph and replays it, forced tokens included: per token the host issues one replay and reads one word
    (util_layernorm.GREEDY_GRAPH; model/graph_decode.py, GreedyStepGraph; default OFF).  For its call it implies
    set_graph_decode and set_greedy_advance; a call it cannot take -- one of those says why, one of them is passed as False,
    beam search -- decodes as without it (``model.last_greedy_graph.reason``).  OSQ_GREEDY_GRAPH=1 turns it on at load;
    ``generate(..., greedy_graph=True)`` asks for one call."""
    from . import util_layernorm
    util_layernorm.GREEDY_GRAPH = bool(on)


def set_sample_advance(on=True):
    """sample() takes a step with ops.sample_advance -- the banned tokens of the logits processors, temperature, top-k / top-p,
    the seeded draw, the pad / eos arithmetic, the new token into the sequence and the stopping word in one kernel call
    (util_layernorm.SAMPLE_ADVANCE; csrc/sample_advance.hip; default OFF) -- instead of the torch lines; a call it cannot
    take runs those (``model.last_sample_advance.reason``).  OSQ_SAMPLE_ADVANCE=1 turns it on at load;
    ``sample(..., sample_advance=True)`` asks for one call."""
    from . import util_layernorm
    util_layernorm.SAMPLE_ADVANCE = bool(on)


def set_sample_graph(on=True):
    """sample() captures a whole step -- the token copy, the model step and ops.sample_advance_at -- into one hipGraph and
    replays it (util_layernorm.SAMPLE_GRAPH; model/graph_decode.py, SampleStepGraph; default OFF).  For its call it implies
    set_graph_decode and set_sample_advance; a call it cannot take decodes as without it
    (``model.last_sample_graph.reason``).  OSQ_SAMPLE_GRAPH=1 turns it on at load; ``sample(..., sample_graph=True)`` asks
    for one call."""
    from . import util_layernorm
    util_layernorm.SAMPLE_GRAPH = bool(on)


def set_sample_nucleus(on=True):
    """Where sample() takes a step with one kernel call (set_sample_advance, set_sample_graph), a nucleus over the whole
    vocabulary -- ``top_k=0, top_p<1``, the form ops.sample_advance does not have -- goes to ops.sample_nucleus
    (util_layernorm.SAMPLE_NUCLEUS; csrc/sample_nucleus.hip; default OFF) instead of falling back to the torch lines with the
    reason "top_p below 1 without top_k".  OSQ_SAMPLE_NUCLEUS=1 turns it on at load; ``sample(..., sample_nucleus=True)``
    asks for one call."""
    from . import util_layernorm
    util_layernorm.SAMPLE_NUCLEUS = bool(on)


def sample_nucleus_from_environment(environ=None):
    """What OSQ_SAMPLE_NUCLEUS asks for: unset, empty or "0" -> False, anything else -> True."""
    return _env_on("OSQ_SAMPLE_NUCLEUS", environ)


def set_share_cross_kv(on=True):
    """Beam search holds the cross-attention keys / values once per batch row -- they are identical for the beams of a row --
    and a step's cross-attention serves all beams of a (row, head) from one pass over them (util_layernorm.SHARE_CROSS_KV;
    ops.decode_attention_shared, csrc/decode_attention.hip; default OFF): the cross part of the cache shrinks by the
    factor num_beams, the words computed are those of the one-launch attention on the repeated tensors.
    OSQ_SHARE_CROSS_KV=1 turns it on at load; ``generate(..., share_cross_kv=True)`` asks for one call;
    ``model.last_share_cross_kv`` tells what happened.  ``score(..., num_candidates=n)`` follows the switch as well: the
    candidates of an input share one copy of its cross-attention keys / values in the teacher-forced pass."""
    from . import util_layernorm
    util_layernorm.SHARE_CROSS_KV = bool(on)


def set_fast_lm_loss(on=True):
    """``forward(labels=...)`` of QuantizedBartForConditionalGeneration computes its loss through the scoring kernels --
    ops.lm_loss: every logit read once, no tensor of the logits' size written, the backward one streaming launch from the
    rows' log-sum-exp (util_layernorm.FAST_LM_LOSS; csrc/token_logprob.hip; model/losses.py, FusedLmLoss; default OFF) --
    instead of F.cross_entropy, with autograd on or off; a call the kernels do not take runs F.cross_entropy
    (``model.last_lm_loss``: fused, eager, reason).  Tolerance-equal, not bit-equal.  OSQ_FAST_LM_LOSS=1 turns it on at
    load.  ``model.score()`` uses the kernels on the GPU whatever this says."""
    from . import util_layernorm
    util_layernorm.FAST_LM_LOSS = bool(on)


def fast_lm_loss_from_environment(environ=None):
    """What OSQ_FAST_LM_LOSS asks for: unset, empty or "0" -> False, anything else -> True."""
    return _env_on("OSQ_FAST_LM_LOSS", environ)


def share_cross_kv_from_environment(environ=None):
    """What OSQ_SHARE_CROSS_KV asks for: unset, empty or "0" -> False, anything else -> True."""
    return _env_on("OSQ_SHARE_CROSS_KV", environ)


def sample_advance_from_environment(environ=None):
    """What OSQ_SAMPLE_ADVANCE asks for: unset, empty or "0" -> False, anything else -> True."""
    return _env_on("OSQ_SAMPLE_ADVANCE", environ)


def sample_graph_from_environment(environ=None):
    """What OSQ_SAMPLE_GRAPH asks for: unset, empty or "0" -> False, anything else -> True."""
    return _env_on("OSQ_SAMPLE_GRAPH", environ)


def greedy_advance_from_environment(environ=None):
    """What OSQ_GREEDY_ADVANCE asks for: unset, empty or "0" -> False, anything else -> True."""
    return _env_on("OSQ_GREEDY_ADVANCE", environ)


def greedy_graph_from_environment(environ=None):
    """What OSQ_GREEDY_GRAPH asks for: unset, empty or "0" -> False, anything else -> True."""
    return _env_on("OSQ_GREEDY_GRAPH", environ)


def beam_graph_from_environment(environ=None):
    """What OSQ_BEAM_GRAPH asks for: unset, empty or "0" -> False, anything else -> True."""
    return _env_on("OSQ_BEAM_GRAPH", environ)


def beam_advance_from_environment(environ=None):
    """What OSQ_BEAM_ADVANCE asks for: unset, empty or "0" -> False, anything else -> True."""
    return _env_on("OSQ_BEAM_ADVANCE", environ)


def beam_select_from_environment(environ=None):
    """What OSQ_BEAM_SELECT asks for: unset, empty or "0" -> False, anything else -> True."""
    return _env_on("OSQ_BEAM_SELECT", environ)


def graph_decode_from_environment(environ=None):
    """What OSQ_GRAPH_DECODE asks for: unset, empty or "0" -> False, anything else -> True."""
    return _env_on("OSQ_GRAPH_DECODE", environ)


def cache_codes_from_environment(environ=None):
    """What OSQ_CACHE_CODES asks for: unset, empty or "0" -> False, anything else -> True."""
    return _env_on("OSQ_CACHE_CODES", environ)


def reset_tier(_lib=None):
    """The package's default tier, as the environment states it (applied when the library is first loaded): MSEFast sums in
    the reference's one-thread order, the backward's sums order-free; OSQ_STRICT=1 / 0 force both; OSQ_FAST=0 / 1 the
    one-launch LayerNorm site; OSQ_FAST_SOFTMAX=1 the one-launch attention-probabilities site and OSQ_FAST_DECODE_ATTENTION=1
    the one-launch attention of a cached decoding step (unset: off); OSQ_FAST_ATTENTION=1 the one-launch attention over whole
    sequences and OSQ_FAST_ATTENTION_INT=1 its form on integer codes (unset: off); OSQ_CACHE_CODES=1 KV caches as integer codes (unset: off);
    OSQ_GRAPH_DECODE=1 generate() replays a captured decoding step (unset: off); OSQ_BEAM_SELECT=1 beam search selects a step's
    continuations with one kernel call (unset: off); OSQ_BEAM_ADVANCE=1 beam search advances its beams with one kernel call
    (unset: off); OSQ_BEAM_GRAPH=1 beam search replays a whole step, bookkeeping included, as one captured graph (unset: off);
    OSQ_GREEDY_ADVANCE=1 greedy decoding takes a step with one kernel call (unset: off); OSQ_GREEDY_GRAPH=1 greedy decoding
    replays a whole step as one captured graph (unset: off); OSQ_SAMPLE_ADVANCE=1 sample() takes a step with one kernel call
    (unset: off); OSQ_SAMPLE_GRAPH=1 sample() replays a whole step as one captured graph (unset: off); OSQ_SAMPLE_NUCLEUS=1
    that kernel call takes a nucleus over the whole vocabulary too (unset: off); OSQ_SHARE_CROSS_KV=1 beam search holds the
    cross-attention keys / values once per batch row (unset: off); OSQ_FAST_LM_LOSS=1 the BART LM wrapper's loss through the
    scoring kernels (unset: off)."""
    import os
    width = int(os.environ.get("OSQ_STRICT_SIMD", "8"))
    strict = os.environ.get("OSQ_STRICT", "")
    if strict == "":
        set_strict(True, width, backward=False, _lib=_lib)
    else:
        set_strict(strict != "0", width, _lib=_lib)
    # unset: the default (one-launch LayerNorm site ON) -- a set_fast(False) of an earlier caller or test does not leak
    set_fast(os.environ.get("OSQ_FAST", "") != "0")
    set_fast_softmax(_env_on("OSQ_FAST_SOFTMAX"))
    set_fast_decode_attention(_env_on("OSQ_FAST_DECODE_ATTENTION"))
    set_fast_attention(_env_on("OSQ_FAST_ATTENTION"))
    for setter, name in _SWITCHES:
        setter(_env_on(name))


# the switches reset_tier sets to what their environment variable says, off when it is unset
_SWITCHES = ((set_cache_codes, "OSQ_CACHE_CODES"), (set_graph_decode, "OSQ_GRAPH_DECODE"), (set_beam_select, "OSQ_BEAM_SELECT"),
             (set_beam_advance, "OSQ_BEAM_ADVANCE"), (set_beam_graph, "OSQ_BEAM_GRAPH"), (set_greedy_advance, "OSQ_GREEDY_ADVANCE"),
             (set_greedy_graph, "OSQ_GREEDY_GRAPH"), (set_sample_advance, "OSQ_SAMPLE_ADVANCE"),
             (set_sample_graph, "OSQ_SAMPLE_GRAPH"), (set_sample_nucleus, "OSQ_SAMPLE_NUCLEUS"),
             (set_share_cross_kv, "OSQ_SHARE_CROSS_KV"), (set_fast_lm_loss, "OSQ_FAST_LM_LOSS"),
             (set_fast_attention_int, "OSQ_FAST_ATTENTION_INT"))
_apply_environment = reset_tier


def __getattr__(name):
    """export_codes / load_codes (export.py), imported on first use: importing the package itself stays free of torch."""
    if name in ("export_codes", "load_codes"):
        from . import export
        return getattr(export, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")

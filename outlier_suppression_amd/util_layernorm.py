"""LayerNorm wrappers used by Gamma Migration, with the reference's class names.

Reference: quant_transformer/model/util_layernorm.py.  Under autograd the normalisation stays stock
PyTorch-ROCm followed by the HIP quantizer (the eager sequence of the reference).  Four fusions exist for forwards without
autograd (every calibration / evaluation forward):


  * ``FUSE_ACTIVATION`` (default ON): dense -> GELU -> fake-quant as ONE launch -- bit-identical to the two-step form;
  * ``FUSE_QKV`` (default ON): the query / key / value head-split sites of a self-attention block as ONE launch --
    bit-identical to the three calls;
  * ``FUSE_LAYERNORM`` (default ON since round 5): a LayerNorm site -- residual (GammaResidual), normalisation, affine pair
    or beta/gamma shift, output fake-quant -- as ONE launch (``ops.residual_layernorm_fake_quant``: 52 us
    instead of 168 us on [256,128,768], 14-19 against 25-38 us at [32,128,768]).  Its row moments are two-pass sums in a
    wave, torch-ROCm's LayerNorm kernel is Welford: against float64 both carry an error proportional to the row's
    condition number kappa = 1 + |mean|/sigma (2-3e-7 x kappa of the output's magnitude, as torch's CPU kernel does:
    tests/test_gpu_site_accuracy.py, profiles/site_accuracy.txt), and NEITHER is bit-comparable with the
    reference's CPU LayerNorm.  Against the reference's own run at BERT-base width (tests/golden/ln_site.npz,
    tests/test_gpu_ln_site.py, profiles/r05_ln_site_parity.txt) the one-launch site is no further away than the eager
    one: max |LayerNorm output - reference| 2.3e-5 / 5.7e-6 / 3.1e-5 against 2.3e-5 / 5.7e-6 / 2.3e-5 on values up to
    136 (2e-7 relative; BASELINE.json's bar is 1e-5), and 0 / 0 / 0 integer entries of 3.1 M different from the
    reference's integer tensor against 0 / 1 / 0.  ``outlier_suppression_amd.set_fast(False)`` / ``OSQ_FAST=0`` /
    ``util_layernorm.FUSE_LAYERNORM = False`` keep the eager sequence.
  * ``FUSE_SOFTMAX`` (default OFF): the attention-probabilities site -- pre-softmax scaling + additive mask, softmax,
    fake-quant (quant_bert.py:169-185, quant_bart.py:232-256) -- as ONE launch (``ops.attention_softmax_fake_quant``,
    csrc/attention.hip: 8 B per element instead of about 28 on the largest activation of the block).  Its exp is ocml's
    expf, not the Sleef routine of the reference's CPU softmax: probabilities agree with the reference to a tolerance,
    not bit for bit (tests/golden/attention_site.npz, tests/test_gpu_attention_site.py).  In the plain quantising state
    the whole site is one launch; with the observer on, the quantizer disabled or per-channel, one launch computes the
    probabilities and the quantizer then runs its own path.  Autograd passes and active dropout keep the eager sequence.
    ``outlier_suppression_amd.set_fast_softmax(True)`` / ``OSQ_FAST_SOFTMAX=1`` turn it on.  Measured on MI355X
    (profiles/attention_site_ab.txt): [32,12,384,384] 116 us against 220 us eager with fake-quant, 81 against 153 us
    softmax only; [32,12,128,128] 26 against 32 us, and slower than eager softmax only (23 against 22 us).

Incremental decoding has a fifth, ``FUSE_DECODE_ATTENTION`` (default OFF): everything a cached decoding step's attention
block runs after its q / k / v + append launch -- bmm, mask add, softmax, probabilities quantizer, bmm, merge heads, context
quantizer (quant_bart.py:232-268) -- as ONE launch for the step's single query token (``ops.decode_attention_fake_quant``,
csrc/decode_attention.hip).  Its dot products are fp32 sums in the kernel's own fixed order, not rocBLAS's, and its exp is
ocml's: the result is tolerance-equal to the eager sequence, not bit-equal, hence off by default.
``outlier_suppression_amd.set_fast_decode_attention(True)`` / ``OSQ_FAST_DECODE_ATTENTION=1`` turn it on.

``FUSE_ATTENTION`` (default OFF) is its counterpart for more than one query token: BERT and RoBERTa as a whole, BART's encoder,
the teacher-forced decoder and a multi-token prefill.  Everything between the q / k / v sites and the output projection -- bmm,
scaling, mask add, softmax, probabilities quantizer, bmm, merge heads, context quantizer -- is ONE launch that keeps a tile of
32 score rows in LDS and never writes the [B, h, T, S] scores (``ops.attention_fake_quant``, csrc/attention_block.hip; both
products on the fp32-input matrix instruction).  Tolerance-equal to the eager sequence for the same reasons, hence off by
default; head sizes 16 / 32 / 64 / 128 and S <= 1024, anything else keeps the eager sequence (or FUSE_SOFTMAX), as do autograd
passes, active dropout and observer passes.  Measured on MI355X (profiles/attention_block_ab.txt), the block alone: 1.40x the
eager sequence at [32,12,128,128,64] and 1.22x at [192,16,62,62,64], but 0.84x / 0.79x / 0.72x at 384 / 512 / 512 keys, where
FUSE_SOFTMAX is the faster switch.  ``outlier_suppression_amd.set_fast_attention(True)`` / ``OSQ_FAST_ATTENTION=1`` turn it on.

``FUSE_ATTENTION_INT`` (default OFF) is the same block on the INTEGER CODES of its q / k / v / probabilities quantizers
(``ops.attention_int_fake_quant``, csrc/attention_int.hip): every operand of both products is ``s * n`` with an integer
|n| <= 255, so both run exactly on the bf16 matrix instruction, the scales are applied once to the exact sums, nothing of
S's size is kept on chip and S may reach 16384.  Tolerance-equal to the eager sequence (and closer to float64 than it), hence
off by default; it needs all four quantizers per-tensor with at most 256 codes, and is tried before FUSE_ATTENTION when both
are on.  ``outlier_suppression_amd.set_fast_attention_int(True)`` / ``OSQ_FAST_ATTENTION_INT=1`` turn it on; the measured
outcome per shape is in profiles/attention_int_ab.txt and README.

``CACHE_CODES`` (default OFF) is no fusion but a storage format: new KV caches (model/quant_bart.py, QuantizedBartCache) hold
integer codes, one byte per element, written by ``ops.fake_quant_kv_append_codes`` and read as they are by
``ops.decode_attention_codes`` (csrc/kv_codes.hip, csrc/decode_attention.hip); the words computed are those of the fp32 cache.
``outlier_suppression_amd.set_cache_codes(True)`` / ``OSQ_CACHE_CODES=1`` turn it on; it is independent of the switch above.

``GRAPH_DECODE`` (default OFF) is neither: ``generate()`` captures a cached decoding step into a hipGraph and replays it
(model/graph_decode.py).  The step's position then comes from a device word: the append and the self-attention take the
position-from-device launches (``ops.fake_quant_kv_append_at`` / ``_codes_at``, ``ops.decode_attention_at``), which write and
compute the words of the static launches at that position.  A captured step always uses the one-launch attention.
``outlier_suppression_amd.set_graph_decode(True)`` / ``OSQ_GRAPH_DECODE=1`` / ``generate(..., graph=True)`` turn it on.

``BEAM_SELECT`` (default OFF) is tolerance-equal as well: beam search hands a step's log-softmax, banned tokens, score add and
top-k to ``ops.beam_select`` (csrc/beam_select.hip) instead of the torch lines, on every step whose logits processors are the
no-repeat-ngram and min-length ones; ties come out in a strict index order where torch.topk has none.
``outlier_suppression_amd.set_beam_select(True)`` / ``OSQ_BEAM_SELECT=1`` / ``generate(..., beam_select=True)`` turn it on.

``BEAM_ADVANCE`` (default OFF): beam search hands the bookkeeping after the selection -- which continuations finished, the
beams that go on, the merge into the finished set, the cache rows, the early-stop heuristic and the stopping word -- to
``ops.beam_advance`` (csrc/beam_advance.hip) instead of about forty torch launches; the state then lives in two alternating
sets of device buffers.  Word-equal to the torch lines where those have no ties; ties come out in the strict index order.
``outlier_suppression_amd.set_beam_advance(True)`` / ``OSQ_BEAM_ADVANCE=1`` / ``generate(..., beam_advance=True)`` turn it on.

``BEAM_GRAPH`` (default OFF): beam search captures a WHOLE step -- the token copy, the model step, the selection
(``ops.beam_select_at``), the bookkeeping (``ops.beam_advance_at``) and the copy of the cache's row index -- into one graph per
direction of the alternating buffers and replays it (model/graph_decode.py, BeamStepGraphs); a token then costs the host one
replay and one read of the stopping word.  For its call it implies the three switches above; the words are theirs.
``outlier_suppression_amd.set_beam_graph(True)`` / ``OSQ_BEAM_GRAPH=1`` / ``generate(..., beam_graph=True)`` turn it on.

``GREEDY_ADVANCE`` (default OFF): greedy decoding hands everything after the model step -- the banned tokens of the logits
processors, the arg-max, the pad / eos arithmetic, the new token into the sequence and the stopping word -- to
``ops.greedy_advance`` (csrc/greedy_advance.hip) instead of the torch lines; the state then lives in one set of device buffers.
Token-for-token equal to the torch lines: the kernel's order is torch.argmax's (first maximum, NaN above every number).
``outlier_suppression_amd.set_greedy_advance(True)`` / ``OSQ_GREEDY_ADVANCE=1`` / ``generate(..., greedy_advance=True)`` turn
it on.

``GREEDY_GRAPH`` (default OFF): greedy decoding captures a WHOLE step -- the token copy, the model step and
``ops.greedy_advance_at`` on the graph's own logits -- into one graph and replays it (model/graph_decode.py, GreedyStepGraph),
forced tokens included; a token then costs the host one replay and one read of the stopping word.  For its call it implies
``GRAPH_DECODE`` and ``GREEDY_ADVANCE``.
``outlier_suppression_amd.set_greedy_graph(True)`` / ``OSQ_GREEDY_GRAPH=1`` / ``generate(..., greedy_graph=True)`` turn it on.

``SAMPLE_ADVANCE`` (default OFF): sample() hands everything after the model step -- the banned tokens, temperature, top-k /
top-p, the seeded draw, the pad / eos arithmetic, the new token into the sequence and the stopping word -- to
``ops.sample_advance`` (csrc/sample_advance.hip) instead of the torch lines (model/sampling.py).  The same rule and the same
uniforms; the sums are fp32 in another order, so a draw within rounding of a boundary may select the neighbouring token.
``outlier_suppression_amd.set_sample_advance(True)`` / ``OSQ_SAMPLE_ADVANCE=1`` / ``sample(..., sample_advance=True)`` turn it on.

``SAMPLE_GRAPH`` (default OFF): sample() captures a WHOLE step -- the token copy, the model step and ``ops.sample_advance_at``
-- into one graph and replays it (model/graph_decode.py, SampleStepGraph); the generator is keyed by (seed, row, position), so
one graph serves every step.  For its call it implies ``GRAPH_DECODE`` and ``SAMPLE_ADVANCE``.
``outlier_suppression_amd.set_sample_graph(True)`` / ``OSQ_SAMPLE_GRAPH=1`` / ``sample(..., sample_graph=True)`` turn it on.

``SAMPLE_NUCLEUS`` (default OFF): under the two switches above, ``top_k=0, top_p<1`` -- a nucleus over the whole vocabulary,
which ``ops.sample_advance`` refuses -- goes to ``ops.sample_nucleus`` (csrc/sample_nucleus.hip: the row in registers, two
bisections over a fixed-order sum, no sort) instead of falling back to the torch lines.  The same rule and uniforms, fp32 sums
in another order.  Off, every path and every fallback reason is unchanged.
``outlier_suppression_amd.set_sample_nucleus(True)`` / ``OSQ_SAMPLE_NUCLEUS=1`` / ``sample(..., sample_nucleus=True)`` turn it on.

Beam search has ``SHARE_CROSS_KV`` (default OFF): the cross-attention keys / values, identical for the beams of a batch row,
are projected, quantized and held once per batch row (``QuantizedBartCache(cross_group=num_beams)``), and a step's
cross-attention is ONE launch in which a workgroup serves the beams of a (row, head) from a single pass over K and V
(``ops.decode_attention_shared``, csrc/decode_attention.hip): the words of the one-launch attention on the repeated
tensors.  ``outlier_suppression_amd.set_share_cross_kv(True)`` / ``OSQ_SHARE_CROSS_KV=1`` / ``generate(..., share_cross_kv=True)``
turn it on.  ``score(..., num_candidates=n)`` follows the same switch (``score(..., share_cross_kv=True)``): the candidates of an
input attend to ONE copy of its keys / values, projected and quantized once per decoder layer, through the whole-sequence
launches with ``group=n`` (``ops.attention_fake_quant`` / ``ops.attention_int_fake_quant``; the row map of csrc/attention_seq.h).
"""
import torch
import torch.nn.functional as F
from torch import nn

from . import ops
from .quantization import QuantizedModule, Quantizer
from .quantization.fake_quant import _LearnableFakeQuantize

FUSE_LAYERNORM = True
FUSE_ACTIVATION = True
FUSE_QKV = True          # the query / key / value head-split sites of a self-attention block as one launch (bit-identical)
FUSE_SOFTMAX = False     # the attention-probabilities site as one launch (tolerance-equal; set_fast_softmax / OSQ_FAST_SOFTMAX=1)
FUSE_DECODE_ATTENTION = False   # a cached decoding step's attention after the append as one launch (tolerance-equal; set_fast_decode_attention / OSQ_FAST_DECODE_ATTENTION=1)
FUSE_ATTENTION = False   # an attention block over a whole sequence as one launch (tolerance-equal; set_fast_attention / OSQ_FAST_ATTENTION=1)
FUSE_ATTENTION_INT = False   # an attention block over a whole sequence as one launch on the quantizers' integer codes, exact products on the bf16 matrix instruction, tried before FUSE_ATTENTION (tolerance-equal to eager; set_fast_attention_int / OSQ_FAST_ATTENTION_INT=1)
FUSE_KV_APPEND = True    # incremental decoding: a step's q / k / v sites + KV-cache append (+ beam reorder) as one launch (bit-identical)
GRAPH_DECODE = False     # generate(): capture a cached decoding step into a graph and replay it (set_graph_decode / OSQ_GRAPH_DECODE=1 / generate(graph=True))
BEAM_SELECT = False      # generate(): a beam step's log-softmax + processors + score add + top-k as one kernel call (tolerance-equal; set_beam_select / OSQ_BEAM_SELECT=1 / generate(beam_select=True))
BEAM_ADVANCE = False     # generate(): a beam step's bookkeeping after the selection as one kernel call on alternating state buffers (set_beam_advance / OSQ_BEAM_ADVANCE=1 / generate(beam_advance=True))
BEAM_GRAPH = False       # generate(): capture a whole beam-search step -- model, selection, bookkeeping, cache row index -- into one graph (implies the three above for the call; set_beam_graph / OSQ_BEAM_GRAPH=1 / generate(beam_graph=True))
GREEDY_ADVANCE = False   # generate(): a greedy step's processors, arg-max, pad / eos lines, sequence append and stopping word as one kernel call (set_greedy_advance / OSQ_GREEDY_ADVANCE=1 / generate(greedy_advance=True))
GREEDY_GRAPH = False     # generate(): capture a whole greedy step -- token copy, model, the kernel call above -- into one graph (implies GRAPH_DECODE and GREEDY_ADVANCE for the call; set_greedy_graph / OSQ_GREEDY_GRAPH=1 / generate(greedy_graph=True))
SAMPLE_ADVANCE = False   # sample(): a sampling step's processors, temperature / top-k / top-p, seeded draw, pad / eos lines, sequence append and stopping word as one kernel call (set_sample_advance / OSQ_SAMPLE_ADVANCE=1 / sample(sample_advance=True))
SAMPLE_GRAPH = False     # sample(): capture a whole sampling step -- token copy, model, the kernel call above -- into one graph (implies GRAPH_DECODE and SAMPLE_ADVANCE for the call; set_sample_graph / OSQ_SAMPLE_GRAPH=1 / sample(sample_graph=True))
SAMPLE_NUCLEUS = False   # sample(): under the two switches above, top_k=0 with top_p<1 (a nucleus over the whole vocabulary) goes to ops.sample_nucleus instead of the torch lines (set_sample_nucleus / OSQ_SAMPLE_NUCLEUS=1 / sample(sample_nucleus=True))
SHARE_CROSS_KV = False   # generate(): beam search holds the cross-attention keys / values once per batch row and attends to them from every beam of the row in one launch (set_share_cross_kv / OSQ_SHARE_CROSS_KV=1 / generate(share_cross_kv=True))
FAST_LM_LOSS = False     # forward(labels=...) of the BART LM wrapper: the loss through the scoring kernels -- ops.lm_loss, backward from lse alone -- instead of F.cross_entropy (tolerance-equal; set_fast_lm_loss / OSQ_FAST_LM_LOSS=1); score() uses the kernels whatever this says
CACHE_CODES = False      # incremental decoding: new KV caches hold integer codes, one byte per element (same words read back; set_cache_codes / OSQ_CACHE_CODES=1)


class _Numel:
    """Stands for a tensor of which a quantizer's grad factor needs the element count only."""

    def __init__(self, n):
        self.n = n

    def numel(self):
        return self.n


def _site_record(q, numel):
    """The launch record of quantizer ``q`` at a one-launch site, (scale, zero_point, quant_min, quant_max, mode, grad_factor)
    as the ops functions take it -- the one statement of it; whether the site is fusable is each caller's own condition (a
    per-tensor quantizer that only fake-quantises, in every one).  ``numel``: the elements of the tensor the quantizer would
    see, which a learnable quantizer's grad factor goes by.  With the observer off a learnable quantizer's parameter repair
    (fake_quant.py:188-191) rides in the launch under PARAM_SANITIZE: a kernel may then write scale / zero_point, so the
    quantizer is told (_touch_qparams).  For the activation quantizers of these sites nobody observes that: _qparam_epoch is
    read by quantization/weight_cache.py alone, for weight quantizers."""
    mode = q.param_mode
    if isinstance(q, _LearnableFakeQuantize):
        mode |= ops.PARAM_SANITIZE
        q._touch_qparams()
    return (q.scale.data, q.zero_point.data, q.quant_min, q.quant_max, mode,
            q._grad_factor(_Numel(numel)) if q.param_mode != ops.PARAM_FIXED else 1.0)


def _fused_site(mod, x, hidden, gamma, weight, bias, eps, observation_mask):
    """One launch for residual + LayerNorm (+ fake-quant when the site's quantizer is in its plain quantising state)."""
    q = mod.layernorm_post_act_fake_quantize if mod.qoutput else None
    quant = None
    if q is not None and q.fake_quant_enabled == 1 and q.observer_enabled != 1 and q.ch_axis == -1 and q.scale.is_cuda:
        quant = _site_record(q, x.numel())
    y = ops.residual_layernorm_fake_quant(x, hidden, gamma, weight, bias, eps, quant)
    if q is not None and quant is None:           # observing, disabled, or per-channel: the quantizer's own path
        y = q(y, observation_mask, 1)
    return y


def _can_fuse(x, *operands):
    return (FUSE_LAYERNORM and not torch.is_grad_enabled() and x.dim() >= 2 and ops.layernorm_fusable(x, *operands))


def residual_layernorm(residual, layernorm, shortcut, hidden_states, observation_mask=None):
    """``layernorm(residual(shortcut, hidden_states), observation_mask)`` -- the pair every transformer block ends
    its two halves with (quant_bert.py:211-216, 298-303; quant_bart.py:342-353) -- as one launch when possible."""
    gamma = residual.gamma.data if residual.mul_gamma else None
    if shortcut.shape == hidden_states.shape and _can_fuse(shortcut, hidden_states, gamma):
        return layernorm.forward_fused(shortcut, hidden_states, gamma, observation_mask)
    return layernorm(residual(shortcut, hidden_states), observation_mask)


class QuantizedLayerNorm(QuantizedModule):
    """util_layernorm.py:6-18: LayerNorm followed by an activation quantizer (seq axis 1)."""

    def __init__(self, org_module, w_qconfig, a_qconfig, qoutput=True, backend="academic"):
        super().__init__(backend=backend)
        self.qoutput = qoutput
        self.layernorm = org_module
        if qoutput:
            self.layernorm_post_act_fake_quantize = Quantizer(None, a_qconfig)

    def forward_fused(self, x, hidden, gamma, observation_mask=None):
        ln = self.layernorm
        if len(ln.normalized_shape) != 1 or not ops.layernorm_fusable(x, ln.weight, ln.bias):
            if hidden is not None:
                x = ops.gamma_residual(x, hidden, gamma)
            return self.forward(x, observation_mask, _fused=False)
        return _fused_site(self, x, hidden, gamma, None if ln.weight is None else ln.weight.data,
                           None if ln.bias is None else ln.bias.data, ln.eps, observation_mask)

    def forward(self, hidden_states, observation_mask=None, _fused=True):
        if _fused and isinstance(self.layernorm, nn.LayerNorm) and _can_fuse(hidden_states):
            return self.forward_fused(hidden_states, None, None, observation_mask)
        hidden_states = self.layernorm(hidden_states)
        if self.qoutput:
            hidden_states = self.layernorm_post_act_fake_quantize(hidden_states, observation_mask, 1)
        return hidden_states


class QuantizedSplitLayerNorm(QuantizedModule):
    """util_layernorm.py:21-37: the non-scaling LayerNorm  X' = (x - mu)/sigma + beta/gamma.

    Two reference quirks are kept on purpose: the inner LayerNorm is built
    with PyTorch's default eps = 1e-5 (not the model's), and the output quantizer is a NEW one.
    """

    def __init__(self, org_module, w_qconfig, a_qconfig, qoutput=True, backend="academic"):
        super().__init__(backend=backend)
        self.qoutput = qoutput
        self.layernorm = nn.LayerNorm(org_module.normalized_shape, elementwise_affine=False)
        beta, gamma = org_module.bias.data.detach(), org_module.weight.data.detach()
        if beta.is_cuda:
            shifted = ops.gamma_split_bias(beta, gamma)
        else:
            raise RuntimeError("QuantizedSplitLayerNorm: LayerNorm parameters must be on a HIP device "
                               "(gamma migration runs after model.cuda(), ptq_glue_quant.py:212-232)")
        self.bias = nn.Parameter(shifted)
        if qoutput:
            self.layernorm_post_act_fake_quantize = Quantizer(None, a_qconfig)

    def forward_fused(self, x, hidden, gamma, observation_mask=None):
        if len(self.layernorm.normalized_shape) != 1 or not ops.layernorm_fusable(x, self.bias):
            if hidden is not None:
                x = ops.gamma_residual(x, hidden, gamma)
            return self.forward(x, observation_mask, _fused=False)
        return _fused_site(self, x, hidden, gamma, None, self.bias.data, self.layernorm.eps, observation_mask)

    def forward(self, hidden_states, observation_mask=None, _fused=True):
        if _fused and _can_fuse(hidden_states):
            return self.forward_fused(hidden_states, None, None, observation_mask)
        hidden_states = F.layer_norm(hidden_states, self.layernorm.normalized_shape, None, None, self.layernorm.eps)
        hidden_states += self.bias
        if self.qoutput:
            hidden_states = self.layernorm_post_act_fake_quantize(hidden_states, observation_mask, 1)
        return hidden_states


class GammaResidual(nn.Module):
    """util_layernorm.py:40-52: shortcut that re-applies gamma after migration: input*gamma + hidden."""

    def __init__(self):
        super().__init__()
        self.mul_gamma = False

    def set_gamma(self, gamma):
        self.mul_gamma = True
        self.gamma = nn.Parameter(gamma.data.detach().clone())

    def forward(self, input, hidden_states):
        needs_graph = torch.is_grad_enabled() and (input.requires_grad or hidden_states.requires_grad or
                                                   (self.mul_gamma and self.gamma.requires_grad))
        if (not needs_graph and input.is_cuda and input.dtype == torch.float32 and input.shape == hidden_states.shape):
            return ops.gamma_residual(input, hidden_states, self.gamma.data if self.mul_gamma else None)
        if self.mul_gamma:
            input = input * self.gamma
        return input + hidden_states


def activation_fake_quant(act_fn, quantizer, hidden_states, observation_mask=None):
    """``quantizer(act_fn(hidden_states), observation_mask, 1)`` -- the intermediate-activation site
    (quant_bert.py:277-280, quant_bart.py:347-348).  With autograd off, an exact GELU and the quantizer in its plain
    quantising state this is ONE launch (``ops.gelu_fake_quant_per_tensor``: bit-identical to the two-step form,
    half the traffic on the largest activation of the block); otherwise the two steps."""
    q = quantizer
    if (FUSE_ACTIVATION and q is not None and not torch.is_grad_enabled() and q.fake_quant_enabled == 1
            and q.observer_enabled != 1 and q.ch_axis == -1 and hidden_states.is_cuda and hidden_states.dtype == torch.float32
            and hidden_states.is_contiguous() and hidden_states.numel() and hidden_states.data_ptr() % 16 == 0
            and q.scale.is_cuda and ops.is_exact_gelu(act_fn)):
        return ops.gelu_fake_quant_per_tensor(hidden_states, *_site_record(q, hidden_states.numel()))
    hidden_states = act_fn(hidden_states)
    if q is not None:
        hidden_states = q(hidden_states, observation_mask, 1)
    return hidden_states


def _not_plain(q):
    """Why quantizer ``q`` is not in its plain quantising state -- one phrase -- or None when it is: it only fake-quantises
    (observer off) and is per-tensor.  The one statement of that state: _plain_quantizing and the reasons of
    attention_int_refusal both read it."""
    if q is None:
        return "is missing"
    if q.ch_axis != -1:
        return "is per-channel"
    if q.fake_quant_enabled != 1 or q.observer_enabled == 1:
        return "is observing or disabled"
    return None


def _plain_quantizing(q, x):
    """The quantizer only fake-quantises (observer off), per tensor, on the device, and nobody wants a gradient: its
    result depends on the VALUES of x alone, so x may be handed over as any view of its memory."""
    return (_not_plain(q) is None and not torch.is_grad_enabled() and x.is_cuda and x.dtype == torch.float32
            and bool(x.numel()) and q.scale.is_cuda)


def merge_heads_fake_quant(quantizer, ctx, observation_mask=None):
    """``quantizer(ctx.permute(0, 2, 1, 3).contiguous().view(B, T, h*d), observation_mask, 1)`` for ctx [B,h,T,d] -- the
    context site (quant_bert.py:184-188, quant_bart.py:262-268).  In the plain quantising state the permuted VIEW goes to
    the strided fake-quant kernel, which writes the merged layout itself: one pass instead of copy + fake-quant, same bits."""
    b, h, t, d = ctx.shape
    if _plain_quantizing(quantizer, ctx) and ctx.is_contiguous() and d % 4 == 0:
        y = quantizer(ctx.permute(0, 2, 1, 3))
        if y.is_contiguous():
            return y.view(b, t, h * d)
    ctx = ctx.permute(0, 2, 1, 3).contiguous().view(b, t, h * d)
    if quantizer is not None:
        ctx = quantizer(ctx, observation_mask, 1)
    return ctx


def split_heads_fake_quant(quantizer, x, heads, observation_mask=None):
    """``quantizer(x, observation_mask, 1).view(B, T, h, d).transpose(1, 2).contiguous()`` for x [B,T,h*d]
    (quant_bart.py:226-243): in the plain quantising state the head-split view is quantised straight into the
    [B,h,T,d] layout (one pass, same bits)."""
    b, t, width = x.shape
    d = width // heads
    if _plain_quantizing(quantizer, x) and x.is_contiguous() and d % 4 == 0:
        y = quantizer(x.view(b, t, heads, d).transpose(1, 2))
        if y.is_contiguous():
            return y
    if quantizer is not None:
        x = quantizer(x, observation_mask, 1)
    return x.view(b, t, heads, d).transpose(1, 2).contiguous()



def qkv_heads_fake_quant(quantizers, projections, heads):
    """The three activation quantizers behind the query / key / value projections of a self-attention block
    (quant_bert.py:148-155: ``q = Q_q(heads(query(x)), mask, 2)``, ``k^T = Q_k(heads(key(x)).transpose(-1, -2), mask, 3)``,
    ``v = Q_v(heads(value(x)), mask, 2)``) as ONE launch when all three only fake-quantise (observers off, per tensor, no
    gradient wanted) and the projections are contiguous [B, T, h*d] tensors of one shape.  Returns [q, k, v] as dense
    [B, h, T, d] tensors (the caller transposes k), or None: the caller then runs the three sites one by one.  A site's
    result depends on its own tensor and parameters only, so the order of the three calls does not matter; every site's
    LSQ / LSQ+ parameter repair (fake_quant.py:188-191) rides in the launch as it does in the per-site form."""
    if not FUSE_QKV:
        return None
    x0 = projections[0]
    if x0.dim() != 3 or x0.shape[-1] % heads or (x0.shape[-1] // heads) % 4:
        return None
    params = []
    for q, x in zip(quantizers, projections):
        if not (_plain_quantizing(q, x) and x.is_contiguous() and x.shape == x0.shape and x.data_ptr() % 16 == 0):
            return None
        params.append(_site_record(q, x.numel()))
    return ops.fake_quant_headsplit_multi(list(projections), params, heads)


def kv_append_fake_quant(sites, heads, pos=None, numels=None):
    """Incremental decoding (model/quant_bart.py, QuantizedBartCache): the activation quantizers of one attention block's
    step, each site ``(quantizer, x, y, offset, src, src_rows)``, as ONE launch (ops.fake_quant_kv_append): site i writes
    the head-split fake-quant of its [B, t, h*d] projection x at positions [offset, offset + t) of the [B, h, cap, d]
    buffer y, after copying ``src.index_select(0, src_rows)[:, :, :offset]`` (or ``src[:, :, :offset]``) in front of it.
    The cache contents are word for word what ``torch.cat([past.index_select(0, idx), split_heads(quantizer(x))], 2)``
    gives.  Only when every quantizer is in its plain quantising state (as qkv_heads_fake_quant); returns the list of y,
    or None (nothing launched): the caller then runs the eager form.  ``pos``: None, or the device int32 a site whose
    offset is None appends at (ops.fake_quant_kv_append_at: the position is read by the launch).  ``numels``: None, or per
    site the element count a learnable quantizer's grad factor goes by (None: that of x) -- keys / values held once for
    several rows take the factor of the tensor they stand for."""
    if not FUSE_KV_APPEND:
        return None
    for q, x, *_ in sites:
        if not (_plain_quantizing(q, x) and x.dim() == 3 and x.is_contiguous() and x.data_ptr() % 16 == 0):
            return None
    table = []
    for j, (q, x, y, offset, src, rows) in enumerate(sites):
        numel = x.numel() if numels is None or numels[j] is None else numels[j]
        table.append((x, y, offset, _site_record(q, numel), src, rows))
    return ops.fake_quant_kv_append(table, heads) if pos is None else ops.fake_quant_kv_append_at(table, heads, pos)


def kv_site_params(q, x, numel=None):
    """(scale, zero_point, quant_min, quant_max, mode, grad_factor) of quantizer q for the [B, t, h*d] projection x as a site
    of a KV-append launch, or None when kv_append_fake_quant would not take the site (the quantizer not in its plain
    quantising state, x not dense and 16-byte aligned, the one-launch append switched off).  ``numel``: the element count
    the grad factor goes by, where it is not x's (kv_append_fake_quant, ``numels``).  scale and zero_point are the quantizer's
    own tensors here, not their ``.data``: a coded cache tells by their identity and version whether a site still has the
    parameters of its first append (model/quant_bart.py, _code_identity)."""
    if not (FUSE_KV_APPEND and _plain_quantizing(q, x) and x.dim() == 3 and x.is_contiguous() and x.data_ptr() % 16 == 0):
        return None
    return (q.scale, q.zero_point) + _site_record(q, x.numel() if numel is None else numel)[2:]


def kv_append_codes_fake_quant(sites, heads, rejected, pos=None):
    """kv_append_fake_quant for a cache that holds integer codes (ops.fake_quant_kv_append_codes): each site
    ``(quantizer, params, x, y, offset, src, src_rows, record, write_record)`` with ``params`` what kv_site_params gave for
    it; record None is an fp32 site as there, record ``(scale_eff, zp_eff)`` a coded one whose y / src are uint8 buffers.
    Dequantised with the record, the bytes are the words kv_append_fake_quant writes.  Returns the list of y, or None
    (nothing launched).  ``pos`` as in kv_append_fake_quant (ops.fake_quant_kv_append_codes_at)."""
    table = []
    for q, params, x, y, offset, src, rows, record, write_record in sites:
        table.append((x, y, offset, params, src, rows, record, write_record))
    if pos is not None:
        return ops.fake_quant_kv_append_codes_at(table, heads, rejected, pos)
    return ops.fake_quant_kv_append_codes(table, heads, rejected)


def _decode_site_params(q, *sites):
    """The launch parameters of a decoding step's quantizers, ``sites`` = (quantizer, numel) pairs: per site None (no
    quantizer) or (scale, zero_point, quant_min, quant_max, mode, grad_factor), a learnable quantizer's grad factor by the
    ``numel`` elements of the tensor it would see; or None when a quantizer is not in its plain quantising state."""
    params = []
    for quantizer, numel in sites:
        if quantizer is None:
            params.append(None)
            continue
        if not _plain_quantizing(quantizer, q):
            return None
        params.append(_site_record(quantizer, numel))
    return params


def decode_attention_fake_quant(probs_quantizer, ctx_quantizer, q, k, v, mask=None, dropout=None, codes=None):
    """Incremental decoding: what follows the q / k / v + append launch of a step's attention block
    (QuantizedBartAttention._attend: bmm, mask add, softmax, ``probs_quantizer``, bmm, merge heads, ``ctx_quantizer``) as ONE
    launch (ops.decode_attention_fake_quant), for q = [B, h, 1, d] (one query token) and k / v = [B, h, S, d] views of the
    cache buffers or the cross-attention tensors.  Only with FUSE_DECODE_ATTENTION on, autograd off, dropout inactive and
    each quantizer either None or in its plain quantising state (the LSQ / LSQ+ parameter repair rides in the launch as in
    the other one-launch sites).  ``codes``: None, or ``(k_record, v_record, rejected)`` of a coded cache -- k / v are then
    its uint8 code tensors (ops.decode_attention_codes: the same words as on the dequantised tensors).  Returns the
    [B, 1, h*d] context, or None (nothing launched): the caller runs the eager sequence."""
    if not FUSE_DECODE_ATTENTION or torch.is_grad_enabled() or _dropout_active(dropout):
        return None
    if q.dim() != 4 or q.shape[2] != 1 or k.dim() != 4:
        return None
    # the grad factors go by the size of the tensor a quantizer would see: probabilities [B*h, 1, S], context [B, 1, h*d]
    params = _decode_site_params(q, (probs_quantizer, q.shape[0] * q.shape[1] * k.shape[2]), (ctx_quantizer, q.numel()))
    if params is None:
        return None
    if codes is not None:
        return ops.decode_attention_codes(q, k, v, mask, params[0], params[1], *codes)
    return ops.decode_attention_fake_quant(q, k, v, mask, params[0], params[1])


def attention_block_fake_quant(probs_quantizer, ctx_quantizer, q, k, v, mask=None, alpha=None, divisor=None, dropout=None,
                               group=1):
    """An attention block over a whole sequence, from the fake-quantised q [B, h, T, d] and k / v [B, h, S, d] to the merged,
    fake-quantised context [B, T, h*d] -- matmul, ``alpha`` / ``divisor`` and mask as attention_probs_fake_quant takes them,
    softmax, ``probs_quantizer``, matmul, merge heads, ``ctx_quantizer`` -- as ONE launch (ops.attention_fake_quant).  Gated
    as decode_attention_fake_quant is: only with FUSE_ATTENTION on, autograd off, dropout inactive and each quantizer either
    None or in its plain quantising state.  The grad factors go by the tensors the eager quantizers would see:
    probabilities [B, h, T, S], context [B, T, h*d].  ``group`` = G > 1: q is [B * G, h, T, d] and its rows b * G ..
    b * G + G - 1 share row b of k, v and mask (ops.attention_fake_quant, ``group``); the grad factors go by q's rows, so the
    words are those of this function on k, v and mask repeated G times.  Returns the context, or None (nothing launched):
    the caller goes on with the eager sequence."""
    if not FUSE_ATTENTION or torch.is_grad_enabled() or _dropout_active(dropout):
        return None
    if q.dim() != 4 or k.dim() != 4 or not ops.attention_fusable(q, k, v, mask, group):
        return None
    params = _decode_site_params(q, (probs_quantizer, q.shape[0] * q.shape[1] * q.shape[2] * k.shape[2]), (ctx_quantizer, q.numel()))
    if params is None:
        return None
    return ops.attention_fake_quant(q, k, v, mask, params[0], params[1], alpha=alpha, divisor=divisor, group=group)


def attention_int_refusal(q_quantizer, k_quantizer, v_quantizer, probs_quantizer, ctx_quantizer, q, k, v, mask=None,
                          dropout=None, group=1):
    """Why attention_int_block_fake_quant would not hand this call to the integer kernel -- one line -- or None when it
    would (the library may still refuse the shape: head size, length, alignment)."""
    if not FUSE_ATTENTION_INT:
        return "FUSE_ATTENTION_INT is off"
    if torch.is_grad_enabled():
        return "autograd is on"
    if _dropout_active(dropout):
        return "dropout is active"
    # the four quantizers of the products are required (both operands of both products as codes), the context's is not
    sites = [("q", q_quantizer), ("k", k_quantizer), ("v", v_quantizer), ("probabilities", probs_quantizer)]
    for name, quantizer in sites + ([("context", ctx_quantizer)] if ctx_quantizer is not None else []):
        state = _not_plain(quantizer)
        if state:
            return f"the {name} quantizer {state}"
    for name, quantizer in sites:
        if quantizer.quant_max - quantizer.quant_min > ops.ATTENTION_INT_MAX_RANGE:
            return f"the {name} quantizer has more than 256 codes"
    if not (q.is_cuda and k.is_cuda and v.is_cuda):
        return "q / k / v are not on a GPU"
    if q.dim() != 4 or k.dim() != 4 or not ops.attention_fusable(q, k, v, mask, group):
        return "the layout of q / k / v / mask is not fusable"
    return None            # where the parameters live is _decode_site_params' to see


def attention_int_block_fake_quant(q_quantizer, k_quantizer, v_quantizer, probs_quantizer, ctx_quantizer, q, k, v, mask=None,
                                   alpha=None, divisor=None, dropout=None, group=1):
    """attention_block_fake_quant on the INTEGER CODES of the block's own quantizers (ops.attention_int_fake_quant,
    csrc/attention_int.hip): ``q_quantizer`` / ``k_quantizer`` / ``v_quantizer`` are the quantizers that PRODUCED q, k and
    v, so that both products run exactly, on the bf16 matrix instruction, over S up to 16384.  Gated as that function is,
    with FUSE_ATTENTION_INT for FUSE_ATTENTION: autograd off, dropout inactive, every quantizer in its plain quantising state
    and per-tensor; q, k, v and the probabilities quantizer are required, ``ctx_quantizer`` may be None
    (attention_int_refusal names the reason of a refusal).  The grad factors go by the tensors the eager quantizers see --
    with ``group`` = G > 1 (as in attention_block_fake_quant) those of the unshared form: k and v by G times their elements.
    Returns the context [B, T, h*d], or None (nothing launched): the caller goes on with attention_block_fake_quant and the
    eager sequence."""
    if attention_int_refusal(q_quantizer, k_quantizer, v_quantizer, probs_quantizer, ctx_quantizer, q, k, v, mask, dropout,
                             group):
        return None
    params = _decode_site_params(q, (q_quantizer, q.numel()), (k_quantizer, k.numel() * group), (v_quantizer, v.numel() * group),
                                 (probs_quantizer, q.shape[0] * q.shape[1] * q.shape[2] * k.shape[2]), (ctx_quantizer, q.numel()))
    if params is None:
        return None
    return ops.attention_int_fake_quant(q, k, v, mask, *params, alpha=alpha, divisor=divisor, group=group)


def attention_sequence_fake_quant(q_quantizer, k_quantizer, v_quantizer, probs_quantizer, ctx_quantizer, q, k, v, mask=None,
                                  alpha=None, divisor=None, dropout=None, group=1):
    """The one-launch attention block over a whole sequence as the models call it: on the integer codes of the block's
    quantizers (attention_int_block_fake_quant, FUSE_ATTENTION_INT), else in fp32 (attention_block_fake_quant,
    FUSE_ATTENTION).  ``group``: the rows of q that share a row of k, v and mask, as both take it.  Returns the context
    [B, T, h*d], or None when neither launched: the caller runs the eager sequence (on expanded k, v and mask, with a group)."""
    out = attention_int_block_fake_quant(q_quantizer, k_quantizer, v_quantizer, probs_quantizer, ctx_quantizer, q, k, v, mask,
                                         alpha=alpha, divisor=divisor, dropout=dropout, group=group)
    if out is None:
        out = attention_block_fake_quant(probs_quantizer, ctx_quantizer, q, k, v, mask, alpha=alpha, divisor=divisor,
                                         dropout=dropout, group=group)
    return out


def decode_attention_shared_fake_quant(probs_quantizer, ctx_quantizer, q, k, v, group, mask=None, dropout=None, codes=None,
                                       force=False):
    """decode_attention_fake_quant for q = [B * group, h, 1, d] whose rows b * group .. b * group + group - 1 share row b of
    k / v = [B, h, S, d] and of mask [B, 1, 1, S] (beam search's cross-attention over a QuantizedBartCache with
    ``cross_group``): ONE launch, every word of K and V read once per 8 query rows (ops.decode_attention_shared).  Gated as
    decode_attention_fake_quant is -- ``force``: the caller asked for the shared form whatever FUSE_DECODE_ATTENTION says
    (generate(share_cross_kv=True)).  The grad factors go by the query rows, as in the unshared form: the words are those of
    decode_attention_fake_quant on k / v / mask repeated ``group`` times.  Returns the [B * group, 1, h*d] context, or None
    (nothing launched): the caller expands k / v / mask and takes the unshared path."""
    if not (FUSE_DECODE_ATTENTION or force) or torch.is_grad_enabled() or _dropout_active(dropout):
        return None
    if q.dim() != 4 or q.shape[2] != 1 or k.dim() != 4:
        return None
    params = _decode_site_params(q, (probs_quantizer, q.shape[0] * q.shape[1] * k.shape[2]), (ctx_quantizer, q.numel()))
    if params is None:
        return None
    return ops.decode_attention_shared(q, k, v, mask, params[0], params[1], group, codes=codes)


def decode_grad_table(quantizer, rows, kv_max):
    """The grad factors of the probabilities quantizer of a decoding step for every length: a float32 CPU tensor of
    ``kv_max + 1`` entries, entry n what decode_attention_fake_quant hands the launch at kv_len == n for ``rows`` = B * h
    rows of probabilities -- the same expression (``quantizer._grad_factor``), rounded to fp32 as a launch argument is.
    Entry 0 is not read.  ops.decode_attention_at reads the table on the device: a captured step holds no host number that
    moves with the position."""
    fixed = quantizer.param_mode == ops.PARAM_FIXED
    return torch.tensor([0.0] + [1.0 if fixed else quantizer._grad_factor(_Numel(rows * n)) for n in range(1, kv_max + 1)],
                        dtype=torch.float64).to(torch.float32)


def decode_attention_at_fake_quant(probs_quantizer, ctx_quantizer, q, k, v, pos, add, kv_max, grad_table, dropout=None,
                                   codes=None):
    """decode_attention_fake_quant over the whole cache buffers k / v = [B, h, cap, d] with the length ``*pos + add`` read
    by the launch (ops.decode_attention_at; self-attention: the cache's position word and the step's own token).
    ``grad_table``: decode_grad_table of the probabilities quantizer on the device.  No mask: a single-token step of the
    decoder's self-attention has none.  The switch FUSE_DECODE_ATTENTION is not asked: a step whose position lives on the
    device has no eager form.  Returns the [B, 1, h*d] context, or None (nothing launched)."""
    if torch.is_grad_enabled() or _dropout_active(dropout) or q.dim() != 4 or q.shape[2] != 1:
        return None
    params = _decode_site_params(q, (probs_quantizer, q.numel()), (ctx_quantizer, q.numel()))    # probs: grad_table serves
    if params is None:
        return None
    return ops.decode_attention_at(q, k, v, pos, add, kv_max, None, params[0], params[1], grad_table=grad_table, codes=codes)


def _dropout_active(dropout):
    if dropout is None:
        return False
    if isinstance(dropout, nn.Module):
        return dropout.training and dropout.p > 0
    p, training = dropout
    return training and p > 0


def _apply_dropout(dropout, x):
    if dropout is None:
        return x
    if isinstance(dropout, nn.Module):
        return dropout(x)
    p, training = dropout
    return F.dropout(x, p=p, training=training)


def attention_probs_fake_quant(quantizer, scores, mask, alpha=None, divisor=None, dropout=None, observation_mask=None,
                               seq_pos=2, heads=None):
    """The attention-probabilities site: ``quantizer(dropout(softmax(pre(scores) + mask, -1)), observation_mask, seq_pos)``.

    pre: ``alpha`` -- ``torch.add(mask, scores, alpha=alpha)``, one stock op (BERT, power-of-two 1/sqrt(d));
    ``divisor`` -- ``scores / divisor`` then ``+ mask`` (BERT, other head sizes or no mask); neither -- ``scores + mask``
    (BART, q scaled beforehand).  ``heads``: scores is BART's [B*h, T, S] view and mask broadcasts against its
    [B, h, T, S] form (quant_bart.py:128-129); the result keeps the layout scores came in.  ``dropout``: an nn.Dropout, or
    (p, training) for the functional form.

    With FUSE_SOFTMAX on, autograd off, dropout inactive and a fusable layout, ONE launch computes the probabilities --
    and, when the quantizer is in its plain quantising state, their fake-quant as well (the LSQ / LSQ+ parameter repair
    riding along as in the other one-launch sites); otherwise the quantizer then runs its own path on them."""
    scores4 = scores.view(scores.shape[0] // heads, heads, *scores.shape[1:]) if heads is not None else scores
    if FUSE_SOFTMAX and not torch.is_grad_enabled() and not _dropout_active(dropout) and \
            ops.attention_softmax_fusable(scores4, mask):
        q = quantizer
        quant = None
        if _plain_quantizing(q, scores):
            quant = _site_record(q, scores.numel())
        probs = ops.attention_softmax_fake_quant(scores4, mask, alpha=alpha, divisor=divisor, quant=quant).view(scores.shape)
        if q is not None and quant is None:
            probs = q(probs, observation_mask, seq_pos)
        return probs
    if alpha is not None:
        v = torch.add(mask, scores, alpha=alpha) if mask is not None else scores * alpha
    else:
        v = scores if divisor is None else scores / divisor
        if mask is not None:
            v = (v.view(scores4.shape) + mask).view(scores.shape)
    probs = _apply_dropout(dropout, F.softmax(v, dim=-1))
    if quantizer is not None:
        probs = quantizer(probs, observation_mask, seq_pos)
    return probs

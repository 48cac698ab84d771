"""Routing of ``QLinear.forward`` to the integer linear launch (``util_layernorm.FUSE_LINEAR_INT``, csrc/linear_int.hip).

In a frozen model a ``QLinear`` multiplies two tensors of integer codes: its weight quantizer's output and the output of the
activation quantizer that PRODUCED its input.  A linear does not see that quantizer, so the model wrappers tell it:
``bind_linear_producers(model)`` (called by ``quantize_model``) walks the known block types and leaves on each ``QLinear`` a
plain ``(owner module, dotted attribute path)`` pair in its ``__dict__`` -- no parameter, no buffer, no sub-module:
``state_dict()``, ``named_modules()`` and ``named_parameters()`` do not change.  The owner is the block (or embedding / head)
module, which nothing replaces, and the path is walked at every call: a quantizer replaced later, or a whole
QuantizedLayerNorm replaced by gamma migration's QuantizedSplitLayerNorm with its new quantizer, is the one found.

The binding describes the wrappers as they run themselves.  Two things it cannot see keep ``F.linear``: a module in training
mode (dropout may sit between a producer and its linear) -- and one it cannot check is the caller's: ``encoder_outputs``
handed to a BART wrapper must be that wrapper's own encoder output (the cross-attention's k_proj / v_proj read the encoder's
last LayerNorm site), else turn the switch off for the call.

``forward(op, x)`` returns the integer path's result, or None with the reason in ``util_layernorm.linear_int``: the caller
then runs its ``F.linear`` line.  The codes of one producer output are made once and shared by its consumers (query / key /
value) inside ``shared_codes()``, which the transformer blocks open for the length of their forward; nothing is kept
beyond it.
"""
import torch

from .. import ops
from . import weight_cache

# A weight quantizer of at most 16 codes has its codes cached two to a byte (ops.weight_codes(bits=4)) and multiplied by the
# packed kernels.  The words of the result are the same either way; on by default because no shape measured in
# profiles/linear_int_w4_ab.txt loses beyond the 8-bit form's own range and the lm_head shapes gain 23 - 29 %.
PACK_W4 = True
# A feed-forward block (fc1 -> GELU -> quantizer -> fc2) whose two linears take the integer launches has fc1's launch write
# fc2's activation codes (ffn below): the block's largest tensor is never written as fp32.  The words are the chain's.
# On by default for the shapes that gain: up to FFN_MAX_ROWS rows (the rows kernels: a decoding step, +15 - 18 % on the block's
# launches) the path is taken; above it the tile kernel's epilogue LOSES 31 - 45 % to the chain it replaces
# (profiles/linear_int_codes_ab.txt), so those calls keep the chain.  FFN_MAX_ROWS = None lifts the limit (A/B, tests).
FUSE_FFN = True
FFN_MAX_ROWS = ops.LINEAR_INT_ROWS_M
_SHARED = []        # the open shared_codes() scopes: {(id(x), version, id(producer)): (x, codes, rowsum)}


class shared_codes:
    """``with shared_codes():`` for the length of a block's forward: one ``ops.activation_codes`` launch per (tensor, version,
    producer) inside it, nothing kept after it."""

    def __enter__(self):
        _SHARED.append({})

    def __exit__(self, *exc):
        _SHARED.pop()


def _resolve(owner, path):
    for name in path.split("."):
        owner = getattr(owner, name, None)
    return owner


def bind(op, owner, path):
    """Tell ``op`` that its input is the output of the activation quantizer at the dotted ``path`` below ``owner`` (absent: no
    producer)."""
    if _resolve(owner, path) is None:
        op.__dict__.pop("_linear_producer", None)
    else:
        op.__dict__["_linear_producer"] = (owner, path)


def producer_of(op):
    """The quantizer that produces ``op``'s input as the model stands NOW, or None."""
    ref = op.__dict__.get("_linear_producer")
    return None if ref is None else _resolve(*ref)


def _ln(owner, name):
    """(owner, path) of the output quantizer of the LayerNorm site ``owner.<name>``: through the owner, because gamma migration
    replaces the site's module."""
    return owner, name + ".layernorm_post_act_fake_quantize"


def _bind_bert_stack(model):
    """QuantizedBertModel / QuantizedRobertaModel: embeddings -> layers -> pooler.  Returns the last layer's producer."""
    prev = _ln(model.embeddings, "LayerNorm")
    for layer in model.encoder.layer:
        att = layer.attention.self
        for proj in (att.query, att.key, att.value):
            bind(proj, *prev)
        bind(layer.attention.output.dense, att, "context_view_post_act_fake_quantize")
        bind(layer.intermediate.dense, *_ln(layer.attention.output, "LayerNorm"))
        bind(layer.output.dense, layer.intermediate, "intermediate_act_fn_post_act_fake_quantize")
        prev = _ln(layer.output, "LayerNorm")
    if getattr(model, "pooler", None) is not None:
        bind(model.pooler.dense, model.pooler, "getitem_post_act_fake_quantize")
    return prev


def _bind_bart_attention(attn, query_from, kv_from):
    bind(attn.q_proj, *query_from)
    bind(attn.k_proj, *kv_from)
    bind(attn.v_proj, *kv_from)
    bind(attn.out_proj, attn, "context_post_act_fake_quantize")


def _bind_bart_model(model):
    """QuantizedBartModel as it runs: the decoder's cross-attention reads the encoder's last LayerNorm site.  Returns the
    decoder's last producer."""
    prev = _ln(model.encoder, "layernorm_embedding")
    for layer in model.encoder.layers:
        _bind_bart_attention(layer.self_attn, prev, prev)
        bind(layer.fc1, *_ln(layer, "self_attn_layer_norm"))
        bind(layer.fc2, layer, "fc1_act_fn_post_act_fake_quantize")
        prev = _ln(layer, "final_layer_norm")
    memory, prev = prev, _ln(model.decoder, "layernorm_embedding")
    for layer in model.decoder.layers:
        _bind_bart_attention(layer.self_attn, prev, prev)
        _bind_bart_attention(layer.encoder_attn, _ln(layer, "self_attn_layer_norm"), memory)
        bind(layer.fc1, *_ln(layer, "encoder_attn_layer_norm"))
        bind(layer.fc2, layer, "fc1_act_fn_post_act_fake_quantize")
        prev = _ln(layer, "final_layer_norm")
    return prev


def _bind_head(head):
    """The RoBERTa / BART classification head: getitem quantizer -> dense -> tanh -> dropout quantizer -> out_proj."""
    bind(head.dense, head, "getitem_post_act_fake_quantize")
    bind(head.out_proj, head, "dropout_post_act_fake_quantize")


def bind_linear_producers(model):
    """Bind every ``QLinear`` of a quantized BERT / RoBERTa / BART wrapper whose input is an activation quantizer's output.
    What it does not know -- user modules, a linear behind an unquantised tensor -- stays without a producer."""
    from ..model import quant_bart as BA, quant_bert as BE, quant_roberta as RO
    for m in model.modules():
        if isinstance(m, (BE.QuantizedBertForSequenceClassification, BE.QuantizedBertForQuestionAnswering)):
            last = _bind_bert_stack(m.bert)
            if hasattr(m, "classifier"):
                bind(m.classifier, m, "dropout_post_act_fake_quantize")
            else:
                bind(m.qa_outputs, *last)
        elif isinstance(m, (RO.QuantizedRobertaForSequenceClassification, RO.QuantizedRobertaForQuestionAnswering)):
            last = _bind_bert_stack(m.roberta)
            if hasattr(m, "classifier"):
                _bind_head(m.classifier)
            else:
                bind(m.qa_outputs, *last)
        elif isinstance(m, BA.QuantizedBartModel):
            _bind_bart_model(m)
        elif isinstance(m, BA.QuantizedBartForConditionalGeneration):
            bind(m.lm_head, *_ln(m.model.decoder.layers[-1], "final_layer_norm"))
        elif isinstance(m, BA.QuantizedBartForQuestionAnswering):
            bind(m.qa_outputs, *_ln(m.model.decoder.layers[-1], "final_layer_norm"))
        elif isinstance(m, BA.QuantizedBartClassificationHead):
            _bind_head(m)
    return model


def why_not(op, x):
    """None when ``op(x)`` takes the integer launches, else the reason -- one phrase -- it runs ``F.linear``."""
    return _why_not(op, x)


def weight_why_not(op):
    """``why_not`` without an input tensor: the producer, the module's and the weight quantizer's state, K, the weight side's
    tensors -- what can be asked of a linear whose input does not exist yet (``ffn`` asks it of fc2)."""
    return _why_not(op, None)


def _why_not(op, x):
    from .. import util_layernorm as UL
    q = producer_of(op)
    if q is None:
        return "no producer"
    state = UL._not_plain(q)
    if state:
        return f"the producer {state}"
    if torch.is_grad_enabled():
        return "autograd is on"
    if op.training:
        return "the module is in training mode"
    fq = op.weight_fake_quant
    if fq.fake_quant_enabled != 1 or fq.observer_enabled == 1 or fq.ch_axis not in (0, -1):
        return "the weight quantizer is not plainly quantising and cacheable"
    record = (q.scale, q.zero_point, q.quant_min, q.quant_max)
    given = () if x is None else (x,)
    why = ops.linear_int_refusal(op.in_features, record, fp32=given + (op.weight, fq.scale, op.bias), last_dim=given)
    if why is None and fq.quant_max - fq.quant_min > ops.LINEAR_INT_MAX_RANGE:
        why = "a quantizer has more than 256 codes"
    if why is None and not ((x is None or x.numel()) and op.weight.is_contiguous() and op.weight.data_ptr() % 16 == 0
                            and (op.bias is None or op.bias.is_contiguous())):
        why = "the operands are not dense, 16-byte aligned tensors"
    if why is None and not (fq.scale.numel() == fq.zero_point.numel() == (op.out_features if fq.ch_axis == 0 else 1)):
        why = "the weight quantizer's parameters do not match its channels"
    if why is None and not (weight_cache.enabled and weight_cache.cacheable(op, fq)):      # last: it asks where the weight lives
        why = "the weight quantizer is not plainly quantising and cacheable"
    return why


def _input_codes(op, x):
    """(codes, rowsum, record) of ``op``'s input under its producer: one ``ops.activation_codes`` launch per (tensor, version,
    producer) of the open ``shared_codes()`` scope."""
    from .. import util_layernorm as UL
    q = producer_of(op)
    record = UL._site_record(q, x.numel())
    key = (id(x), x._version, id(q))
    held = _SHARED[-1].get(key) if _SHARED else None
    if held is None:
        codes, rowsum = ops.activation_codes(x, record)
        if _SHARED:
            _SHARED[-1][key] = (x, codes, rowsum)      # x itself: its id stays its own while the entry lives
    else:
        _, codes, rowsum = held
    return codes, rowsum, record


def _bias(op):
    return None if op.bias is None else op.bias.detach()


def forward(op, x):
    """``QLinear.forward`` under FUSE_LINEAR_INT: the integer path's [..., N] result, or None (counted, with the reason)."""
    from .. import util_layernorm as UL
    info = UL.linear_int
    why = why_not(op, x)
    entry = None
    if why is None:
        entry = weight_cache.weight_codes(op)
        if entry is None:
            why = "the weight's codes are not made inside a stream capture"
    if why is not None:
        info.eager += 1
        info.reason = why
        return None
    codes, rowsum, record = _input_codes(op, x)
    info.fused += 1
    return ops.linear_int(codes, rowsum, record, entry, _bias(op))


def ffn(fc1, act_fn, q, fc2, x):
    """``fc2(q(act_fn(fc1(x))))`` of a feed-forward block under FUSE_LINEAR_INT and FUSE_FFN: fc1's launch writes the codes
    fc2 reads (``ops.linear_int_codes``), the [..., 4H] fp32 tensor is never made -- or None, nothing launched and nothing
    counted, when the chain must run: the caller's lines then do, and count, what they did before.  The words of the result
    are the chain's.  Everything is asked BEFORE anything is launched: both linears take the integer launches (fc2's input
    side is fc1's output side: N % 16 == 0, N <= 16384), the site is the one ``util_layernorm.activation_fake_quant`` gives
    one launch (FUSE_ACTIVATION, an exact GELU, ``q`` plainly quantising per tensor), ``q`` is fc2's producer, both weights'
    codes exist (they are not made inside a stream capture), and the call has at most FFN_MAX_ROWS rows."""
    from .. import util_layernorm as UL
    if not (FUSE_FFN and UL.FUSE_ACTIVATION and q is not None and producer_of(fc2) is q and ops.is_exact_gelu(act_fn)):
        return None
    if UL._not_plain(q) or not q.scale.is_cuda or why_not(fc1, x) is not None or weight_why_not(fc2) is not None:
        return None
    if not (x.is_contiguous() and fc1.out_features == fc2.in_features):
        return None
    if FFN_MAX_ROWS is not None and x.numel() // x.shape[-1] > FFN_MAX_ROWS:      # the measured loss: the chain is faster
        return None
    entries = weight_cache.weight_codes(fc1), weight_cache.weight_codes(fc2)
    if entries[0] is None or entries[1] is None:
        return None
    codes, rowsum, record = _input_codes(fc1, x)
    mid = UL._site_record(q, codes.numel() // codes.shape[-1] * fc1.out_features)
    codes, rowsum = ops.linear_int_codes(codes, rowsum, record, entries[0], _bias(fc1), mid, "gelu")
    UL.linear_int.fused += 2
    UL.linear_int.ffn += 1
    return ops.linear_int(codes, rowsum, mid, entries[1], _bias(fc2))

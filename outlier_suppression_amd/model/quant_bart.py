"""Quantized BART (encoder-decoder): where the quantizers sit.

Placement table (reference: quant_transformer/model/quant_bart.py):
  attention     q/k/v/out_proj -> QLinear (:120-123).  q*scaling, k, v quantized as [B,T,D] (seq axis 1)
                BEFORE the head split (:156-198); probs are the 3-D [B*h, T, S] tensor with seq axis 2 (:256);
                context [B,T,D] seq axis 1 (:272); out_proj output only if qoutput (:276)
  cross-attn    k/v come from the ENCODER states but are masked with the lengths the decoder layer passes,
                i.e. the decoder's (:167,172,472) -- kept
  probs mask    a length-B mask against B*h rows: observer.py:82's zip covers only the first B rows -- kept
                (ops.token_view(n_lengths=...))
  enc layer     self_attn(qoutput=False) -> GammaResidual -> LayerNorm(+q); fc1 -> act -> quantizer; fc2 ->
                GammaResidual -> LayerNorm(+q unless last layer of a qoutput=False stack) (:281-353)
  dec layer     self-attn block, cross-attn block (own GammaResidual + LayerNorm), ffn block (:369-492)
  embeddings    embed_tokens*embed_scale + learned positions (offset 2, own QEmbedding) -> layernorm_embedding (+q)
  model         shared / encoder.embed_tokens / decoder.embed_tokens are three separate QEmbedding copies
                (:553,698,901); encoder qoutput=True, decoder qoutput = model's (:904-907)
  lm            model(qoutput=True) -> lm_head (QLinear) + final_logits_bias (:1020-1023,1101)
  decoding      past_key_values / use_cache / encoder_outputs (:1036-1164): a step fake-quantizes only its own k / v and
                appends them to the cache; cross-attention k / v are quantized once and reused.  QuantizedBartCache holds
                the buffers and reads as the reference's tuple of (k, v, cross_k, cross_v) per layer; generate()
                (model/generation.py) runs greedy and beam search on it.
"""
import torch
from torch import nn

from . import generation
from .losses import LmLossInfo, classification_loss, lm_loss, span_loss, token_logprob_torch, with_loss
from .. import ops
from .. import util_layernorm as _UL
from ..quantization import QuantizedModule, Quantizer
from ..util_layernorm import (GammaResidual, QuantizedLayerNorm, activation_fake_quant, attention_probs_fake_quant,
                              attention_sequence_fake_quant,
                              decode_attention_at_fake_quant, decode_attention_fake_quant, decode_attention_shared_fake_quant,
                              decode_grad_table,
                              kv_append_codes_fake_quant, kv_append_fake_quant,
                              kv_site_params, merge_heads_fake_quant, qkv_heads_fake_quant, residual_layernorm,
                              split_heads_fake_quant)


def shift_tokens_right(input_ids, pad_token_id, decoder_start_token_id):
    """quant_bart.py:24-37."""
    shifted = input_ids.new_zeros(input_ids.shape)
    shifted[:, 1:] = input_ids[:, :-1].clone()
    shifted[:, 0] = decoder_start_token_id
    shifted.masked_fill_(shifted == -100, pad_token_id)
    return shifted


def _causal_mask(bsz, tgt_len, dtype, device, past=0):
    """quant_bart.py:40-52: -inf above the diagonal, preceded by `past` zero columns for the cached positions."""
    mask = torch.full((tgt_len, tgt_len), float("-inf"), device=device)
    cond = torch.arange(tgt_len, device=device)
    mask.masked_fill_(cond < (cond + 1).view(tgt_len, 1), 0)
    mask = mask.to(dtype)
    if past > 0:
        mask = torch.cat([torch.zeros(tgt_len, past, dtype=dtype, device=device), mask], dim=-1)
    return mask[None, None, :, :].expand(bsz, 1, tgt_len, tgt_len + past)


def _expand_mask(mask, dtype, tgt_len=None):
    """quant_bart.py:55-66: [B,S] -> additive [B,1,T,S] with finfo.min on padding."""
    bsz, src_len = mask.shape
    tgt_len = tgt_len if tgt_len is not None else src_len
    inverted = 1.0 - mask[:, None, None, :].expand(bsz, 1, tgt_len, src_len).to(dtype)
    return inverted.masked_fill(inverted.bool(), torch.finfo(dtype).min)


def _plain_embedding(emb):
    """transformers >= 4.4x wraps BART's token embedding in a scaling nn.Embedding subclass; Quantizer() only
    recognises the exact nn.Embedding type (quantized_module.py:103-107), so rebuild a plain one on the same data."""
    if type(emb) is nn.Embedding:
        return emb
    plain = nn.Embedding(emb.num_embeddings, emb.embedding_dim, padding_idx=emb.padding_idx)
    plain.weight.data = emb.weight.data
    return plain


def _embed_scale(stack):
    """sqrt(d_model) if config.scale_embedding else 1 (stored on the stack in 4.18, on the embedding later)."""
    if hasattr(stack, "embed_scale"):
        return stack.embed_scale
    return getattr(stack.embed_tokens, "embed_scale", 1.0)


class _CodedTensor:
    """A cached tensor held as integer codes, as QuantizedBartAttention sees it: ``codes`` the uint8 [B, h, S, d] tensor (a
    ``[:, :, :S]`` view of a cache buffer, or the whole cross-attention tensor), ``record`` its (scale_eff, zp_eff,
    quant_min), ``rejected`` the cache's counter."""

    __slots__ = ("codes", "record", "rejected")

    def __init__(self, codes, record, rejected):
        self.codes, self.record, self.rejected = codes, record, rejected

    def float(self):
        """The fp32 [B, h, S, d] tensor, a view of a buffer of the coded one's own geometry: the words and strides an fp32
        cache hands out."""
        c = self.codes
        b, h, s, d = c.shape
        row = c.stride(1) if h > 1 else (c.stride(0) if b > 1 else s * d)       # cap * d of the buffer c is a view of
        buf = c if row == s * d else c.as_strided((b, h, row // d, d), (h * row, row, d, 1))
        return ops.dequantize_kv_codes(buf, self.record)[:, :, :s]


class _CodeRecord:
    """What a coded cache tensor keeps besides its bytes: the device pair (scale_eff, zp_eff) its first append wrote, and
    the host-side identity of that append's parameters."""

    __slots__ = ("scale_eff", "zp_eff", "quant_min", "identity", "pinned", "fresh")

    def __init__(self, pair, params):
        self.scale_eff, self.zp_eff = pair[0:1], pair[1:2]
        self.quant_min = params[2]
        self.identity = _code_identity(params)
        self.pinned = params[:2]                                    # keeps the ids in `identity` from being reused
        self.fresh = True                                           # no launch has written the device pair yet

    def triple(self):
        return self.scale_eff, self.zp_eff, self.quant_min


def _code_identity(params):
    """Host-side identity of a site's parameters (util_layernorm.kv_site_params): equal identities give the same effective
    (scale, zero point) words unless somebody wrote the parameters through raw pointers (the launch checks that)."""
    scale, zp, quant_min, quant_max, mode, grad_factor = params
    return (grad_factor, quant_min, quant_max, mode, id(scale), scale._version, id(zp), zp._version)


def _takes_codes(params, x, heads):
    """Whether a site takes codes: the one-launch append takes it (params), its codes fit a byte, the kernels take its head size."""
    return (params is not None and params[3] - params[2] <= 255 and x.shape[2] % heads == 0
            and (x.shape[2] // heads) % 4 == 0)


_SELF, _CROSS = ("k", "v"), ("cross_k", "cross_v")


class QuantizedBartCache:
    """The decoder's KV cache for incremental decoding.

    Per layer: the self-attention keys / values in [B, h, cap, d] buffers with room for `capacity` positions (a step
    appends in place), a ping-pong partner buffer for beam reorders, and the cross-attention keys / values (quantized once,
    at the first step).  ``reorder(beam_idx)`` (what ``_reorder_cache`` calls) only records the row index: the next step's
    append copies the kept prefix through it into the partner buffer in the same launch (util_layernorm.
    kv_append_fake_quant), so a step costs one cache copy when beams move and none for greedy decoding, with no torch.cat.

    The object also reads as the reference's legacy tuple of tuples: ``cache[i] == (k, v, cross_k, cross_v)``, each a
    [B, h, S, d] view, ``cache[0][0].shape[2]`` the past length (quant_bart.py:774).  Reading it applies a pending reorder.
    A step extends the cache in place and returns the same object: views read from it stay valid until the next step.

    ``codes=True``: every tensor whose site qualifies (the one-launch append would take it -- util_layernorm.kv_site_params
    -- and quant_max - quant_min <= 255) is held as integer codes, one byte per element (include/osq_hip.h, "the KV cache as
    integer codes"), with a record of the effective parameters of its first append; the other tensors -- and everything on
    the CPU or wrapped from a tuple -- stay fp32, tensor by tensor.  A later append whose parameters differ on the host
    side (another grad factor, a parameter tensor replaced or written) first DEMOTES that tensor: one dequantise launch,
    fp32 from then on.  Whatever is read from the cache -- ``cache[i]``, iteration, ``to_legacy()``, ``past(i)`` -- is
    fp32, the words an fp32 cache holds.  Elements without a code (NaN, an infinite value, a fractional zero point) are
    counted on the device: ``rejected()`` reads the counter, and attention over a cache with a non-zero counter yields
    NaN.

    ``cross_group=G`` (beam search, generate(share_cross_kv=True)): the decoder runs G rows -- the beams -- per encoder row,
    and the cross-attention keys / values, identical for them, are held ONCE per encoder row: [B, h, S, d] beside
    self-attention buffers of B * G rows.  QuantizedBartAttention projects and quantizes them on B rows (with the grad factor
    of the B * G-row tensor they stand for: the words and records of the unshared cache) and attends to them from every beam
    in one launch (util_layernorm.decode_attention_shared_fake_quant).  Reading the cache -- ``cache[i]``, iteration,
    ``to_legacy()`` -- repeats them to the decoder's row count, materialised on read, so the legacy tuple keeps its shapes;
    ``nbytes()`` counts what is held.  Reorders leave them alone, as ever: a beam never changes its batch row.

    Device-position mode (``enter_device_position()``; model/graph_decode.py is its only user): the past length also lives
    in ONE device int32 shared by all layers, which single-token steps read in their launches (the _at forms of the append
    and of the attention) and the decoder advances after its last layer, so that a captured step can be replayed at every
    position; ``_len`` mirrors it on the host.  ``reorder()`` then copies the index into a static int64 buffer, and both
    buffers of every layer's ping-pong pair exist at ``capacity``.  Reading the cache while a reorder is pending leaves the
    mode (the read re-packs the buffers)."""

    def __init__(self, num_layers, capacity=None, codes=False, cross_group=1):
        if int(cross_group) < 1:
            raise ValueError("cross_group must be at least 1")
        self.capacity = capacity
        self.codes = bool(codes)
        self.cross_group = int(cross_group)        # decoder rows per row of the cross-attention keys / values
        self.cross_one_launch = False              # the shared cross-attention launch whatever FUSE_DECODE_ATTENTION says
        self._k = [None] * num_layers
        self._v = [None] * num_layers
        self._spare = [[None, None] for _ in range(num_layers)]     # partner buffers of k and v, or None
        self._len = [0] * num_layers
        self._rows = [None] * num_layers           # pending beam index per layer
        self._cross = [None] * num_layers          # (k, v) of the cross-attention, or None
        self._records = [{} for _ in range(num_layers)]             # name -> _CodeRecord of the layer's coded tensors
        self._record_pairs = None                  # [num_layers * 4, 2] fp32 on the device: every record's (scale_eff, zp_eff)
        self._rejected = None                      # one int32 on the device
        self._demoted = []
        self._pos = None                           # device-position mode: one int32 on the device, the past length
        self._rows_buf = None                      # ... and the static int64 [B] row index reorder() copies into
        self._tables = {}                          # ... grad-factor tables of the probabilities quantizers, on the device

    @classmethod
    def wrap(cls, past, num_layers, capacity=None, codes=None):
        """``past``: None, a QuantizedBartCache (returned as it is), or the reference's tuple of per-layer (k, v[, cross_k,
        cross_v]) tensors, which stay fp32.  ``codes``: whether a new cache holds integer codes (None: the package switch,
        set_cache_codes / OSQ_CACHE_CODES)."""
        if isinstance(past, cls):
            return past
        cache = cls(num_layers, capacity, codes=_UL.CACHE_CODES if codes is None else codes)
        if past is not None:
            if len(past) != num_layers:
                raise ValueError(f"past_key_values has {len(past)} layers, the decoder {num_layers}")
            for i, layer in enumerate(past):
                cache._k[i], cache._v[i] = layer[0], layer[1]
                cache._len[i] = layer[0].shape[2]
                if len(layer) >= 4:
                    cache._cross[i] = (layer[2], layer[3])
        return cache

    def get_seq_length(self, layer=0):
        return self._len[layer]

    def reorder(self, beam_idx):
        """Select the rows ``beam_idx`` of every self-attention cache, lazily; returns self."""
        if self._pos is not None:
            pending = self._rows[0] is not None
            self._rows_buf.copy_(self._rows_buf.index_select(0, beam_idx) if pending else beam_idx)
            self._rows = [self._rows_buf] * len(self._k)
            return self
        for i in range(len(self._k)):
            if self._k[i] is not None:
                self._rows[i] = beam_idx if self._rows[i] is None else self._rows[i].index_select(0, beam_idx)
        return self

    def _materialise(self, i):
        rows = self._rows[i]
        if rows is not None:
            if self._pos is not None:              # the re-packed tensors are not the static buffers a captured step names
                self._pos = None
                self._rows = [None if r is None else r.clone() for r in self._rows]
                rows = self._rows[i]
            n = self._len[i]
            self._k[i] = self._k[i][:, :, :n].index_select(0, rows)
            self._v[i] = self._v[i][:, :, :n].index_select(0, rows)
            self._rows[i] = None

    def __len__(self):
        return len(self._k)

    def __getitem__(self, i):
        if self._k[i] is None:
            raise IndexError(f"layer {i} of the cache holds nothing yet")
        if self._cross[i] is None:
            return self.past(i)
        cross = tuple(self._fp32(i, name, t) for name, t in zip(_CROSS, self._cross[i]))
        if self.cross_group > 1:                   # one copy per encoder row is held: the tuple shows the decoder's rows
            cross = tuple(t.repeat_interleave(self.cross_group, dim=0) for t in cross)
        return self.past(i) + cross

    def __iter__(self):
        return (self[i] for i in range(len(self)))

    def to_legacy(self):
        return tuple(self)

    # ---- integer codes
    def _operand(self, i, name, t):
        """Tensor t of layer i as attention takes it: itself, or a _CodedTensor."""
        rec = self._records[i].get(name)
        return t if rec is None else _CodedTensor(t, rec.triple(), self._rejected)

    def _fp32(self, i, name, t):
        rec = self._records[i].get(name)
        return t if rec is None else _CodedTensor(t, rec.triple(), self._rejected).float()

    def _tensor(self, i, name):
        if name in _SELF:
            return (self._k[i], self._v[i])[_SELF.index(name)]
        return None if self._cross[i] is None else self._cross[i][_CROSS.index(name)]

    def plan(self, i, names, params, xs, heads):
        """Before an append of the projections ``xs`` with the site parameters ``params`` (util_layernorm.kv_site_params, None
        for a site the one-launch append does not take) to the tensors ``names`` of layer i: which of them take codes.  A tensor not yet held takes codes when the cache holds codes and its site qualifies; a coded one
        goes on as such while its site qualifies with the parameters of its first append, and is demoted to fp32 first
        otherwise.  Host decisions only, no sync."""
        coded = []
        for name, p, x in zip(names, params, xs):
            rec, held = self._records[i].get(name), self._tensor(i, name)
            if held is None:
                if self.codes and _takes_codes(p, x, heads):
                    if self._record_pairs is None:
                        self._record_pairs = x.new_empty((len(self._k) * 4, 2))
                        self._rejected = torch.zeros(1, dtype=torch.int32, device=x.device)
                    slot = i * 4 + (_SELF + _CROSS).index(name)
                    rec = self._records[i][name] = _CodeRecord(self._record_pairs[slot], p)
            elif rec is not None and (p is None or _code_identity(p) != rec.identity):
                self.demote(i, name)
                rec = None
            coded.append(rec is not None)
        return coded

    def record(self, i, name):
        """(record pair, write_record) of a coded tensor for ops.fake_quant_kv_append_codes, or (None, False)."""
        rec = self._records[i].get(name)
        return (None, False) if rec is None else ((rec.scale_eff, rec.zp_eff), rec.fresh)

    def appended(self, i, names):
        for name in names:
            rec = self._records[i].get(name)
            if rec is not None:
                rec.fresh = False

    def demote(self, i, name):
        """Turn a coded tensor into the fp32 tensor it stands for (one dequantise launch with its record); a tensor planned
        but never written just loses its record.  The cache goes on as an fp32 cache for it."""
        rec = self._records[i].pop(name, None)
        held = self._tensor(i, name)
        if rec is None or held is None or rec.fresh:
            return
        full = ops.dequantize_kv_codes(held, rec.triple())
        if name in _SELF:
            j = _SELF.index(name)
            if j == 0:
                self._k[i] = full
            else:
                self._v[i] = full
            self._spare[i][j] = None
        else:
            pair = list(self._cross[i])
            pair[_CROSS.index(name)] = full
            self._cross[i] = tuple(pair)
        self._demoted.append((i, name))

    def coded(self):
        """(layer, name) of every tensor held as codes, name one of k, v, cross_k, cross_v."""
        return sorted((i, name) for i, recs in enumerate(self._records) for name, rec in recs.items() if not rec.fresh)

    def demoted(self):
        """(layer, name) of every tensor that was held as codes and has been demoted to fp32, in the order it happened."""
        return list(self._demoted)

    def rejected(self):
        """Elements the cache holds no code for (plus record mismatches), read from the device counter: a host sync."""
        return 0 if self._rejected is None else int(self._rejected.item())

    def nbytes(self):
        """Bytes of device (or host) memory the cache holds: buffers, partner buffers, cross-attention tensors, records and
        the counter."""
        held = [t for t in self._k + self._v if t is not None]
        held += [t for pair in self._spare for t in pair if t is not None]
        held += [t for pair in self._cross if pair is not None for t in pair]
        held += [t for t in (self._record_pairs, self._rejected) if t is not None]
        return sum(t.numel() * t.element_size() for t in held)

    # ---- what QuantizedBartAttention uses
    def append_targets(self, i, bsz, heads, head_dim, t, like, coded=(False, False)):
        """Destination buffers for a step of t tokens at layer i: (k_dst, v_dst, k_src, v_src, rows).  In place when no
        reorder is pending and the buffer has room, else the partner buffer (the kept prefix is copied through rows).
        ``coded``: whether a new buffer of k / of v holds codes (uint8) instead of fp32 words."""
        n, k, v, rows = self._len[i], self._k[i], self._v[i], self._rows[i]
        want = n + t
        if k is not None and rows is None and k.shape[2] >= want and k.shape[0] == bsz and k.is_contiguous():
            return k, v, None, None, None
        cap = max(want, self.capacity or 0, 2 * n)
        dst = []
        for spare, as_codes in zip(self._spare[i], coded):
            dtype = torch.uint8 if as_codes else like.dtype
            if spare is None or spare.shape[0] != bsz or spare.shape[2] < want or spare.dtype != dtype:
                spare = like.new_empty((bsz, heads, cap, head_dim), dtype=dtype)
            dst.append(spare)
        if k is None:
            return dst[0], dst[1], None, None, None
        return dst[0], dst[1], k[:, :, :n], v[:, :, :n], rows

    def commit(self, i, k, v, length):
        if k is not self._k[i]:
            for j, old in enumerate((self._k[i], self._v[i])):
                if old is not None and old.is_contiguous() and old.dim() == 4:
                    self._spare[i][j] = old
            self._k[i], self._v[i] = k, v
        self._len[i] = length
        self._rows[i] = None

    def past(self, i):
        """The self-attention (k, v) of layer i as fp32 [B, h, S, d] views, any pending reorder applied (eager form), or None."""
        if self._k[i] is None:
            return None
        self._materialise(i)
        n = self._len[i]
        return self._fp32(i, "k", self._k[i][:, :, :n]), self._fp32(i, "v", self._v[i][:, :, :n])

    def operands(self, i, n):
        """The self-attention (k, v) of layer i over its first n positions as attention takes them."""
        return self._operand(i, "k", self._k[i][:, :, :n]), self._operand(i, "v", self._v[i][:, :, :n])

    def cross_operands(self, i):
        return tuple(self._operand(i, name, t) for name, t in zip(_CROSS, self._cross[i]))

    def keep_cross_rows(self, i):
        """The cross-attention tensors of layer i were computed on the expanded encoder rows (a form the shared launches do
        not take): keep every cross_group-th row, the one copy per encoder row."""
        self._cross[i] = tuple(t[::self.cross_group].contiguous() for t in self._cross[i])

    def slot(self, i):
        return _CacheSlot(self, i)

    # ---- device-position mode
    def enter_device_position(self):
        """After the first step: the position moves to a device word and every layer gets both buffers of its pair at
        ``capacity``.  Needs every layer to hold contiguous [B, h, capacity, d] buffers of one length."""
        n = self._len[0]
        for i, (k, v) in enumerate(zip(self._k, self._v)):
            if (k is None or self._len[i] != n or k.dim() != 4 or not (k.is_contiguous() and v.is_contiguous())
                    or k.shape != v.shape or k.shape[2] != self.capacity):
                raise ValueError(f"layer {i} of the cache does not hold [B, h, capacity, d] buffers of length {n}")
            for j, t in enumerate((k, v)):
                spare = self._spare[i][j]
                if spare is None or spare.shape != t.shape or spare.dtype != t.dtype or not spare.is_contiguous():
                    self._spare[i][j] = torch.empty_like(t)
        k = self._k[0]
        self._rows_buf = torch.arange(k.shape[0], dtype=torch.int64, device=k.device)
        if self._rows[0] is not None:
            self._rows_buf.copy_(self._rows[0])
            self._rows = [self._rows_buf] * len(self._k)
        self._pos = torch.tensor([n], dtype=torch.int32, device=k.device)
        return self

    def positioned(self):
        return self._pos is not None

    def position(self):
        """The past length: an int, or in device-position mode the device word a step's launches read."""
        return self._len[0] if self._pos is None else self._pos

    def reorder_pending(self):
        return self._rows[0] is not None

    def at_targets(self, i):
        """(k_dst, v_dst, k_src, v_src, rows) of a single-token step in device-position mode: in place, or into the partner
        buffers with the prefix copied from the whole current buffers through the static row index."""
        if self._rows[i] is None:
            return self._k[i], self._v[i], None, None, None
        return self._spare[i][0], self._spare[i][1], self._k[i], self._v[i], self._rows_buf

    def commit_at(self, i, k, v, t=1):
        """Host bookkeeping of a device-position step of layer i (also for a replayed one: ``stepped``)."""
        if k is not self._k[i]:
            self._spare[i] = [self._k[i], self._v[i]]
            self._k[i], self._v[i] = k, v
        self._len[i] += t
        self._rows[i] = None

    def advance(self, t):
        """After the decoder's last layer: the device word follows (a launch of the step, so a captured step carries it)."""
        if self._pos is not None:
            self._pos.add_(t)

    def stepped(self):
        """A captured step was replayed: what its launches did, on the host side."""
        for i in range(len(self._k)):
            if self._rows[i] is None:
                self.commit_at(i, self._k[i], self._v[i])
            else:
                self.commit_at(i, *self._spare[i])

    def reorder_carried(self):
        """A captured step was replayed whose graph also carried the copy of the new row index into the static buffer
        (what ``reorder`` launches): the reorder is pending, on the host side.  No launch."""
        self._rows = [self._rows_buf] * len(self._k)

    def record_at(self, i, name, params):
        """The record pair of a coded tensor for a device-position append (None: an fp32 tensor).  Such a step cannot demote:
        parameters that differ from those of the first append are an error."""
        rec = self._records[i].get(name)
        if rec is None:
            return None
        if rec.fresh or _code_identity(params) != rec.identity:
            raise RuntimeError(f"the quantizer parameters of cache tensor {name} of layer {i} changed while its position "
                               "lives on the device")
        return rec.scale_eff, rec.zp_eff

    def grad_table(self, quantizer, rows):
        """decode_grad_table of a probabilities quantizer on the device, built once per (quantizer settings, rows)."""
        key = (rows, self.capacity, quantizer.param_mode, quantizer.quant_max, getattr(quantizer, "use_grad_scaling", False),
               getattr(quantizer, "numel_multiplier", 1), quantizer.ch_axis)
        table = self._tables.get(key)
        if table is None:
            table = self._tables[key] = decode_grad_table(quantizer, rows, self.capacity).to(self._pos.device)
        return table


class _CacheSlot:
    """One decoder layer's view of a QuantizedBartCache: the ``past_key_value`` a QuantizedBartAttention takes."""

    def __init__(self, cache, layer):
        self.cache, self.layer = cache, layer


class QuantizedBartLearnedPositionalEmbedding(QuantizedModule):
    def __init__(self, org_module, w_qconfig, a_qconfig, qoutput=True, backend="academic"):
        super().__init__(backend=backend)
        self.offset = 2
        self.qoutput = qoutput
        n, d = org_module.weight.shape
        plain = nn.Embedding(n, d)
        plain.weight.data = org_module.weight.data.clone()
        self.position_embeddings = Quantizer(plain, w_qconfig)

    def forward(self, input_ids_shape, past_key_values_length=0):
        seq_len = input_ids_shape[1]
        if isinstance(past_key_values_length, torch.Tensor):        # a device word (QuantizedBartCache in device-position mode)
            positions = past_key_values_length.to(torch.long) + torch.arange(seq_len, dtype=torch.long,
                                                                             device=past_key_values_length.device)
            return self.position_embeddings(positions + self.offset)
        positions = torch.arange(past_key_values_length, past_key_values_length + seq_len, dtype=torch.long,
                                 device=self.position_embeddings.weight.device)
        return self.position_embeddings(positions + self.offset)


class QuantizedBartAttention(QuantizedModule):
    def __init__(self, org_module, w_qconfig, a_qconfig, qoutput=True, backend="academic"):
        super().__init__(backend=backend)
        self.qoutput = qoutput
        self.embed_dim, self.num_heads, self.head_dim = org_module.embed_dim, org_module.num_heads, org_module.head_dim
        self.dropout = org_module.dropout
        self.scaling = self.head_dim ** -0.5
        self.is_decoder = org_module.is_decoder
        self.k_proj = Quantizer(org_module.k_proj, w_qconfig)
        self.v_proj = Quantizer(org_module.v_proj, w_qconfig)
        self.q_proj = Quantizer(org_module.q_proj, w_qconfig)
        self.out_proj = Quantizer(org_module.out_proj, w_qconfig)
        self.query_post_act_fake_quantize = Quantizer(None, a_qconfig)
        self.key_post_act_fake_quantize = Quantizer(None, a_qconfig)
        self.value_post_act_fake_quantize = Quantizer(None, a_qconfig)
        self.attention_probs_post_act_fake_quantize = Quantizer(None, a_qconfig)
        self.context_post_act_fake_quantize = Quantizer(None, a_qconfig)
        if qoutput:
            self.out_proj_post_act_fake_quantize = Quantizer(None, a_qconfig)

    def _cached_qkv(self, slot, hidden_states, key_value_states, observation_mask, expanded=False):
        """q / k / v of a decoding step (quant_bart.py:156-198): self-attention fake-quantizes the step's keys / values and
        appends them to the cache, cross-attention quantizes the encoder's once and reuses them.  k / v come back as
        [B, h, S, d] views of the cache buffers -- as _CodedTensor where the cache holds them as integer codes."""
        cache, i, heads, d = slot.cache, slot.layer, self.num_heads, self.head_dim
        bsz, t, _ = hidden_states.shape
        xq = self.q_proj(hidden_states) * self.scaling
        qs = (self.query_post_act_fake_quantize, self.key_post_act_fake_quantize, self.value_post_act_fake_quantize)
        if key_value_states is not None:
            if cache._cross[i] is not None:
                return (split_heads_fake_quant(qs[0], xq, heads, observation_mask),) + cache.cross_operands(i)
            if cache.cross_group > 1 and not expanded:
                return self._shared_cross_qkv(slot, xq, hidden_states, key_value_states, observation_mask)
            xk, xv = self.k_proj(key_value_states), self.v_proj(key_value_states)
            s = xk.shape[1]
            ps = [kv_site_params(q, x) for q, x in zip(qs, (xq, xk, xv))] if cache.codes else None
            coded = cache.plan(i, ("cross_k", "cross_v"), ps[1:], (xk, xv), heads) if cache.codes else ()
            if any(coded):
                ys = [x.new_empty((bsz, heads, s, d), dtype=torch.uint8 if c else x.dtype) for x, c in zip((xk, xv), coded)]
                out = None if any(p is None for p in ps) else kv_append_codes_fake_quant(
                    [(qs[0], ps[0], xq, xq.new_empty((bsz, heads, t, d)), 0, None, None, None, False),
                     (qs[1], ps[1], xk, ys[0], 0, None, None) + cache.record(i, "cross_k"),
                     (qs[2], ps[2], xv, ys[1], 0, None, None) + cache.record(i, "cross_v")], heads, cache._rejected)
                if out is not None:
                    cache._cross[i] = (out[1], out[2])
                    cache.appended(i, ("cross_k", "cross_v"))
                    return (out[0],) + cache.cross_operands(i)
                cache.demote(i, "cross_k")
                cache.demote(i, "cross_v")
            out = kv_append_fake_quant([(qs[0], xq, xq.new_empty((bsz, heads, t, d)), 0, None, None),
                                        (qs[1], xk, xk.new_empty((bsz, heads, s, d)), 0, None, None),
                                        (qs[2], xv, xv.new_empty((bsz, heads, s, d)), 0, None, None)], heads)
            if out is None:
                out = [split_heads_fake_quant(q, x, heads, observation_mask) for q, x in zip(qs, (xq, xk, xv))]
            cache._cross[i] = (out[1], out[2])
            return tuple(out)
        xk, xv = self.k_proj(hidden_states), self.v_proj(hidden_states)
        n = cache.get_seq_length(i)
        ps = [kv_site_params(q, x) for q, x in zip(qs, (xq, xk, xv))] if cache.codes else None
        coded = cache.plan(i, ("k", "v"), ps[1:], (xk, xv), heads) if cache.codes else ()
        if any(coded):
            kd, vd, ks, vs, rows = cache.append_targets(i, bsz, heads, d, t, xk, coded)
            out = None if any(p is None for p in ps) else kv_append_codes_fake_quant(
                [(qs[0], ps[0], xq, xq.new_empty((bsz, heads, t, d)), 0, None, None, None, False),
                 (qs[1], ps[1], xk, kd, n, ks, rows) + cache.record(i, "k"),
                 (qs[2], ps[2], xv, vd, n, vs, rows) + cache.record(i, "v")], heads, cache._rejected)
            if out is not None:
                cache.commit(i, kd, vd, n + t)
                cache.appended(i, ("k", "v"))
                return (out[0],) + cache.operands(i, n + t)
            cache.demote(i, "k")          # a geometry the coded append does not take: this layer goes on in fp32
            cache.demote(i, "v")
        kd, vd, ks, vs, rows = cache.append_targets(i, bsz, heads, d, t, xk)
        out = kv_append_fake_quant([(qs[0], xq, xq.new_empty((bsz, heads, t, d)), 0, None, None),
                                    (qs[1], xk, kd, n, ks, rows), (qs[2], xv, vd, n, vs, rows)], heads)
        if out is not None:
            cache.commit(i, kd, vd, n + t)
            return out[0], kd[:, :, :n + t], vd[:, :, :n + t]
        # the reference's eager form: quantizer, head split, then index_select (pending reorder) and torch.cat
        q, k, v = [split_heads_fake_quant(q, x, heads, observation_mask) for q, x in zip(qs, (xq, xk, xv))]
        past = cache.past(i)
        if past is not None:
            k, v = torch.cat([past[0], k], dim=2), torch.cat([past[1], v], dim=2)
        cache.commit(i, k, v, n + t)
        return q, k, v

    def _shared_cross_qkv(self, slot, xq, hidden_states, key_value_states, observation_mask):
        """The first cross-attention step over a cache with cross_group = G > 1: ``key_value_states`` has B rows, the step B * G.
        Keys / values are projected and quantized on the B rows, in a launch of their own beside the query's.  Their LSQ /
        LSQ+ grad factor is that of the [B * G, S, h*d] tensor they stand for -- it enters the last bits of the effective
        scale -- so the words, and under codes the bytes and records, are those the unshared form stores.  Where a launch
        does not take the step, the unshared computation runs on the expanded rows and one copy per encoder row is kept."""
        cache, i, heads, d = slot.cache, slot.layer, self.num_heads, self.head_dim
        group = cache.cross_group
        bsz, t, _ = xq.shape
        b = key_value_states.shape[0]
        if b * group != bsz:
            raise ValueError(f"a cache with cross_group={group} takes encoder states of {bsz // group} rows for {bsz} decoder "
                             f"rows, got {b}")
        qs = (self.query_post_act_fake_quantize, self.key_post_act_fake_quantize, self.value_post_act_fake_quantize)
        xk, xv = self.k_proj(key_value_states), self.v_proj(key_value_states)
        s = xk.shape[1]
        numel = xk.numel() * group
        kv = None
        ps = [kv_site_params(qs[1], xk, numel), kv_site_params(qs[2], xv, numel)]
        coded = cache.plan(i, _CROSS, ps, (xk, xv), heads) if cache.codes else ()
        if any(coded) and None not in ps:
            ys = [x.new_empty((b, heads, s, d), dtype=torch.uint8 if c else x.dtype) for x, c in zip((xk, xv), coded)]
            kv = kv_append_codes_fake_quant([(qs[1], ps[0], xk, ys[0], 0, None, None) + cache.record(i, "cross_k"),
                                             (qs[2], ps[1], xv, ys[1], 0, None, None) + cache.record(i, "cross_v")],
                                            heads, cache._rejected)
            if kv is not None:
                cache.appended(i, _CROSS)
        if kv is None:
            if any(coded):
                cache.demote(i, "cross_k")
                cache.demote(i, "cross_v")
            kv = kv_append_fake_quant([(qs[1], xk, xk.new_empty((b, heads, s, d)), 0, None, None),
                                       (qs[2], xv, xv.new_empty((b, heads, s, d)), 0, None, None)], heads, numels=(numel, numel))
        if kv is None:
            out = self._cached_qkv(slot, hidden_states, key_value_states.repeat_interleave(group, dim=0), observation_mask,
                                   expanded=True)
            cache.keep_cross_rows(i)
            return (out[0],) + cache.cross_operands(i)
        cache._cross[i] = (kv[0], kv[1])
        q = kv_append_fake_quant([(qs[0], xq, xq.new_empty((bsz, heads, t, d)), 0, None, None)], heads)
        if q is None:
            q = [split_heads_fake_quant(qs[0], xq, heads, observation_mask)]
        return (q[0],) + cache.cross_operands(i)

    def forward(self, hidden_states, key_value_states=None, attention_mask=None, observation_mask=None,
                past_key_value=None, cross_group=1):
        """``past_key_value``: None (no cache; returns the output alone, as before) or a layer slot of a
        QuantizedBartCache (QuantizedBartCache.slot(i)), which this call extends: returns (output, past_key_value).
        ``cross_group`` = G > 1 (cross-attention without a cache; score()): ``key_value_states`` and ``attention_mask`` have
        one row per G rows of ``hidden_states`` (_cross_shared); ``self.last_cross_shared`` then says whether the keys and
        values were held once."""
        bsz, tgt_len, _ = hidden_states.shape
        heads = self.num_heads
        if cross_group > 1:
            if past_key_value is not None or key_value_states is None:
                raise ValueError("cross_group is for cross-attention without a cache (a cache has a cross_group of its own)")
            return self._cross_shared(hidden_states, key_value_states, attention_mask, observation_mask, cross_group)
        if past_key_value is not None:
            if key_value_states is None and past_key_value.cache.positioned():
                return self._step_at(past_key_value, hidden_states, attention_mask, observation_mask), past_key_value
            q, k, v = self._cached_qkv(past_key_value, hidden_states, key_value_states, observation_mask)
            cache = past_key_value.cache
            if key_value_states is not None and cache.cross_group > 1:
                out = self._attend_shared(q, k, v, bsz, tgt_len, attention_mask, observation_mask, cache.cross_group,
                                          cache.cross_one_launch)
            else:
                out = self._attend(q, k, v, bsz, tgt_len, attention_mask, observation_mask, cached=True)
            return out, past_key_value
        source = hidden_states if key_value_states is None else key_value_states
        xq, xk, xv = self.q_proj(hidden_states) * self.scaling, self.k_proj(source), self.v_proj(source)
        # self-attention in the plain quantising state: the three head-split sites in one launch (same bits); cross-attention
        # (keys / values of another length) and every other state: site by site
        fused = qkv_heads_fake_quant((self.query_post_act_fake_quantize, self.key_post_act_fake_quantize, self.value_post_act_fake_quantize),
                                     (xq, xk, xv), heads) if xk.shape == xq.shape else None
        if fused is not None:
            q, k, v = fused
        else:
            q = split_heads_fake_quant(self.query_post_act_fake_quantize, xq, heads, observation_mask)
            k = split_heads_fake_quant(self.key_post_act_fake_quantize, xk, heads, observation_mask)
            v = split_heads_fake_quant(self.value_post_act_fake_quantize, xv, heads, observation_mask)
        return self._attend(q, k, v, bsz, tgt_len, attention_mask, observation_mask)

    def _cross_shared(self, hidden_states, key_value_states, attention_mask, observation_mask, group):
        """Teacher-forced cross-attention of [B * G, T, H] decoder states over [B, S, H] encoder states and a [B, 1, T, S] mask
        that the G rows of an input share.  Keys / values are projected on the B rows and their two sites run as one launch
        into [B, h, S, d] tensors, with the LSQ / LSQ+ grad factor of the [B * G, S, h*d] tensor they stand for, as
        _shared_cross_qkv does for a cache: the words are those the expanded form computes.  Where that launch does not take
        the layer, the layer runs on expanded rows as without a group."""
        bsz, tgt_len, _ = hidden_states.shape
        heads, d = self.num_heads, self.head_dim
        b = key_value_states.shape[0]
        if b * group != bsz:
            raise ValueError(f"cross_group={group} takes encoder states of {bsz // group} rows for {bsz} decoder rows, got {b}")
        xk, xv = self.k_proj(key_value_states), self.v_proj(key_value_states)
        s = xk.shape[1]
        numel = xk.numel() * group
        kv = kv_append_fake_quant([(self.key_post_act_fake_quantize, xk, xk.new_empty((b, heads, s, d)), 0, None, None),
                                   (self.value_post_act_fake_quantize, xv, xv.new_empty((b, heads, s, d)), 0, None, None)],
                                  heads, numels=(numel, numel))
        self.last_cross_shared = kv is not None
        if kv is None:
            if attention_mask is not None:
                attention_mask = attention_mask.repeat_interleave(group, dim=0)
            return self.forward(hidden_states, key_value_states.repeat_interleave(group, dim=0), attention_mask, observation_mask)
        q = split_heads_fake_quant(self.query_post_act_fake_quantize, self.q_proj(hidden_states) * self.scaling, heads,
                                   observation_mask)
        return self._attend(q, kv[0], kv[1], bsz, tgt_len, attention_mask, observation_mask, group=group)

    def _step_at(self, slot, hidden_states, attention_mask, observation_mask):
        """Self-attention of a single-token step over a cache in device-position mode: the append and the attention read the
        position in their launches (the _at forms), so the same two launches serve every step -- and a captured graph of
        them.  They write and compute the words of _cached_qkv + _attend with the one-launch attention at that position.
        There is no eager form to fall back to: a launch that refuses is an error."""
        cache, i, heads, d = slot.cache, slot.layer, self.num_heads, self.head_dim
        bsz, t, _ = hidden_states.shape
        if t != 1 or attention_mask is not None:
            raise RuntimeError("a cache in device-position mode takes single-token steps without a decoder mask")
        xq = self.q_proj(hidden_states) * self.scaling
        xk, xv = self.k_proj(hidden_states), self.v_proj(hidden_states)
        qs = (self.query_post_act_fake_quantize, self.key_post_act_fake_quantize, self.value_post_act_fake_quantize)
        ps = [kv_site_params(q, x) for q, x in zip(qs, (xq, xk, xv))]
        if any(p is None for p in ps):
            raise RuntimeError("device-position step: a q / k / v site does not take the one-launch append")
        recs = [cache.record_at(i, name, p) for name, p in zip(_SELF, ps[1:])]
        if (recs[0] is None) != (recs[1] is None):
            raise RuntimeError("device-position step: keys and values must both be held as codes, or both as fp32 words")
        kd, vd, ks, vs, rows = cache.at_targets(i)
        qy = xq.new_empty((bsz, heads, t, d))
        if recs[0] is not None:
            out = kv_append_codes_fake_quant([(qs[0], ps[0], xq, qy, 0, None, None, None, False),
                                              (qs[1], ps[1], xk, kd, None, ks, rows, recs[0], False),
                                              (qs[2], ps[2], xv, vd, None, vs, rows, recs[1], False)], heads, cache._rejected,
                                             pos=cache._pos)
            codes = (cache._records[i]["k"].triple(), cache._records[i]["v"].triple(), cache._rejected)
        else:
            out = kv_append_fake_quant([(qs[0], xq, qy, 0, None, None), (qs[1], xk, kd, None, ks, rows),
                                        (qs[2], xv, vd, None, vs, rows)], heads, pos=cache._pos)
            codes = None
        if out is None:
            raise RuntimeError("device-position step: the one-launch append refused the step")
        cache.commit_at(i, kd, vd, t)
        probs_q = self.attention_probs_post_act_fake_quantize
        ctx = decode_attention_at_fake_quant(probs_q, self.context_post_act_fake_quantize, out[0], kd, vd, cache._pos, t,
                                             cache.capacity, cache.grad_table(probs_q, bsz * heads),
                                             dropout=(self.dropout, self.training), codes=codes)
        if ctx is None:
            raise RuntimeError("device-position step: the one-launch attention refused the step")
        return self._project(ctx, observation_mask)

    def _attend_shared(self, q, k, v, bsz, tgt_len, attention_mask, observation_mask, group, force):
        """_attend for [B * G, h, T, d] q over [B, h, S, d] k / v and a [B, 1, T, S] mask that the G rows of an encoder row
        share: a single-token step as ONE launch that reads K and V once for (up to 8 of) the rows that share them.  A call
        that launch does not take -- several tokens (a prefill), a refusal -- goes to _attend with the group: the grouped
        whole-sequence launch where it takes the call, else k, v and the mask expanded."""
        if tgt_len == 1:
            both = isinstance(k, _CodedTensor) and isinstance(v, _CodedTensor)
            kk, vv = ((k.codes, v.codes) if both else (x.float() if isinstance(x, _CodedTensor) else x for x in (k, v)))
            out = decode_attention_shared_fake_quant(self.attention_probs_post_act_fake_quantize,
                                                     self.context_post_act_fake_quantize, q, kk, vv, group, attention_mask,
                                                     dropout=(self.dropout, self.training),
                                                     codes=(k.record, v.record, k.rejected) if both else None, force=force)
            if out is not None:
                return self._project(out, observation_mask)
        return self._attend(q, k, v, bsz, tgt_len, attention_mask, observation_mask, cached=True, group=group)

    def _attend(self, q, k, v, bsz, tgt_len, attention_mask, observation_mask, cached=False, group=1):
        """[B, h, T, d] q and [B, h, S, d] k / v (dense, or views of a cache buffer) -> the block's output.  ``cached``: a
        call of the cached path, whose single-token steps have a one-launch form (util_layernorm.FUSE_DECODE_ATTENTION).
        k / v held as integer codes (_CodedTensor) go to that form as they are when both are; everything else -- one of the
        two in fp32, the switch off, several tokens, dropout, a length the kernel does not take -- sees them dequantised.
        ``group`` = G > 1: q has G rows per row of k, v and the mask.  Several tokens go to the one-launch forms with the
        group (the words of the call on expanded k, v and mask, by the kernels' contract); what they do not take, and every
        other form, runs on k, v and the mask expanded here."""
        if group > 1:
            k, v = (x.float() if isinstance(x, _CodedTensor) else x for x in (k, v))
            if tgt_len > 1:
                out = attention_sequence_fake_quant(self.query_post_act_fake_quantize, self.key_post_act_fake_quantize,
                                                    self.value_post_act_fake_quantize, self.attention_probs_post_act_fake_quantize,
                                                    self.context_post_act_fake_quantize, q, k, v, attention_mask,
                                                    dropout=(self.dropout, self.training), group=group)
                if out is not None:
                    return self._project(out, observation_mask)
            k, v = k.repeat_interleave(group, dim=0), v.repeat_interleave(group, dim=0)
            if attention_mask is not None:
                attention_mask = attention_mask.repeat_interleave(group, dim=0)
        codes = None
        if isinstance(k, _CodedTensor) and isinstance(v, _CodedTensor) and cached and tgt_len == 1:
            codes = (k.record, v.record, k.rejected)
        else:
            k, v = (x.float() if isinstance(x, _CodedTensor) else x for x in (k, v))
        if cached and tgt_len == 1:
            out = decode_attention_fake_quant(self.attention_probs_post_act_fake_quantize, self.context_post_act_fake_quantize,
                                              q, k.codes if codes else k, v.codes if codes else v, attention_mask,
                                              dropout=(self.dropout, self.training), codes=codes)
            if out is not None:
                return self._project(out, observation_mask)
            if codes:
                k, v = k.float(), v.float()
        if tgt_len > 1:
            # several query tokens -- the encoder, a teacher-forced decoder, cross-attention, a prefill: one launch, on the
            # integer codes of q / k / v (keys and values from a cache included: they are their quantizers' outputs) under
            # FUSE_ATTENTION_INT, else in fp32 under FUSE_ATTENTION
            out = attention_sequence_fake_quant(self.query_post_act_fake_quantize, self.key_post_act_fake_quantize,
                                                self.value_post_act_fake_quantize, self.attention_probs_post_act_fake_quantize,
                                                self.context_post_act_fake_quantize, q, k, v, attention_mask,
                                                dropout=(self.dropout, self.training))
            if out is not None:
                return self._project(out, observation_mask)
        proj = (bsz * self.num_heads, -1, self.head_dim)
        q, k, v = q.view(*proj), k.view(*proj), v.view(*proj)
        w = torch.bmm(q, k.transpose(1, 2))
        # [B*h, T, S] scores + [B, 1, T, S] mask -> softmax -> dropout -> probs quantizer (quant_bart.py:232-256); one
        # launch under FUSE_SOFTMAX
        probs = attention_probs_fake_quant(self.attention_probs_post_act_fake_quantize, w, attention_mask,
                                           dropout=(self.dropout, self.training), observation_mask=observation_mask,
                                           seq_pos=2, heads=self.num_heads)
        out = merge_heads_fake_quant(self.context_post_act_fake_quantize,
                                     torch.bmm(probs, v).view(bsz, self.num_heads, tgt_len, self.head_dim), observation_mask)
        return self._project(out, observation_mask)

    def _project(self, out, observation_mask):
        out = self.out_proj(out)
        if self.qoutput:
            out = self.out_proj_post_act_fake_quantize(out, observation_mask, 1)
        return out


class QuantizedBartEncoderLayer(QuantizedModule):
    def __init__(self, org_module, w_qconfig, a_qconfig, qoutput=True, backend="academic"):
        super().__init__(backend)
        self.qoutput = qoutput
        self.embed_dim = org_module.embed_dim
        self.self_attn = QuantizedBartAttention(org_module.self_attn, w_qconfig, a_qconfig, qoutput=False, backend=backend)
        self.before_self_attn_layer_norm_residual = GammaResidual()
        self.self_attn_layer_norm = QuantizedLayerNorm(org_module.self_attn_layer_norm, w_qconfig, a_qconfig,
                                                       qoutput=True, backend=backend)
        self.dropout = org_module.dropout
        self.fc1 = Quantizer(org_module.fc1, w_qconfig)
        self.activation_fn = org_module.activation_fn
        self.activation_dropout = org_module.activation_dropout
        self.fc1_act_fn_post_act_fake_quantize = Quantizer(None, a_qconfig)
        self.fc2 = Quantizer(org_module.fc2, w_qconfig)
        self.before_final_layer_norm_residual = GammaResidual()
        self.final_layer_norm = QuantizedLayerNorm(org_module.final_layer_norm, w_qconfig, a_qconfig, qoutput=qoutput,
                                                   backend=backend)

    def _drop(self, x, p):
        return nn.functional.dropout(x, p=p, training=self.training)

    def forward(self, hidden_states, attention_mask, observation_mask=None):
        residual = hidden_states
        h = self._drop(self.self_attn(hidden_states, attention_mask=attention_mask, observation_mask=observation_mask),
                       self.dropout)
        h = residual_layernorm(self.before_self_attn_layer_norm_residual, self.self_attn_layer_norm, residual, h, observation_mask)
        residual = h
        if self.training and self.activation_dropout > 0:
            h = self._drop(self.activation_fn(self.fc1(h)), self.activation_dropout)
            h = self.fc1_act_fn_post_act_fake_quantize(h, observation_mask, 1)
        else:
            h = activation_fake_quant(self.activation_fn, self.fc1_act_fn_post_act_fake_quantize, self.fc1(h), observation_mask)
        h = self._drop(self.fc2(h), self.dropout)
        return residual_layernorm(self.before_final_layer_norm_residual, self.final_layer_norm, residual, h, observation_mask)


class QuantizedBartDecoderLayer(QuantizedModule):
    def __init__(self, org_module, w_qconfig, a_qconfig, qoutput=True, backend="academic"):
        super().__init__(backend)
        self.qoutput = qoutput
        self.embed_dim = org_module.embed_dim
        self.self_attn = QuantizedBartAttention(org_module.self_attn, w_qconfig, a_qconfig, qoutput=False, backend=backend)
        self.dropout = org_module.dropout
        self.before_self_attn_layer_norm_residual = GammaResidual()
        self.self_attn_layer_norm = QuantizedLayerNorm(org_module.self_attn_layer_norm, w_qconfig, a_qconfig,
                                                       qoutput=True, backend=backend)
        self.encoder_attn = QuantizedBartAttention(org_module.encoder_attn, w_qconfig, a_qconfig, qoutput=False,
                                                   backend=backend)
        self.before_encoder_attn_layer_norm_residual = GammaResidual()
        self.encoder_attn_layer_norm = QuantizedLayerNorm(org_module.encoder_attn_layer_norm, w_qconfig, a_qconfig,
                                                          qoutput=True, backend=backend)
        self.fc1 = Quantizer(org_module.fc1, w_qconfig)
        self.activation_fn = org_module.activation_fn
        self.activation_dropout = org_module.activation_dropout
        self.fc1_act_fn_post_act_fake_quantize = Quantizer(None, a_qconfig)
        self.fc2 = Quantizer(org_module.fc2, w_qconfig)
        self.before_final_layer_norm_residual = GammaResidual()
        self.final_layer_norm = QuantizedLayerNorm(org_module.final_layer_norm, w_qconfig, a_qconfig, qoutput=qoutput,
                                                   backend=backend)

    def _drop(self, x, p):
        return nn.functional.dropout(x, p=p, training=self.training)

    def forward(self, hidden_states, attention_mask=None, encoder_hidden_states=None, encoder_attention_mask=None,
                observation_mask=None, past_key_value=None, cross_group=1):
        """``past_key_value``: None, or this layer's slot of a QuantizedBartCache (extended in place).  ``cross_group``: the
        rows of ``hidden_states`` per row of the encoder's states and mask (QuantizedBartAttention.forward; no cache)."""
        def attn(module, x, **kw):
            if past_key_value is None:
                return module(x, observation_mask=observation_mask, **kw)
            return module(x, observation_mask=observation_mask, past_key_value=past_key_value, **kw)[0]
        residual = hidden_states
        h = self._drop(attn(self.self_attn, hidden_states, attention_mask=attention_mask), self.dropout)
        h = residual_layernorm(self.before_self_attn_layer_norm_residual, self.self_attn_layer_norm, residual, h, observation_mask)
        if encoder_hidden_states is not None:
            residual = h
            h = self._drop(attn(self.encoder_attn, h, key_value_states=encoder_hidden_states,
                                attention_mask=encoder_attention_mask,
                                **(dict(cross_group=cross_group) if cross_group > 1 else {})), self.dropout)
            h = residual_layernorm(self.before_encoder_attn_layer_norm_residual, self.encoder_attn_layer_norm, residual, h, observation_mask)
        residual = h
        if self.training and self.activation_dropout > 0:
            h = self._drop(self.activation_fn(self.fc1(h)), self.activation_dropout)
            h = self.fc1_act_fn_post_act_fake_quantize(h, observation_mask, 1)
        else:
            h = activation_fake_quant(self.activation_fn, self.fc1_act_fn_post_act_fake_quantize, self.fc1(h), observation_mask)
        h = self._drop(self.fc2(h), self.dropout)
        return residual_layernorm(self.before_final_layer_norm_residual, self.final_layer_norm, residual, h, observation_mask)


class _BartStack(QuantizedModule):
    """Shared front end of encoder and decoder: token + position embeddings -> LayerNorm(+quantizer)."""

    layer_cls = None

    def __init__(self, org_module, w_qconfig, a_qconfig, qoutput=True, backend="academic"):
        super().__init__(backend=backend)
        self.qoutput = qoutput
        self.config = org_module.config
        self.dropout = org_module.dropout
        self.layerdrop = org_module.layerdrop
        self.padding_idx = org_module.padding_idx
        self.embed_scale = _embed_scale(org_module)
        self.embed_tokens = Quantizer(_plain_embedding(org_module.embed_tokens), w_qconfig)
        self.embed_positions = QuantizedBartLearnedPositionalEmbedding(org_module.embed_positions, w_qconfig, a_qconfig,
                                                                       qoutput=False, backend=backend)
        self.layernorm_embedding = QuantizedLayerNorm(org_module.layernorm_embedding, w_qconfig, a_qconfig, qoutput=True,
                                                      backend=backend)
        n = len(org_module.layers)
        self.layers = nn.ModuleList(
            self.layer_cls(org_module.layers[i], w_qconfig, a_qconfig, qoutput=(True if i != n - 1 else qoutput),
                           backend=backend) for i in range(n))

    def _embed(self, input_ids, observation_mask, past=0):
        x = self.embed_tokens(input_ids) * self.embed_scale + self.embed_positions(input_ids.shape, past)
        x = self.layernorm_embedding(x, observation_mask)
        return nn.functional.dropout(x, p=self.dropout, training=self.training)


class QuantizedBartEncoder(_BartStack):
    layer_cls = QuantizedBartEncoderLayer

    def forward(self, input_ids, attention_mask=None, observation_mask=None):
        h = self._embed(input_ids, observation_mask)
        mask = _expand_mask(attention_mask, h.dtype) if attention_mask is not None else None
        for layer in self.layers:
            h = layer(h, mask, observation_mask=observation_mask)
        return h


class QuantizedBartDecoder(_BartStack):
    layer_cls = QuantizedBartDecoderLayer

    def forward(self, input_ids, attention_mask=None, encoder_hidden_states=None, encoder_attention_mask=None,
                observation_mask=None, past_key_values=None, use_cache=False, cross_group=1):
        """Without ``use_cache`` / ``past_key_values``: the hidden states.  With either: (hidden states, cache), the cache a
        QuantizedBartCache (``past_key_values`` may also be the reference's tuple of per-layer tensors; positions and the
        causal mask start after its length, quant_bart.py:774-787) extended by this step.  ``attention_mask`` then covers
        past + new positions.  ``cross_group`` = G > 1, without a cache: ``input_ids`` has G rows per row of
        ``encoder_hidden_states`` and ``encoder_attention_mask``, rows b * G .. b * G + G - 1 for encoder row b (a cache
        says the same with its own ``cross_group``)."""
        bsz, tgt_len = input_ids.shape
        cache = None
        if use_cache or past_key_values is not None:
            if cross_group != 1:
                raise ValueError("cross_group is for a decoder without a cache; give the cache its cross_group")
            cache = QuantizedBartCache.wrap(past_key_values, len(self.layers))
        past = cache.get_seq_length() if cache is not None else 0
        h = self._embed(input_ids, observation_mask, cache.position() if cache is not None else 0)
        mask = _causal_mask(bsz, tgt_len, h.dtype, h.device, past) if tgt_len > 1 else None
        if attention_mask is not None:
            pad = _expand_mask(attention_mask, h.dtype, tgt_len=tgt_len)
            mask = pad if mask is None else pad + mask
        enc_mask = None
        if encoder_hidden_states is not None and encoder_attention_mask is not None:
            enc_mask = _expand_mask(encoder_attention_mask, h.dtype, tgt_len=tgt_len)
        for i, layer in enumerate(self.layers):
            h = layer(h, attention_mask=mask, encoder_hidden_states=encoder_hidden_states,
                      encoder_attention_mask=enc_mask, observation_mask=observation_mask,
                      past_key_value=cache.slot(i) if cache is not None else None,
                      **(dict(cross_group=cross_group) if cross_group > 1 else {}))
        if cache is not None:
            cache.advance(tgt_len)
        return h if cache is None else (h, cache)


class QuantizedBartModel(QuantizedModule):
    def __init__(self, org_module, w_qconfig, a_qconfig, qoutput=True, backend="academic"):
        super().__init__(backend=backend)
        self.qoutput = qoutput
        self.config = org_module.config
        self.shared = Quantizer(_plain_embedding(org_module.shared), w_qconfig)
        self.encoder = QuantizedBartEncoder(org_module.encoder, w_qconfig, a_qconfig, qoutput=True, backend=backend)
        self.decoder = QuantizedBartDecoder(org_module.decoder, w_qconfig, a_qconfig, qoutput=qoutput, backend=backend)

    def get_encoder(self):
        return self.encoder

    def get_decoder(self):
        return self.decoder

    def forward(self, input_ids=None, attention_mask=None, decoder_input_ids=None, decoder_attention_mask=None,
                observation_mask=None, decoder_observation_mask=None, encoder_outputs=None, past_key_values=None,
                use_cache=False, cross_group=1):
        """(decoder states, encoder states); with ``use_cache`` or ``past_key_values``: (decoder states, cache, encoder
        states).  ``encoder_outputs``: the encoder states (a tensor, or a tuple / ModelOutput whose first entry they are),
        which skips the encoder.  ``cross_group``: QuantizedBartDecoder.forward's."""
        if decoder_input_ids is None:
            decoder_input_ids = shift_tokens_right(input_ids, self.config.pad_token_id, self.config.decoder_start_token_id)
        if encoder_outputs is None:
            enc = self.encoder(input_ids, attention_mask=attention_mask, observation_mask=observation_mask)
        else:
            enc = encoder_outputs if isinstance(encoder_outputs, torch.Tensor) else encoder_outputs[0]
        caching = use_cache or past_key_values is not None
        dec = self.decoder(decoder_input_ids, attention_mask=decoder_attention_mask, encoder_hidden_states=enc,
                           encoder_attention_mask=attention_mask, observation_mask=decoder_observation_mask,
                           **(dict(past_key_values=past_key_values, use_cache=True) if caching else {}),
                           **(dict(cross_group=cross_group) if cross_group != 1 else {}))
        return (dec[0], dec[1], enc) if caching else (dec, enc)


class QuantizedBartForConditionalGeneration(QuantizedModule):
    def __init__(self, org_module, w_qconfig, a_qconfig, qoutput=True, backend="academic", is_remove_padding=False):
        super().__init__(backend)
        self.is_remove_padding = is_remove_padding
        self.config = org_module.config
        self.qoutput = qoutput
        self.model = QuantizedBartModel(org_module.model, w_qconfig, a_qconfig, qoutput=True, backend=backend)
        self.lm_head = Quantizer(org_module.lm_head, w_qconfig)
        self.register_buffer("final_logits_bias", org_module.final_logits_bias.clone())
        self.main_input_name = getattr(org_module, "main_input_name", "input_ids")
        self.generation_config = getattr(org_module, "generation_config", None)     # generate()'s defaults

    def get_encoder(self):
        return self.model.get_encoder()

    def get_decoder(self):
        return self.model.get_decoder()

    def forward(self, input_ids=None, attention_mask=None, decoder_input_ids=None, decoder_attention_mask=None,
                labels=None, encoder_outputs=None, past_key_values=None, use_cache=None, cross_group=1, **unused):
        """(logits, encoder states) -- [loss first with labels].  With ``use_cache=True`` (or ``past_key_values`` given and
        ``use_cache`` not False): (logits, past_key_values, encoder states), the reference's return_dict=False order; the
        cache is a QuantizedBartCache.  ``labels`` turn the cache off (quant_bart.py:1076-1082).  Unlike the reference,
        ``use_cache`` does not default to config.use_cache: a plain call returns what it always did.  ``cross_group`` = G > 1
        (no cache): the decoder's inputs have G rows per row of the encoder's states and of ``attention_mask``
        (QuantizedBartDecoder.forward)."""
        obs = dec_obs = None
        if self.is_remove_padding:                      # quant_bart.py:1064-1072
            obs = attention_mask.sum(1)
            dec_obs = obs if decoder_attention_mask is None else decoder_attention_mask.sum(1)
            rows = None if decoder_input_ids is None else decoder_input_ids.shape[0]
            if decoder_attention_mask is None and rows and rows != obs.shape[0] and rows % obs.shape[0] == 0:
                dec_obs = obs.repeat_interleave(rows // obs.shape[0])   # several decoder rows per encoder row (cross_group)
        if labels is not None:
            use_cache = False
            if decoder_input_ids is None:
                decoder_input_ids = shift_tokens_right(labels, self.config.pad_token_id, self.config.decoder_start_token_id)
        caching = use_cache if use_cache is not None else past_key_values is not None
        out = self.model(input_ids, attention_mask, decoder_input_ids, decoder_attention_mask,
                         observation_mask=obs, decoder_observation_mask=dec_obs, encoder_outputs=encoder_outputs,
                         **(dict(past_key_values=past_key_values, use_cache=caching)
                            if caching or past_key_values is not None else {}),
                         **(dict(cross_group=cross_group) if cross_group != 1 else {}))
        logits = self.lm_head(out[0]) + self.final_logits_bias
        rest = (out[1], out[2]) if caching else (out[-1],)
        info = None
        if labels is not None:
            self.last_lm_loss = info = LmLossInfo()
        return with_loss(lm_loss(logits, labels, self.config.vocab_size, info), (logits,) + rest)

    @torch.no_grad()
    def score(self, input_ids, labels, attention_mask=None, num_candidates=1, ignore_index=-100, share_cross_kv=None):
        """How likely the model finds GIVEN target sequences, teacher-forced: (token_logprobs [B * n, T] fp32, the
        log-probability of every label under the model's own distribution -- not the warped one of sample()'s
        ``return_logprobs`` -- and 0 where the label is ``ignore_index``; sequence_logprob [B * n], their sum per row in
        position order; lengths [B * n] int64, the scored positions per row).  ``labels``: int64 [B * n, T] with the
        ``n = num_candidates`` candidates of input b at rows b * n .. b * n + n - 1, the layout of ``sample(num_samples=n)``.
        The encoder runs once, on the B inputs; its states and the attention mask are expanded with repeat_interleave(n);
        the decoder's inputs are shift_tokens_right(labels).  On the GPU the logits go through ops.token_logprob
        (csrc/token_logprob.hip) whatever set_fast_lm_loss says, on the CPU through losses.token_logprob_torch.  Raises
        ValueError for a label outside the vocabulary (the kernel counts them; the count is read once, at the end).
        ``share_cross_kv`` (None: the package switch, set_share_cross_kv): neither the encoder states nor the mask are
        expanded; every decoder layer projects and quantizes the cross-attention keys / values once per input and its n
        candidates attend to that one copy (``cross_group``; ops.attention_fake_quant with ``group``).
        ``self.last_share_cross_kv`` then says what happened: ``shared`` / ``eager`` decoder layers, and the ``reason``
        when nothing was shared (generation.score_share_why_not)."""
        n = int(num_candidates)
        if n < 1:
            raise ValueError("score(): num_candidates must be at least 1")
        if labels.dim() != 2 or labels.shape[0] != input_ids.shape[0] * n:
            raise ValueError("score(): labels must be [B * num_candidates, T], the candidates of an input adjacent")
        labels = labels.to(torch.int64)
        if attention_mask is None:
            attention_mask = torch.ones_like(input_ids)
        enc = self.get_encoder()(input_ids, attention_mask=attention_mask)
        share = self.last_share_cross_kv = generation.ShareCrossKvInfo.asked(share_cross_kv, "SHARE_CROSS_KV")
        if share.reason is None:
            share.reason = generation.score_share_why_not(self, enc.device, n)
        group = n if share.reason is None else 1
        if n > 1 and group == 1:
            enc = enc.repeat_interleave(n, dim=0)
            attention_mask = attention_mask.repeat_interleave(n, dim=0)
        dec_in = shift_tokens_right(labels.masked_fill(labels == ignore_index, -100), self.config.pad_token_id,
                                    self.config.decoder_start_token_id)
        dec_in.clamp_(0, self.config.vocab_size - 1)    # a label outside the vocabulary is refused below, not looked up
        logits = self.forward(attention_mask=attention_mask, decoder_input_ids=dec_in, encoder_outputs=(enc,),
                              **(dict(cross_group=group) if group > 1 else {}))[0]
        if group > 1:
            took = [layer.encoder_attn.last_cross_shared for layer in self.model.decoder.layers]
            share.shared, share.eager = sum(took), len(took) - sum(took)
            if not share.shared:
                share.reason = "no decoder layer's key / value sites took the one launch (util_layernorm.FUSE_KV_APPEND)"
        rows, steps = labels.shape
        vocab = logits.shape[-1]
        scored = labels != ignore_index
        counts = None
        if logits.is_cuda:
            flat = logits.reshape(rows * steps, vocab).float()
            _, logprob, _, counts = ops.lm_loss(flat, labels.reshape(-1), ignore_index)
            token_logprobs = logprob.view(rows, steps)
        else:
            self._score_refuse(int((scored & ((labels < 0) | (labels >= vocab))).sum()), vocab)
            token_logprobs = token_logprob_torch(logits.float(), labels, ignore_index)
        sequence_logprob = torch.zeros(rows, dtype=torch.float32, device=logits.device)
        for t in range(steps):                          # position order: a row's sum does not depend on the batch
            sequence_logprob += token_logprobs[:, t]
        lengths = scored.sum(1)
        if counts is not None:
            self._score_refuse(int(counts[1]), vocab)   # the call's one synchronisation
        return token_logprobs, sequence_logprob, lengths

    @staticmethod
    def _score_refuse(bad, vocab):
        if bad:
            raise ValueError(f"score(): {bad} labels lie outside the vocabulary [0, {vocab}) and are not ignore_index")

    def prepare_inputs_for_generation(self, decoder_input_ids, past=None, attention_mask=None, head_mask=None,
                                      decoder_head_mask=None, cross_attn_head_mask=None, use_cache=None,
                                      encoder_outputs=None, **kwargs):
        """quant_bart.py:1125-1149: only the last token once a cache exists."""
        if past is not None:
            decoder_input_ids = decoder_input_ids[:, -1:]
        return {"input_ids": None, "encoder_outputs": encoder_outputs, "past_key_values": past,
                "decoder_input_ids": decoder_input_ids, "attention_mask": attention_mask, "head_mask": head_mask,
                "decoder_head_mask": decoder_head_mask, "cross_attn_head_mask": cross_attn_head_mask,
                "use_cache": use_cache}

    def prepare_decoder_input_ids_from_labels(self, labels):
        return shift_tokens_right(labels, self.config.pad_token_id, self.config.decoder_start_token_id)

    @staticmethod
    def _reorder_cache(past, beam_idx):
        """quant_bart.py:1155-1164: the self-attention rows follow beam_idx, the cross-attention entries stay.  A
        QuantizedBartCache records the index and applies it in its next append (returned as it is)."""
        if isinstance(past, QuantizedBartCache):
            return past.reorder(beam_idx)
        return tuple(tuple(s.index_select(0, beam_idx) for s in layer[:2]) + tuple(layer[2:]) for layer in past)

    @torch.no_grad()
    def generate(self, input_ids, attention_mask=None, max_length=None, num_beams=None, **kwargs):
        """Greedy or beam-search decoding with a KV cache (model/generation.py): token ids [B * num_return_sequences, L]
        padded with pad_token_id, as transformers' generate returns them.  Defaults come from the wrapped model's
        generation_config / config.  ``cache_codes``: the cache holds integer codes (None: the package switch,
        set_cache_codes); raises RuntimeError when the cache ended up with elements that have no code.  ``graph``: capture
        a decoding step into a hipGraph and replay it (None: the package switch, set_graph_decode; model/graph_decode.py);
        ``self.last_decode_graph`` then says what happened (captured, replays, reason).  ``beam_select``: beam search
        selects a step's continuations with one kernel call (None: the package switch, set_beam_select; ops.beam_select);
        ``self.last_beam_select`` then says how many steps took it (selected, eager, reason).  ``beam_advance``: beam search
        advances its beams with one kernel call per step (None: the package switch, set_beam_advance; ops.beam_advance);
        ``self.last_beam_advance`` then says how many steps took it (advanced, eager, reason).  ``beam_graph``: beam search
        captures a whole step -- model, selection, bookkeeping -- into one graph and replays it (None: the package switch,
        set_beam_graph; it implies the three above for the call; model/graph_decode.py, BeamStepGraphs);
        ``self.last_beam_graph`` then says what happened (captured, replays, issued, reason).  ``greedy_advance``: greedy
        decoding takes everything after the model step -- processors, arg-max, pad / eos, the stopping word -- with one kernel
        call per token (None: the package switch, set_greedy_advance; ops.greedy_advance); ``self.last_greedy_advance`` then
        says how many steps took it (advanced, eager, reason).  ``greedy_graph``: greedy decoding captures a whole step into
        one graph and replays it (None: the package switch, set_greedy_graph; it implies ``graph`` and ``greedy_advance`` for
        the call; model/graph_decode.py, GreedyStepGraph); ``self.last_greedy_graph`` then says what happened (captured,
        replays, reason).  ``share_cross_kv``: beam search holds the cross-attention keys / values once per batch row and
        attends to them from every beam of the row in one launch (None: the package switch, set_share_cross_kv;
        ops.decode_attention_shared); ``self.last_share_cross_kv`` then says what happened (shared, eager, reason)."""
        return generation.generate(self, input_ids, attention_mask=attention_mask, max_length=max_length,
                                   num_beams=num_beams, **kwargs)

    @torch.no_grad()
    def sample(self, input_ids, attention_mask=None, max_length=None, seed=None, temperature=1.0, top_k=50, top_p=1.0, **kwargs):
        """Seeded sampling with a KV cache (model/generation.py, sample; model/sampling.py): token ids [B, L] padded with
        pad_token_id, a function of the inputs and ``seed`` alone (None: one drawn from torch's default CPU generator).  The
        random stream is the package's own, so the tokens are not transformers'; generate() keeps refusing ``do_sample``.
        ``temperature``, ``top_k`` (0: every token; exactly k survive, ties by smaller token) and ``top_p`` (over the
        renormalised survivors) shape the distribution; settings, ``cache_codes`` and ``graph`` as in generate().
        ``sample_advance``: everything after the model step in one kernel call per token (None: the package switch,
        set_sample_advance; ops.sample_advance); ``self.last_sample_advance`` then says how many steps took it (advanced,
        eager, reason).  ``sample_graph``: a whole step captured into one graph and replayed (None: the package switch,
        set_sample_graph; it implies ``graph`` and ``sample_advance`` for the call); ``self.last_sample_graph`` then says
        what happened (captured, replays, reason).  ``sample_nucleus`` (None: the package switch, set_sample_nucleus): under
        either, ``top_k=0`` with ``top_p<1`` is one kernel call too (ops.sample_nucleus) instead of the torch lines.
        ``num_samples=n``: n sequences per input, [B * n, L] with an input's rows adjacent; the encoder runs once and, with
        ``share_cross_kv`` (None: the package switch, set_share_cross_kv), the cross-attention keys / values are held once
        per input (``self.last_share_cross_kv``: shared, eager, reason).  ``return_logprobs=True``: (sequences, logprobs),
        the fp32 log-probability with which each token was drawn."""
        return generation.sample(self, input_ids, attention_mask=attention_mask, max_length=max_length, seed=seed,
                                 temperature=temperature, top_k=top_k, top_p=top_p, **kwargs)


class QuantizedBartClassificationHead(QuantizedModule):
    """quant_bart.py:505-529: the sentence representation, the tanh layer's output (and the logits) are quantizer sites;
    flat [B, H] tensors -- no mask, no sequence axis."""

    def __init__(self, org_module, w_qconfig, a_qconfig, qoutput=True, backend="academic"):
        super().__init__(backend)
        self.qoutput = qoutput
        self.getitem_post_act_fake_quantize = Quantizer(None, a_qconfig)
        self.dense = Quantizer(org_module.dense, w_qconfig)
        self.dropout = org_module.dropout
        self.dropout_post_act_fake_quantize = Quantizer(None, a_qconfig)
        self.out_proj = Quantizer(org_module.out_proj, w_qconfig)
        if qoutput:
            self.out_proj_post_act_fake_quantize = Quantizer(None, a_qconfig)

    def forward(self, hidden_states):
        hidden_states = self.getitem_post_act_fake_quantize(self.dropout(hidden_states))
        hidden_states = self.dropout(torch.tanh(self.dense(hidden_states)))
        hidden_states = self.out_proj(self.dropout_post_act_fake_quantize(hidden_states))
        if self.qoutput:
            hidden_states = self.out_proj_post_act_fake_quantize(hidden_states)
        return hidden_states


def _observation_masks(is_remove_padding, attention_mask, decoder_attention_mask):
    """quant_bart.py:1064-1072 / 1205-1213 / 1334-1342."""
    if not is_remove_padding:
        return None, None
    obs = attention_mask.sum(1)
    return obs, (obs if decoder_attention_mask is None else decoder_attention_mask.sum(1))


class QuantizedBartForSequenceClassification(QuantizedModule):
    """quant_bart.py:1167-1289: the decoder state at the last <eos> token through the quantized classification head."""

    def __init__(self, org_module, w_qconfig, a_qconfig, qoutput=True, backend="academic", is_remove_padding=False):
        super().__init__(backend)
        self.is_remove_padding = is_remove_padding
        self.qoutput = qoutput
        self.config = org_module.config
        self.model = QuantizedBartModel(org_module.model, w_qconfig, a_qconfig, qoutput=False, backend=backend)
        self.classification_head = QuantizedBartClassificationHead(org_module.classification_head, w_qconfig, a_qconfig,
                                                                   qoutput=qoutput, backend=backend)

    def forward(self, input_ids=None, attention_mask=None, decoder_input_ids=None, decoder_attention_mask=None, labels=None,
                **unused):
        obs, dec_obs = _observation_masks(self.is_remove_padding, attention_mask, decoder_attention_mask)
        dec, enc = self.model(input_ids, attention_mask, decoder_input_ids, decoder_attention_mask,
                              observation_mask=obs, decoder_observation_mask=dec_obs)
        eos_mask = input_ids.eq(self.config.eos_token_id)
        if len(torch.unique_consecutive(eos_mask.sum(1))) > 1:
            raise ValueError("All examples must have the same number of <eos> tokens.")
        sentence = dec[eos_mask, :].view(dec.size(0), -1, dec.size(-1))[:, -1, :]
        logits = self.classification_head(sentence)
        return with_loss(classification_loss(self.config, self.config.num_labels, logits, labels), (logits, enc))


class QuantizedBartForQuestionAnswering(QuantizedModule):
    """quant_bart.py:1292-1408: start / end logits from the (quantized) decoder output."""

    def __init__(self, org_module, w_qconfig, a_qconfig, qoutput=True, backend="academic", is_remove_padding=False):
        super().__init__(backend)
        self.is_remove_padding = is_remove_padding
        self.qoutput = qoutput
        self.num_labels = org_module.num_labels
        self.config = org_module.config
        self.model = QuantizedBartModel(org_module.model, w_qconfig, a_qconfig, qoutput=True, backend=backend)
        self.qa_outputs = Quantizer(org_module.qa_outputs, w_qconfig)
        if qoutput:
            self.qa_outputs_post_act_fake_quantize = Quantizer(None, a_qconfig)

    def forward(self, input_ids=None, attention_mask=None, decoder_input_ids=None, decoder_attention_mask=None,
                start_positions=None, end_positions=None, **unused):
        obs, dec_obs = _observation_masks(self.is_remove_padding, attention_mask, decoder_attention_mask)
        dec, enc = self.model(input_ids, attention_mask, decoder_input_ids, decoder_attention_mask,
                              observation_mask=obs, decoder_observation_mask=dec_obs)
        logits = self.qa_outputs(dec)
        if self.qoutput:
            logits = self.qa_outputs_post_act_fake_quantize(logits)
        start, end = logits.split(1, dim=-1)
        start, end = start.squeeze(-1).contiguous(), end.squeeze(-1).contiguous()
        return with_loss(span_loss(start, end, start_positions, end_positions), (start, end, enc))

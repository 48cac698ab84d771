"""A calibrated model's weights as packed integer codes, and back.

``export_codes(model)`` returns what ``torch.save`` can write: for every weight-quantized operator whose weight quantizer
is frozen (observer off, fake-quant on) the integers its fake-quantised weight stands for -- ``<name>.weight_codes``
(uint8, one code per byte, or two per byte when the range fits four bits), the effective ``<name>.weight_scale`` /
``<name>.weight_zero_point`` (fp32, one per channel) and the integers ``weight_quant_min`` / ``weight_quant_max`` /
``weight_code_bits`` / ``weight_ch_axis`` plus ``weight_shape`` -- in place of the fp32 ``<name>.weight``; every other
``state_dict()`` entry as it is.  ``load_codes(model, packed)`` loads that into a model of the same structure
(``quantize_model`` of the same architecture): the plain entries through ``load_state_dict``, every coded weight
dequantised into the operator's ``weight`` -- all table-eligible ones in ONE launch (``osq_dequantize_codes_multi``).

The loaded weight is the source model's FAKE-QUANTISED weight word for word (format and arithmetic: include/osq_hip.h,
"integer codes"), and fake-quantising it again with the same parameters returns it unchanged, so the loaded model's
logits equal the source's bit for bit with the weight quantizers still enabled.  ``model.state_dict()`` is untouched by
both calls.
"""
import torch

from . import _hip, ops
from .quantization.fake_quant import QuantizeBase
from .quantization.quantized_module import QuantizedOperator

FORMAT_KEY = "__weight_codes_format__"
FORMAT = 1
_FIELDS = ("codes", "scale", "zero_point", "quant_min", "quant_max", "code_bits", "ch_axis", "shape")

stats = {"multi_launches": 0, "multi_tensors": 0, "single_launches": 0}


def _weight_quantized(model):
    for name, m in model.named_modules():
        fq = m.__dict__.get("_modules", {}).get("weight_fake_quant")
        if isinstance(m, QuantizedOperator) and isinstance(fq, QuantizeBase) and getattr(m, "weight", None) is not None:
            yield name, m, fq


def export_codes(model):
    """Flat dict of CPU tensors and ints (see the module text).  An operator whose weight quantizer is disabled keeps its
    fp32 weight; one that is still observing raises RuntimeError naming the module; a weight with elements that have no
    integer code (NaN, a fractional zero point) raises ValueError naming it."""
    coded = {}
    for name, op, fq in _weight_quantized(model):
        if fq.observer_enabled == 1:
            raise RuntimeError(f"export_codes: the weight quantizer of '{name}' is still observing (observer enabled): freeze the "
                               "model first (enable_quantization)")
        if fq.fake_quant_enabled != 1:
            continue
        try:
            coded[name] = fq.to_codes(op.weight.detach())
        except ValueError as e:
            raise ValueError(f"export_codes: '{name}.weight': {e}") from None
    packed = {FORMAT_KEY: FORMAT}
    skip = {(name + "." if name else "") + "weight" for name in coded}
    for key, value in model.state_dict().items():
        if key not in skip:
            packed[key] = value.detach().cpu()
    for name, rec in coded.items():
        prefix = (name + "." if name else "") + "weight_"
        packed[prefix + "codes"] = rec.codes.cpu()
        packed[prefix + "scale"] = rec.scale.cpu()
        packed[prefix + "zero_point"] = rec.zero_point.cpu()
        packed[prefix + "quant_min"], packed[prefix + "quant_max"] = rec.quant_min, rec.quant_max
        packed[prefix + "code_bits"], packed[prefix + "ch_axis"] = rec.code_bits, rec.ch_axis
        packed[prefix + "shape"] = torch.tensor(rec.shape, dtype=torch.int64)
    return packed


def _table_entry(weight, rec):
    """Layout rules of osq_dequantize_codes_multi (those of weight_cache._table_entry): row-major rows of the channel
    axis 0 (or one scale for all rows), inner % 4 == 0, 16-byte aligned fp32 weight."""
    if weight.dim() < 2 or weight.data_ptr() % 16 or rec.ch_axis not in (0, -1):
        return None
    rows = weight.shape[0]
    inner = weight.numel() // rows if rows else 0
    if rows == 0 or inner == 0 or inner % 4:
        return None
    return rows, (rows if rec.ch_axis == 0 else 1), inner


def load_codes(model, packed):
    """Load what export_codes wrote into ``model`` (same structure, already on its HIP device).  The quantizers keep their
    state (flags) and take their parameters from the plain entries; the coded weights land in the operators' ``weight``."""
    if packed.get(FORMAT_KEY) != FORMAT:
        raise ValueError(f"load_codes: not a dict written by export_codes (format {packed.get(FORMAT_KEY)!r}, expected {FORMAT})")
    ops_by_name = {name: op for name, op, _ in _weight_quantized(model)}
    names = [k[:-len("weight_codes")].rstrip(".") for k in packed if k.endswith("weight_codes")]
    extras = {(n + "." if n else "") + "weight_" + f for n in names for f in _FIELDS} | {FORMAT_KEY}
    plain = {k: v for k, v in packed.items() if k not in extras}
    result = model.load_state_dict(plain, strict=False)
    expected_missing = {(n + "." if n else "") + "weight" for n in names}
    if set(result.missing_keys) != expected_missing or result.unexpected_keys:
        raise RuntimeError(f"load_codes: the model does not match the packed dict: missing {sorted(set(result.missing_keys) - expected_missing)}, "
                           f"unexpected {sorted(result.unexpected_keys)}, coded but present {sorted(expected_missing - set(result.missing_keys))}")
    lib = _hip.load()
    table, singles = [], []
    for n in names:
        op = ops_by_name.get(n)
        if op is None:
            raise RuntimeError(f"load_codes: '{n}' is not a weight-quantized operator of this model")
        prefix = (n + "." if n else "") + "weight_"
        w = op.weight.data
        _hip.require_device(w)
        shape = tuple(int(s) for s in packed[prefix + "shape"].tolist())
        if shape != tuple(w.shape) or w.dtype != torch.float32 or not w.is_contiguous():
            raise RuntimeError(f"load_codes: '{n}.weight' is {tuple(w.shape)} {w.dtype}, the codes are for a contiguous float32 {shape}")
        rec = ops.Codes(packed[prefix + "codes"].to(w.device), packed[prefix + "scale"].to(w.device),
                        packed[prefix + "zero_point"].to(w.device), int(packed[prefix + "quant_min"]),
                        int(packed[prefix + "quant_max"]), int(packed[prefix + "code_bits"]), shape, int(packed[prefix + "ch_axis"]))
        geo = _table_entry(w, rec)
        if geo is not None and rec.codes.numel() == (w.numel() * rec.code_bits + 7) // 8 and rec.scale.numel() == geo[1] == rec.zero_point.numel():
            table.append((w, rec, geo))
        else:
            singles.append((w, rec))
    by_device = {}
    for entry in table:
        by_device.setdefault(entry[0].device, []).append(entry)
    for dev, entries in by_device.items():
        descs = (_hip.CodesDesc * len(entries))()
        row_end, total = [], 0
        for d, (w, rec, (rows, channels, inner)) in zip(descs, entries):
            d.codes, d.y, d.scale_eff, d.zp_eff = rec.codes.data_ptr(), w.data_ptr(), rec.scale.data_ptr(), rec.zero_point.data_ptr()
            d.rows, d.channels, d.inner = rows, channels, inner
            d.quant_min, d.code_bits = rec.quant_min, rec.code_bits
            total += rows
            row_end.append(total)
        with torch.cuda.device(dev):
            dev_table = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(dev)
            ends = torch.tensor(row_end, dtype=torch.int64, device=dev)
            _hip.check(lib.osq_dequantize_codes_multi(dev_table.data_ptr(), ends.data_ptr(), len(entries), total, _hip.stream_ptr(dev)),
                       "dequantize_codes_multi")
        stats["multi_launches"] += 1
        stats["multi_tensors"] += len(entries)
    for w, rec in singles:                     # what the table cannot hold: odd row lengths, a channel axis in the middle
        with torch.cuda.device(w.device):
            ops.dequantize_codes(rec, out=w)
        stats["single_launches"] += 1
    ops.weight_epoch += 1                      # weights were written through raw pointers: kept fake-quantised weights are stale
    return model

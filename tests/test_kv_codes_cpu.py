"""CPU: the KV cache as integer codes (QuantizedBartCache(codes=True), set_cache_codes / OSQ_CACHE_CODES) where no GPU is
involved: the switch and its environment variable, a coded cache on CPU tensors (it stays fp32 and equals the fp32 cache),
``wrap`` of a tuple, and the new entry points in the header against ``_hip.SIGNATURES``.  The coded cache itself runs on
the GPU (tests/test_gpu_kv_codes.py, tests/test_gpu_kv_codes_model.py)."""
import ctypes
import os
import re

import pytest
import torch

from test_bart_decode_cpu import batch, tiny_bart, wrapped

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def switch():
    from outlier_suppression_amd import util_layernorm as UL
    old = UL.CACHE_CODES
    yield UL
    UL.CACHE_CODES = old


def test_switch_is_off_by_default_and_settable(switch):
    import outlier_suppression_amd as osq
    assert switch.CACHE_CODES is False or os.environ.get("OSQ_CACHE_CODES", "") not in ("", "0")
    osq.set_cache_codes(True)
    assert switch.CACHE_CODES is True
    osq.set_cache_codes(False)
    assert switch.CACHE_CODES is False
    osq.set_cache_codes()
    assert switch.CACHE_CODES is True


@pytest.mark.parametrize("value, want", [(None, False), ("", False), ("0", False), ("1", True), ("yes", True)])
def test_environment_variable(value, want):
    import outlier_suppression_amd as osq
    env = {} if value is None else {"OSQ_CACHE_CODES": value}
    assert osq.cache_codes_from_environment(env) is want


def test_environment_reaches_reset_tier(switch, monkeypatch):
    """reset_tier (what loading the library applies) sets the switch from the environment; its other settings go to the
    library, which a stand-in takes here."""
    import outlier_suppression_amd as osq
    from outlier_suppression_amd import ops
    monkeypatch.setattr(ops, "set_tuning", lambda key, value, lib=None: None)
    monkeypatch.setenv("OSQ_CACHE_CODES", "1")
    osq.reset_tier()
    assert switch.CACHE_CODES is True
    monkeypatch.delenv("OSQ_CACHE_CODES")
    osq.reset_tier()
    assert switch.CACHE_CODES is False


def _steps(q, ids, mask, dec, cache):
    logits = []
    with torch.no_grad():
        out, cache, enc = q(ids, mask, decoder_input_ids=dec[:, :2], past_key_values=cache, use_cache=True)
        logits.append(out[:, -1])
        for t in range(2, dec.shape[1]):
            out, cache, _ = q(attention_mask=mask, decoder_input_ids=dec[:, t:t + 1], encoder_outputs=(enc,),
                              past_key_values=cache, use_cache=True)
            logits.append(out[:, -1])
    return torch.stack(logits, 1), cache


def test_cpu_cache_with_codes_stays_fp32():
    from outlier_suppression_amd.model.quant_bart import QuantizedBartCache
    q = wrapped(tiny_bart())
    ids, mask = batch()
    dec = torch.randint(3, 120, (3, 6), generator=torch.Generator().manual_seed(3))
    a, plain = _steps(q, ids, mask, dec, QuantizedBartCache(2))
    b, coded = _steps(q, ids, mask, dec, QuantizedBartCache(2, codes=True))
    assert coded.codes and not plain.codes
    assert torch.equal(a, b)
    assert coded.coded() == [] and coded.demoted() == [] and coded.rejected() == 0
    assert coded.nbytes() == plain.nbytes() > 0
    for x, y in zip(plain, coded):
        assert len(x) == len(y) == 4
        for s, t in zip(x, y):
            assert t.dtype == torch.float32 and torch.equal(s, t)
    # a reorder on the coded cache reads like the fp32 one's
    idx = torch.tensor([2, 0, 0])
    for x, y in zip(plain.reorder(idx).to_legacy(), coded.reorder(idx).to_legacy()):
        for s, t in zip(x, y):
            assert torch.equal(s, t)


def test_use_cache_forward_follows_the_switch(switch):
    q = wrapped(tiny_bart())
    ids, mask = batch()
    with torch.no_grad():
        _, off, _ = q(ids, mask, decoder_input_ids=ids[:, :2], use_cache=True)
        switch.CACHE_CODES = True
        _, on, _ = q(ids, mask, decoder_input_ids=ids[:, :2], use_cache=True)
    assert off.codes is False and on.codes is True


def test_wrap_of_a_tuple_stays_fp32(switch):
    from outlier_suppression_amd.model.quant_bart import QuantizedBartCache
    q = wrapped(tiny_bart())
    ids, mask = batch()
    with torch.no_grad():
        _, cache, _ = q(ids, mask, decoder_input_ids=ids[:, :3], use_cache=True)
    legacy = tuple(tuple(t.clone() for t in layer) for layer in cache)
    for codes in (None, True, False):
        switch.CACHE_CODES = True
        w = QuantizedBartCache.wrap(legacy, 2, codes=codes)
        assert w.coded() == [] and w.get_seq_length() == 3
        for x, y in zip(w, legacy):
            for s, t in zip(x, y):
                assert s.dtype == torch.float32 and torch.equal(s, t)
    assert QuantizedBartCache.wrap(cache, 2, codes=True) is cache
    assert QuantizedBartCache.wrap(None, 2, codes=True).codes and not QuantizedBartCache.wrap(None, 2, codes=False).codes
    switch.CACHE_CODES = False
    assert not QuantizedBartCache.wrap(None, 2).codes


def test_generate_takes_cache_codes_on_the_cpu():
    q = wrapped(tiny_bart())
    ids, mask = batch()
    with torch.no_grad():
        a = q.generate(ids, attention_mask=mask, max_length=8, num_beams=2)
        b = q.generate(ids, attention_mask=mask, max_length=8, num_beams=2, cache_codes=True)
    assert torch.equal(a, b)


_C = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "float": ctypes.c_float}


def _declared_args(header, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", header, re.S)
    assert m, f"{name} is not declared in include/osq_hip.h"
    return [a.strip() for a in m.group(1).replace("\n", " ").split(",")]


@pytest.mark.parametrize("name", ["osq_fake_quant_kv_append_codes", "osq_decode_attention_codes"])
def test_header_matches_signatures(name):
    """Argument by argument: a pointer (or osq_stream) is a void pointer or a pointer to the table's struct, a scalar the
    ctypes type of its C type."""
    from outlier_suppression_amd import _hip
    header = open(os.path.join(ROOT, "include", "osq_hip.h")).read()
    args = _declared_args(header, name)
    res, argtypes = _hip.SIGNATURES[name]
    assert res is ctypes.c_int and len(args) == len(argtypes), (args, argtypes)
    for decl, ct in zip(args, argtypes):
        ctype = decl.rsplit(" ", 1)[0].replace("const ", "").strip()
        if "*" in decl or ctype == "osq_stream":
            assert ct is ctypes.c_void_p or issubclass(ct, ctypes._Pointer), (decl, ct)
        else:
            assert ct is _C[ctype], (decl, ct)
    assert name in header.split("#define OSQ_ABI_VERSION")[0], f"{name} missing from the 'Added within 10' list"


def test_site_struct_matches_header():
    from outlier_suppression_amd import _hip
    header = open(os.path.join(ROOT, "include", "osq_hip.h")).read()
    body = re.search(r"typedef struct osq_kv_codes_site \{(.*?)\} osq_kv_codes_site;", header, re.S).group(1)
    fields = []
    for line in body.strip().splitlines():
        decl = line.strip().rstrip(";")
        if "*" in decl:
            fields.append((decl.rsplit(" ", 1)[1].lstrip("*"), ctypes.c_void_p))
            continue
        ctype, names = decl.split(" ", 1)
        fields += [(n.strip(), _C[ctype]) for n in names.split(",")]
    assert [(n, t) for n, t in _hip.KvCodesSite._fields_] == fields
    assert ctypes.sizeof(_hip.KvCodesSite) % 8 == 0

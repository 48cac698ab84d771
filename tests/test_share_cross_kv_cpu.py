"""CPU: what sharing the cross-attention keys / values among the beams of a row (generate(share_cross_kv=True);
csrc/decode_attention.hip) needs where no GPU is involved: the two entry points in the header's "Added within 10" list
and in ``_hip.SIGNATURES``; the switch, its setter and its environment variable; the reasons generate() and sample() give
where nothing can be shared -- CPU tensors, one beam -- with the tokens of the call without the switch; and the cache's
``cross_group`` on the CPU, where the shared launches do not run: the legacy tuple keeps its shapes, ``nbytes`` counts one copy.
The kernel and the model run on the GPU (tests/test_gpu_decode_attention_shared.py, tests/test_gpu_share_cross_kv_model.py)."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("osq_decode_attention_shared", "osq_decode_attention_shared_codes")


def test_entry_points_are_listed_and_bound():
    from outlier_suppression_amd import _hip
    header = open(os.path.join(ROOT, "include", "osq_hip.h")).read()
    added = re.search(r"Added within 10 \(no existing signature changed\):(.*?)\*/", header, re.S).group(1)
    listed = set(re.findall(r"osq_\w+", added))
    for name in SYMBOLS:
        assert name in listed, f"{name} is not in the header's 'Added within 10' list"
        assert re.search(r"^int " + name + r"\(", header, re.M), f"{name} is not declared"
        assert name in _hip.SIGNATURES
    assert re.search(r"#define OSQ_ABI_VERSION 10\b", header) and _hip.ABI_VERSION == 10
    # the arguments of the two static functions plus `group`, an int64 after `batch`
    for shared, static in (("osq_decode_attention_shared", "osq_decode_attention_fake_quant"),
                           ("osq_decode_attention_shared_codes", "osq_decode_attention_codes")):
        a, b = _hip.SIGNATURES[shared], _hip.SIGNATURES[static]
        assert a[0] is b[0] and a[1] == b[1][:7] + [b[1][6]] + b[1][7:], shared
        decl = re.search(r"^int " + shared + r"\((.*?)\);", header, re.M | re.S).group(1)
        assert len(decl.split(",")) == len(a[1]) and re.search(r"int64_t batch, int64_t group, int64_t heads", decl)
    csrc = os.path.join(ROOT, "outlier_suppression_amd", "csrc")
    makefile = open(os.path.join(csrc, "Makefile")).read()
    assert len(re.findall(r"\bdecode_attention\.hip\b", makefile)) == 2    # the library's and the development build's sources
    source = open(os.path.join(csrc, "decode_attention.hip")).read()
    for name in SYMBOLS:
        assert re.search(r'^extern "C" int ' + name + r"\(", source, re.M), f"{name} is not defined in decode_attention.hip"


@pytest.fixture()
def switch():
    from outlier_suppression_amd import util_layernorm as UL
    old = UL.SHARE_CROSS_KV
    yield UL
    UL.SHARE_CROSS_KV = old


@pytest.mark.parametrize("value, want", [(None, False), ("", False), ("0", False), ("1", True), ("yes", True)])
def test_environment_variable(value, want):
    import outlier_suppression_amd as osq
    env = {} if value is None else {"OSQ_SHARE_CROSS_KV": value}
    assert osq.share_cross_kv_from_environment(env) is want


def test_switch_and_environment_reach_util_layernorm(switch, monkeypatch):
    import outlier_suppression_amd as osq
    from outlier_suppression_amd import ops
    assert switch.SHARE_CROSS_KV is False or os.environ.get("OSQ_SHARE_CROSS_KV", "") not in ("", "0")
    osq.set_share_cross_kv()
    assert switch.SHARE_CROSS_KV is True
    osq.set_share_cross_kv(False)
    assert switch.SHARE_CROSS_KV is False
    monkeypatch.setattr(ops, "set_tuning", lambda key, value, lib=None: None)
    monkeypatch.setenv("OSQ_SHARE_CROSS_KV", "1")
    osq.reset_tier()
    assert switch.SHARE_CROSS_KV is True
    monkeypatch.delenv("OSQ_SHARE_CROSS_KV")
    osq.reset_tier()
    assert switch.SHARE_CROSS_KV is False


def test_generate_on_the_cpu_decodes_as_before_and_says_why(switch):
    from test_bart_decode_cpu import batch, tiny_bart, wrapped
    q = wrapped(tiny_bart())
    ids, mask = batch()
    kw = dict(attention_mask=mask, max_length=12, num_beams=3, min_length=5, no_repeat_ngram_size=2)
    with torch.no_grad():
        want = q.generate(ids, **kw)
        info = q.last_share_cross_kv
        assert (info.shared, info.reason) == (0, "not asked for") and info.eager >= 4, info
        got = q.generate(ids, share_cross_kv=True, **kw)
        info = q.last_share_cross_kv
        assert torch.equal(got, want)
        assert info.shared == 0 and info.eager >= 4 and "CPU" in info.reason, info
        switch.SHARE_CROSS_KV = True                   # the package switch asks as the argument does
        assert torch.equal(q.generate(ids, **kw), want) and "CPU" in q.last_share_cross_kv.reason
        assert torch.equal(q.generate(ids, share_cross_kv=False, **kw), want) and q.last_share_cross_kv.reason == "not asked for"
        # one beam: nothing to share, whatever the device
        greedy = q.generate(ids, attention_mask=mask, max_length=6, num_beams=1, share_cross_kv=False)
        assert torch.equal(q.generate(ids, attention_mask=mask, max_length=6, num_beams=1), greedy)
        assert q.last_share_cross_kv.shared == 0 and "num_beams == 1" in q.last_share_cross_kv.reason
        drawn = q.sample(ids, attention_mask=mask, max_length=6, seed=3, share_cross_kv=False)
        assert q.last_share_cross_kv.reason == "not asked for"
        assert torch.equal(q.sample(ids, attention_mask=mask, max_length=6, seed=3), drawn)
        assert q.last_share_cross_kv.shared == 0 and "num_beams == 1" in q.last_share_cross_kv.reason
        assert "use_cache=False" in _reason(q, ids, use_cache=False, **kw)
    with torch.enable_grad():
        from outlier_suppression_amd.model import generation
        assert generation._share_why_not(q, torch.device("cuda:0"), True, 3, 14) == "autograd is on"


def _reason(q, ids, **kw):
    q.generate(ids, **kw)
    return q.last_share_cross_kv.reason


def test_cache_with_a_cross_group_on_the_cpu():
    """A cache built with cross_group=3 and fed encoder states of B rows on the CPU, where the shared launches do not run: the
    attention module computes on the expanded rows and keeps one copy.  The logits are those of the unshared cache, the
    legacy tuple has its shapes, the cross entries hold B rows and ``nbytes`` is smaller by their (G - 1) / G."""
    from test_bart_decode_cpu import batch, tiny_bart, wrapped
    from outlier_suppression_amd.model.quant_bart import QuantizedBartCache
    q = wrapped(tiny_bart())
    ids, mask = batch()
    g, b = 3, ids.shape[0]
    layers = len(q.model.decoder.layers)
    dec = torch.randint(3, 50, (b * g, 4), generator=torch.Generator().manual_seed(2))
    with torch.no_grad():
        enc = q.get_encoder()(ids, attention_mask=mask)
        outs, caches = [], []
        for share in (True, False):
            e, m = (enc, mask) if share else (enc.repeat_interleave(g, 0), mask.repeat_interleave(g, 0))
            cache = QuantizedBartCache(layers, capacity=4, cross_group=g if share else 1)
            steps = [q(attention_mask=m, decoder_input_ids=dec[:, a:c], encoder_outputs=(e,), past_key_values=cache,
                       use_cache=True)[0] for a, c in ((0, 2), (2, 3), (3, 4))]
            outs.append(torch.cat(steps, 1))
            caches.append(cache)
    assert torch.allclose(outs[0], outs[1], atol=1e-5, rtol=0)
    shared, plain = caches
    cross = 0
    for i in range(layers):
        for a, c in zip(shared._cross[i], plain._cross[i]):
            assert a.shape == (b,) + c.shape[1:] and torch.equal(a.repeat_interleave(g, 0), c)
            cross += c.numel() * c.element_size()
        assert [t.shape for t in shared[i]] == [t.shape for t in plain[i]]
        assert all(torch.equal(x, y) for x, y in zip(shared[i][2:], plain[i][2:]))
    assert plain.nbytes() - shared.nbytes() == cross // g * (g - 1)
    assert [t.shape for layer in shared.to_legacy() for t in layer] == [t.shape for layer in plain.to_legacy() for t in layer]
    with pytest.raises(ValueError):
        QuantizedBartCache(layers, cross_group=0)

"""score(num_candidates=n, share_cross_kv=True) on the tiny W6A6 LSQ+ BART of test_gpu_bart_decode.py (head_dim 16, 3 inputs,
source 14), n = 3: every decoder layer projects and quantizes the cross-attention keys / values once per input and the n
candidates attend to that copy (QuantizedBartAttention._cross_shared, ``cross_group``; the grouped whole-sequence launch of
tests/test_gpu_attention_shared.py under FUSE_ATTENTION / FUSE_ATTENTION_INT).

Under each of: all one-launch attention switches off, FUSE_SOFTMAX, FUSE_ATTENTION, FUSE_ATTENTION_INT -- the shared call
returns token_logprobs, sequence_logprob and lengths WORD-EQUAL to the unshared call under the same switches (the key / value
sites store the unshared form's words at this model, test_gpu_share_cross_kv_model.py::test_c, and the attention kernels'
contract is word equality), reports two shared layers, and each encoder-attention k_proj sees B rows.  Then the fallbacks,
the package switch, and a prefill over a ``cross_group`` cache."""
import copy

import pytest
import torch

import _token_logprob as TL
from test_gpu_bart_decode import FUSED_VS_EAGER_LOGITS, setup  # noqa: F401  (setup: that file's module fixture, instantiated here)

pytestmark = pytest.mark.gpu

VOCAB = 120
N = 3
SWITCHES = ("off", "FUSE_SOFTMAX", "FUSE_ATTENTION", "FUSE_ATTENTION_INT")


@pytest.fixture()
def switches():
    """Every one-launch attention switch off and the package's share switch off; restored afterwards."""
    from outlier_suppression_amd import _hip, util_layernorm as UL
    _hip.load()                      # the first load applies the environment's tier, these switches included
    names = ("FUSE_SOFTMAX", "FUSE_ATTENTION", "FUSE_ATTENTION_INT", "SHARE_CROSS_KV")
    old = {n: getattr(UL, n) for n in names}
    for n in names:
        setattr(UL, n, False)
    yield UL
    for n, v in old.items():
        setattr(UL, n, v)


def _labels(s):
    """test_gpu_token_logprob_model.py::test_d's: three candidates per input, one row with an ignored tail."""
    g = torch.Generator().manual_seed(5)
    labels = torch.randint(3, VOCAB, (3 * N, 10), generator=g).to(s.dev)
    labels[4, 7:] = TL.IGNORE
    return labels


class _KProjRows:
    """The rows every encoder-attention k_proj saw, by a forward hook on the module."""

    def __init__(self, model):
        self.rows = []
        self.handles = [layer.encoder_attn.k_proj.register_forward_hook(lambda mod, args, out: self.rows.append(args[0].shape[0]))
                        for layer in model.model.decoder.layers]

    def __enter__(self):
        return self.rows

    def __exit__(self, *exc):
        for h in self.handles:
            h.remove()


def _same_words(got, want):
    return all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                           b.view(torch.int32) if b.dtype == torch.float32 else b) for a, b in zip(got, want))


@pytest.mark.parametrize("switch", SWITCHES)
def test_a_shared_score_is_the_unshared_score(setup, switches, switch):
    m, labels = setup.q, _labels(setup)
    if switch != "off":
        setattr(switches, switch, True)
    with _KProjRows(m) as rows:
        want = m.score(setup.ids, labels, attention_mask=setup.mask, num_candidates=N)
        info = m.last_share_cross_kv
        assert rows == [3 * N, 3 * N] and (info.shared, info.eager, info.reason) == (0, 0, "not asked for"), (rows, info)
        del rows[:]
        got = m.score(setup.ids, labels, attention_mask=setup.mask, num_candidates=N, share_cross_kv=True)
        info = m.last_share_cross_kv
        assert rows == [3, 3], rows                                  # B rows, not B * n
    assert (info.shared, info.eager, info.reason) == (2, 0, None), info
    assert got[0].shape == (3 * N, 10) and got[2].tolist() == [10, 10, 10, 10, 7, 10, 10, 10, 10]
    d = (got[0] - want[0]).abs().max().item()
    print(f"\n{switch}: largest |token_logprob shared - unshared| {d:.3g}, sequence {(got[1] - want[1]).abs().max().item():.3g}")
    assert _same_words(got, want), (switch, d)


def test_b_the_one_launch_forms_take_the_group(setup, switches, monkeypatch):
    """Under FUSE_ATTENTION_INT, and under FUSE_ATTENTION, each layer's cross-attention is ONE grouped launch: the call
    through util_layernorm.attention_sequence_fake_quant with group = n returns a context."""
    from outlier_suppression_amd.model import quant_bart
    m, labels = setup.q, _labels(setup)
    taken = []
    inner = quant_bart.attention_sequence_fake_quant

    def spy(*args, group=1, **kw):
        out = inner(*args, group=group, **kw)
        if group > 1:
            taken.append((group, tuple(args[5].shape), tuple(args[6].shape), out is not None))
        return out
    monkeypatch.setattr(quant_bart, "attention_sequence_fake_quant", spy)
    for switch in ("FUSE_ATTENTION_INT", "FUSE_ATTENTION"):
        del taken[:]
        setattr(switches, switch, True)
        m.score(setup.ids, labels, attention_mask=setup.mask, num_candidates=N, share_cross_kv=True)
        setattr(switches, switch, False)
        assert taken == [(N, (3 * N, 4, 10, 16), (3, 4, 14, 16), True)] * 2, (switch, taken)
    del taken[:]
    m.score(setup.ids, labels, attention_mask=setup.mask, num_candidates=N, share_cross_kv=True)
    assert taken == [(N, (3 * N, 4, 10, 16), (3, 4, 14, 16), False)] * 2, taken         # switches off: k, v and mask are expanded


def test_c_fallbacks(setup, switches):
    import outlier_suppression_amd as osq
    m, labels = setup.q, _labels(setup)
    kw = dict(attention_mask=setup.mask)
    # one candidate per input: nothing to share; the words of the plain call
    want = m.score(setup.ids, labels[::N], **kw)
    got = m.score(setup.ids, labels[::N], share_cross_kv=True, **kw)
    info = m.last_share_cross_kv
    assert (info.shared, info.eager) == (0, 0) and "num_candidates == 1" in info.reason, info
    assert _same_words(got, want)
    # a cross-attention quantizer with its observer on: layer and site are named; the words of the unshared form
    # (an observing quantizer changes as it runs: each form gets a copy of the model of its own)
    want = m.score(setup.ids, labels, num_candidates=N, **kw)
    plain, asked = copy.deepcopy(m), copy.deepcopy(m)
    for x in (plain, asked):
        x.model.decoder.layers[1].encoder_attn.value_post_act_fake_quantize.enable_observer()
    observed = plain.score(setup.ids, labels, num_candidates=N, **kw)
    with _KProjRows(asked) as rows:
        got = asked.score(setup.ids, labels, num_candidates=N, share_cross_kv=True, **kw)
        assert rows == [3 * N, 3 * N], rows
    info = asked.last_share_cross_kv
    assert info.shared == 0 and "not in the plain quantising state (decoder layer 1, value)" in info.reason, info
    assert _same_words(got, observed)
    # the package switch alone turns it on; unset, k_proj sees B * n rows
    with _KProjRows(m) as rows:
        m.score(setup.ids, labels, num_candidates=N, **kw)
        assert rows == [3 * N, 3 * N] and m.last_share_cross_kv.reason == "not asked for"
        del rows[:]
        osq.set_share_cross_kv(True)
        try:
            got = m.score(setup.ids, labels, num_candidates=N, **kw)
            info = m.last_share_cross_kv
            assert rows == [3, 3] and (info.shared, info.eager, info.reason) == (2, 0, None), (rows, info)
            del rows[:]
            m.score(setup.ids, labels, num_candidates=N, share_cross_kv=False, **kw)
            assert rows == [3 * N, 3 * N] and m.last_share_cross_kv.reason == "not asked for"
        finally:
            osq.set_share_cross_kv(False)
    assert _same_words(got, want)
    # the reasons known before the decoder runs
    from outlier_suppression_amd.model import generation
    assert generation.score_share_why_not(m, torch.device("cpu"), N) == "the tensors are on the CPU"
    assert generation.score_share_why_not(m, setup.dev, N) == "autograd is on"           # score() itself runs without it
    layer = m.model.decoder.layers[0]
    old = layer.encoder_attn.dropout
    with torch.no_grad():
        assert generation.score_share_why_not(m, setup.dev, N) is None
        layer.encoder_attn.dropout = 0.1
        m.model.decoder.train()
        try:
            assert generation.score_share_why_not(m, setup.dev, N) == "dropout is active"
        finally:
            layer.encoder_attn.dropout = old
            m.model.decoder.eval()
        assert generation.score_share_why_not(m, setup.dev, N) is None
    # a decoder with a cache has the cache's cross_group, not the keyword
    with torch.no_grad(), pytest.raises(ValueError):
        m(attention_mask=setup.mask, decoder_input_ids=labels[:, :2], encoder_outputs=(m.get_encoder()(setup.ids, setup.mask),),
          use_cache=True, cross_group=N)


def test_d_prefill_over_a_cross_group_cache_takes_the_grouped_launch(setup, switches, monkeypatch):
    """A first call of 4 tokens on a cache with cross_group = 3 under FUSE_ATTENTION_INT: its cross-attention is the grouped
    launch (before, k, v and the mask were expanded), and the logits are those of the same call with the switch off, compared
    as test_gpu_share_cross_kv_model.py::test_f compares its two paths."""
    from outlier_suppression_amd.model import quant_bart
    from outlier_suppression_amd.model.quant_bart import QuantizedBartCache
    m = setup.q
    g = torch.Generator().manual_seed(5)
    dec = torch.randint(3, VOCAB, (3 * N, 6), generator=g).to(setup.dev)
    taken = []
    inner = quant_bart.attention_sequence_fake_quant

    def spy(*args, group=1, **kw):
        out = inner(*args, group=group, **kw)
        if group > 1:
            taken.append(out is not None)
        return out
    monkeypatch.setattr(quant_bart, "attention_sequence_fake_quant", spy)

    def prefill():
        with torch.no_grad():
            enc = m.get_encoder()(setup.ids, attention_mask=setup.mask)
            cache = QuantizedBartCache(len(m.model.decoder.layers), capacity=8, cross_group=N)
            first = m(attention_mask=setup.mask, decoder_input_ids=dec[:, :4], encoder_outputs=(enc,), past_key_values=cache,
                      use_cache=True)[0]
            second = m(attention_mask=setup.mask, decoder_input_ids=dec[:, 4:6], encoder_outputs=(enc,), past_key_values=cache,
                       use_cache=True)[0]
        assert cache._cross[0][0].shape[0] == 3
        return torch.cat([first, second], 1)
    want = prefill()
    assert taken == [False] * 4, taken
    del taken[:]
    switches.FUSE_ATTENTION_INT = True
    got = prefill()
    assert taken == [True] * 4, taken                                 # two layers, two several-token calls
    d = (got - want).abs().max().item()
    print(f"\nprefill over a cross_group cache, FUSE_ATTENTION_INT on vs off, max |logit diff|: {d:.3g}")
    assert d < FUSED_VS_EAGER_LOGITS, d

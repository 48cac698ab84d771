"""sample(num_samples=3, return_logprobs=True) (model/generation.py::sample) on the tiny W6A6 LSQ+ BART of
test_gpu_bart_decode.py, settings of test_gpu_sample_advance_model.py: under every form of the step -- launch by launch, over a
cache of codes, with the model step replayed, with the whole step captured, through the nucleus kernel, without a cache --
and with share_cross_kv on and off, the tokens are those of the torch lines of the same call, shared and unshared forms give
the same tokens, ``last_share_cross_kv`` counts shared steps exactly where sharing applies, and the cache's cross-attention
part is one third of the unshared one.  The log-probabilities of every form agree with those of the eager form (the torch
lines, sampling.token_logprob) within twice the bound of tests/_sample_group.py, taken at the float64 restatement on the
scores the eager steps saw.  What sharing does not take -- more than 64 sequences, CPU tensors -- decodes expanded with a
reason.

The kernel and the torch lines add the same fp32 weights in different orders, so a draw within 2e-5 W of a boundary of the
running sums may select the neighbouring token; the seed below was not met by such a draw."""
import pytest
import torch

import _sample_group as SG
from test_gpu_bart_decode import setup  # noqa: F401  (that file's module fixture)

pytestmark = pytest.mark.gpu

L, N, SEED = 12, 3, 3
SETTINGS = dict(max_length=L, min_length=L - 1, no_repeat_ngram_size=2, forced_bos_token_id=0)
TOP_K = dict(top_k=8, temperature=1.3)
NUCLEUS = dict(top_k=0, top_p=0.9, temperature=1.3)
# form -> (the call's switches, the switches of its torch lines, the draw)
FORMS = {"plain": (dict(sample_advance=True), dict(), TOP_K),
         "codes": (dict(sample_advance=True, cache_codes=True), dict(cache_codes=True), TOP_K),
         "graph": (dict(sample_advance=True, graph=True), dict(graph=True), TOP_K),
         "sample_graph": (dict(sample_graph=True), dict(graph=True), TOP_K),
         "nucleus": (dict(sample_advance=True, sample_nucleus=True), dict(), NUCLEUS),
         "no-cache": (dict(sample_advance=True, use_cache=False), dict(use_cache=False), TOP_K)}


@pytest.fixture()
def switches():
    from outlier_suppression_amd import _hip, util_layernorm as UL
    _hip.load()                      # the first load applies the environment's tier, these switches included
    names = ("SAMPLE_GRAPH", "SAMPLE_ADVANCE", "SAMPLE_NUCLEUS", "SHARE_CROSS_KV", "GRAPH_DECODE", "CACHE_CODES")
    old = [getattr(UL, n) for n in names]
    for n in names:
        setattr(UL, n, False)
    yield UL
    for n, v in zip(names, old):
        setattr(UL, n, v)


@pytest.fixture()
def caches(monkeypatch):
    """The caches sample() builds, in order."""
    from outlier_suppression_amd.model import quant_bart
    made = []

    class Recorded(quant_bart.QuantizedBartCache):
        def __init__(self, *args, **kwargs):
            super().__init__(*args, **kwargs)
            made.append(self)
    monkeypatch.setattr(quant_bart, "QuantizedBartCache", Recorded)
    return made


def _cross_bytes(cache):
    return sum(t.numel() * t.element_size() for pair in cache._cross if pair is not None for t in pair)


@pytest.fixture(scope="module")
def eager(setup):
    """Per draw: the eager form's (tokens, logprobs) and, per position and row, the float64 restatement with its bound on the
    scores that step saw."""
    from outlier_suppression_amd.model import sampling
    out = {}
    for name, draw in (("top-k", TOP_K), ("nucleus", NUCLEUS)):
        steps, select = [], sampling.select_torch

        def recording(scores, u, temperature=1.0, top_k=0, top_p=1.0):
            token = select(scores, u, temperature, top_k, top_p)
            steps.append((scores.cpu().numpy(), token.cpu().numpy()))
            return token
        sampling.select_torch = recording
        try:
            seq, lps = setup.q.sample(setup.ids, attention_mask=setup.mask, seed=SEED, num_samples=N, return_logprobs=True,
                                      sample_advance=False, sample_graph=False, graph=False, cache_codes=False,
                                      share_cross_kv=False, **SETTINGS, **draw)
        finally:
            sampling.select_torch = select
        want = [[SG.logprob64(scores[r], (), draw["temperature"], draw["top_k"], draw.get("top_p", 1.0), token[r])
                 for r in range(seq.shape[0])] for scores, token in steps]
        out[name] = (seq, lps, want)
    return out


def _check_logprobs(lps, eager_of_draw, label, factor):
    seq, _, want = eager_of_draw
    lps = lps.cpu()
    assert lps.shape == seq.shape and lps.dtype == torch.float32 and (lps[:, 0] == 0).all()
    worst = 0.0
    for cur, row in enumerate(want, start=1):
        for r, (lp64, tol) in enumerate(row):
            worst = max(worst, SG.within(float(lps[r, cur]), (lp64, factor * tol), (label, cur, r)) / tol)
    return worst


def test_a_the_eager_form_is_the_restatement(setup, switches, eager):
    for name, (seq, lps, want) in eager.items():
        assert seq.shape == (3 * N, L) and len(want) == L - 1
        assert (seq[:, 1] == 0).all() and (seq[:, -1] == 2).all()           # the forced bos; the configuration's forced eos
        _check_logprobs(lps, eager[name], name, 1.0)
        assert (lps[:, 1] == 0).all() and (lps[:, -1] == 0).all() and (lps[:, 2:-1] < 0).all()
        assert len({tuple(r) for r in seq[:N].tolist()}) > 1


@pytest.mark.parametrize("form", list(FORMS))
def test_b_three_samples_under_every_form_shared_and_unshared(setup, switches, caches, eager, form):
    asked, lines, draw = FORMS[form]
    m, base = setup.q, dict(SETTINGS, attention_mask=setup.mask, seed=SEED, num_samples=N, **draw)
    want = m.sample(setup.ids, sample_advance=False, **lines, **base)       # the torch lines of the same call
    assert want.shape == (3 * N, L) and m.last_sample_advance.advanced == 0
    assert torch.equal(want, eager["nucleus" if form == "nucleus" else "top-k"][0])
    applies = asked.get("use_cache", True)
    seq, lps = m.sample(setup.ids, sample_advance=False, share_cross_kv=True, return_logprobs=True, **lines, **base)
    assert torch.equal(seq, want) and m.last_sample_advance.eager == L - 1  # the torch lines over the shared keys / values
    assert m.last_share_cross_kv.shared == (L - 1 if applies else 0), m.last_share_cross_kv
    _check_logprobs(lps, eager["nucleus" if form == "nucleus" else "top-k"], (form, "torch lines, shared"), 2.0)
    got = {}
    for share in (False, True):
        del caches[:]
        seq, lps = m.sample(setup.ids, share_cross_kv=share, return_logprobs=True, **asked, **base)
        info, steps = m.last_share_cross_kv, L - 1
        assert seq.shape == want.shape and seq.dtype == want.dtype and torch.equal(seq, want), (form, share)
        assert (m.last_sample_advance.advanced, m.last_sample_advance.eager, m.last_sample_advance.reason) == (steps, 0, None)
        if share and applies:
            assert (info.shared, info.eager, info.reason) == (steps, 0, None), info
        else:
            assert (info.shared, info.eager) == (0, steps), info
            assert info.reason == ("use_cache=False: there is no cache" if share else "not asked for")
        if form == "sample_graph":
            whole = m.last_sample_graph
            assert whole.reason is None and whole.captured == 1 and whole.replays == steps - 2, whole
        if asked.get("graph") or form == "sample_graph":
            assert m.last_decode_graph.captured == 1 and m.last_decode_graph.reason is None
        assert len(caches) == (1 if applies else 0)
        got[share] = (seq, lps, caches[0] if applies else None)
        _check_logprobs(lps, eager["nucleus" if form == "nucleus" else "top-k"], (form, share), 2.0)
    assert torch.equal(got[False][0], got[True][0])
    if applies:
        plain, shared = got[False][2], got[True][2]
        assert (plain.cross_group, shared.cross_group) == (1, N)
        cross = _cross_bytes(plain)
        assert cross > 0 and cross % N == 0 and _cross_bytes(shared) == cross // N
        assert plain.nbytes() - shared.nbytes() == cross // N * (N - 1)
    # asking for the log-probabilities changes no token; one sample is today's call
    assert torch.equal(m.sample(setup.ids, share_cross_kv=True, **asked, **base), want)
    one = m.sample(setup.ids, **asked, **dict(base, num_samples=1))
    assert torch.equal(one, m.sample(setup.ids, **asked, **{k: v for k, v in base.items() if k != "num_samples"}))
    assert torch.equal(one, want[::N])


def test_c_what_sharing_does_not_take_decodes_expanded_with_a_reason(setup, switches):
    m = setup.q
    kw = dict(attention_mask=setup.mask, max_length=4, seed=SEED, top_k=8, sample_advance=True)
    many = m.sample(setup.ids, num_samples=65, share_cross_kv=True, **kw)
    info = m.last_share_cross_kv
    assert many.shape == (3 * 65, 4) and (info.shared, info.eager) == (0, 3) and "64" in info.reason
    assert torch.equal(many.view(3, 65, 4)[:, :N], m.sample(setup.ids, num_samples=N, share_cross_kv=True, **kw).view(3, N, 4))
    assert m.last_share_cross_kv.shared == 3
    from test_bart_decode_cpu import batch, tiny_bart, wrapped
    q = wrapped(tiny_bart())
    ids, mask = batch()
    kw = dict(attention_mask=mask, max_length=8, min_length=8, seed=4, top_k=8, num_samples=N)
    want = q.sample(ids, **kw)
    got, lps = q.sample(ids, share_cross_kv=True, sample_graph=True, return_logprobs=True, **kw)
    assert torch.equal(got, want) and got.shape == lps.shape == (3 * N, 8)
    assert "CPU" in q.last_share_cross_kv.reason and "CPU" in q.last_sample_graph.reason and q.last_share_cross_kv.shared == 0


def test_d_the_switch(setup, switches):
    import outlier_suppression_amd as osq
    m, kw = setup.q, dict(SETTINGS, attention_mask=setup.mask, seed=SEED, num_samples=N, sample_advance=True, **TOP_K)
    want = m.sample(setup.ids, **kw)
    assert m.last_share_cross_kv.reason == "not asked for"
    osq.set_share_cross_kv(True)
    assert torch.equal(m.sample(setup.ids, **kw), want) and m.last_share_cross_kv.shared == L - 1
    assert torch.equal(m.sample(setup.ids, share_cross_kv=False, **kw), want) and m.last_share_cross_kv.shared == 0
    m.sample(setup.ids, **dict(kw, num_samples=1))                          # one sequence per input: nothing to share
    assert m.last_share_cross_kv.reason is not None and m.last_share_cross_kv.shared == 0
    osq.set_share_cross_kv(False)

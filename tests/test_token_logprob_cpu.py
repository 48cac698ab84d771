"""Teacher-forced scoring without a GPU: the float64 restatement of tests/_token_logprob.py against F.cross_entropy and autograd
in float64; losses.token_logprob_torch against the restatement; losses.lm_loss with the switch off (F.cross_entropy's words)
and on over CPU tensors (a fall-back with its reason, the same words); and score() on the tiny CPU BART of
test_bart_decode_cpu.py."""
import numpy as np
import pytest
import torch
from torch.nn import functional as F

import _token_logprob as TL
from test_bart_decode_cpu import batch, tiny_bart, wrapped


@pytest.fixture()
def switch():
    from outlier_suppression_amd import util_layernorm as UL
    old = UL.FAST_LM_LOSS
    yield UL
    UL.FAST_LM_LOSS = old


def _labels(kind, rng, rows, vocab):
    labels = rng.integers(0, vocab, rows).astype(np.int64)
    if kind == "mixed":
        labels[::3] = TL.IGNORE
    elif kind == "all":
        labels[:] = TL.IGNORE
    return labels


@pytest.mark.parametrize("kind", ("mixed", "none", "all"))
@pytest.mark.parametrize("ignore_index", (TL.IGNORE, 7))
def test_a_the_restatement_is_cross_entropy_in_float64(kind, ignore_index):
    rng = np.random.default_rng(3)
    rows, vocab = 23, 131
    logits = (rng.standard_normal((rows, vocab)) * 3).astype(np.float32)
    labels = _labels(kind, rng, rows, vocab)
    labels[labels == TL.IGNORE] = ignore_index
    want = TL.forward64(logits, labels, ignore_index)
    z = torch.from_numpy(logits).double().requires_grad_(True)
    t = torch.from_numpy(labels)
    none = F.cross_entropy(z, t, reduction="none", ignore_index=ignore_index)
    np.testing.assert_allclose(-none.detach().numpy(), want["lp"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(torch.logsumexp(z, -1).detach().numpy(), want["lse"], rtol=0, atol=1e-12)
    mean = F.cross_entropy(z, t, ignore_index=ignore_index)
    assert int(want["scored"].sum()) == int((t != ignore_index).sum()) and not want["bad"].any()
    if kind == "all":
        assert np.isnan(want["loss"]) and torch.isnan(mean)
    else:
        assert abs(float(mean.detach()) - want["loss"]) < 1e-12
    # backward: reduction='none' under a random upstream gradient, and the mean
    up = rng.standard_normal(rows)
    (grad,) = torch.autograd.grad((none * torch.from_numpy(up)).sum(), z, retain_graph=True)
    d, tol = TL.backward64(logits, labels, up, ignore_index)
    np.testing.assert_allclose(grad.numpy(), d, rtol=0, atol=1e-12)
    assert (d[labels == ignore_index] == 0).all() and (tol[labels == ignore_index] == 0).all()
    assert (tol[labels != ignore_index] > 0).all() and tol.max() < 1e-3
    if kind != "all":
        (grad,) = torch.autograd.grad(mean * 1.5, z)
        d, _ = TL.backward64(logits, labels, np.full(rows, 1.5 / want["scored"].sum()), ignore_index)
        np.testing.assert_allclose(grad.numpy(), d, rtol=0, atol=1e-12)


def test_b_the_restatement_on_the_constructed_rows():
    logits, labels, notes = TL.constructed_case(np.random.default_rng(5), 37)
    want = TL.forward64(logits, labels)
    at = {n: i for i, n in enumerate(notes)}
    assert want["lp"][at["survivor, label on it"]] == 0.0 and want["lse"][at["survivor, label on it"]] == -3.25
    assert want["lp"][at["survivor, label elsewhere"]] == -np.inf
    for n in ("all -inf", "a NaN", "+inf", "label -1", "label V"):
        assert np.isnan(want["lp"][at[n]]), n
    assert want["lp"][at["ordinary, ignored"]] == 0.0 and np.isfinite(want["lse"][at["ordinary, ignored"]])
    assert np.isfinite(want["lp"][at["near 1e+30"]]) and np.isfinite(want["lp"][at["near -1e+30"]])
    assert want["bad"].sum() == 2 and want["scored"].sum() == len(notes) - 3 and np.isnan(want["loss"])
    d, tol = TL.backward64(logits, labels, np.ones(len(notes)))
    for n in ("ordinary, ignored", "label -1", "label V"):
        assert (d[at[n]] == 0).all() and (tol[at[n]] == 0).all()
    assert TL.seams(8193) == [0, 3, 4, 1023, 1024, 4095, 4096, 8191, 8192]
    assert TL.seams(1) == [0] and TL.seams(4096)[-2:] == [1024, 4095]


def test_c_token_logprob_torch_is_the_restatement():
    from outlier_suppression_amd.model.losses import token_logprob_torch
    rng = np.random.default_rng(11)
    logits, labels = TL.random_case(rng, 40, 97)
    assert (labels == TL.IGNORE).any()
    want = TL.forward64(logits, labels)
    got = token_logprob_torch(torch.from_numpy(logits), torch.from_numpy(labels))
    assert got.dtype == torch.float32 and got.shape == (40,)
    assert (np.abs(got.numpy() - want["lp"]) <= want["tol"]).all()
    assert (got.numpy()[labels == TL.IGNORE] == 0).all()
    # any leading shape, another ignore_index
    labels[labels == TL.IGNORE] = 5
    got = token_logprob_torch(torch.from_numpy(logits).view(5, 8, 97), torch.from_numpy(labels).view(5, 8), ignore_index=5)
    want = TL.forward64(logits, labels, 5)
    assert got.shape == (5, 8) and (np.abs(got.numpy().ravel() - want["lp"]) <= want["tol"]).all()


def test_d_lm_loss_switch_off_is_cross_entropy_and_on_falls_back_on_the_cpu(switch):
    from outlier_suppression_amd.model import losses
    import outlier_suppression_amd as osq
    rng = np.random.default_rng(13)
    logits, labels = TL.random_case(rng, 24, 120)
    z, t = torch.from_numpy(logits).view(3, 8, 120), torch.from_numpy(labels).view(3, 8)
    want = F.cross_entropy(z.view(-1, 120), t.view(-1))
    osq.set_fast_lm_loss(False)
    assert switch.FAST_LM_LOSS is False
    info = losses.LmLossInfo()
    got = losses.lm_loss(z, t, 120, info)
    assert got.view(torch.int32) == want.view(torch.int32)
    assert (info.fused, info.eager, info.reason, info.bad_labels) == (0, 1, "not asked for", None)
    assert losses.lm_loss(z, t, 120).view(torch.int32) == want.view(torch.int32) and losses.lm_loss(z, None, 120) is None
    osq.set_fast_lm_loss(True)
    assert switch.FAST_LM_LOSS is True
    info = losses.LmLossInfo()
    got = losses.lm_loss(z, t, 120, info)
    assert got.view(torch.int32) == want.view(torch.int32)
    assert (info.fused, info.eager, info.bad_labels) == (0, 1, None) and "CPU" in info.reason
    zg = z.clone().requires_grad_(True)
    losses.lm_loss(zg, t, 120).backward()
    ze = z.clone().requires_grad_(True)
    F.cross_entropy(ze.view(-1, 120), t.view(-1)).backward()
    assert torch.equal(zg.grad, ze.grad)
    assert osq.fast_lm_loss_from_environment({}) is False and osq.fast_lm_loss_from_environment({"OSQ_FAST_LM_LOSS": "0"}) is False
    assert osq.fast_lm_loss_from_environment({"OSQ_FAST_LM_LOSS": "1"}) is True


@pytest.fixture(scope="module")
def model():
    return wrapped(tiny_bart())


def _targets(rows, steps, seed=2):
    g = torch.Generator().manual_seed(seed)
    labels = torch.randint(3, 120, (rows, steps), generator=g)
    labels[1, steps - 2:] = TL.IGNORE
    return labels


def test_e_score_is_the_cross_entropy_of_forwards_own_logits(model, switch):
    ids, mask = batch()
    labels = _targets(3, 7)
    tok, seq, lengths = model.score(ids, labels, attention_mask=mask)
    with torch.no_grad():
        out = model(ids, mask, labels=labels)
    loss, logits = out[0], out[1]
    assert model.last_lm_loss.reason == "not asked for" and model.last_lm_loss.eager == 1
    want = -F.cross_entropy(logits.view(-1, 120), labels.view(-1), reduction="none").view(3, 7)
    assert tok.dtype == torch.float32 and tok.shape == (3, 7) and seq.shape == (3,) and lengths.tolist() == [7, 5, 7]
    assert torch.allclose(tok, want, rtol=0, atol=1e-6) and (tok[labels == TL.IGNORE] == 0).all()
    assert torch.allclose(-tok.sum() / lengths.sum(), loss, rtol=0, atol=1e-6)
    run = torch.zeros(3)
    for t in range(7):
        run += tok[:, t]
    assert torch.equal(seq, run)
    # another ignore_index, no attention mask given
    other = labels.masked_fill(labels == TL.IGNORE, 1)
    tok1, _, lengths1 = model.score(ids, other, ignore_index=1)
    assert lengths1.tolist() == [7, 5, 7] and (tok1[other == 1] == 0).all()


def test_f_three_candidates_are_the_expanded_forward_word_for_word(model):
    from outlier_suppression_amd.model.losses import token_logprob_torch
    from outlier_suppression_amd.model.quant_bart import shift_tokens_right
    ids, mask = batch()
    n = 3
    labels = _targets(3 * n, 6, seed=4)
    tok, seq, lengths = model.score(ids, labels, attention_mask=mask, num_candidates=n)
    with torch.no_grad():
        enc = model.get_encoder()(ids, attention_mask=mask).repeat_interleave(n, dim=0)
        logits = model(attention_mask=mask.repeat_interleave(n, dim=0), encoder_outputs=(enc,),
                       decoder_input_ids=shift_tokens_right(labels, 1, 2))[0]
    assert tok.shape == (9, 6) and torch.equal(tok, token_logprob_torch(logits, labels))
    # the row layout b * n + j: candidate j of input b scored alone, with that input alone
    for b, j in ((0, 0), (1, 2), (2, 1)):
        r = b * n + j
        one, one_seq, one_len = model.score(ids[b:b + 1], labels[r:r + 1], attention_mask=mask[b:b + 1])
        assert torch.allclose(one[0], tok[r], rtol=0, atol=1e-5) and one_len[0] == lengths[r]
        assert torch.allclose(one_seq[0], seq[r], rtol=0, atol=1e-5)
    with pytest.raises(ValueError):
        model.score(ids, labels[:8], attention_mask=mask, num_candidates=n)


def test_g_a_label_outside_the_vocabulary_is_refused(model):
    ids, mask = batch()
    for where, value in (((0, 2), 120), ((2, 6), 4000), ((1, 0), -1)):
        labels = _targets(3, 7)
        labels[where] = value
        with pytest.raises(ValueError, match="outside the vocabulary"):
            model.score(ids, labels, attention_mask=mask)

"""Teacher-forced scoring on the tiny W6A6 LSQ+ BART of test_gpu_bart_decode.py: forward(labels=...) with set_fast_lm_loss on
against off (the loss inside the kernel's bound, logits.grad inside the backward bound -- the logits are the same words, so
the kernel bounds of tests/_token_logprob.py apply -- and a quantizer scale's gradient), score() against the float64
restatement on its own logits, three candidates per input word-equal to the forward over the expanded encoder states, and
score()'s sequence log-probability of sample(num_samples=3, top_k=0, top_p=1.0)'s sequences against that call's own summed
log-probabilities up to each row's first eos."""
import numpy as np
import pytest
import torch

import _token_logprob as TL
from test_gpu_bart_decode import setup  # noqa: F401  (that file's module fixture)

pytestmark = pytest.mark.gpu

VOCAB = 120


@pytest.fixture()
def switch():
    from outlier_suppression_amd import _hip, util_layernorm as UL
    _hip.load()                      # the first load applies the environment's tier, this switch included
    old = UL.FAST_LM_LOSS
    UL.FAST_LM_LOSS = False
    yield UL
    UL.FAST_LM_LOSS = old


def _labels(setup):
    labels = setup.dec.clone()
    labels[1, 9:] = TL.IGNORE
    return labels


def test_a_forward_loss_with_the_switch_on_against_off(setup, switch):
    import outlier_suppression_amd as osq
    m, labels = setup.q, _labels(setup)
    with torch.no_grad():
        eager, logits = m(setup.ids, setup.mask, labels=labels)[:2]
    assert (m.last_lm_loss.fused, m.last_lm_loss.eager, m.last_lm_loss.reason) == (0, 1, "not asked for")
    assert m.last_lm_loss.bad_labels is None
    osq.set_fast_lm_loss(True)
    with torch.no_grad():
        fused, logits_on = m(setup.ids, setup.mask, labels=labels)[:2]
    info = m.last_lm_loss
    assert (info.fused, info.eager, info.reason) == (1, 0, None) and info.bad_labels == 0
    assert torch.equal(logits, logits_on) and fused.shape == eager.shape and fused.dtype == torch.float32
    want = TL.forward64(logits.view(-1, VOCAB).cpu().numpy(), labels.view(-1).cpu().numpy())
    print(f"loss: fused {float(fused):.9g} eager {float(eager):.9g} float64 {want['loss']:.12g} bound {want['loss_tol']:.3g}")
    assert abs(float(fused) - want["loss"]) <= want["loss_tol"]
    assert abs(float(fused) - float(eager)) <= 2 * want["loss_tol"]
    # what the kernels do not take falls back with its reason
    from outlier_suppression_amd.model import losses
    li = losses.LmLossInfo()
    got = losses.lm_loss(logits.double(), labels, VOCAB, li)
    assert (li.fused, li.eager) == (0, 1) and "float64" in li.reason and got.dtype == torch.float64


def test_b_gradients_with_the_switch_on_against_off(setup, switch):
    import outlier_suppression_amd as osq
    m, labels = setup.q, _labels(setup)
    scales = [p for n, p in m.named_parameters() if n.endswith("scale") and p.requires_grad]
    assert scales, "the LSQ+ activation quantizers have learnable scales"
    grads = {}
    for on in (False, True):
        osq.set_fast_lm_loss(on)
        m.zero_grad(set_to_none=True)
        out = m(setup.ids, setup.mask, labels=labels)
        loss, logits = out[0], out[1]
        logits.retain_grad()
        (loss * 1.5).backward()
        assert m.last_lm_loss.fused == int(on)
        grads[on] = (logits.detach().clone(), logits.grad.detach().clone(), [p.grad.detach().clone() for p in scales])
    m.zero_grad(set_to_none=True)
    assert torch.equal(grads[False][0], grads[True][0])                             # the same logits
    z = grads[True][0].view(-1, VOCAB).cpu().numpy()
    t = labels.view(-1).cpu().numpy()
    n = int((t != TL.IGNORE).sum())
    d, tol = TL.backward64(z, t, np.full(t.shape[0], 1.5 / n))
    fused = grads[True][1].view(-1, VOCAB).cpu().numpy().astype(np.float64)
    eager = grads[False][1].view(-1, VOCAB).cpu().numpy().astype(np.float64)
    print(f"logits.grad: max |fused - float64| {np.abs(fused - d).max():.3g}, max |eager - float64| {np.abs(eager - d).max():.3g}, "
          f"largest bound {tol.max():.3g}")
    assert (np.abs(fused - d) <= tol).all()
    assert (np.abs(fused - eager) <= 2 * tol + 2.0 ** -22 * np.abs(d)).all()       # torch's own rounding of the same quantity
    assert (fused[t == TL.IGNORE] == 0).all()
    assert all(torch.isfinite(g).all() for g in grads[True][2])
    assert any(float(g.abs().max()) > 0 for g in grads[True][2])
    worst = max(float((a - b).abs().max() / b.abs().max().clamp_min(1e-30)) for a, b in zip(grads[True][2], grads[False][2]))
    print(f"quantizer scale gradients: largest relative difference fused against eager {worst:.3g}")


def test_c_score_against_float64_on_its_own_logits(setup, switch):
    m, labels = setup.q, _labels(setup)
    tok, seq, lengths = m.score(setup.ids, labels, attention_mask=setup.mask)
    with torch.no_grad():
        logits = m(setup.ids, setup.mask, labels=labels)[1]
    want = TL.forward64(logits.view(-1, VOCAB).cpu().numpy(), labels.view(-1).cpu().numpy())
    assert tok.shape == labels.shape and tok.dtype == torch.float32 and lengths.tolist() == [12, 9, 12]
    got = tok.view(-1).cpu().numpy().astype(np.float64)
    assert (np.abs(got - want["lp"]) <= want["tol"]).all() and (tok[labels == TL.IGNORE] == 0).all()
    run = torch.zeros(3, device=tok.device)
    for t in range(tok.shape[1]):
        run += tok[:, t]
    assert torch.equal(seq, run)
    bad = labels.clone()
    bad[2, 11] = VOCAB
    with pytest.raises(ValueError, match="outside the vocabulary"):
        m.score(setup.ids, bad, attention_mask=setup.mask)


def test_d_three_candidates_are_the_expanded_forward(setup, switch):
    from outlier_suppression_amd import ops
    from outlier_suppression_amd.model.quant_bart import shift_tokens_right
    m, n = setup.q, 3
    g = torch.Generator().manual_seed(5)
    labels = torch.randint(3, VOCAB, (3 * n, 10), generator=g).to(setup.dev)
    labels[4, 7:] = TL.IGNORE
    tok, seq, lengths = m.score(setup.ids, labels, attention_mask=setup.mask, num_candidates=n)
    with torch.no_grad():
        enc = m.get_encoder()(setup.ids, attention_mask=setup.mask).repeat_interleave(n, dim=0)
        logits = m(attention_mask=setup.mask.repeat_interleave(n, dim=0), encoder_outputs=(enc,),
                   decoder_input_ids=shift_tokens_right(labels, 1, 2))[0]
    want, _ = ops.token_logprob(logits.view(-1, VOCAB), labels.view(-1))
    assert tok.shape == (9, 10) and torch.equal(tok, want.view(9, 10)) and lengths.tolist() == [10, 10, 10, 10, 7, 10, 10, 10, 10]
    ref = TL.forward64(logits.view(-1, VOCAB).cpu().numpy(), labels.view(-1).cpu().numpy())
    assert (np.abs(tok.view(-1).cpu().numpy() - ref["lp"]) <= ref["tol"]).all()
    # the layout b * n + j: with the inputs reversed and their groups of candidates moved along, the rows move with them
    order = torch.tensor([2, 1, 0], device=setup.dev)
    moved = labels.view(3, n, 10)[order].reshape(3 * n, 10)
    tok2, seq2, lengths2 = m.score(setup.ids[order], moved, attention_mask=setup.mask[order], num_candidates=n)
    assert torch.allclose(tok2.view(3, n, 10), tok.view(3, n, 10)[order], rtol=0, atol=1e-4)
    assert torch.allclose(seq2.view(3, n), seq.view(3, n)[order], rtol=0, atol=1e-3)
    assert torch.equal(lengths2.view(3, n), lengths.view(3, n)[order])


def test_e_the_sequences_of_sample_score_as_that_call_says(setup, switch):
    """sample() over the whole vocabulary draws from the model's own distribution, so its log-probabilities are score()'s --
    but for the last column, where the configuration's forced eos makes sample() say 0: it is left out, as is what follows a
    row's first eos (sample() pads there).  Two model paths are compared here (cached steps against one teacher-forced
    pass), not the kernel."""
    m, n, L = setup.q, 3, 12
    seqs, lps = m.sample(setup.ids, attention_mask=setup.mask, seed=3, num_samples=n, top_k=0, top_p=1.0, max_length=L,
                         return_logprobs=True)
    assert seqs.shape == (3 * n, L) and lps.shape == seqs.shape
    labels = seqs[:, 1:L - 1].clone()                  # column 0 is the decoder's start token: score() shifts it back in
    T = labels.shape[1]
    eos = labels == 2
    first = torch.where(eos.any(1), eos.int().argmax(1), torch.full((3 * n,), T - 1, device=labels.device))
    keep = torch.arange(T, device=labels.device)[None, :] <= first[:, None]           # up to and including the first eos
    labels[~keep] = TL.IGNORE
    tok, seq, lengths = m.score(setup.ids, labels, attention_mask=setup.mask, num_candidates=n)
    assert lengths.tolist() == (first + 1).tolist()
    with torch.no_grad():
        enc = m.get_encoder()(setup.ids, attention_mask=setup.mask).repeat_interleave(n, dim=0)
        logits = m(attention_mask=setup.mask.repeat_interleave(n, dim=0), decoder_input_ids=seqs[:, :T], encoder_outputs=(enc,))[0]
    ref = TL.forward64(logits.view(-1, VOCAB).cpu().numpy(), labels.reshape(-1).cpu().numpy())
    tol = 2 * ref["tol"].reshape(3 * n, T).sum(1)                  # twice the per-token bound over the row's scored tokens
    said = (lps[:, 1:L - 1] * keep).double().sum(1).cpu().numpy()
    off = np.abs(seq.double().cpu().numpy() - said)
    print("sequence log-probability, score() against sample()'s own: |difference| per row", off, "bound", tol)
    assert (off <= tol).all()

"""One loss.backward() of the tiny W6A6 BERT (and a tiny BART) in learn_scale's state with FUSE_HEADS_BACKWARD, against the
eager run.

The forward is bit-identical, so the loss is word-equal.  The four head sites per layer: scale.grad / zero_point.grad within
the order-free tier's bar, max(3 e_ref, 4) U + 1 ulp (tests/_lsq_backward_reference.py), of the exact float64 sums over the
site's own (x, dy), which hooks take from the eager run.  Every other quantizer: within 4x the largest relative distance the
eager default tier keeps from the eager strict tier on this model, the bar of tests/test_gpu_site_backward_model.py.  Figures
are printed before they are asserted (profiles/heads_backward_accuracy.txt)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _lsq_backward_reference as R  # noqa: E402
from conftest import bits_equal  # noqa: E402
from test_gpu_site_backward_model import A_Q, W_Q, _distance  # noqa: E402

from oracle import fake_quant_oracle as FQ  # noqa: E402

pytestmark = pytest.mark.gpu
HEAD_SITES = ("query_permute_post", "key_transpose_post", "value_permute_post", "context_view_post")
N = lambda t: t.detach().cpu().numpy()      # noqa: E731


def _learn_scale_state(fp, batch, call):
    """The quantized model calibrated on ``batch`` and put in learn_scale's state; (model, target, quantizers)."""
    from outlier_suppression_amd import token_wise_clipping as TWC
    from outlier_suppression_amd.quant_model import quantize_model
    from outlier_suppression_amd.quantization import disable_all
    from outlier_suppression_amd.quantization.state import set_observer_name
    with torch.no_grad():
        target = call(fp)[0].detach()
    model = quantize_model(fp, W_Q, A_Q).to(target.device)
    disable_all(model)
    set_observer_name(model)
    TWC.set_ratio(model, 1.0)
    TWC.calibrate(model, [batch])
    disable_all(model)
    quantizers = dict(TWC._act_quantizers(model))
    for q in quantizers.values():
        q.enable_fake_quant()
        q.disable_observer()
    return model, target, quantizers


@pytest.fixture(scope="module")
def bert():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from transformers import BertConfig, BertForSequenceClassification
    dev = torch.device("cuda:0")
    torch.manual_seed(5)
    cfg = BertConfig(vocab_size=90, hidden_size=32, num_hidden_layers=2, num_attention_heads=2, intermediate_size=64,
                     max_position_embeddings=48, num_labels=2, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    gen = torch.Generator().manual_seed(3)
    lengths = torch.tensor([40, 33, 17, 8])
    mask = (torch.arange(40)[None, :] < lengths[:, None]).long()
    ids = torch.randint(1, 90, (4, 40), generator=gen) * mask
    batch = {"input_ids": ids.to(dev), "attention_mask": mask.to(dev), "token_type_ids": torch.zeros_like(ids).to(dev)}
    return _learn_scale_state(BertForSequenceClassification(cfg).eval().to(dev), batch, lambda m: m(**batch)) + (batch,)


@pytest.fixture(scope="module")
def bart():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from transformers import BartConfig, BartForConditionalGeneration
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    cfg = BartConfig(vocab_size=120, d_model=32, encoder_layers=1, decoder_layers=1, encoder_attention_heads=2,
                     decoder_attention_heads=2, encoder_ffn_dim=64, decoder_ffn_dim=64, max_position_embeddings=40,
                     dropout=0.0, attention_dropout=0.0, activation_dropout=0.0, pad_token_id=1, bos_token_id=0,
                     eos_token_id=2, decoder_start_token_id=2)
    g = torch.Generator().manual_seed(1)
    ids, dec = torch.randint(3, 120, (2, 9), generator=g).to(dev), torch.randint(3, 120, (2, 5), generator=g).to(dev)
    batch = {"input_ids": ids, "attention_mask": torch.ones_like(ids), "decoder_input_ids": dec}
    return _learn_scale_state(BartForConditionalGeneration(cfg).eval().to(dev), batch, lambda m: m(**batch)) + (batch,)


def _grads(state, heads=False, strict=False, capture=None):
    """(loss, {name: (scale.grad, zero_point.grad)}) of one backward.  ``capture``: a dict that receives, per named
    quantizer, the (x, dy) its eager call saw."""
    import outlier_suppression_amd as osq
    from outlier_suppression_amd import ops, token_wise_clipping as TWC, util_layernorm as U
    model, target, quantizers, batch = state
    params = [p for q in quantizers.values() for p in (q.scale, q.zero_point)]
    saved = (U.FUSE_HEADS_BACKWARD, {k: ops._tuning.get(k, 0) for k in ("mse_sum_order", "bwd_sum_order")})
    U.FUSE_HEADS_BACKWARD = heads
    if strict:
        osq.set_strict(True)
    U.heads_backward.reset()
    hooks = []
    for n in (capture if capture is not None else ()):
        def hook(_m, args, out, n=n):
            out.register_hook(lambda g, n=n, x=args[0].detach(): capture.__setitem__(n, (N(x), N(g))))
        hooks.append(quantizers[n].register_forward_hook(hook))
    try:
        with TWC._only_these_learn(model, params):
            for p in params:
                p.grad = None
            loss = TWC.batch_loss(model(**batch), batch, target, "glue")
            loss.backward()
        return loss.detach(), {n: (q.scale.grad.clone(), q.zero_point.grad.clone()) for n, q in quantizers.items()}
    finally:
        for h in hooks:
            h.remove()
        U.FUSE_HEADS_BACKWARD = saved[0]
        for k, v in saved[1].items():
            ops.set_tuning(k, v)


def test_bert_one_backward(bert):
    from outlier_suppression_amd import util_layernorm as U
    quantizers = bert[2]
    head = [n for n in quantizers if any(s in n for s in HEAD_SITES)]
    others = [n for n in quantizers if n not in head]
    assert len(head) == 8 and others
    seen = dict.fromkeys(head)
    loss_e, eager = _grads(bert, capture=seen)
    _, strict = _grads(bert, strict=True)
    loss_f, fused = _grads(bert, heads=True)
    r = U.heads_backward
    assert (r.split, r.merge, r.eager) == (2, 2, 0), r
    assert bits_equal(N(loss_f), N(loss_e))
    for n in head:
        q, (x, dy) = quantizers[n], seen[n]
        gf = q._grad_factor(U._Numel(x.size))
        s, z = N(q.scale).astype(np.float32), N(q.zero_point).astype(np.float32)
        e = FQ.lsq_backward_exact(x, dy, s, z, q.quant_min, q.quant_max, gf, "lsqplus")
        _, ref_s, ref_z = FQ.lsq_backward_reference_order(x, dy, s, z, q.quant_min, q.quant_max, gf, "lsqplus")
        for got, exact, A, ref, name in ((fused[n][0], e.dscale, e.A_s, ref_s, "ds"), (fused[n][1], e.dzp, e.A_z, ref_z, "dz")):
            fac = FQ.lsq_grad_factors(np.float32(gf), "lsqplus")[name == "dz"]
            e_k, bar = R.units(N(got), exact, A, fac), R.bar_units(R.units(ref, exact, A, fac), exact, A, fac)
            print(f"model     {n:<76} {name} {float(exact[0]):+.4e}  e_k {float(e_k.max()):.3f} units  bar {float(bar.max()):.3f}")
            assert (e_k <= bar).all(), (n, name, e_k, bar)
    tiers, got = _distance(strict, eager, others), _distance(fused, eager, others)
    print(f"model     tiny BERT, head sites fused: other quantizers' distance from eager {got:.3e}; eager default from strict {tiers:.3e}; bar {4 * tiers:.3e}")
    assert got <= 4 * tiers

    _grads(bert, heads=True, strict=True)
    assert (r.split, r.merge, r.eager) == (0, 0, 4) and r.reason == "the strict summation tier is defined on the eager tensors"


def test_bart_one_backward(bart):
    """Encoder and decoder self-attention: the three sites in one launch each; cross-attention (keys / values of another
    length): split_heads_fake_quant, three single-site launches; bmm hands every key's gradient back as the transposed view."""
    from outlier_suppression_amd import util_layernorm as U
    loss_e, eager = _grads(bart)
    _, strict = _grads(bart, strict=True)
    loss_f, fused = _grads(bart, heads=True)
    r = U.heads_backward
    assert (r.split, r.merge, r.eager) == (2 + 3, 3, 0), r
    assert bits_equal(N(loss_f), N(loss_e))
    assert all(torch.isfinite(g).all() for pair in fused.values() for g in pair)
    tiers, got = _distance(strict, eager, list(eager)), _distance(fused, eager, list(eager))
    print(f"model     tiny BART, head sites fused: every quantizer's distance from eager {got:.3e}; eager default from strict {tiers:.3e}; bar {4 * tiers:.3e}")
    assert got <= 4 * tiers

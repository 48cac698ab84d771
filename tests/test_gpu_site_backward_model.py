"""One loss.backward() of the tiny W6A6 BERT in learn_scale's state with FUSE_BACKWARD, against the eager run.

GELU-site quantizers: scale.grad / zero_point.grad word-equal to eager (bit-identical forward, word-equal sums).  Every other
quantizer sits upstream of a fused dx that differs from eager's by roundings: its gradient's relative distance from the eager
run stays within 4x the largest relative distance the eager default tier keeps from the eager strict tier on this model -- both
are accepted forms of the same gradient.  Figures are printed before they are asserted (profiles/site_backward_accuracy.txt)."""
from types import SimpleNamespace as NS

import pytest
import torch

from conftest import bits_equal

pytestmark = pytest.mark.gpu
A_Q = NS(quantizer="LSQPlusFakeQuantize", observer="AvgPruneMinMaxObserver", bit=6, symmetric=False, ch_axis=-1)
W_Q = NS(quantizer="FixedFakeQuantize", observer="MinMaxObserver", bit=6, symmetric=True, ch_axis=0)
GELU_SITE = "act_fn_post_act_fake_quantize"


@pytest.fixture(scope="module")
def model_and_batch():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from transformers import BertConfig, BertForSequenceClassification
    from outlier_suppression_amd import token_wise_clipping as TWC
    from outlier_suppression_amd.quant_model import quantize_model
    from outlier_suppression_amd.quantization import disable_all
    from outlier_suppression_amd.quantization.state import set_observer_name
    dev = torch.device("cuda:0")
    torch.manual_seed(5)
    cfg = BertConfig(vocab_size=90, hidden_size=32, num_hidden_layers=2, num_attention_heads=2, intermediate_size=64,
                     max_position_embeddings=48, num_labels=2, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    fp = BertForSequenceClassification(cfg).eval().to(dev)
    gen = torch.Generator().manual_seed(3)
    lengths = torch.tensor([40, 33, 17, 8])
    mask = (torch.arange(40)[None, :] < lengths[:, None]).long()
    ids = torch.randint(1, 90, (4, 40), generator=gen) * mask
    batch = {"input_ids": ids.to(dev), "attention_mask": mask.to(dev), "token_type_ids": torch.zeros_like(ids).to(dev)}
    with torch.no_grad():
        target = fp(**batch)[0].detach()
    model = quantize_model(fp, W_Q, A_Q).to(dev)
    disable_all(model)
    set_observer_name(model)
    TWC.set_ratio(model, 1.0)
    TWC.calibrate(model, [batch])
    disable_all(model)                      # learn_scale's state: activation quantizers quantise, only their parameters learn
    quantizers = dict(TWC._act_quantizers(model))
    for q in quantizers.values():
        q.enable_fake_quant()
        q.disable_observer()
    return model, batch, target, quantizers


def _grads(model_and_batch, backward=False, softmax=False, strict=False):
    """``strict``: the public switch, outlier_suppression_amd.set_strict(True) (both summation orders the reference's)."""
    import outlier_suppression_amd as osq
    from outlier_suppression_amd import ops, token_wise_clipping as TWC, util_layernorm as U
    model, batch, target, quantizers = model_and_batch
    params = [p for q in quantizers.values() for p in (q.scale, q.zero_point)]
    saved = (U.FUSE_BACKWARD, U.FUSE_SOFTMAX, {k: ops._tuning.get(k, 0) for k in ("mse_sum_order", "bwd_sum_order")})
    U.FUSE_BACKWARD, U.FUSE_SOFTMAX = backward, softmax
    if strict:
        osq.set_strict(True)
    U.site_backward.reset()
    try:
        with TWC._only_these_learn(model, params):
            for p in params:
                p.grad = None
            TWC.batch_loss(model(**batch), batch, target, "glue").backward()
        return {n: (q.scale.grad.clone(), q.zero_point.grad.clone()) for n, q in quantizers.items()}
    finally:
        U.FUSE_BACKWARD, U.FUSE_SOFTMAX = saved[:2]
        for k, v in saved[2].items():
            ops.set_tuning(k, v)


def _distance(a, b, names):
    """Largest relative distance between two runs' gradients over the named quantizers."""
    return max(float((x - y).abs().max() / y.abs().max().clamp_min(1e-30)) for n in names for x, y in zip(a[n], b[n]))


def test_one_backward_three_ways(model_and_batch):
    from outlier_suppression_amd import util_layernorm as U
    eager = _grads(model_and_batch)
    strict = _grads(model_and_batch, strict=True)
    gelu = [n for n in eager if GELU_SITE in n]
    others = [n for n in eager if GELU_SITE not in n]
    assert len(gelu) == 2 and others

    fused = _grads(model_and_batch, backward=True)
    assert (U.site_backward.gelu, U.site_backward.softmax) == (2, 0) and U.site_backward.reason == "FUSE_SOFTMAX is off"
    for n in gelu:
        assert all(bits_equal(a.cpu().numpy(), b.cpu().numpy()) for a, b in zip(fused[n], eager[n])), n
    tiers, got = _distance(strict, eager, others), _distance(fused, eager, others)
    print(f"model     tiny BERT, GELU site fused: other quantizers' distance from eager {got:.3e}; eager default from strict {tiers:.3e}; bar {4 * tiers:.3e}")
    assert got <= 4 * tiers

    both = _grads(model_and_batch, backward=True, softmax=True)
    assert (U.site_backward.gelu, U.site_backward.softmax, U.site_backward.eager) == (2, 2, 0), U.site_backward
    assert all(torch.isfinite(g).all() for pair in both.values() for g in pair)
    print(f"model     tiny BERT, GELU + softmax sites fused: every quantizer's distance from eager {_distance(both, eager, list(eager)):.3e} (recorded only: the forward differs by a few ulp)")

    _grads(model_and_batch, backward=True, softmax=True, strict=True)
    assert (U.site_backward.gelu, U.site_backward.softmax, U.site_backward.eager) == (0, 0, 4)
    assert U.site_backward.reason == "the strict summation tier is defined on the eager tensors"

"""Losses of the task-model wrappers (part of their forward contract: SURVEY 8f N2).

The reference's task models return the loss in front of their outputs when ``labels`` (or ``start_positions`` /
``end_positions``) are given (model/quant_bert.py:656-680, 744-765, quant_bart.py:1104-1111, 1248-1274, 1376-1392); an
evaluation loop (HF ``Trainer.evaluate``) reads ``outputs[0]`` as the loss then.  The wrappers of this package return plain
tuples (no ``ModelOutput``, ``return_dict`` is ignored); with labels the tuple starts with the loss, computed exactly as the
reference does."""
import torch
from torch.nn import functional as F


def classification_loss(config, num_labels, logits, labels):
    """quant_bert.py:656-680 (the same block in quant_roberta.py and quant_bart.py:1248-1270); sets config.problem_type
    on first use as the reference does."""
    if labels is None:
        return None
    if config.problem_type is None:
        if num_labels == 1:
            config.problem_type = "regression"
        elif num_labels > 1 and labels.dtype in (torch.long, torch.int):
            config.problem_type = "single_label_classification"
        else:
            config.problem_type = "multi_label_classification"
    if config.problem_type == "regression":
        return F.mse_loss(logits.squeeze(), labels.squeeze()) if num_labels == 1 else F.mse_loss(logits, labels)
    if config.problem_type == "single_label_classification":
        return F.cross_entropy(logits.view(-1, num_labels), labels.view(-1))
    return F.binary_cross_entropy_with_logits(logits, labels)


def span_loss(start_logits, end_logits, start_positions, end_positions):
    """quant_bert.py:748-765 (quant_roberta.py, quant_bart.py:1376-1392)."""
    if start_positions is None or end_positions is None:
        return None
    if start_positions.dim() > 1:
        start_positions = start_positions.squeeze(-1)
    if end_positions.dim() > 1:
        end_positions = end_positions.squeeze(-1)
    ignored = start_logits.size(1)      # positions outside the inputs are ignored
    start_positions, end_positions = start_positions.clamp(0, ignored), end_positions.clamp(0, ignored)
    return (F.cross_entropy(start_logits, start_positions, ignore_index=ignored) +
            F.cross_entropy(end_logits, end_positions, ignore_index=ignored)) / 2


def token_logprob_torch(logits, labels, ignore_index=-100):
    """The torch lines of ops.token_logprob: the log-probability ``logits`` [..., vocab] give ``labels`` [...], 0 where the
    label is ``ignore_index``.  The CPU path of score() and what a call the kernels do not take runs."""
    ignored = labels == ignore_index
    picked = torch.log_softmax(logits, dim=-1).gather(-1, labels.masked_fill(ignored, 0).unsqueeze(-1)).squeeze(-1)
    return picked.masked_fill(ignored, 0.0)


class LmLossInfo:
    """What the last ``forward(labels=...)`` did with set_fast_lm_loss: ``fused`` losses through ops.lm_loss, ``eager``
    ones through F.cross_entropy and, for those, the ``reason``.  ``bad_labels`` reads the kernel's count of labels
    outside the vocabulary (F.cross_entropy asserts on the device there; the kernels give a NaN loss and count): the one
    synchronisation, which forward does not make.  None where no kernel ran."""

    def __init__(self, reason=None):
        self.fused, self.eager, self.reason, self._counts = 0, 0, reason, None

    @property
    def bad_labels(self):
        return None if self._counts is None else int(self._counts[1])

    def __repr__(self):
        return f"LmLossInfo(fused={self.fused}, eager={self.eager}, reason={self.reason!r})"


def fused_lm_loss_why_not(logits, labels):
    """None where ops.lm_loss takes the call, else the reason F.cross_entropy runs."""
    from .. import ops
    if not (logits.is_cuda and labels.is_cuda):
        return "the tensors are on the CPU"
    if logits.dtype != torch.float32:
        return f"the logits are {logits.dtype}, not float32"
    if labels.dtype != torch.int64:
        return f"the labels are {labels.dtype}, not int64"
    if not ops.token_logprob_fits(logits.numel() // logits.shape[-1], logits.shape[-1]):
        return "more logits than one launch indexes"
    return None


class FusedLmLoss(torch.autograd.Function):
    """``F.cross_entropy(logits, labels, ignore_index=...)`` over fp32 [rows, vocab] logits on the device through
    ops.lm_loss and ops.token_logprob_backward: (loss, counts).  The backward keeps ``lse`` [rows] and the counts, not a
    tensor of the logits' size; the gradient is one streaming launch."""

    @staticmethod
    def forward(ctx, logits, labels, ignore_index):
        from .. import ops
        loss, _, lse, counts = ops.lm_loss(logits, labels, ignore_index)
        ctx.save_for_backward(logits, labels, lse, counts)
        ctx.ignore_index = ignore_index
        ctx.mark_non_differentiable(counts)
        return loss, counts

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_loss, _grad_counts):
        from .. import ops
        logits, labels, lse, counts = ctx.saved_tensors
        grad = grad_loss.to(torch.float32).contiguous()
        return ops.token_logprob_backward(logits, labels, lse, scalar_grad=grad, counts=counts,
                                          ignore_index=ctx.ignore_index), None, None


def lm_loss(logits, labels, vocab_size, info=None):
    """quant_bart.py:1104-1107.  With set_fast_lm_loss (util_layernorm.FAST_LM_LOSS) the same number through the scoring
    kernels (FusedLmLoss), where they take the call; ``info`` (an LmLossInfo) records what happened."""
    if labels is None:
        return None
    from .. import util_layernorm
    if util_layernorm.FAST_LM_LOSS:
        info = LmLossInfo() if info is None else info
        info.reason = fused_lm_loss_why_not(logits, labels)
        if info.reason is None:
            loss, info._counts = FusedLmLoss.apply(logits.view(-1, vocab_size), labels.reshape(-1), -100)
            info.fused += 1
            return loss
        info.eager += 1
    elif info is not None:
        info.reason = "not asked for"
        info.eager += 1
    return F.cross_entropy(logits.view(-1, vocab_size), labels.view(-1))


def with_loss(loss, outputs):
    return outputs if loss is None else (loss,) + tuple(outputs)

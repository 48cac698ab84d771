"""Seeded inputs of the attention-probabilities-site fixture (tests/golden/attention_site.npz): shared by the generator that
runs the reference (tests/golden/make_golden_attention_site.py) and by the tests that re-draw the same tensors.  The
scores are not stored (28 MB at [2,12,384,384]); torch's CPU generator is deterministic for a given build, the draws go
through +, * and / only (tests/_site_size.py::site_input: no exp / sqrt, whose vectorised forms differ between hosts), and
the fixture keeps each tensor's bit-pattern checksum."""
import math

import torch

from _site_size import checksum, site_lengths  # noqa: F401  (re-exported)

PROBS_SLICE = (slice(0, 1), slice(0, 1), slice(0, 64))   # [sample 0, head 0, queries 0-63]: the float probabilities stored
XQ_SLICE = (slice(0, 1), slice(0, 4))       # [sample 0, heads 0-3]: the integer tensor stored entry by entry; the whole
                                            # tensor as a histogram of its values (a single-step difference moves one count)

# name, mask kind, shape [B, h, T, S], head size d, quantizer, observer, percentile, bit, seed
#   bert: BertModel's extended mask [B,1,1,S] = (1 - mask) * -10000 (quant_bert.py:169-176: scores / sqrt(d) + mask)
#   bart: the decoder's causal mask (-inf above the diagonal) + the finfo.min padding mask, [B,1,T,S], added to the
#         [B*h, T, S] scores viewed as [B,h,T,S] (quant_bart.py:232-256); the quantizer sees the 3-D tensor
CASES = (
    ("bert_minmax", "bert", (8, 12, 128, 128), 64, "FixedFakeQuantize", "MinMaxObserver", None, 8, 6101),
    ("bert_lsqplus", "bert", (2, 12, 384, 384), 64, "LSQPlusFakeQuantize", "AvgPruneMinMaxObserver", 0.95, 6, 6102),
    ("bart_causal", "bart", (4, 12, 128, 128), 64, "FixedFakeQuantize", "MinMaxObserver", None, 8, 6103),
    # a head size whose sqrt is no power of two (scores / sqrt(48): the divide form) and a row width that is not a multiple
    # of 4 (the kernel's generic path)
    ("bert_odd", "bert", (4, 12, 77, 77), 48, "LSQPlusFakeQuantize", "AvgMinMaxObserver", None, 8, 6104),
)
OBSERVER_NAME = "encoder.layer.0.attention.self.attention_probs_post_act_fake_quantize.observer"


def attention_site_inputs(seed, kind, shape, d):
    """(scores, mask, lengths): raw q.k^T scores [B,h,T,S] (before the 1/sqrt(d) of BERT; BART's q is already scaled, so its
    scores are used as they are), the additive mask and the valid lengths handed to the probs quantizer."""
    gen = torch.Generator().manual_seed(seed)
    b, h, t, s = shape
    scores = torch.randn(*shape, generator=gen) * (2.0 * math.sqrt(d) if kind == "bert" else 2.0)
    # a few keys every query attends to strongly (the outlier tokens the paper talks about): peaked rows
    hot = torch.randint(0, s, (3,), generator=gen)
    scores[..., hot] += 4.0 * (math.sqrt(d) if kind == "bert" else 1.0)
    lengths = site_lengths(gen, shape, 2)
    valid = (torch.arange(s)[None, :] < lengths[:, None]).float()              # [B, S] attention mask of the tokenizer
    if kind == "bert":
        mask = (1.0 - valid[:, None, None, :]) * -10000.0                      # [B,1,1,S]
    else:
        inverted = 1.0 - valid[:, None, None, :].expand(b, 1, t, s)
        pad = inverted.masked_fill(inverted.bool(), torch.finfo(torch.float32).min)
        causal = torch.full((t, s), float("-inf"))
        cond = torch.arange(t)
        causal.masked_fill_(cond < (cond + 1).view(t, 1), 0)
        mask = pad + causal[None, None].expand(b, 1, t, s)                     # [B,1,T,S]
    return scores, mask, lengths


def scaling(kind, d):
    """What the eager site does before the mask: BERT divides by sqrt(d), BART adds the scores as they are."""
    return math.sqrt(d) if kind == "bert" else None

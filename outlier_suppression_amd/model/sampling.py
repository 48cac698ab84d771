"""Seeded sampling for the quantized BART wrapper: the host side of csrc/sample_advance.hip.

The random stream is the package's own, not torch.multinomial's: the uniform of batch row ``b`` at history length ``cur`` is
word 0 of Philox4x32-10 with the key (seed & 0xffffffff, seed >> 32) and the counter (b, cur, 0, 0), its top 24 bits times
2^-24; with several sequences per input (``group``), sequence ``j`` of input ``b`` draws at the counter (b, cur, j, 0).  The
generator has no state to advance: a call is reproducible from its seed whatever the launch shape, and a captured graph of a
step serves every step.  ``philox4x32`` and ``uniforms`` restate it in integer arithmetic on the host; ``token_logprob`` is
the log of the probability with which the rule drew a token, for sample(return_logprobs=True) where the kernel does not run;
``select_torch`` / ``sample_step_torch`` are the rule of include/osq_hip.h (osq_sample_advance) as torch lines in fp32, fed
those uniforms: the eager form, which serves on the CPU, under autograd and wherever the kernel does not take a call
(``top_k > 64``; ``top_k == 0`` with ``top_p < 1`` unless ``sample_nucleus`` hands it to csrc/sample_nucleus.hip, whose rule
these lines state too -- and then a vocabulary above 51200).

Where the rule departs from transformers' warpers: exactly ``top_k`` survivors under ties at the k-th value (transformers keeps
every tie), equal values by smaller token; a NaN logit counts as banned.
"""
import torch

_M0, _M1, _W0, _W1, _MASK = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF


def philox4x32(counter, key, rounds=10):
    """Philox4x32 (Salmon et al., SC'11): the four output words for a counter of four and a key of two 32-bit words."""
    c0, c1, c2, c3 = (int(c) & _MASK for c in counter)
    k0, k1 = (int(k) & _MASK for k in key)
    for _ in range(rounds):
        p0, p1 = _M0 * c0, _M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & _MASK, (p0 >> 32) ^ c3 ^ k1, p0 & _MASK
        k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
    return c0, c1, c2, c3


def uniforms(seed, bsz, cur, group=1):
    """The draws of a step at history length ``cur`` for ``bsz`` inputs of ``group`` sequences each: fp32 [bsz * group] on the
    CPU, row b * group + j from the counter (b, cur, j, 0), each (word 0 >> 8) * 2^-24, in [0, 1)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    key = (seed & _MASK, seed >> 32)
    words = [philox4x32((b, cur, j, 0), key)[0] >> 8 for b in range(bsz) for j in range(group)]
    return torch.tensor(words, dtype=torch.float64).mul_(2.0 ** -24).to(torch.float32)      # 24 bits: exact in both formats


def select_torch(scores, u, temperature=1.0, top_k=0, top_p=1.0):
    """Rules 3-8 on ``scores`` [bsz, vocab] fp32 whose banned tokens hold -inf: the token [bsz] int64 each row's ``u`` [bsz]
    selects.  ``top_k == 0`` with ``top_p == 1`` draws from every token in token order; anything else from the survivors
    in rank order (larger first, equal values by smaller token), ``top_k == 0`` meaning all of them."""
    vocab = scores.shape[-1]
    neg = float("-inf")
    z = scores / torch.full((1,), float(temperature), dtype=scores.dtype, device=scores.device)      # a true division on every device
    z = torch.where(torch.isnan(z), neg, z)
    ranked = top_k > 0 or top_p < 1.0
    tokens = None
    if ranked:
        z, tokens = torch.sort(z, dim=-1, descending=True, stable=True)
        keep = vocab if top_k == 0 else min(int(top_k), vocab)
        z, tokens = z[:, :keep], tokens[:, :keep]
    m = z.max(dim=-1, keepdim=True)[0]
    alive = z > neg
    w = torch.where(z == m, 1.0, torch.exp(z - m))
    w = torch.where(alive, w, 0.0)
    if top_p < 1.0:                               # rank i stays iff the weights above it sum below top_p * total
        upto = torch.cumsum(w, dim=-1)
        stay = (upto - w) < top_p * upto[:, -1:]
        stay[:, 0] = True
        alive = alive & stay
        w = torch.where(alive, w, 0.0)
    upto = torch.cumsum(w, dim=-1)
    target = u.to(device=scores.device, dtype=scores.dtype)[:, None] * upto[:, -1:]
    first = (upto <= target).sum(dim=-1)          # the first position whose running sum passes the target
    live = torch.where(alive, torch.arange(z.shape[-1], device=z.device)[None, :], -1).max(dim=-1)[0]    # the last kept one
    pick = torch.minimum(first, live)
    none = live < 0
    pick = pick.clamp_(min=0)
    token = pick if tokens is None else tokens.gather(1, pick[:, None])[:, 0]
    return torch.where(none, 0, token)


def token_logprob(scores, token, temperature=1.0, top_k=0, top_p=1.0):
    """The log of the probability with which select_torch drew ``token`` [bsz] from ``scores`` [bsz, vocab]: over its kept
    survivors, (z_tok - m) - log(W), the first term 0 where z_tok == m (m = +inf included), W the kept weights' fp32 total;
    -inf for a row without a survivor (and for a token that is not kept).  fp32 [bsz]."""
    vocab = scores.shape[-1]
    neg = float("-inf")
    z = scores / torch.full((1,), float(temperature), dtype=scores.dtype, device=scores.device)
    z = torch.where(torch.isnan(z), neg, z)
    tokens = torch.arange(vocab, device=scores.device)[None, :].expand_as(z)
    if top_k > 0 or top_p < 1.0:
        z, tokens = torch.sort(z, dim=-1, descending=True, stable=True)
        keep = vocab if top_k == 0 else min(int(top_k), vocab)
        z, tokens = z[:, :keep], tokens[:, :keep]
    m = z.max(dim=-1, keepdim=True)[0]
    alive = z > neg
    w = torch.where(alive, torch.where(z == m, 1.0, torch.exp(z - m)), 0.0)
    if top_p < 1.0:
        upto = torch.cumsum(w, dim=-1)
        stay = (upto - w) < top_p * upto[:, -1:]
        stay[:, 0] = True
        alive = alive & stay
        w = torch.where(alive, w, 0.0)
    total = torch.cumsum(w, dim=-1)[:, -1]
    at = (tokens == token.to(scores.device)[:, None]) & alive
    z_tok = torch.where(at, z, neg).max(dim=-1)[0]
    m = m[:, 0]
    lp = torch.where(z_tok == m, torch.zeros_like(m), z_tok - m) - torch.log(total)
    return torch.where(at.any(dim=-1), lp, neg).to(torch.float32)


def sample_step_torch(logits, seq, cur, max_length, u, temperature=1.0, top_k=0, top_p=1.0, ngram=0, ban_ids=None, forced=None,
                      eos_ids=None, pad=0, unfinished=None):
    """One sampling step at history length ``cur`` as torch lines, with the arguments of ops.sample_advance: (token [bsz],
    unfinished [bsz] or None, go_on).  ``seq`` [bsz, >= cur] holds the history, ``u`` [bsz] the draws."""
    bsz, vocab = logits.shape
    if forced is not None and forced >= 0:
        token = torch.full((bsz,), int(forced), dtype=torch.long, device=logits.device)
    else:
        scores = logits.to(torch.float32).clone()
        if ban_ids is not None and len(ban_ids):
            ids = torch.as_tensor(ban_ids, device=logits.device).long()
            scores[:, ids[(ids >= 0) & (ids < vocab)]] = float("-inf")
        if ngram > 0 and cur >= ngram:
            from transformers.generation.logits_process import NoRepeatNGramLogitsProcessor
            scores = NoRepeatNGramLogitsProcessor(int(ngram))(seq[:, :cur], scores)
        token = select_torch(scores, u, temperature, top_k, top_p)
    if eos_ids is not None and len(eos_ids):
        eos = torch.as_tensor(eos_ids, device=logits.device).long()
        alive = unfinished.to(torch.bool)
        token = torch.where(alive, token, int(pad))
        unfinished = (alive & ~torch.isin(token, eos)).to(unfinished.dtype)
        go_on = bool(unfinished.any())
    else:
        go_on = True
    return token, unfinished, int(cur + 1 < max_length and go_on)

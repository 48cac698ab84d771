#!/usr/bin/env python3
"""Incremental-decoding golden vectors: the REFERENCE's quantized tiny BART decoded step by step through its own
``forward(past_key_values=..., use_cache=True, return_dict=False)``.

Build-container only (imports the reference unmodified, CPU, one thread).  The model and its calibration are those of
make_golden_model.main_bart -- the same seeded tiny BART (tiny_bart), the same batches and the same pipeline (wrap ->
gamma migration -> weight calibration -> one observer pass at percentile 0.9 -> activation quantization); the batches
and weights are read back from bart_tiny_pipeline.npz so both fixtures describe one model.  Then, for the encoder
inputs of calibration batch 1 (3 samples), 12 greedy steps from decoder_start_token_id:

  step_logits   [3, 12, V]  last-position logits of each cached step (the reference's own KV cache)
  tokens        [3, 13]     the greedy sequence (start token first)
  margin        [3, 12]     top-1 minus top-2 logit of each step
  full_logits   [3, 12, V]  the same steps without a cache (the whole prefix each step)
  cache_layer0_{k,v,cross_k,cross_v}   the final KV cache of decoder layer 0
  q_names / q_scale::i / q_zp::i       every quantizer's parameters after calibration

The reference's own generate() does not run under the installed transformers (its GenerationMixin asks the wrapper
for a ``generation_config`` it does not have), so no generate() output is stored; what the script saw is printed.
Data only.
"""
import copy
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden_model as M  # noqa: E402

STEPS = 12


def main():
    QB, GM, TWC, ST, QuantizeBase = M.import_reference()
    gu = types.ModuleType("transformers.generation_utils")
    from transformers.generation import GenerationMixin
    gu.GenerationMixin = GenerationMixin
    sys.modules["transformers.generation_utils"] = gu
    from quant_transformer.model import quant_bart as RB
    torch.set_num_threads(1)
    cfg, fp = M.tiny_bart()
    g = np.load(os.path.join(M.OUT, "bart_tiny_pipeline.npz"))
    fp.load_state_dict({k[4:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd::")})
    keys = ("input_ids", "attention_mask", "decoder_input_ids", "decoder_attention_mask")
    batches = [{k: torch.from_numpy(g[k][b]) for k in keys} for b in range(g["input_ids"].shape[0])]
    a_q = M.Cfg(quantizer="LSQPlusFakeQuantize", observer="AvgPruneMinMaxObserver", bit=6, symmetric=False, ch_axis=-1)
    w_q = M.Cfg(quantizer="FixedFakeQuantize", observer="MinMaxObserver", bit=6, symmetric=True, ch_axis=0)
    model = RB.QuantizedBartForConditionalGeneration(copy.deepcopy(fp), w_q, a_q, qoutput=False, backend="academic",
                                                     is_remove_padding=True).eval()
    kw = dict(use_cache=False, return_dict=False)
    model = GM.delay_ln(model, M.Cfg(a_qconfig=a_q, w_qconfig=w_q), M.Cfg(model_type="bart", task_type="summ"))
    ST.enable_calibration_woquantization(model, quantizer_type="weight_fake_quant")
    with torch.no_grad():
        model(**batches[0], **kw)
    ST.disable_all(model)
    ST.set_observer_name(model)
    TWC.set_ratio(model, 0.9)
    with torch.no_grad():
        for b in batches:
            model(**b, **kw)
    TWC.enable_quantization(model)
    names, scales, zps = M.quantizer_table(model, QuantizeBase)
    with torch.no_grad():
        check = model(**batches[0], **kw)[0].numpy()
    assert np.abs(check - g["logits_act_quant"][0]).max() == 0, "not the model of bart_tiny_pipeline.npz"

    ids, mask = batches[1]["input_ids"], batches[1]["attention_mask"]
    B = ids.shape[0]
    tokens = torch.full((B, 1), cfg.decoder_start_token_id, dtype=torch.long)
    step_logits, full_logits, margin = [], [], []
    past = None
    with torch.no_grad():
        for _ in range(STEPS):
            inp = tokens if past is None else tokens[:, -1:]
            out = model(input_ids=ids, attention_mask=mask, decoder_input_ids=inp, past_key_values=past, use_cache=True,
                        return_dict=False)
            logits, past = out[0][:, -1], out[1]
            full = model(input_ids=ids, attention_mask=mask, decoder_input_ids=tokens, use_cache=False,
                         return_dict=False)[0][:, -1]
            top = torch.topk(logits, 2, dim=-1).values
            step_logits.append(logits.numpy())
            full_logits.append(full.numpy())
            margin.append((top[:, 0] - top[:, 1]).numpy())
            tokens = torch.cat([tokens, logits.argmax(-1, keepdim=True)], dim=1)
    out = {"input_ids": ids.numpy(), "attention_mask": mask.numpy(), "tokens": tokens.numpy(),
           "step_logits": np.stack(step_logits, 1), "full_logits": np.stack(full_logits, 1), "margin": np.stack(margin, 1),
           "q_names": np.array(names)}
    for i, (s, z) in enumerate(zip(scales, zps)):
        out[f"q_scale::{i}"], out[f"q_zp::{i}"] = s, z
    for name, t in zip(("k", "v", "cross_k", "cross_v"), past[0]):
        out[f"cache_layer0_{name}"] = t.numpy()
    try:
        model.generate(ids, attention_mask=mask, max_length=STEPS + 1, num_beams=1)
        print("the reference's generate() ran (its outputs are not part of the fixture)")
    except Exception as e:             # recorded: the reference's GenerationMixin does not fit the installed transformers
        print("the reference's generate() does not run here:", type(e).__name__, str(e)[:120])
    path = os.path.join(M.OUT, "bart_decode.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes; cached vs uncached max |diff|",
          np.abs(out["step_logits"] - out["full_logits"]).max(), "; min margin", out["margin"].min())


if __name__ == "__main__":
    main()

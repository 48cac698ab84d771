"""The attention-site fixture (tests/golden/attention_site.npz) on the CPU: the re-drawn inputs are the tensors the
reference ran on (bit-pattern checksums), and the stored integer tensors are consistent with the stored parameters."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _attention_site import CASES, XQ_SLICE, attention_site_inputs, checksum  # noqa: E402


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_attention_site_inputs_match_fixture(golden, case):
    name, kind, shape, d = case[:4]
    g = golden("attention_site")
    scores, mask, L = attention_site_inputs(case[-1], kind, shape, d)
    assert [checksum(scores), checksum(mask.contiguous()), int(L.sum())] == list(g[name + "_sums"]), "the seeded inputs drifted"
    assert g[name + "_xq"].shape == np.zeros(shape)[XQ_SLICE].shape
    assert int(g[name + "_xq_hist"].sum()) == int(np.prod(shape))          # the histogram covers every entry
    assert np.all(np.bincount(g[name + "_xq"].reshape(-1), minlength=g[name + "_xq_hist"].size) <= g[name + "_xq_hist"])
    # the stored float probabilities are rows of a softmax (sample 0, head 0), and the integer tensor of the same rows is
    # their rounding
    p = g[name + "_probs"].astype(np.float64)
    assert np.all(np.abs(p.sum(-1) - 1.0) < 1e-5)
    scale, zp = np.float32(g[name + "_scale"][0]), np.float32(g[name + "_zp"][0])
    xq = g[name + "_xq"][:, :1, :p.shape[2]].astype(np.float32)
    assert np.abs(np.clip(np.rint(p / scale) + zp, 0, None) - xq).max() <= 1

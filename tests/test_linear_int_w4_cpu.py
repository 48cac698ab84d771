"""Packed 4-bit weights of the integer linear layers (csrc/linear_int.hip) without a GPU: the two entry points in the header, in
its "Added within 10" list and in ``_hip.SIGNATURES``, and the refusal of a weight quantizer with more than 16 codes."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name, like", (("osq_weight_codes_sums_w4", "osq_weight_codes_sums"), ("osq_linear_int_w4", "osq_linear_int")))
def test_entry_points_are_listed_and_bound(name, like):
    from outlier_suppression_amd import _hip
    header = open(os.path.join(ROOT, "include", "osq_hip.h")).read()
    above = header[:header.index("#define OSQ_ABI_VERSION")]
    added = re.search(r"Added within 10 \(no existing signature changed\):(.*?)\*/", above, re.S).group(1)
    assert name in set(re.findall(r"osq_\w+", added))
    decl, twin = (re.search(rf"^int {n}\((.*?)\);", header, re.M | re.S).group(1) for n in (name, like))
    assert " ".join(decl.split()) == " ".join(twin.split()) and _hip.SIGNATURES[name] == _hip.SIGNATURES[like]


def test_a_packed_weight_of_17_codes_is_refused():
    from outlier_suppression_amd import ops
    w, scale, zp = torch.zeros(4, 32), torch.ones(4), torch.zeros(4, dtype=torch.int32)
    with pytest.raises(ValueError, match="a packed weight has more than 16 codes"):
        ops.weight_codes(w, scale, zp, 0, 0, 16, bits=4)
    assert "GPU" in ops.linear_int_refusal(32, (scale[:1], zp[:1], 0, 15), packed=True)

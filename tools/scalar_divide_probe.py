"""Which words torch's GPU true-divide of an fp32 tensor by a Python scalar gives, against four candidate forms: the correctly
rounded division, a multiplication by 1.0f / float(div), a multiplication by float(1.0 / div) with the reciprocal taken in
double, and a division in double.  ops.beam_advance's ``reciprocal`` form is the one without mismatches (DESIGN.md, section 4,
"Advancing the beams"; profiles/beam_advance_division.txt).

    python tools/scalar_divide_probe.py > profiles/beam_advance_division.txt
"""
import numpy as np
import torch

F = np.float32
rng = np.random.default_rng(0)
v = np.concatenate([-(rng.permutation(4096)[:512].astype(F) + F(1)) / F(64),
                    -(rng.permutation(1024)[:512].astype(F) + F(1)) * F(200) - rng.random(512).astype(F)])
tot = {k: 0 for k in "ABCD"}
n = 0
for cur in (2, 3, 5, 7, 8, 13, 31, 61):
    for lp in (0.8, 1, 1.0, 2, 2.0, 0.5):
        div = cur ** lp
        got = (torch.from_numpy(v).cuda() / div).cpu().numpy().view(np.uint32)
        cpu = (torch.from_numpy(v) / div).numpy().view(np.uint32)
        cands = {"A": v / F(div), "B": v * (F(1) / F(div)), "C": v * F(1.0 / float(div)),
                 "D": (v.astype(np.float64) / float(div)).astype(F)}
        row = {k: int((c.view(np.uint32) != got).sum()) for k, c in cands.items()}
        for k in row:
            tot[k] += row[k]
        n += len(v)
        print(f"cur {cur:2d} lp {lp!r:4}: mismatches vs GPU  A(v/div) {row['A']:4d}  B(v*(1f/div)) {row['B']:4d}  "
              f"C(v*f32(1/div in double)) {row['C']:4d}  D(double) {row['D']:4d}   CPU torch vs A: {int((cpu != cands['A'].view(np.uint32)).sum())}")
print("total mismatches of", n, tot)

"""The tie-free cases of tests/_decode_attention.py against the reference's own arithmetic on the CPU: the eager torch fp32
sequence of quant_bart.py:232-268 for one query token -- bmm, + mask, softmax, fake-quant (oracle/fake_quant_oracle.py),
bmm, fake-quant -- must give the helper's float64 integer codes EXACTLY ("0 entries differ"), in two summation orders: as
written, and with the cache positions reversed.  This is what entitles tests/test_gpu_decode_attention.py to compare the
kernel's words with the helper's: the bound behind "tie-free" is verified here, not on the kernel under test.

That holds for all seven head sizes the kernels are instantiated for, for the coded variant (the eager sequence then runs on
the numpy-dequantised K / V) and for the limit cases.  The one case without a tie-free instance (DA.RELAXED_CASE) is held to
the rule it is compared by, on the reference alone first.  The last part restates what NaN and infinity do to the formula
with the same eager sequence, so that the patterns the GPU tests expect come from the reference's arithmetic."""
import numpy as np
import pytest
import torch

import _decode_attention as DA
from conftest import same_f32
from oracle import fake_quant_oracle as FQ


def _fake_quant(x, g):
    s, z = FQ.lsq_effective(g.scale_after, g.zp_after, g.grad_factor, g.mode)
    xq = FQ.quantize_affine(x, np.float32(s), np.float32(z), g.qmin, g.qmax)
    return xq, FQ.dequantize_affine(xq, np.float32(s), np.float32(z))


def _eager(ref, reverse, inputs=None):
    """(probabilities codes [B, h, 1, S], context codes [B, h, d], output [B, 1, h*d], probabilities [B, h, 1, S]) of the eager
    sequence on the instance's tensors, or on ``inputs`` (q, k, v, mask) in their place."""
    case = ref["case"]
    b, h, d, s = case.batch, case.heads, case.head_dim, case.kv_len
    src = ref if inputs is None else inputs
    q, k, v = (torch.from_numpy(src[n]) for n in "qkv")
    mask = None if src["mask"] is None else torch.from_numpy(src["mask"])
    if reverse:
        k, v = k.flip(2).contiguous(), v.flip(2).contiguous()
        mask = None if mask is None else mask.flip(3).contiguous()
    w = torch.bmm(q.view(b * h, 1, d), k.view(b * h, s, d).transpose(1, 2))
    if mask is not None:
        w = (w.view(b, h, 1, s) + mask).view(b * h, 1, s)
    probs = torch.softmax(w, dim=-1)
    p_codes, p_fq = _fake_quant(probs.numpy(), ref["probs_q"])
    ctx = torch.bmm(torch.from_numpy(p_fq), v.view(b * h, s, d)).view(b, h, 1, d)
    ctx = ctx.permute(0, 2, 1, 3).contiguous().view(b, 1, h * d)
    c_codes, out = _fake_quant(ctx.numpy(), ref["ctx_q"])
    p_codes, p_fq = p_codes.reshape(b, h, 1, s), p_fq.reshape(b, h, 1, s)
    if reverse:
        p_codes, p_fq = p_codes[..., ::-1], p_fq[..., ::-1]
    return p_codes, c_codes.reshape(b, h, d), out, p_fq


def _check(case):
    ref = DA.reference(case)
    assert ref["margin"] > 0
    for reverse in (False, True):
        p_codes, c_codes, out, _ = _eager(ref, reverse)
        bad_p, bad_c = int((p_codes != ref["probs_codes"]).sum()), int((c_codes != ref["ctx_codes"]).sum())
        assert bad_p == 0 and bad_c == 0, (case, ref["seed"], reverse, bad_p, bad_c, ref["margin"], ref["worst_g"])
        assert same_f32(out, ref["out"]), (case, reverse)
    return ref


def _check_table(head_dim, coded):
    """Every case of the table has a tie-free instance (DA.reference raises where it has none: nothing is skipped) and the
    eager sequence has its codes."""
    with torch.no_grad():
        worst = max((_check(case)["seed"] - DA.first_seed(case), case) for case in DA.table(head_dim, coded))
    print(f"head_dim {head_dim} {'codes' if coded else 'fp32'}: {len(DA.table(head_dim, coded))} cases, "
          f"largest seed offset {worst[0]} of {DA.SEED_BUDGET} at {tuple(worst[1][:8])}")


@pytest.mark.parametrize("head_dim", DA.HEAD_DIMS)
def test_eager_sequence_gives_the_float64_codes(head_dim):
    _check_table(head_dim, False)


@pytest.mark.parametrize("head_dim", DA.HEAD_DIMS)
def test_eager_sequence_gives_the_float64_codes_of_coded_cases(head_dim):
    """The eager sequence on the numpy-dequantised K / V."""
    _check_table(head_dim, True)


def test_eager_sequence_at_the_kv_limit():
    with torch.no_grad():
        _check(DA.LIMIT_CASE)


@pytest.mark.parametrize("case", DA.LIMIT_CASES[1:], ids=lambda c: f"{c.head_dim}-{c.kv_len}")
def test_eager_sequence_at_the_kv_limit_of_the_other_head_sizes(case):
    with torch.no_grad():
        _check(case)


def test_relaxed_case_on_the_reference_and_the_eager_sequence():
    """head_dim 256 at kv_len 4096.  On the reference alone: its probabilities are tie-free, at least 0.9 of the context
    entries are further than 4 g from a tie, and no other entry's 4 g reaches half a step (so it is at most one step off).
    Then the eager sequence in both orders keeps to exactly that: the probabilities' codes, the words of the sure entries,
    one step elsewhere."""
    ref = DA.reference(DA.RELAXED_CASE)
    sure, worst = DA.sure_entries(ref)
    share = float(sure.mean())
    print(f"relaxed case {tuple(DA.RELAXED_CASE[:2])}: seed {ref['seed']}, margin {ref['margin']:.4f}, sure share {share:.4f} "
          f"({int((~sure).sum())} of {sure.size} entries unsure), largest 4 g among them {worst:.4f}")
    assert ref["probs_margin"] > 0 and ref["margin"] <= 0          # else it would not need the rule
    assert share >= 0.9 and worst < 0.5
    step = float(ref["ctx_q"].scale_eff)
    with torch.no_grad():
        for reverse in (False, True):
            p_codes, _, out, _ = _eager(ref, reverse)
            assert int((p_codes != ref["probs_codes"]).sum()) == 0
            assert same_f32(out[sure], ref["out"][sure])
            assert (np.abs(out - ref["out"]) <= step * (1 + 1e-6)).all()


def test_no_other_case_is_relaxed():
    cases = [c for d in DA.HEAD_DIMS for coded in (False, True) for c in DA.table(d, coded)] + list(DA.LIMIT_CASES) + DA.nonfinite_cases()
    assert DA.RELAXED_CASE not in cases


def test_coded_values_are_two_fp32_operations():
    """((u + quant_min) as fp32 - zp_eff) * scale_eff is util_quant.py:14 on the integer code (oracle/fake_quant_oracle.py), for
    6-bit and 8-bit records; both widths occur in every coded table, with fractional zero points."""
    for d in DA.HEAD_DIMS:
        widths = set()
        for case in DA.table(d, True):
            if case.kv_len != DA.kv_lens(d, True)[3]:
                continue
            ref = DA.reference(case)
            for name in "kv":
                rec, codes = ref[name + "_record"], ref[name + "_codes"]
                assert codes.dtype == np.uint8 and rec[1] != round(rec[1])
                top = 63 if rec[2] == 0 else 255
                assert int(codes.max()) <= top
                widths.add(top)
                x_quant = (codes.astype(np.int64) + rec[2]).astype(np.float32)
                assert same_f32(ref[name], FQ.dequantize_affine(x_quant, np.float32(rec[0]), np.float32(rec[1])))
        assert widths == {63, 255}


def test_table_covers_what_it_claims():
    """Every head size meets every quantizer variant with every mask and cap variant, bad raw parameters included, some
    batch > 1 and some heads > 1; its kv_lens lie on both sides of one trip of the workgroup and of the trips of loads in
    flight plus one wave's rows (16 trips for code bytes, where that fits below 4096: the rule of test_gpu_kv_codes.py); and a
    fully masked row gives the uniform row of the eager formula."""
    import test_gpu_kv_codes
    assert DA.HEAD_DIMS == (4, 8, 16, 32, 64, 128, 256)
    for head_dim in DA.HEAD_DIMS:
        r = DA.rows_per_wave(head_dim)
        for coded in (False, True):
            t = DA.table(head_dim, coded)
            assert {(c.bits, c.mode, c.mask) for c in t} == {(b, m, k) for b, m in DA.QUANTS for k in DA.MASKS}
            assert {(c.mask, c.cap) for c in t} == {(m, c) for m in DA.MASKS for c in DA.CAPS}
            assert any(c.bad_params for c in t) and {c.kv_len for c in t} == set(DA.kv_lens(head_dim, coded))
            assert any(c.batch > 1 for c in t) and any(c.heads > 1 for c in t) and all(c.coded == coded for c in t)
            lens = {c.kv_len for c in t}
            trip = 4 * r
            assert any(n <= trip for n in lens) and any(n > trip for n in lens) and trip in lens and trip + 1 in lens
            in_flight = DA.trips_in_flight(coded) * trip + r
            if in_flight + 1 <= 4096:
                assert any(trip < n <= in_flight for n in lens) and in_flight + 1 in lens
            else:
                assert 4096 in lens
        assert DA.kv_lens(head_dim, True) == test_gpu_kv_codes.kv_lens(head_dim)
    assert {DA.trips_in_flight(False), DA.trips_in_flight(True)} == {4, 16}
    assert {(c.head_dim, c.kv_len) for c in DA.LIMIT_CASES} == {(4, 4096), (8, 4096), (16, 4096), (32, 4096), (256, 1024)}
    assert all(c[2:] == DA.LIMIT_CASE[2:] for c in DA.LIMIT_CASES + (DA.RELAXED_CASE,))
    case = next(c for c in DA.table(64) if c.mask == "full" and c.kv_len == 17 and c.batch == 2 and c.bits == "sym8")
    ref = DA.reference(case)
    g = ref["probs_q"]
    uniform = g.quantize(np.float64(np.float32(1.0) / np.float32(case.kv_len)) / float(g.scale_eff) * np.ones(1))[1][0]
    assert (ref["probs"][-1] == uniform).all()


# ------------------------------------------------------------------------------------------------ non-finite inputs

@pytest.mark.parametrize("kind", DA.NONFINITE_KINDS)
def test_what_nan_and_infinity_do_to_the_eager_sequence(kind):
    """DA.nonfinite()'s patterns are the eager sequence's: exactly the stated words of probabilities and output are NaN,
    every other word is the clean instance's (for -inf in part of a mask row: the words with finfo.min there, and the
    probability at those positions is the quantizer's zero)."""
    with torch.no_grad():
        for case in DA.nonfinite_cases():
            ref = DA.reference(case)
            x = DA.nonfinite(ref, kind)
            _, _, out, probs = _eager(ref, False, x)
            want_probs, want_out = ref["probs"], ref["out"]
            if x["twin_mask"] is not None:
                _, _, want_out, want_probs = _eager(ref, False, dict(x, mask=x["twin_mask"]))
                at = np.isneginf(x["mask"][0, 0, 0])
                assert at.any() and not at.all() and (probs[0][..., at] == 0).all()
            assert (np.isnan(probs) == x["nan_probs"]).all(), (case, kind)
            assert (np.isnan(out) == x["nan_out"]).all(), (case, kind)
            assert same_f32(probs[~x["nan_probs"]], want_probs[~x["nan_probs"]]), (case, kind)
            assert same_f32(out[~x["nan_out"]], want_out[~x["nan_out"]]), (case, kind)


def test_finfo_min_row_is_uniform_where_neg_inf_row_is_nan():
    """The contrast the whole-row case rests on: finfo.min everywhere gives the uniform row, -inf everywhere NaN."""
    ref = DA.reference(DA.nonfinite_cases()[3])
    x = DA.nonfinite(ref, "neg_inf_row")
    with torch.no_grad():
        _, _, _, probs = _eager(ref, False, dict(x, mask=np.where(np.isneginf(x["mask"]), np.float32(DA.FMIN), x["mask"])))
    assert not np.isnan(probs).any() and (probs[1] == probs[1].flat[0]).all() and probs[1].flat[0] != 0


# The seeds of the instances that existed before the other head sizes, the coded variant and the larger seed budget came:
# DA.table(16), DA.table(64), DA.table(128) in table order, and DA.LIMIT_CASE.  They must not move.
SEEDS_BEFORE = {
    16: [2500, 3200, 3900, 4600, 3600, 4300, 5000, 5700, 2900, 3600, 4300, 5000, 4000, 4700, 5401, 6100, 14900, 15600, 16300,
         17000, 16000, 16700, 17400, 18100, 15100, 15800, 16501, 17201, 16200, 16900, 17600, 18300, 15300, 16000, 16700, 17401,
         16400, 17100, 17800, 18500, 28900, 29600, 30300, 31000, 30000, 30700, 31400, 32101, 56900, 57600, 58303, 59000, 58000,
         58700, 59403, 60100],
    64: [7300, 8000, 8700, 9400, 8400, 9100, 9800, 10500, 7700, 8400, 9100, 9800, 8800, 9500, 10201, 10900, 10100, 10800, 11500,
         12200, 11200, 11900, 12601, 13300, 10300, 11000, 11700, 12400, 11400, 12100, 12801, 13500, 10500, 11200, 11900, 12600,
         11600, 12300, 13001, 13701, 14500, 15200, 15903, 16600, 15600, 16300, 17000, 17701, 20900, 21600, 22301, 23000, 22000,
         22700, 23400, 24104],
    128: [13700, 14400, 15100, 15800, 14800, 15500, 16200, 16900, 14100, 14800, 15500, 16200, 15200, 15900, 16600, 17308, 14900,
          15600, 16300, 17000, 16001, 16703, 17400, 18100, 15100, 15800, 16500, 17200, 16203, 16900, 17600, 18301, 15300, 16001,
          16700, 17400, 16404, 17100, 17804, 18504, 17700, 18400, 19101, 19800, 18800, 19500, 20220, 20901, 20500, 21200, 21900,
          22601, 21600, 22300, 23005, 23700],
}


def test_existing_instances_keep_their_seeds():
    for head_dim, seeds in SEEDS_BEFORE.items():
        assert [DA.reference(c)["seed"] for c in DA.table(head_dim)] == seeds, head_dim
    assert DA.reference(DA.LIMIT_CASE)["seed"] == 822202

"""CPU: the NumPy oracle against the REFERENCE ITSELF on seeded random inputs that no other fixture holds.

The committed goldens (tests/golden/*.npz) pin the oracle on fixed vectors; here the cases are drawn at random (shapes, bit
widths, masks, percentiles, one-sided ranges: tests/_reference_live_cases.py) and the reference's own functions and
observer classes were run on exactly these draws by tests/golden/make_golden_reference_live.py, which stored what they
returned in tests/golden/reference_live.npz (and the `quant:` sections of the reference's exp/*/config.yaml in
tests/golden/reference_quant_sections.json).  Bit-exact on everything.
"""
import json
import os

import numpy as np
import pytest
import torch

import _reference_live_cases as C

F32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def ref():
    """{key: array} of what the reference returned on the cases of tests/_reference_live_cases.py."""
    with np.load(os.path.join(GOLDEN, "reference_live.npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=F32)).view(np.uint32)


def test_fake_quant_random_cases(ref):
    from oracle import fake_quant_oracle as FQ
    for c in C.fake_quant_cases():
        trial, x, qmin, qmax = c["trial"], c["x"], c["qmin"], c["qmax"]
        want = ref[f"fq/{trial}/y"]
        _, got = FQ.fake_quantize_per_tensor_affine(x.numpy(), F32(c["scale"]), F32(c["zp"]), qmin, qmax)
        assert np.array_equal(_bits(got), _bits(want)), (trial, c["bit"], c["sym"], c["shape"])
        if x.dim() >= 2:
            want = ref[f"fq/{trial}/y_channel"]
            _, got = FQ.fake_quantize_per_channel_affine(x.numpy(), c["s"].numpy(), c["z"].numpy(), 0, qmin, qmax)
            assert np.array_equal(_bits(got), _bits(want)), (trial, "per-channel")


def test_observers_random_sequences(ref):
    from oracle import observer_oracle as OB
    fns = {"MinMaxObserver": OB.observe_minmax, "AvgMinMaxObserver": OB.observe_avg_minmax,
           "AvgPruneMinMaxObserver": OB.observe_avg_prune_minmax}
    for c in C.observer_cases():
        trial, cls_name = c["trial"], c["cls_name"]
        fn = fns[cls_name]
        st = OB.ObserverState(bit=c["bit"], symmetric=c["sym"], name=c["name"])
        if cls_name == "AvgPruneMinMaxObserver":
            st.percentile = c["pct"]
        for it, (x, L, sp) in enumerate(c["batches"]):
            if c["masked"]:
                fn(st, x.numpy(), L.numpy(), sp)
            elif cls_name == "AvgPruneMinMaxObserver":
                fn(st, x.numpy(), None, sp)          # no mask, seq_pos given: reshape_batch_embedding path
            else:
                fn(st, x.numpy())
            key = f"obs/{trial}/{it}/"
            assert np.array_equal(_bits(st.min_val), _bits(ref[key + "min_val"])), (trial, cls_name, it)
            assert np.array_equal(_bits(st.max_val), _bits(ref[key + "max_val"])), (trial, cls_name, it)
            s_or, z_or = st.qparams()
            assert np.array_equal(_bits(s_or), _bits(ref[key + "scale"])), (trial, "scale")
            assert np.array_equal(np.asarray(z_or, dtype=np.float64).reshape(-1),
                                  ref[key + "zero_point"].astype(np.float64).reshape(-1)), (trial, "zero_point")


def test_lsqplus_forward_backward_random_cases(ref):
    """util_quant.py:48-55 with autograd against the oracle's closed-form forward / backward."""
    from oracle import fake_quant_oracle as FQ
    for c in C.lsqplus_cases():
        trial, x, qmin, qmax, g = c["trial"], c["x"].numpy(), c["qmin"], c["qmax"], c["g"]
        scale, zp = F32(c["scale"].item()), F32(c["zp"].item())
        key = f"lsqplus/{trial}/"
        _, y_o = FQ.fake_quantize_learnableplus_per_tensor(x, scale, zp, qmin, qmax, g)
        assert np.array_equal(_bits(y_o), _bits(ref[key + "y"])), (trial, "y")
        dx, ds, dz = FQ.lsqplus_backward_per_tensor(x, c["gy"].numpy(), scale, zp, qmin, qmax, g)
        assert np.array_equal(_bits(dx), _bits(ref[key + "dx"])), (trial, "dx")
        np.testing.assert_allclose(ds, ref[key + "dscale"].item(), rtol=3e-5, atol=1e-7)
        np.testing.assert_allclose(dz, ref[key + "dzero_point"].item(), rtol=3e-5, atol=1e-7)


def test_msefast_equals_reference_when_the_loss_is_summed_like_torch(ref):
    """MSEFast, per-channel and per-tensor (1-D and nested 2-D searches): with torch's own fp32 mean plugged into the
    oracle's loss -- the one step whose order is the machine's, not the algorithm's -- the oracle reproduces the
    reference's ranges bit for bit and spends the same number of loss evaluations.  Everything else (float64
    qparams, fp32 fake-quant, np.float32 function values inside scipy's bounded minimiser) is restated exactly."""
    from oracle import observer_oracle as OB
    weights, acts, one_sided = C.msefast_cases()
    old = OB.MEAN_LIKE_TORCH
    OB.MEAN_LIKE_TORCH = lambda sq: torch.from_numpy(np.ascontiguousarray(sq)).mean().numpy()
    torch_threads = torch.get_num_threads()
    torch.set_num_threads(1)                  # the reference's run: one thread
    try:
        for cols, bit, w in weights:
            st = OB.ObserverState(bit=bit, symmetric=True, ch_axis=0)
            OB.observe_msefast(st, w.numpy())
            key = f"msefast/weights/{cols}/"
            assert np.array_equal(st.min_val, ref[key + "min_val"]) and np.array_equal(st.max_val, ref[key + "max_val"]), cols
        for j, (sym, shape, x) in enumerate(acts):
            st = OB.ObserverState(bit=6, symmetric=sym)
            for it in range(2):
                OB.observe_msefast(st, x.numpy() * (it + 1), average=True)
                key = f"msefast/acts/{j}/{it}/"
                assert float(st.min_val) == float(ref[key + "min_val"]) and float(st.max_val) == float(ref[key + "max_val"]), (sym, shape, it)
        # one-sided data over four batches: the dtype of min_val decides whether the NEXT batch is searched on a float64
        # copy (observer.py:524 / 549) -- float32 for ever on non-negative data (the zeros_like of :491), float64 from the
        # second batch on otherwise; both observers, values and dtypes
        for avg, side, xs in one_sided:
            name = "AvgMSEFastObserver" if avg else "MSEFastObserver"
            st = OB.ObserverState(bit=6, symmetric=False)
            for it, x in enumerate(xs):
                OB.observe_msefast(st, x.numpy(), average=avg)
                key = f"msefast/one_sided/{int(avg)}/{side}/{it}/"
                assert float(st.min_val) == float(ref[key + "min_val"]) and float(st.max_val) == float(ref[key + "max_val"]), (name, side, it)
                assert np.asarray(st.min_val).dtype == ref[key + "min_val"].dtype, (name, side, it)
    finally:
        OB.MEAN_LIKE_TORCH = old
        torch.set_num_threads(torch_threads)


def test_shipped_quant_sections_equal_the_reference_yaml():
    """ptq.SHIPPED_QUANT_SECTIONS against the `quant:` section of every config.yaml under the reference's exp/ (15 files,
    four distinct sections, stored in tests/golden/reference_quant_sections.json): same keys and values."""
    from outlier_suppression_amd import ptq
    with open(os.path.join(GOLDEN, "reference_quant_sections.json")) as f:
        sections = json.load(f)
    assert len(sections) >= 15

    def plain(ns):
        return {k: (plain(v) if hasattr(v, "__dict__") else v) for k, v in vars(ns).items()}
    seen = set()
    for rel, quant in sorted(sections.items()):
        kind = rel.split("/")[1]
        assert kind in ptq.SHIPPED_QUANT_SECTIONS, rel
        assert plain(ptq.SHIPPED_QUANT_SECTIONS[kind]) == quant, rel
        assert plain(ptq.namespace(quant)) == quant
        seen.add(kind)
    assert seen == set(ptq.SHIPPED_QUANT_SECTIONS)


def test_qparams_of_mixed_dtype_statistics(ref):
    """calculate_qparams on the statistics per-tensor MSEFast leaves behind: a float32 min_val beside a float64 max_val (and
    the other three combinations) -- torch promotes to float64 as soon as either is; values and dtype equal the reference's."""
    from oracle import observer_oracle as OB
    cases = list(C.mixed_dtype_cases())
    assert len(cases) == len(ref["mixed/scale"])
    for i, (sym, k, mn, mx) in enumerate(cases):
        qmin, qmax = (-128, 127) if sym else (0, 255)
        so, zo = OB.calculate_qparams(np.asarray(mn), np.asarray(mx), qmin, qmax, sym)
        assert float(so) == float(ref["mixed/scale"][i]) and float(zo) == float(ref["mixed/zero_point"][i]), (sym, k)
        assert (np.asarray(so).dtype == np.float64) == bool(ref["mixed/scale_is_f64"][i]), (sym, k)

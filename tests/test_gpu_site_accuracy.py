"""The three one-launch producer sites against float64 (tests/_site_reference.py, pinned to the reference project's runs
by tests/test_oracle_site_reference.py):

    residual -> LayerNorm -> shift -> fake-quant    csrc/layernorm.hip   residual_layernorm_fq_kernel<R>, R in 1,2,3,4,8,16
    mask -> softmax -> fake-quant                   csrc/attention.hip   register kernel <R,PRE,MASK,WT> + generic kernel
    GELU -> fake-quant                              csrc/fake_quant.hip  fq_tensor_vec_kernel<..., GELU=true>

Two kinds of check.

EXACT (word for word, no tolerance) -- what catches indexing, grid-stride and stale-register slips: a row's result does not
depend on where the row sits or what its neighbours hold (more rows than the grid cap, so every wave takes several trips and
every distinct row -- the edge rows included -- is at some point a prefetched row); fused == fake_quant(plain output); zero
rows; non-finite rows stay contained; one-hot / all-equal / masked softmax entries.

ACCURACY against float64.  The bar is never a fixed number and never comes from the kernel: it is 3x the error of torch's
CPU fp32 kernel (one thread) on the same values in the same metric against the same float64 reference, with a floor of
4u (u = 2**-24) on torch's figure.  Both are fp32 summations in different orders: a CPU emulation of the LayerNorm kernel's
two-pass order sits at 1.0-1.45x torch's CPU error from kappa = 1 to kappa = 1e5, so 3x leaves room for the wave tree and
1/sqrtf without admitting an error that grows with the row's condition number kappa = 1 + |mean|/sigma (which is what a
variance taken around a wrong mean, or as E[r^2] - mean^2, produces).  torch-ROCm's eager result goes through the same
metric and is recorded next to it; it sets no bar.

Measured on MI355X (profiles/site_accuracy.txt holds every figure; the worst ones are quoted in the docstrings of the
accuracy tests; profiles/site_accuracy_kernel_stats.md lists the template instances and grids the file launches).  The
whole file takes about 10 s.

With OSQ_SITE_ACCURACY_OUT=<path> the figures of a run are written to that file (how profiles/site_accuracy.txt is made)."""
import os
import sys
import time

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _site_reference as R  # noqa: E402
from conftest import bits_equal  # noqa: E402

from oracle import fake_quant_oracle as FQ  # noqa: E402

pytestmark = pytest.mark.gpu

RESULTS = []            # (site, width, data class, torch-CPU error, torch-ROCm eager error, kernel error, kernel / bar)
NOTES = []


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from outlier_suppression_amd import _hip
    _hip.load()
    torch.set_num_threads(1)
    t0 = time.time()
    yield torch.device("cuda:0")
    out = os.environ.get("OSQ_SITE_ACCURACY_OUT")
    if out:
        with open(out, "w") as f:
            f.write("# tests/test_gpu_site_accuracy.py: error against float64 (tests/_site_reference.py); LayerNorm figures are\n"
                    "# kappa-normalised (max over rows of row error / max(1, max|y64|) / kappa), softmax figures relative to p64.\n"
                    "# ratio = kernel / (3 x max(torch-CPU, 4u)), u = 2**-24: what the test asserts to be <= 1.\n"
                    f"# device: {torch.cuda.get_device_name(0)}; wall time of the file: {time.time() - t0:.1f} s\n")
            f.write(f"{'site':<10}{'width':>6}  {'class':<20}{'torch-CPU':>12}{'torch-ROCm':>12}{'kernel':>12}{'ratio':>8}\n")
            for site, width, cls, e_cpu, e_rocm, e_k, ratio in RESULTS:
                f.write(f"{site:<10}{width:>6}  {cls:<20}{e_cpu:>12.3e}{e_rocm:>12.3e}{e_k:>12.3e}{ratio:>8.3f}\n")
            for line in NOTES:
                f.write(line + "\n")


def _d(t, dev):
    return None if t is None else t.to(dev)


def _words(t):
    return t.contiguous().view(torch.int32)


def _same_words(a, b):
    """Word equality on the device, NaNs canonicalised (payloads are not part of the contract)."""
    a, b = a.contiguous(), b.contiguous()
    if a.shape != b.shape:
        return False
    both_nan = torch.isnan(a) & torch.isnan(b)
    return bool(((_words(a) == _words(b)) | both_nan).all())


def _quant_variants(dev, scale6, scale8, zp6, zp8):
    """Fixed with an int32 zero point and LSQ+ with a float one, at 6 and 8 bit."""
    from outlier_suppression_amd import ops
    out = []
    for scale, zp, qmax in ((scale6, zp6, 63), (scale8, zp8, 255)):
        s = torch.tensor([scale], device=dev)
        out.append(("fixed%d" % qmax, (s, torch.tensor([zp], dtype=torch.int32, device=dev), 0, qmax, ops.PARAM_FIXED, 1.0)))
        out.append(("lsqplus%d" % qmax, (s, torch.tensor([float(zp)], device=dev), 0, qmax, ops.PARAM_LSQPLUS, 1e-4)))
    return out


# =====================================================================================================================
# LayerNorm site
# =====================================================================================================================

LN_ROW_WIDTHS = (252, 508, 764, 1020, 1028, 4092)     # one ragged width per template instance R = 1, 2, 3, 4, 8, 16
LN_GRID_ROWS = 4096                                   # ln_blocks (1024 workgroups) x 4 waves: rows of one trip
K_DISTINCT = 37


def _ln(dev, x, hidden, gamma, weight, bias, eps, quant=None):
    from outlier_suppression_amd import ops
    with torch.no_grad():
        return ops.residual_layernorm_fake_quant(_d(x, dev), _d(hidden, dev), _d(gamma, dev), _d(weight, dev), _d(bias, dev),
                                                 eps, quant)


def test_row_widths_cover_every_instance():
    assert [R.ln_template_r(c) for c in LN_ROW_WIDTHS] == [1, 2, 3, 4, 8, 16]
    assert all(c % 256 for c in LN_ROW_WIDTHS)
    assert [R.softmax_template_r(c) for c in SM_ROW_WIDTHS] == [1, 2, 4, 8]


@pytest.mark.parametrize("cols", LN_ROW_WIDTHS)
def test_layernorm_rows_are_independent(dev, cols):
    """K distinct rows computed in a [K, H] call, then as the rows of tensors with more rows than one trip of the grid
    (4096): every output row is word-equal to the row of the small call.  One wave reduces one row with a fixed tree, so
    this holds by construction -- and fails if the grid stride, the per-column operands kept in registers across rows, the
    clamped column index or the row base is wrong.  Tensors stay under 140 MB (4092 columns: at most 8191 rows)."""
    gen = torch.Generator().manual_seed(900 + cols)
    xs = R.distinct_rows(K_DISTINCT, cols, gen).to(dev)
    hs = R.distinct_rows(K_DISTINCT, cols, gen, 0.5).to(dev)
    gamma = (torch.rand(cols, generator=gen) * 1.5 + 0.2).to(dev)
    weight = (torch.rand(cols, generator=gen) * 1.5 + 0.2).to(dev)
    bias = (torch.randn(cols, generator=gen) * 0.3).to(dev)
    quant = _quant_variants(dev, 0.11, 0.021, 29, 120)[1][1]
    forms = ((hs, None, weight, bias, 1e-12), (hs, gamma, None, bias, 1e-5), (None, None, weight, bias, 1e-12))
    row_counts = (4096, 4097, 8191) if cols > 1028 else (4096, 4097, 8191, 32768, 32771)
    for rows in row_counts:
        assert rows * cols * 4 <= 140e6
        idx = R.row_map(rows, K_DISTINCT, rows + cols).to(dev)
        x = xs[idx].contiguous()
        for hid, gam, w, b, eps in forms:
            h = None if hid is None else hid[idx].contiguous()
            for q in (None, quant):
                small = _ln(dev, xs, hid, gam, w, b, eps, q)
                big = _ln(dev, x, h, gam, w, b, eps, q)
                same = (_words(big) == _words(small[idx])).all(dim=1)
                assert bool(same.all()), (cols, rows, int((~same).sum()), "first differing row %d" % int((~same).nonzero()[0]))
        del x


@pytest.mark.parametrize("cols", R.LN_WIDTHS)
def test_layernorm_fused_equals_two_step(dev, cols):
    """residual_layernorm_fake_quant(..., quant) is word-equal to fake_quant_per_tensor of the same call without quant, at every
    width, each operand form, Fixed / int32 zero point and LSQ+ / float zero point, 6 and 8 bit.  (This is why the LayerNorm
    site needs no tie exclusion: integer parity follows from the accuracy of the plain output.)"""
    from outlier_suppression_amd import ops
    for combo in R.LN_COMBOS:
        x, hidden, gamma, weight, bias = R.ln_inputs(cols, "outliers", combo)
        for eps in R.LN_EPS:
            y = _ln(dev, x, hidden, gamma, weight, bias, eps)
            for name, q in _quant_variants(dev, 0.11, 0.021, 29, 120):
                yq = _ln(dev, x, hidden, gamma, weight, bias, eps, q)
                two = ops.fake_quant_per_tensor(y, q[0], q[1], q[2], q[3], q[4], q[5])
                assert _same_words(yq, two), (cols, combo[0], eps, name)


@pytest.mark.parametrize("cols", R.LN_WIDTHS)
def test_layernorm_zero_rows(dev, cols):
    """x = hidden = 0: mean 0, variance 0, 0 * rstd = 0 (rstd = 1e6 at eps = 1e-12): the output is the bias word for word;
    without a bias a zero with the sign torch's CPU run of the eager sequence gives."""
    rows = 4100 if cols <= 1028 else 70
    for combo in R.LN_COMBOS:
        _, hidden, gamma, weight, bias = R.ln_inputs(cols, "randn", combo, rows=1)
        x = torch.zeros(rows, cols)
        h = None if hidden is None else torch.zeros(rows, cols)
        for eps in R.LN_EPS:
            y = _ln(dev, x, h, gamma, weight, bias, eps).cpu().numpy()
            ref = R.eager_layernorm(x, weight, bias, eps).numpy()
            if bias is not None:
                assert bits_equal(ref, np.broadcast_to(bias.numpy(), ref.shape)), "torch's CPU run does not return the bias"
            assert bits_equal(y, ref), (cols, combo[0], eps)


@pytest.mark.parametrize("cols", LN_ROW_WIDTHS)
def test_layernorm_nonfinite_rows_stay_contained(dev, cols):
    """Rows holding one NaN, one +inf, one -inf at the first / middle / last column, within the first trip of the grid and
    beyond it: those rows carry the NaN pattern of torch's CPU F.layer_norm, every other row is word-equal to the run
    without the poisoned rows."""
    rows = LN_GRID_ROWS + 512
    for combo in (R.LN_COMBOS[0], R.LN_COMBOS[1], R.LN_COMBOS[2]):
        x, hidden, gamma, weight, bias = R.ln_inputs(cols, "randn", combo, rows=rows)
        target = x if hidden is None else hidden
        clean = _ln(dev, x, hidden, gamma, weight, bias, 1e-12)
        poisoned, n = [], 0
        for base in (3, LN_GRID_ROWS + 5):
            for value in (float("nan"), float("inf"), float("-inf")):
                for col in (0, cols // 2, cols - 1):
                    row = base + 11 * n % 400
                    n += 1
                    target[row, col] = value
                    poisoned.append(row)
        assert len(set(poisoned)) == 18 and min(poisoned) < LN_GRID_ROWS <= max(poisoned)
        y = _ln(dev, x, hidden, gamma, weight, bias, 1e-12)
        keep = torch.ones(rows, dtype=torch.bool)
        keep[poisoned] = False
        assert bool((_words(y)[keep.to(dev)] == _words(clean)[keep.to(dev)]).all()), (cols, combo[0])
        r = torch.from_numpy(R.residual_f32(x[poisoned], None if hidden is None else hidden[poisoned], gamma))
        ref = R.eager_layernorm(r, weight, bias, 1e-12)
        assert torch.equal(torch.isnan(y[poisoned].cpu()), torch.isnan(ref)), (cols, combo[0])
        assert bool(torch.isnan(ref).all())


@pytest.mark.parametrize("cols", R.LN_WIDTHS)
def test_layernorm_accuracy_vs_float64(dev, cols):
    """Plain output (quant=None) against layernorm_site_f64, per data class (tests/_site_reference.py::ln_inputs), the
    four operand forms x eps in {1e-12, 1e-5} folded into one figure per (width, class).  Asserted: kernel error <=
    3 x max(torch-CPU error, 4u), both kappa-normalised.

    Measured on MI355X (profiles/site_accuracy.txt), kappa-normalised, worst over the 21 widths per class, as
    torch-CPU / torch-ROCm / kernel: randn 2.4e-7 / 2.5e-7 / 2.8e-7, outliers 2.9e-7 / 2.3e-7 / 2.6e-7, offset10 1.5e-7 /
    2.3e-7 / 0.9e-7, offset1e3 (kappa to 1.2e4) 1.0e-7 / 1.6e-7 / 0.7e-7, spike 2.7e-7 / 2.9e-7 / 2.7e-7, huge 2.2e-7 /
    2.3e-7 / 2.4e-7, gamma_outliers 2.4e-7 / 2.4e-7 / 2.4e-7, tiny 8.6e-14 for all three (outputs of 1e-14: this class only
    catches a NaN, an inf or a flush that reaches the output).  Worst kernel / bar: 0.39 (1536 columns, randn); where
    torch's figure is above the 4u floor the kernel is at most 1.07x torch's CPU error.  With the variance taken in one
    pass as E[r^2] - mean^2 the same test gives 5.7e-6 at (4 columns, offset10) against a bar of 7.2e-7 and fails at every
    width; with the guard of the row sum dropped in the R = 8 instance it gives 0.68 at 1028 columns."""
    for cls in R.LN_CLASSES:
        e_cpu = e_rocm = e_k = 0.0
        for combo in R.LN_COMBOS:
            x, hidden, gamma, weight, bias = R.ln_inputs(cols, cls, combo)
            r = torch.from_numpy(R.residual_f32(x, hidden, gamma))
            xd, hd, gd = _d(x, dev), _d(hidden, dev), _d(gamma, dev)
            rd = xd if hd is None else (xd * gd if gd is not None else xd) + hd
            assert torch.equal(_words(rd).cpu(), _words(r)), "the residual is not bit-defined"
            for eps in R.LN_EPS:
                y64, kappa = R.layernorm_site_f64(x, hidden, gamma, weight, bias, eps)
                e_cpu = max(e_cpu, R.ln_error(R.eager_layernorm(r, weight, bias, eps).numpy(), y64, kappa))
                with torch.no_grad():
                    e_rocm = max(e_rocm, R.ln_error(R.eager_layernorm(rd, _d(weight, dev), _d(bias, dev), eps).cpu().numpy(), y64, kappa))
                e_k = max(e_k, R.ln_error(_ln(dev, x, hidden, gamma, weight, bias, eps).cpu().numpy(), y64, kappa))
        bar = R.bar_from(e_cpu)
        RESULTS.append(("layernorm", cols, cls, e_cpu, e_rocm, e_k, e_k / bar))
        print(f"layernorm {cols:5d} {cls:<15} torch-CPU {e_cpu:.3e}  torch-ROCm {e_rocm:.3e}  kernel {e_k:.3e}  bar {bar:.3e}")
        assert e_k <= bar, (cols, cls, e_k, bar)


# =====================================================================================================================
# softmax site
# =====================================================================================================================

SM_ROW_WIDTHS = (252, 260, 516, 1028)                 # one ragged width per register instance R = 1, 2, 4, 8
SM_GRID_ROWS = 8192                                   # attn_blocks (2048 workgroups) x 4 waves


def _sm(dev, scores, mask, quant=None, **pre):
    from outlier_suppression_amd import ops
    with torch.no_grad():
        return ops.attention_softmax_fake_quant(scores, mask, quant=quant, **pre)


def _misaligned(t, dev):
    """A contiguous device copy of t whose first element sits 4 bytes past a 16-byte boundary: the generic kernel."""
    buf = torch.empty(t.numel() + 1, dtype=torch.float32, device=dev)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _odd_stride_mask(mask, dev):
    """The mask with a row stride of S + 1 elements (a [..., :S] view): contiguous last axis, rows not 16-byte aligned."""
    s = mask.shape[-1]
    buf = torch.zeros(mask.shape[:-1] + (s + 1,), dtype=torch.float32, device=dev)
    v = buf[..., :s]
    v.copy_(mask)
    return v


@pytest.mark.parametrize("cols", SM_ROW_WIDTHS + (255,))
def test_softmax_rows_are_independent(dev, cols):
    """As for LayerNorm, with more rows than one trip of the grid (8192); the distinct rows include the edge rows of
    test_edge_rows_match_torch_cpu (a NaN, a +inf, all -inf, finfo.min, half -inf), so that each of them is at some point
    the row prefetched behind another and the row ahead of one.  With a full-size mask (MASK = true) and without; 255
    columns is the generic kernel.  1028 columns: 32771 rows at most (135 MB)."""
    gen = torch.Generator().manual_seed(700 + cols)
    s_edge, m_edge = R.softmax_edge_rows(cols, gen)
    k = K_DISTINCT - 5
    ss = torch.cat([R.distinct_rows(k, cols, gen, 2.0), s_edge]).to(dev)
    ms = torch.cat([torch.where(torch.rand(k, cols, generator=gen) < 0.2, torch.tensor(-10000.0), torch.tensor(0.0)), m_edge]).to(dev)
    quant = _quant_variants(dev, 1.0 / 63, 1.0 / 255, 0, 0)[1][1]
    row_counts = (8192, 8193, 32771) if cols > 516 else (8192, 8193, 49155)
    variants = ((ss, ms, {}), (ss + ms, None, dict(alpha=0.125)), (ss, ms, dict(divisor=float(np.sqrt(48.0)))))
    for rows in row_counts:
        assert rows * cols * 4 <= 140e6 and rows >= SM_GRID_ROWS
        idx = R.row_map(rows, K_DISTINCT, rows + cols).to(dev)
        for s_small, m_small, pre in variants:
            s_big = s_small[idx].contiguous().view(1, 1, rows, cols)
            m_big = None if m_small is None else m_small[idx].contiguous().view(1, 1, rows, cols)
            for q in (None, quant):
                small = _sm(dev, s_small.view(1, 1, K_DISTINCT, cols), None if m_small is None else m_small.view(1, 1, K_DISTINCT, cols),
                            q, **pre).view(K_DISTINCT, cols)
                big = _sm(dev, s_big, m_big, q, **pre).view(rows, cols)
                want = small[idx]
                same = ((_words(big) == _words(want)) | (torch.isnan(big) & torch.isnan(want))).all(dim=1)
                assert bool(same.all()), (cols, rows, sorted(pre), int((~same).sum()), "first differing row %d" % int((~same).nonzero()[0]))
                assert bool(torch.isnan(small[k:k + 3]).all()) and not bool(torch.isnan(small[k + 3:]).any())
            del s_big, m_big


@pytest.mark.parametrize("cols", R.SM_REGISTER_WIDTHS + R.SM_GENERIC_WIDTHS)
def test_softmax_exact_rows(dev, cols):
    """A one-hot row (one score 1e4, the rest 0) is exactly 1.0 / +0.0; an all-equal row of a power-of-two width S is exactly
    1 / S; entries under a -inf mask are exactly +0.0 -- in every pre-softmax form, aligned (register kernel where the width
    allows) and misaligned (generic kernel)."""
    rows = 9
    hot = torch.zeros(1, 1, rows, cols)
    where = torch.arange(rows) * (cols - 1) // (rows - 1)
    hot[0, 0, torch.arange(rows), where] = 1e4
    want_hot = torch.zeros(rows, cols)
    want_hot[torch.arange(rows), where] = 1.0
    equal = torch.full((1, 1, rows, cols), 3.0)
    mask = torch.zeros(1, 1, rows, cols)
    mask[..., cols // 2:] = float("-inf")                     # hides the upper half (cols >= 4: never the whole row)
    for name, pre in R.SM_PRE:
        back = 1.0 / pre["alpha"] if "alpha" in pre else pre.get("divisor", 1.0)
        for place in (lambda t: t.to(dev), lambda t: _misaligned(t, dev)):
            y = _sm(dev, place(hot * back), None, **pre).view(rows, cols).cpu()
            assert bits_equal(y.numpy(), want_hot.numpy()), (cols, name)
            y = _sm(dev, place(equal), None, **pre).view(rows, cols).cpu().numpy()
            if cols & (cols - 1) == 0:
                assert bits_equal(y, np.full((rows, cols), 1.0 / cols, np.float32)), (cols, name)
            else:
                assert (y == y[0, 0]).all() and abs(float(y[0, 0]) * cols - 1.0) <= 4 * R.U
            y = _sm(dev, place(equal), mask.to(dev), **pre).view(rows, cols).cpu().numpy()
            assert bits_equal(y[:, cols // 2:], np.zeros((rows, cols - cols // 2), np.float32)), (cols, name)
            assert (y[:, :cols // 2] == y[0, 0]).all() and abs(float(y[0, 0]) * (cols // 2) - 1.0) <= 4 * R.U


@pytest.mark.parametrize("cols", R.SM_REGISTER_WIDTHS + R.SM_GENERIC_WIDTHS)
def test_softmax_fused_equals_two_step(dev, cols):
    """attention_softmax_fake_quant(..., quant) word-equal to fake_quant_per_tensor of its own plain output: every width,
    both kernels, Fixed / int32 zero point and LSQ+ / float zero point, 6 and 8 bit."""
    from outlier_suppression_amd import ops
    for pre in R.SM_PRE:
        scores, mask = R.softmax_inputs(cols, "peaked", pre)
        for place in (lambda t: t.to(dev), lambda t: _misaligned(t, dev)):
            sd = place(scores)
            for m in (mask.to(dev), None):
                p = _sm(dev, sd, m, **pre[1])
                for name, q in _quant_variants(dev, 1.0 / 63, 1.0 / 255, 0, 0):
                    yq = _sm(dev, sd, m, q, **pre[1])
                    assert _same_words(yq, ops.fake_quant_per_tensor(p, q[0], q[1], q[2], q[3], q[4], q[5])), (cols, pre[0], name)


def _softmax_figures(dev, cols, kind, generic_only):
    """(torch-CPU, torch-ROCm, register-or-aligned kernel, misaligned/generic kernel, register-vs-generic, row-sum) errors
    of one (width, kind), folded over the three pre-softmax forms and mask / no mask."""
    e_cpu = e_rocm = e_k = e_g = e_rg = e_sum = 0.0
    for pre in R.SM_PRE:
        scores, mask = R.softmax_inputs(cols, kind, pre)
        for m in (mask, None):
            v32, p64 = R.softmax_site_f64(scores, m, **pre[1])
            v = torch.from_numpy(v32)
            e_cpu = max(e_cpu, R.softmax_error(torch.softmax(v, -1).numpy(), p64))
            e_rocm = max(e_rocm, R.softmax_error(torch.softmax(v.to(dev), -1).cpu().numpy(), p64))
            md = _d(m, dev)
            p = _sm(dev, scores.to(dev), md, **pre[1]).cpu().numpy()
            pg = _sm(dev, _misaligned(scores, dev), md, **pre[1]).cpu().numpy()
            e_k = max(e_k, R.softmax_error(p, p64))
            e_g = max(e_g, R.softmax_error(pg, p64))
            for out in (p, pg):
                e_sum = max(e_sum, float(np.abs(out.astype(np.float64).sum(-1) - 1.0).max()))
            if m is not None:
                assert bits_equal(p[np.broadcast_to(m.numpy(), p.shape) == -np.inf], np.zeros(int((np.broadcast_to(m.numpy(), p.shape) == -np.inf).sum()), np.float32))
                if cols in (256, 1024):           # a mask whose rows are not 16-byte aligned: the generic kernel, same words
                    po = _sm(dev, scores.to(dev), _odd_stride_mask(m, dev), **pre[1]).cpu().numpy()
                    assert bits_equal(po, pg), (cols, kind, pre[0])
            d = np.abs(p.astype(np.float64) - pg.astype(np.float64))
            big = p64 >= R.SOFTMAX_REL_FLOOR
            d[big] /= p64[big]
            e_rg = max(e_rg, float(d.max()))
    return e_cpu, e_rocm, e_k, e_g, e_rg, e_sum


@pytest.mark.parametrize("cols", R.SM_REGISTER_WIDTHS + R.SM_GENERIC_WIDTHS)
def test_softmax_accuracy_vs_float64(dev, cols):
    """Plain probabilities against softmax_site_f64: |p - p64| relative to p64 where p64 >= 2**-100, absolute below; peaked
    rows (the tests/_attention_site.py recipe) and flat rows; the three pre-softmax forms, with and without mask.
    Asserted per (width, kind): kernel error <= 3 x max(torch-CPU fp32 softmax error on the same pre-softmax values, 4u),
    for the aligned call (register kernel up to 2048 columns) and for the 4-byte-misaligned copy (generic kernel); row sums
    within the same bar of 1; the two kernels within twice the bar of each other on the same rows.

    Measured on MI355X (profiles/site_accuracy.txt), worst over the widths as torch-CPU / torch-ROCm / kernel: peaked
    1.2e-6 / 1.4e-6 / 1.1e-6 (dominated by the fp32 rounding of v - max, which all three share), flat
    2.8e-7 / 2.0e-7 / 2.3e-7.  Worst kernel / bar 0.36 (8 columns, peaked), row sums at most 0.22 of the bar, register
    against generic kernel at most 0.39 of the bar (allowed: 2)."""
    generic_only = cols in R.SM_GENERIC_WIDTHS
    for kind in R.SM_KINDS:
        e_cpu, e_rocm, e_k, e_g, e_rg, e_sum = _softmax_figures(dev, cols, kind, generic_only)
        bar = R.bar_from(e_cpu)
        site = "softmax-g" if generic_only else "softmax"
        RESULTS.append((site, cols, kind, e_cpu, e_rocm, e_k, e_k / bar))
        if not generic_only:
            RESULTS.append(("softmax-g", cols, kind + "/misaligned", e_cpu, e_rocm, e_g, e_g / bar))
        print(f"softmax {cols:5d} {kind:<7} torch-CPU {e_cpu:.3e}  torch-ROCm {e_rocm:.3e}  kernel {e_k:.3e}  generic {e_g:.3e}  "
              f"register-vs-generic {e_rg:.3e}  row sums {e_sum:.3e}  bar {bar:.3e}")
        assert e_k <= bar, (cols, kind, e_k, bar)
        assert e_g <= bar, (cols, kind, e_g, bar)
        assert e_sum <= bar, (cols, kind, e_sum, bar)
        assert e_rg <= 2 * bar, (cols, kind, e_rg, bar)


# =====================================================================================================================
# GELU site
# =====================================================================================================================

def _gelu(dev, x, scale, zp, bits, lsqplus):
    """(y, s, z, qmin, qmax): the site's output and the fp32 parameters that reached its quantizer."""
    from outlier_suppression_amd import ops
    s, z, qmin, qmax, gf = R.effective_params(scale, zp, bits, lsqplus, x.size)
    st = torch.tensor([scale], device=dev)
    zt = torch.tensor([float(zp)], device=dev) if lsqplus else torch.tensor([zp], dtype=torch.int32, device=dev)
    xd = torch.from_numpy(x).to(dev)
    assert xd.data_ptr() % 16 == 0                      # the one-launch path, not the two-launch one for unaligned slices
    with torch.no_grad():
        y = ops.gelu_fake_quant_per_tensor(xd, st, zt, qmin, qmax, ops.PARAM_LSQPLUS if lsqplus else ops.PARAM_FIXED, gf)
    return y.cpu().numpy(), s, z, qmin, qmax, gf


@pytest.mark.parametrize("lsqplus", [False, True], ids=["fixed", "lsqplus"])
def test_gelu_integers_vs_float64(dev, lsqplus):
    """There is no un-quantised output, so the site is judged on integers: q64 = clamp(rint(gelu_f64(x) / s) + zp).  The
    device's integers (y / s + zp rounded) differ from q64 by at most one step, and only where gelu_f64(x) / s lies within
    delta / s of a half-integer, delta = 2 x the largest |torch-CPU fp32 F.gelu - gelu_f64| on the same input.  Before the
    comparison: that neighbourhood holds at most 2e-3 of the entries for every (input, scale).

    Measured on MI355X (profiles/site_accuracy.txt): delta 2.5e-6 (3 * randn), 2.1e-6 (tail ladder), 4.6e-7 (rising ladder);
    tie shares 0 to 1.05e-3; 0-6 integers of 4.2 M (randn), 0 of 197 k (tail) and 0-5 of 1.44 M (rise) differ, each by one
    step, the farthest of them 4.3e-8 from its rounding boundary (torch's CPU fp32 GELU: 2-27, 0-4 and 0-4 differing)."""
    for name, x in R.gelu_inputs().items():
        g64 = R.gelu_f64(x)
        delta = R.gelu_delta(x)
        for scale, zp, bits in R.GELU_QUANT:
            y, s, z, qmin, qmax, _ = _gelu(dev, x, scale, zp, bits, lsqplus)
            q64, dist = R.gelu_q64(g64, s, z, qmin, qmax)
            near = dist <= delta
            share = float(near.mean())
            assert share <= R.GELU_TIE_SHARE, (name, scale, share)
            diff = R.integers_of(y, s, z) - q64
            moved = diff != 0
            implied = float(dist[moved].max()) if moved.any() else 0.0
            line = (f"gelu {name:<12} s={scale:<7} {'lsqplus' if lsqplus else 'fixed':<8} delta {delta:.3e}  tie share {share:.3e}  "
                    f"integers differing {int(moved.sum())} of {x.size}  largest implied deviation {implied:.3e}")
            print(line)
            NOTES.append(line)
            assert np.abs(diff).max() <= 1, (name, scale, float(np.abs(diff).max()))
            assert not moved[~near].any(), (name, scale, int(moved[~near].sum()), implied, delta)


@pytest.mark.parametrize("lsqplus", [False, True], ids=["fixed", "lsqplus"])
def test_gelu_specials(dev, lsqplus):
    """+-0, +-subnormal, +-40, +-inf and NaN at the head, in the float4 body and in the scalar tail: the output is word-equal
    to the oracle's fake-quant (oracle/fake_quant_oracle.py) of torch's CPU F.gelu (the sign of zero included: gelu(-0.0),
    gelu(-40) = -0)."""
    import torch.nn.functional as F
    for x, pos in R.gelu_special_inputs():
        g32 = F.gelu(torch.from_numpy(x)).numpy()
        for scale, zp, bits in R.GELU_QUANT:
            y, s, z, qmin, qmax, gf = _gelu(dev, x, scale, zp, bits, lsqplus)
            if lsqplus:
                _, ref = FQ.fake_quantize_learnableplus_per_tensor(g32, np.float32(scale), np.float32(zp), qmin, qmax, gf)
            else:
                _, ref = FQ.fake_quantize_per_tensor_affine(g32, scale, zp, qmin, qmax)
            assert bits_equal(y[pos], ref[pos]), (x.size, scale, x[pos][~(y[pos] == ref[pos])])

"""osq_token_logprob / osq_token_logprob_backward (csrc/token_logprob.hip) through the C ABI, against the float64 restatement
of tests/_token_logprob.py.

Vocabularies on both sides of every seam of the layout (a 128-bit access, the 1024 tokens one access of the workgroup covers,
the 4096-token chunk, 13 and 15 chunks), 1 to 257 rows, rows of odd strides that start 4, 8 and 12 bytes past a 16-byte
boundary with NaN between them, the label and the row's maximum planted on every seam, and the rows the rule names one by one.
Outputs and workspace are NaN / sentinel-filled before every launch, every launch runs twice and must give the same words.
Forward: every row inside 2e-5 + 2**-21 * (|z_t - m| + |ln W|), the loss inside the mean of its rows' bounds.  Backward: the
elementwise bound derived in tests/_token_logprob.py, ignored rows exactly 0, and the sum of a scored row within vocab ulps of
its coefficient.  The largest excursions go to profiles/token_logprob_accuracy.txt when OSQ_TOKEN_LOGPROB_ACCURACY_OUT=<path>
is set."""
import os

import numpy as np
import pytest
import torch

import _token_logprob as TL

pytestmark = pytest.mark.gpu

SENTINEL = -77.0
_seen = {}             # what -> (excursion, bound, where): the largest excursion relative to its bound


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _note(what, off, tol, where):
    if tol > 0 and (what not in _seen or off / tol > _seen[what][0] / _seen[what][1]):
        _seen[what] = (off, tol, where)


def _place(logits, dev, pad=0, offset=0, fill=float("nan")):
    """The rows of ``logits`` on the device ``vocab + pad`` elements apart, the first one ``offset`` elements into a 16-byte
    aligned buffer, ``fill`` everywhere else."""
    rows, vocab = logits.shape
    stride = vocab + pad
    flat = torch.full((offset + rows * stride + 4,), fill, dtype=torch.float32, device=dev)
    assert flat.data_ptr() % 16 == 0
    view = flat[offset:offset + rows * stride].view(rows, stride)[:, :vocab]
    view.copy_(torch.from_numpy(np.ascontiguousarray(logits)))
    return flat, view, stride


def _forward(dev, view, stride, labels, ignore_index=TL.IGNORE, reduce=True):
    """Two launches over sentinel-filled outputs and a NaN-filled workspace, word-equal; (lp, lse, loss, counts) as numpy."""
    from outlier_suppression_amd import _hip
    lib = _hip.load()
    rows, vocab = view.shape
    t = torch.from_numpy(np.asarray(labels, dtype=np.int64)).to(dev)
    nbytes = int(lib.osq_token_logprob_workspace_bytes(rows, vocab))
    assert nbytes == rows * ((vocab + TL.CHUNK - 1) // TL.CHUNK) * 8
    runs = []
    for _ in range(2):
        lp = torch.full((rows + 2,), SENTINEL, device=dev)
        lse = torch.full((rows + 2,), SENTINEL, device=dev)
        loss = torch.full((3,), SENTINEL, device=dev)
        counts = torch.full((4,), -7, dtype=torch.int64, device=dev)
        ws = torch.full((nbytes // 4 + 2,), float("nan"), device=dev)
        rc = lib.osq_token_logprob(view.data_ptr(), stride, t.data_ptr(), rows, vocab, ignore_index, lp[1:].data_ptr(),
                                   lse[1:].data_ptr(), loss[1:].data_ptr() if reduce else None,
                                   counts[1:].data_ptr() if reduce else None, ws.data_ptr(), _hip.raw_stream(dev))
        assert rc == 0, lib.osq_last_error()
        torch.cuda.synchronize()
        out = [x.cpu().numpy() for x in (lp, lse, loss, counts)]
        for x in out[:2]:                                                   # nothing beside the rows' words
            assert x[0] == SENTINEL and x[-1] == SENTINEL
        assert out[2][0] == SENTINEL and out[2][2] == SENTINEL and out[3][0] == -7 and out[3][3] == -7
        if not reduce:
            assert out[2][1] == SENTINEL and out[3][1] == -7
        assert torch.isnan(ws[-2:]).all()
        runs.append((out[0][1:-1], out[1][1:-1], out[2][1], out[3][1:3]))
    for a, b in zip(*runs):
        assert np.array_equal(np.asarray(a).view(np.uint32 if np.asarray(a).dtype == np.float32 else np.int64),
                              np.asarray(b).view(np.uint32 if np.asarray(b).dtype == np.float32 else np.int64))
    return runs[0]


def _check(got, want, label):
    lp, lse, loss, counts = got
    off, tol = TL.check_forward(lp, lse, want, label)
    _note("forward |lp - lp64|", off, tol, label)
    assert counts.tolist() == [int(want["scored"].sum()), int(want["bad"].sum())], label
    if np.isnan(want["loss"]):
        assert np.isnan(loss), (label, loss)
    else:
        assert abs(float(loss) - want["loss"]) <= want["loss_tol"], (label, loss, want["loss"], want["loss_tol"])
        _note("forward |loss - loss64|", abs(float(loss) - want["loss"]), want["loss_tol"], label)


PLACES = ((0, 0), (1, 1), (5, 3), (2, 2), (0, 1))       # (pad, offset): odd and even strides, every alignment of the first row


@pytest.mark.parametrize("vocab", TL.VOCABS)
def test_a_every_vocabulary_and_row_count_against_float64(dev, vocab):
    rng = np.random.default_rng(vocab)
    logits, labels = TL.random_case(rng, max(TL.ROWS), vocab)
    labels[0] = vocab - 1
    want = TL.forward64(logits, labels)
    first = {}
    for rows, (pad, offset) in zip(TL.ROWS, PLACES):
        sub = {k: (v[:rows] if isinstance(v, np.ndarray) else v) for k, v in want.items()}
        n = int(sub["scored"].sum())
        sub["loss"] = -sub["lp"].sum() / n if n else np.nan
        sub["loss_tol"] = sub["tol"][sub["scored"]].mean() if n else 0.0
        _, view, stride = _place(logits[:rows], dev, pad, offset)
        got = _forward(dev, view, stride, labels[:rows])
        _check(got, sub, f"vocab {vocab}, {rows} rows, stride {stride}, offset {offset}")
        # a row's words do not depend on the rows of the launch, on the stride or on the alignment
        for r in range(min(rows, 3)):
            words = (got[0][r].view(np.uint32), got[1][r].view(np.uint32))
            assert first.setdefault(r, words) == words, (vocab, rows, r)
        plain = _forward(dev, view, stride, labels[:rows], reduce=False)      # without loss and counts: the same words
        assert np.array_equal(plain[0].view(np.uint32), got[0].view(np.uint32))
        assert np.array_equal(plain[1].view(np.uint32), got[1].view(np.uint32))


@pytest.mark.parametrize("vocab", (5, 4097, 8193, 50265, 57345))
def test_b_label_and_maximum_planted_on_every_seam(dev, vocab):
    logits, labels = TL.planted_case(np.random.default_rng(vocab + 1), vocab)
    want = TL.forward64(logits, labels)
    for pad, offset in ((0, 0), (1, 3)):
        _, view, stride = _place(logits, dev, pad, offset)
        _check(_forward(dev, view, stride, labels), want, f"planted, vocab {vocab}, stride {stride}, offset {offset}")


@pytest.mark.parametrize("vocab", (1, 5, 4097, 50265))
def test_c_the_constructed_rows(dev, vocab):
    logits, labels, notes = TL.constructed_case(np.random.default_rng(vocab + 2), vocab)
    want = TL.forward64(logits, labels)
    at = {n: i for i, n in enumerate(notes)}
    _, view, stride = _place(logits, dev, 1, 1)
    lp, lse, loss, counts = got = _forward(dev, view, stride, labels)
    _check(got, want, f"constructed, vocab {vocab}")
    r = at["survivor, label on it"]
    assert lp[r].view(np.uint32) == 0 and lse[r] == np.float32(-3.25)              # exactly +0.0
    if vocab > 1:
        assert lp[at["survivor, label elsewhere"]] == -np.inf
    for n in ("all -inf", "a NaN", "+inf", "label -1", "label V"):
        assert np.isnan(lp[at[n]]), n
    assert lp[at["ordinary, ignored"]].view(np.uint32) == 0 and np.isfinite(lse[at["ordinary, ignored"]])
    assert counts.tolist() == [len(notes) - 3, 2] and np.isnan(loss)
    # the two labels outside the vocabulary leave every other row's words untouched
    fine = labels.copy()
    fine[[at["label -1"], at["label V"]]] = 0
    lp2, lse2, _, counts2 = _forward(dev, view, stride, fine)
    others = [i for i, n in enumerate(notes) if n not in ("label -1", "label V")]
    assert np.array_equal(lp[others].view(np.uint32), lp2[others].view(np.uint32))
    assert np.array_equal(lse.view(np.uint32), lse2.view(np.uint32)) and counts2.tolist() == [len(notes) - 1, 0]


@pytest.mark.parametrize("vocab", (65, 4097, 50265))
def test_d_a_rows_words_do_not_depend_on_the_launch(dev, vocab):
    rng = np.random.default_rng(vocab + 3)
    logits, labels = TL.random_case(rng, 257, vocab, ignored=0.0)
    row, label = logits[100:101].copy(), labels[100:101]
    _, view, stride = _place(row, dev)
    alone = _forward(dev, view, stride, label)
    for r in (0, 256):
        many = logits.copy()
        many[r] = row[0]
        t = labels.copy()
        t[r] = label[0]
        _, view, stride = _place(many, dev, 1, 2)
        got = _forward(dev, view, stride, t)
        assert got[0][r].view(np.uint32) == alone[0][0].view(np.uint32) and got[1][r].view(np.uint32) == alone[1][0].view(np.uint32)


def test_e_inside_a_captured_graph(dev):
    from outlier_suppression_amd import ops
    rng = np.random.default_rng(9)
    logits, labels = TL.random_case(rng, 33, 8193)
    other, _ = TL.random_case(rng, 33, 8193)
    _, view, _ = _place(logits, dev, 1, 1)
    t = torch.from_numpy(labels).to(dev)
    want = [x.clone() for x in ops.lm_loss(view, t)]                               # sizes the workspace, too
    want_other = [x.clone() for x in ops.lm_loss(torch.from_numpy(other).to(dev), t)]
    out = (torch.empty((), device=dev), torch.empty(33, device=dev), torch.empty(33, device=dev),
           torch.empty(2, dtype=torch.int64, device=dev))
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        ops.lm_loss(view, t, out=out)                                              # this stream's workspace
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            got = ops.lm_loss(view, t, out=out)
    torch.cuda.current_stream().wait_stream(stream)
    assert all(g is o for g, o in zip(got, out))
    for expect, source in ((want, None), (want_other, other), (want, logits)):
        if source is not None:
            view.copy_(torch.from_numpy(source))
        for o in out:
            o.fill_(-5)
        graph.replay()
        torch.cuda.synchronize()
        for g, w in zip(out, expect):
            assert torch.equal(g, w)
    TL.check_forward(out[1].cpu().numpy(), out[2].cpu().numpy(), TL.forward64(logits, labels), "replayed")


def _backward(dev, view, stride, labels, lse, row_grad=None, scalar_grad=None, counts=None, pad=3, ignore_index=TL.IGNORE):
    from outlier_suppression_amd import _hip
    lib = _hip.load()
    rows, vocab = view.shape
    t = torch.from_numpy(np.asarray(labels, dtype=np.int64)).to(dev)
    dstride = vocab + pad
    runs = []
    for _ in range(2):
        flat = torch.full((1 + rows * dstride + 4,), SENTINEL, device=dev)
        rc = lib.osq_token_logprob_backward(view.data_ptr(), stride, t.data_ptr(), lse.data_ptr(), _hip.ptr(row_grad),
                                            _hip.ptr(scalar_grad), _hip.ptr(counts), rows, vocab, ignore_index,
                                            flat[1:].data_ptr(), dstride, _hip.raw_stream(dev))
        assert rc == 0, lib.osq_last_error()
        torch.cuda.synchronize()
        body = flat[1:1 + rows * dstride].view(rows, dstride)
        assert flat[0] == SENTINEL and (flat[1 + rows * dstride:] == SENTINEL).all() and (body[:, vocab:] == SENTINEL).all()
        runs.append(body[:, :vocab].cpu().numpy())
    assert np.array_equal(runs[0].view(np.uint32), runs[1].view(np.uint32))
    return runs[0]


def _check_backward(got, d, tol, coef, live, vocab, label):
    """The elementwise bound and the exact zeros, asserted here; returns what the row sums miss their bound by (rows, worst
    ratio), asserted by the caller after every form of the case has been through the elementwise check."""
    off = np.abs(got.astype(np.float64) - d)
    assert (off <= tol).all(), (label, float((off - tol).max()), np.unravel_index(np.argmax(off - tol), off.shape))
    assert (got[~live] == 0).all(), label                                           # ignored and bad rows: exactly 0
    i = np.unravel_index(np.argmax(np.where(tol > 0, off / np.where(tol > 0, tol, 1.0), 0.0)), off.shape)
    _note("backward |dlogits - dlogits64|", float(off[i]), float(tol[i]), label)
    sums = np.abs(got.astype(np.float64).sum(axis=1))
    ulps = vocab * 2.0 ** -23 * np.abs(coef)                                        # one ulp of coef: at most 2**-23 |coef|
    if not live.any():
        return 0, 0.0
    ratio = np.where(live, sums / np.where(ulps > 0, ulps, 1.0), 0.0)
    r = int(np.argmax(ratio))
    print(f"{label}: largest |sum_v dlogits| / (vocab ulps of coef) = {ratio[r]:.3f} (row {r})")
    _note(f"backward |sum_v dlogits| of a row, vocab {vocab}", float(sums[r]), float(ulps[r]), label)
    return int((ratio > 1.0).sum()), float(ratio[r])


@pytest.mark.parametrize("vocab, rows", ((1, 3), (2, 257), (5, 3), (65, 257), (257, 3), (1025, 257), (4097, 257), (8193, 3),
                                         (50265, 3), (50265, 40), (57345, 2)))
def test_f_backward_against_float64(dev, vocab, rows):
    """The sum of a scored row's dlogits within vocab ulps of coef holds because a row of one chunk is divided by the
    workgroup's own sum of its expf(z - lse) (include/osq_hip.h): with the bare expf(z - lse) the rounding of the fp32 lse, up
    to 2**-24 * |lse|, moves every exponent of the row alike and alone passes vocab * 2**-23 once |lse| > 2 * vocab -- measured
    2.44 times the bound at [2-257] before the division.  From 4097 tokens on the bound is 4.9e-4 |coef| and more."""
    rng = np.random.default_rng(vocab * 7 + rows)
    logits, labels = TL.random_case(rng, rows, vocab)
    labels[0] = vocab - 1
    if rows > 2:
        labels[1], labels[2] = TL.IGNORE, vocab                                    # an ignored row and a bad label
    for p, r in zip(TL.seams(vocab), range(3, rows)):
        labels[r] = p
    _, view, stride = _place(logits, dev, 1, 1)
    lp, lse, loss, counts = _forward(dev, view, stride, labels)
    want = TL.forward64(logits, labels)
    live = want["scored"]
    lse_d = torch.from_numpy(lse.copy()).to(dev)
    # reduction='none': a per-row upstream gradient
    up = rng.standard_normal(rows).astype(np.float32)
    got = _backward(dev, view, stride, labels, lse_d, row_grad=torch.from_numpy(up).to(dev))
    d, tol = TL.backward64(logits, labels, up.astype(np.float64))
    missed = [_check_backward(got, d, tol, up.astype(np.float64), live, vocab, f"none, vocab {vocab}, {rows} rows")]
    # the mean: upstream / scored, both read on the device
    g = torch.tensor([1.75], device=dev)
    n = torch.tensor([int(live.sum()), int(want["bad"].sum())], dtype=torch.int64, device=dev)
    assert counts.tolist() == n.tolist()
    got = _backward(dev, view, stride, labels, lse_d, scalar_grad=g, counts=n, pad=0)
    coef = np.full(rows, 1.75 / max(int(live.sum()), 1))
    d, tol = TL.backward64(logits, labels, coef)
    missed.append(_check_backward(got, d, tol, coef, live, vocab, f"mean, vocab {vocab}, {rows} rows"))
    assert all(n == 0 for n, _ in missed), ("rows whose |sum_v dlogits| exceeds vocab ulps of coef, and the worst ratio", missed)


def test_g_arguments(dev):
    from outlier_suppression_amd import _hip
    lib = _hip.load()
    st = _hip.raw_stream(dev)
    x = torch.zeros(4, 8, device=dev)
    t = torch.zeros(4, dtype=torch.int64, device=dev)
    lp, lse, loss = torch.full((4,), SENTINEL, device=dev), torch.full((4,), SENTINEL, device=dev), torch.full((1,), SENTINEL, device=dev)
    counts = torch.full((2,), -7, dtype=torch.int64, device=dev)
    ws = torch.zeros(64, device=dev)
    dx = torch.full((4, 8), SENTINEL, device=dev)
    P = lambda v: v.data_ptr()  # noqa: E731
    good = [P(x), 8, P(t), 4, 8, -100, P(lp), P(lse), P(loss), P(counts), P(ws), st]
    for i, bad in ((0, None), (2, None), (6, None), (7, None), (10, None), (4, 0), (4, 2 ** 31), (1, 7), (3, -1)):
        args = list(good)
        args[i] = bad
        assert lib.osq_token_logprob(*args) == -1, (i, bad)
    back = [P(x), 8, P(t), P(lse), P(lp), None, None, 4, 8, -100, P(dx), 8, st]
    for i, bad in ((0, None), (2, None), (3, None), (10, None), (4, None), (8, 0), (1, 7), (11, 7), (7, -1)):
        args = list(back)
        args[i] = bad
        assert lib.osq_token_logprob_backward(*args) == -1, (i, bad)
    assert lib.osq_token_logprob_workspace_bytes(-1, 8) == 0 and lib.osq_token_logprob_workspace_bytes(4, 0) == 0
    assert lib.osq_token_logprob_workspace_bytes(2 ** 31, 8) == 0 and lib.osq_token_logprob_workspace_bytes(0, 8) == 0
    torch.cuda.synchronize()
    assert (lp == SENTINEL).all() and (lse == SENTINEL).all() and (loss == SENTINEL).all() and (dx == SENTINEL).all()
    # no rows: loss = NaN, counts = 0, nothing else -- and no pointer but those is needed
    assert lib.osq_token_logprob(None, 8, None, 0, 8, -100, None, None, P(loss), P(counts), None, st) == 0
    assert lib.osq_token_logprob_backward(None, 8, None, None, P(lp), None, None, 0, 8, -100, None, 8, st) == 0
    torch.cuda.synchronize()
    assert torch.isnan(loss).all() and counts.tolist() == [0, 0] and (lp == SENTINEL).all()


def test_h_ops_and_autograd(dev):
    from outlier_suppression_amd import ops
    from outlier_suppression_amd.model.losses import FusedLmLoss
    rng = np.random.default_rng(21)
    logits, labels = TL.random_case(rng, 37, 4099)
    want = TL.forward64(logits, labels)
    _, view, stride = _place(logits, dev, 2, 1)
    t = torch.from_numpy(labels).to(dev)
    loss, lp, lse, counts = ops.lm_loss(view, t)
    lp2, lse2 = ops.token_logprob(view, t)
    base = _forward(dev, view, stride, labels)
    assert np.array_equal(lp.cpu().numpy().view(np.uint32), base[0].view(np.uint32)) and torch.equal(lp, lp2) and torch.equal(lse, lse2)
    assert float(loss) == float(base[2]) and counts.tolist() == base[3].tolist()
    z = view.detach().clone().requires_grad_(True)
    got, n = FusedLmLoss.apply(z, t, TL.IGNORE)
    (got * 1.75).backward()
    assert float(got.detach()) == float(loss) and n.tolist() == counts.tolist()
    coef = np.full(37, 1.75 / int(want["scored"].sum()))
    d, tol = TL.backward64(logits, labels, coef)
    assert (np.abs(z.grad.cpu().numpy().astype(np.float64) - d) <= tol).all()
    with pytest.raises(TypeError):
        ops.token_logprob(view.half(), t)
    with pytest.raises(ValueError):
        ops.token_logprob(view, t[:5])
    with pytest.raises(RuntimeError):
        ops.token_logprob(view.cpu(), t.cpu())


def test_z_accuracy_record():
    path = os.environ.get("OSQ_TOKEN_LOGPROB_ACCURACY_OUT")
    if path and _seen:
        with open(path, "w") as f:
            f.write("osq_token_logprob / osq_token_logprob_backward against the float64 restatement of tests/_token_logprob.py on the\n"
                    "cases of tests/test_gpu_token_logprob.py (MI355X): per quantity the excursion that came closest to its bound,\n"
                    "beside that bound.  forward: 2e-5 + 2**-21 * (|z_t - m| + |ln W|) per row, its mean over the scored rows for\n"
                    "the loss; backward: the elementwise bound derived in tests/_token_logprob.py, and vocab * 2**-23 * |coef| for\n"
                    "the sum of a scored row.\n\n")
            for what, (off, tol, where) in _seen.items():
                f.write(f"{what:<46} {off:.3e}   bound {tol:.3e}   ({off / tol:.3f} of it)   {where}\n")

"""The position-from-device launches of a decoding step, through ``ops``: ops.decode_attention_at
(osq_decode_attention_fake_quant_at / osq_decode_attention_codes_at) and ops.fake_quant_kv_append_at / _codes_at.

The contract is one sentence: for any position, an _at launch produces the words and bytes of the static entry point
called with that position.  So every case captures ONE hipGraph of the _at launch and replays it once per position; between
two replays the test writes the device word (and, for the attention, poisons the cache beyond the new length); each
replay is compared with the static launch at that position word for word -- no tolerance, no oracle: the static launches
have their own tests (test_gpu_decode_attention.py, test_gpu_kv_codes.py, test_gpu_bart_decode.py).

Attention: every head size the kernel takes; lengths either side of one trip of the workgroup (P = 1024 / head_dim
positions), of four trips (the loads in flight of the fp32 form) and a ragged tail beyond eight; K / V beyond the length
hold NaN words (0xFF bytes), so a read past the length shows; the mask is NULL or a strided buffer with a -inf column; a
length of 0 and of kv_max + 1 gives NaN in every word of out.
Append: the model's three sites (an fp32 query, keys and values fp32 or coded), in place and into a partner through a row
index; offsets at the edges of the 16-byte copy width of a coded prefix (head size 4: 1 and 3 are no multiple of it, 4 and
8 are); the position 12 == cap is refused: nothing written, a coded cache counts it once."""
import math

import numpy as np
import pytest
import torch

from conftest import same_f32

pytestmark = pytest.mark.gpu

B, H = 2, 2
QMIN, QMAX = 0, 63


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from outlier_suppression_amd import _hip
    _hip.load()
    return torch.device("cuda:0")


def captured(dev, launch):
    """``launch`` issued once on a side stream, then captured there: the graph."""
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        launch()
    torch.cuda.current_stream(dev).wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        launch()
    return graph


def lsqplus(scale, zero_point, numel, dev):
    """(scale, zero_point, quant_min, quant_max, mode, grad_factor) of a 6-bit LSQ+ quantizer seeing ``numel`` elements."""
    from outlier_suppression_amd import ops
    return (torch.tensor([scale], dtype=torch.float32, device=dev), torch.tensor([zero_point], dtype=torch.float32, device=dev),
            QMIN, QMAX, ops.PARAM_LSQPLUS | ops.PARAM_SANITIZE, 1.0 / (numel * QMAX) ** 0.5)


# ------------------------------------------------------------------------------------------------ attention

def kv_lens(d):
    p = 1024 // d
    return sorted({n for n in (1, p - 1, p, p + 1, 4 * p, 4 * p + 1, min(4096, 8 * p + 3)) if 1 <= n <= 4096})


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("coded", [False, True], ids=["fp32", "codes"])
@pytest.mark.parametrize("d", [4, 8, 16, 32, 64, 128, 256])
def test_attention_at_equals_static_at_every_length(dev, d, coded, masked):
    from outlier_suppression_amd import ops
    g = torch.Generator(device=dev).manual_seed(1000 * d + 10 * coded + masked)
    lens = kv_lens(d)
    kv_max = lens[-1]
    cap = kv_max + 5
    q = torch.randn(B, H, 1, d, generator=g, device=dev) * d ** -0.5
    if coded:
        k0 = torch.randint(0, QMAX + 1, (B, H, cap, d), generator=g, device=dev).to(torch.uint8)
        v0 = torch.randint(0, QMAX + 1, (B, H, cap, d), generator=g, device=dev).to(torch.uint8)
        records = [(torch.tensor([s], device=dev), torch.tensor([z], device=dev), QMIN) for s, z in ((0.11, 30.0), (0.07, 33.0))]
        rejected = torch.zeros(1, dtype=torch.int32, device=dev)
        poison = 0xFF
    else:
        k0 = torch.randn(B, H, cap, d, generator=g, device=dev)
        v0 = torch.randn(B, H, cap, d, generator=g, device=dev)
        poison = float("nan")
    k, v = k0.clone(), v0.clone()
    mask = None
    if masked:
        width = kv_max + 3                                    # rows further apart than any length: a strided mask
        mask = torch.zeros(B, 1, 1, width, device=dev)
        mask[0, 0, 0, 1] = float("-inf")
        mask[1, 0, 0, 2 % width] = float("-inf")
        mask[1, 0, 0, 5:] = torch.finfo(torch.float32).min      # a padded tail on the second row
    probs_out = torch.full((B, H, 1, kv_max + 2), 7.0, device=dev)
    out = torch.empty(B, 1, H * d, device=dev)
    word = torch.zeros(1, dtype=torch.int32, device=dev)
    # the host's own grad factors of the probabilities quantizer, one per length: what the static call is handed
    table = torch.tensor([0.0] + [1.0 / (B * H * n * QMAX) ** 0.5 for n in range(1, kv_max + 1)], dtype=torch.float64)
    table = table.to(torch.float32).to(dev)
    pq, cq = lsqplus(1.0 / 50, 2.0, B * H, dev), lsqplus(0.05 if not coded else 0.3, 31.0, B * H * d, dev)
    codes = (records[0], records[1], rejected) if coded else None

    def launch():
        got = ops.decode_attention_at(q, k, v, word, 1, kv_max, mask, pq, cq, grad_table=table, codes=codes, out=out,
                                      probs_out=probs_out)
        assert got is out

    word.fill_(lens[-1] - 1)
    graph = captured(dev, launch)
    for n in reversed(lens):                                  # longest first: the poisoned tail only grows
        word.fill_(n - 1)                                     # the launch adds 1, as the self-attention of a step does
        k[:, :, n:] = poison
        v[:, :, n:] = poison
        out.fill_(5.0)
        probs_out.fill_(7.0)
        graph.replay()
        pn = (pq[0].clone(), pq[1].clone(), QMIN, QMAX, pq[4], 1.0 / (B * H * n * QMAX) ** 0.5)
        cn = (cq[0].clone(), cq[1].clone()) + cq[2:]
        mask_n = None if mask is None else mask[..., :n].contiguous()
        if coded:
            want, want_probs = ops.decode_attention_codes(q, k0[:, :, :n], v0[:, :, :n], mask_n, pn, cn, records[0], records[1],
                                                          rejected, want_probs=True)
        else:
            want, want_probs = ops.decode_attention_fake_quant(q, k0[:, :, :n], v0[:, :, :n], mask_n, pn, cn, want_probs=True)
        assert not torch.isnan(want).any(), n
        assert same_f32(out.cpu().numpy(), want.cpu().numpy()), (d, n)
        assert same_f32(probs_out[..., :n].cpu().numpy(), want_probs.cpu().numpy()), (d, n)
        assert bool((probs_out[..., n:] == 7.0).all()), (d, n)             # nothing written beyond the length
    for bad in (0, kv_max + 1):
        word.fill_(bad - 1)
        out.fill_(5.0)
        probs_out.fill_(7.0)
        graph.replay()
        assert bool(torch.isnan(out).all()), bad
        assert bool((probs_out == 7.0).all()), bad
    if coded:
        assert int(rejected.item()) == 0


# ------------------------------------------------------------------------------------------------ append

AB, AH, CAP, SRC_CAP, T = 3, 2, 12, 9, 1
OFFSETS = (0, 1, 3, 4, 8)
SENTINEL_F, SENTINEL_B = -77.0, 0xA5


def _append_buffers(dev, d, coded, g):
    """Destination, partner source (random content of the destination's kind) and record of one cached tensor."""
    if coded:
        y = torch.full((AB, AH, CAP, d), SENTINEL_B, dtype=torch.uint8, device=dev)
        src = torch.randint(0, QMAX + 1, (AB, AH, SRC_CAP, d), generator=g, device=dev).to(torch.uint8)
        record = (torch.full((1,), float("nan"), device=dev), torch.full((1,), float("nan"), device=dev))
    else:
        y = torch.full((AB, AH, CAP, d), SENTINEL_F, device=dev)
        src = torch.randn(AB, AH, SRC_CAP, d, generator=g, device=dev)
        record = None
    return y, src, record


def _bytes(t):
    return t.contiguous().view(torch.uint8).cpu().numpy()


@pytest.mark.parametrize("moved", [False, True], ids=["inplace", "partner"])
@pytest.mark.parametrize("coded", [False, True], ids=["fp32", "codes"])
@pytest.mark.parametrize("d", [4, 64])
def test_append_at_equals_static_at_every_offset(dev, d, coded, moved):
    from outlier_suppression_amd import ops
    g = torch.Generator(device=dev).manual_seed(77 * d + 2 * coded + moved)
    xs = [torch.randn(AB, T, AH * d, generator=g, device=dev) * 2 for _ in range(3)]
    quants = [lsqplus(s, 31.0, x.numel(), dev) for s, x in zip((0.11, 0.07, 0.05), xs)]
    rows = torch.tensor([2, 0, 0], dtype=torch.int64, device=dev) if moved else None
    pos = torch.zeros(1, dtype=torch.int32, device=dev)
    state = {}
    for run in ("at", "static"):
        bufs = [_append_buffers(dev, d, coded, torch.Generator(device=dev).manual_seed(5 + i)) for i in range(2)]
        state[run] = dict(yq=torch.full((AB, AH, T, d), SENTINEL_F, device=dev), ys=[b[0] for b in bufs],
                          srcs=[b[1] for b in bufs], records=[b[2] for b in bufs],
                          rejected=torch.zeros(1, dtype=torch.int32, device=dev),
                          params=[(q[0].clone(), q[1].clone()) + q[2:] for q in quants])

    def sites(run, offset):
        s = state[run]
        # a partner source: the whole buffer for the _at form, its first `offset` positions (a view) for the static one
        src = [None, None] if not moved else (s["srcs"] if offset is None else [t[:, :, :offset] for t in s["srcs"]])
        table = [(xs[0], s["yq"], 0, s["params"][0], None, None),
                 (xs[1], s["ys"][0], offset, s["params"][1], src[0], rows),
                 (xs[2], s["ys"][1], offset, s["params"][2], src[1], rows)]
        if not coded:
            return table
        return [table[0] + (None, False)] + [e + (rec, True) for e, rec in zip(table[1:], s["records"])]

    def reset(run):
        s = state[run]
        s["yq"].fill_(SENTINEL_F)
        for y in s["ys"]:
            y.fill_(SENTINEL_B if coded else SENTINEL_F)
        for rec in s["records"]:
            if rec is not None:
                rec[0].fill_(float("nan"))
                rec[1].fill_(float("nan"))

    def launch_at():
        if coded:
            assert ops.fake_quant_kv_append_codes_at(sites("at", None), AH, state["at"]["rejected"], pos) is not None
        else:
            assert ops.fake_quant_kv_append_at(sites("at", None), AH, pos) is not None

    graph = captured(dev, launch_at)
    state["at"]["rejected"].zero_()
    for offset in OFFSETS:
        for run in state:
            reset(run)
        pos.fill_(offset)
        graph.replay()
        if coded:
            assert ops.fake_quant_kv_append_codes(sites("static", offset), AH, state["static"]["rejected"]) is not None
        else:
            assert ops.fake_quant_kv_append(sites("static", offset), AH) is not None
        a, s = state["at"], state["static"]
        assert same_f32(a["yq"].cpu().numpy(), s["yq"].cpu().numpy()), offset
        for ya, ys in zip(a["ys"], s["ys"]):
            assert np.array_equal(_bytes(ya), _bytes(ys)), offset                  # the WHOLE buffers, sentinel included
        assert not bool((a["ys"][0][:, :, offset] == (SENTINEL_B if coded else SENTINEL_F)).all())       # the step was written
        for ra, rs in zip(a["records"], s["records"]):
            if ra is not None:
                assert np.array_equal(_bytes(ra[0]), _bytes(rs[0])) and np.array_equal(_bytes(ra[1]), _bytes(rs[1]))
                assert not bool(torch.isnan(ra[0]).any())
        assert int(a["rejected"].item()) == int(s["rejected"].item()) == 0
    # a position that does not fit: nothing is written anywhere, a coded cache counts it once
    reset("at")
    before = [t.clone() for t in [state["at"]["yq"]] + state["at"]["ys"]]
    pos.fill_(CAP)
    graph.replay()
    for t, b in zip([state["at"]["yq"]] + state["at"]["ys"], before):
        assert np.array_equal(_bytes(t), _bytes(b))
    for rec in state["at"]["records"]:
        if rec is not None:
            assert bool(torch.isnan(rec[0]).all() and torch.isnan(rec[1]).all())
    assert int(state["at"]["rejected"].item()) == (1 if coded else 0)
    if moved:                       # a prefix longer than its source (9 positions) is refused as well
        pos.fill_(SRC_CAP + 1)
        graph.replay()
        for t, b in zip([state["at"]["yq"]] + state["at"]["ys"], before):
            assert np.array_equal(_bytes(t), _bytes(b))
        assert int(state["at"]["rejected"].item()) == (2 if coded else 0)

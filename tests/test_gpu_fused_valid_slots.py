"""The one-launch step (csrc/fused_step.h) with the number of VALID tokens at every boundary of its phase A1: a streaming
wave holds S slots (9 at 768 features, 6 at 1024, 1 at 3072 / 4096), its valid slots are a prefix of them, and what it
does depends on their count -- it enters the chain of loads, and then the chain of reductions, at its highest valid slot
and falls through to slot 0, then publishes the extrema in one masked store pair, those of the tokens beyond the slots included.  With W = 16 G tokens per slot (G streaming
workgroups = the device's CUs - 2: the library launches one workgroup per CU, two of them select) the valid count V walks
over every multiple of W, one below and one above, so that the boundary falls inside a workgroup and exactly at its edge.

Reference: the three-launch path (ops.set_tuning("fused_step", 0)), which tests/test_gpu_fused_step.py pins to the oracle.
Equality is bit for bit (NaN = NaN) on y, scale, zero_point, min_val and max_val."""
import ctypes
from types import SimpleNamespace as NS

import pytest
import torch

pytestmark = pytest.mark.gpu

T = 128


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from outlier_suppression_amd import _hip
    _hip.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def W(dev):
    return 16 * (torch.cuda.get_device_properties(dev).multi_processor_count - 2)


def make(dev, percentile=0.95):
    from outlier_suppression_amd.quantization import Quantizer
    q = Quantizer(None, NS(quantizer="LSQPlusFakeQuantize", observer="AvgPruneMinMaxObserver", bit=6, symmetric=False, ch_axis=-1)).to(dev)
    q.observer.set_name("encoder.layer.0.output.LayerNorm.layernorm_post_act_fake_quantize.observer")
    q.observer.set_percentile(percentile)
    q.enable_observer()
    q.enable_fake_quant()
    return q


def fused_status(dev):
    from outlier_suppression_amd import _hip
    st = ctypes.c_int(-1)
    _hip.check(_hip.load().osq_fused_step_status(_hip.ptr(_hip.workspace(dev)), ctypes.byref(st), _hip.stream_ptr(dev)), "status")
    return st.value


def lengths_for(V, B, dev):
    """V valid tokens: full samples, one partial sample, empty ones."""
    L = torch.zeros(B, dtype=torch.long)
    L[:V // T] = T
    if V % T:
        L[V // T] = V % T
    assert int(L.sum()) == V
    return L.to(dev)


def bits(t):
    """int32 words of an fp32 tensor, every NaN the same word: -0.0 differs from +0.0, NaN equals NaN."""
    t = t.detach().to(torch.float32).contiguous()
    return torch.where(torch.isnan(t), torch.full_like(t, float("nan")), t).view(torch.int32)


def run(dev, xs, L, fused):
    """Fresh module, one call per batch; with fused = 1 the last call must have been the one-launch kernel (its dispatch
    events recorded), or the comparison would be of the three-launch path with itself."""
    from outlier_suppression_amd import _hip, ops
    lib = _hip.load()
    ops.set_tuning("fused_step", fused)
    try:
        q = make(dev)
        a, b = ctypes.c_void_p(), ctypes.c_void_p()
        _hip.check(lib.osq_timing_events_create(ctypes.byref(a), ctypes.byref(b)), "events")
        with torch.no_grad():
            ys = [q(x, L, 1) for x in xs[:-1]]
            lib.osq_time_next_launch(_hip.TIME_FUSED_STEP, a, b)
            ys.append(q(xs[-1], L, 1))
        torch.cuda.synchronize()
        us = ctypes.c_float()
        seen = lib.osq_timing_elapsed_us(a, b, ctypes.byref(us)) == 0
        lib.osq_time_next_launch(0, None, None)
        lib.osq_timing_events_destroy(a, b)
        assert seen == bool(fused), "one launch expected" if fused else "three launches expected"
    finally:
        ops.set_tuning("fused_step", 1)
    return ys, q.scale, q.zero_point, q.observer.min_val, q.observer.max_val


def check(dev, xs, L, what):
    one, three = run(dev, xs, L, 1), run(dev, xs, L, 0)
    for name, a, b in zip(("scale", "zero_point", "min_val", "max_val"), one[1:], three[1:]):
        assert torch.equal(bits(a), bits(b)), (what, name, a, b)
    for i, (a, b) in enumerate(zip(one[0], three[0])):
        assert torch.equal(bits(a), bits(b)), (what, "y", i)
    assert fused_status(dev) == 0, what


@pytest.fixture(scope="module")
def data(dev):
    """data(B, H): two batches of [B, T, H] with an outlier channel, made once per shape and dropped with the module."""
    cache = {}

    def get(B, H):
        if (B, H) not in cache:
            gd = torch.Generator(device=dev).manual_seed(B + H)
            xs = [torch.randn(B, T, H, device=dev, generator=gd) * (1.0 + 0.5 * i) for i in range(2)]
            for x in xs:
                x[..., 5] *= 20
            cache[(B, H)] = xs
        return cache[(B, H)]
    yield get
    cache.clear()


def sweep_batch(W, slots):
    """Samples of T tokens that hold slots * W + 1 tokens."""
    return (slots * W + 1 + T - 1) // T


def sweep_counts(W, slots, total):
    return {"0": 0, "1": 1, "W-1": W - 1, "W": W, "W+1": W + 1, "BT": total,
            **{f"{m}W{'+' if d > 0 else '-'}1": m * W + d for m in range(2, slots + 1) for d in (-1, 1)}}


SWEEP_768 = ["0", "1", "W-1", "W", "W+1", "BT"] + [f"{m}W{s}1" for m in range(2, 9) for s in "-+"]
SWEEP_1024 = ["0", "1", "W-1", "W", "W+1", "BT"] + [f"{m}W{s}1" for m in range(2, 7) for s in "-+"]


@pytest.mark.parametrize("v", SWEEP_768)
def test_slot_boundaries_768(v, dev, W, data):
    """Nine slots per wave: with 8 W + 1 tokens or more, V = m W - 1, m W + 1 (and W itself) gives some waves m valid slots
    and the others m - 1 -- every count from 0 to 9 --, the last valid token being the last wave of the last workgroup
    (m W - 1: one short of a full slot), the first wave of the first workgroup of the next slot (m W + 1) or the slot's edge (W)."""
    B = sweep_batch(W, 8)
    V = sweep_counts(W, 8, B * T)[v]
    check(dev, data(B, 768), lengths_for(V, B, dev), (v, V))


@pytest.mark.parametrize("v", SWEEP_1024)
def test_slot_boundaries_1024(v, dev, W, data):
    """Six slots per wave (four in registers, two in LDS); the same tensor size as the 768 sweep, so with every token valid
    each wave also reduces tokens beyond its slots."""
    B = sweep_batch(W, 8)
    V = sweep_counts(W, 6, B * T)[v]
    check(dev, data(B, 1024), lengths_for(V, B, dev), (v, V))


@pytest.mark.parametrize("H", [3072, 4096])
@pytest.mark.parametrize("v", ["BT", "W", "W+1", "W+64", "W+65"])
def test_overflow_tokens(v, H, dev, W, data):
    """One slot per wave at 3072 and 4096 features: the valid tokens from W on are reduced by the loop behind the slots, whose
    results also leave in one masked store pair per wave."""
    B = 33
    V = min(B * T, {"BT": B * T, "W": W, "W+1": W + 1, "W+64": W + 64, "W+65": W + 65}[v])
    check(dev, data(B, H), lengths_for(V, B, dev), (v, H, V))


def valid_rows(L):
    """Row b * T + t of the j-th valid token of the kernel's enumeration (valid tokens first, sample-major)."""
    mask = torch.arange(T, device=L.device)[None, :] < L[:, None]
    return mask.flatten().nonzero().flatten()


SPECIALS = {"nan": float("nan"), "-0": -0.0, "+inf": float("inf"), "-inf": float("-inf")}


def plant(x, row, value):
    """A copy of x with `value` in token `row`; for -0.0 the token is made non-negative, so that the zero IS its minimum."""
    x = x.clone()
    tok = x.view(-1, x.shape[-1])[row]
    if value == 0.0:
        tok.abs_()
    tok[77] = value
    return x


@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("value", list(SPECIALS))
def test_special_values_in_the_slots_of_one_wave(value, where, dev, W, data):
    """Wave 5 of streaming workgroup 7 owns tokens k W + 5 G + 7; with V = 5 W + 5 G + 8 it has six valid slots and the last
    valid token of the tensor.  The special value sits in its slot 0, 3 or 5."""
    G = W // 16
    B = sweep_batch(W, 8)
    gwi = 5 * G + 7
    V = 5 * W + gwi + 1
    L = lengths_for(V, B, dev)
    j = {"first": 0, "middle": 3, "last": 5}[where] * W + gwi
    row = int(valid_rows(L)[j])
    xs = data(B, 768)
    check(dev, [plant(xs[0], row, SPECIALS[value]), xs[1]], L, (value, where))


@pytest.mark.parametrize("where", ["first", "last"])
@pytest.mark.parametrize("value", list(SPECIALS))
def test_special_values_in_overflow_tokens(value, where, dev, W, data):
    """[33,128,3072], every token valid: valid tokens W .. B T - 1 go through the loop behind the slots."""
    B = 33
    L = lengths_for(B * T, B, dev)
    row = min(W, B * T - 1) if where == "first" else B * T - 1          # every token valid: token j is row j
    xs = data(B, 3072)
    check(dev, [plant(xs[0], row, SPECIALS[value]), xs[1]], L, (value, where))


def test_graph_replay_of_three_steps(dev, W, data):
    """Three steps captured as one graph and replayed once, behind three eager ones, equal six eager steps (V = 3 W + 1:
    four valid slots in one wave, three in the others)."""
    B = sweep_batch(W, 8)
    xs = data(B, 768)
    xs = [xs[0], xs[1], xs[0]]
    L = lengths_for(3 * W + 1, B, dev)
    with torch.no_grad():
        q = make(dev)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for x in xs:
                q(x, L, 1)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            ys = [q(x, L, 1) for x in xs]
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
    eager = run(dev, xs + xs, L, 1)
    for name, a, b in zip(("scale", "zero_point", "min_val", "max_val"), (q.scale, q.zero_point, q.observer.min_val, q.observer.max_val), eager[1:]):
        assert torch.equal(bits(a), bits(b)), (name, a, b)
    for i, (a, b) in enumerate(zip(ys, eager[0][3:])):
        assert torch.equal(bits(a), bits(b)), i
    assert fused_status(dev) == 0

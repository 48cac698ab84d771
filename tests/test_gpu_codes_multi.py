"""osq_dequantize_codes_multi at every table shape: the bisection of the running row counts in LDS (up to kMultiLdsWeights =
1024 entries) and out of global memory (beyond), mixed code widths, per-tensor and per-channel entries, rows one float4
either side of an unrolled trip (kUnroll 4 x 64 lanes x 4 elements = 1024), entries without rows, and more rows than the
launch has waves (its grid is capped at kMaxBlocks * 4 = 8192 workgroups of 4 waves).  Every y equals
osq_dequantize_codes on that entry alone and the oracle's dequantisation, word for word; nothing else is written."""
import numpy as np
import pytest
import torch

import _codes as C
from oracle import fake_quant_oracle as FQ

pytestmark = pytest.mark.gpu

MULTI_WAVE_CAP = 2048 * 4 * 4
SENTINEL = 0x7FC0BEEF          # a NaN no dequantisation produces: words the launch must not write keep it


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from outlier_suppression_amd import _hip
    _hip.load()
    return torch.device("cuda:0")


def _tiny_entries(count, seed):
    """(rows, channels, inner, range, bits): 0..3 rows of 4..12 elements, both code widths, per-tensor and per-channel."""
    rng = np.random.default_rng(seed)
    es = []
    for k in range(count):
        rows = int(rng.integers(0, 4))
        rn, bits = (("a4", 4), ("s4", 4), ("a2", 4), ("a8", 8), ("s6", 8), ("a4", 8))[int(rng.integers(0, 6))]
        channels = rows if (rows and rng.integers(0, 2)) else 1
        es.append((rows, channels, int(rng.choice([4, 8, 12])), rn, bits))
    es[count // 2] = (0, 1, 8, "a4", 4)               # no rows in the middle ...
    es[-1] = (0, 1, 4, "a8", 8)                       # ... and at the end
    es[-2] = (3, 3, 12, "s4", 4)                      # the last entry WITH rows: the far end of the bisection
    return es


TABLES = {
    "1023-tiny": lambda: _tiny_entries(1023, 1),
    "1024-tiny": lambda: _tiny_entries(1024, 2),
    "1025-tiny": lambda: _tiny_entries(1025, 3),
    "trips": lambda: [(3, 3, 1020, "a8", 8), (2, 1, 1024, "a4", 4), (0, 1, 1024, "a8", 8), (3, 3, 1028, "s4", 4), (2, 1, 1020, "a2", 4),
                      (3, 1, 1028, "s6", 8), (6, 3, 1024, "s8", 8), (2, 2, 2052, "a4", 4), (1, 1, 4, "a4", 8), (0, 1, 4, "a4", 4)],
    "beyond-the-grid": lambda: [(12000, 1, 4, "a8", 8), (12001, 12001, 4, "a4", 4), (0, 1, 4, "a4", 4), (12000, 5, 8, "s4", 4)],
}


def build_table(name):
    rng = np.random.default_rng(list(TABLES).index(name) + 5)
    es, cur, y_off, p_off = [], 0, 0, 0
    codes, scales, zps, ref = [], [], [], []
    for rows, channels, inner, rn, bits in TABLES[name]():
        qmin, qmax = C.RANGES[rn]
        n = rows * inner
        u = rng.integers(0, qmax - qmin + 1, n).astype(np.uint8)
        if n >= 2:
            u[0], u[-1] = qmax - qmin, 0
        s = rng.uniform(1e-3, 30.0, channels).astype(np.float32)
        z = rng.integers(qmin, qmax + 1, channels).astype(np.float32)
        q = (u.astype(np.int32) + qmin).astype(np.float32).reshape(rows, inner)
        ch = np.arange(rows) % channels
        y = FQ.dequantize_affine(q, s[ch][:, None], z[ch][:, None]) if rows else np.zeros((0, inner), np.float32)
        packed = C.pack(u, bits)
        # codes of an entry start on a 4-byte boundary -- every other entry of four code bits two bytes past one, which is all
        # such an entry needs --, y on a 16-byte one with a gap of guard words after it
        codes_off = (cur + 3) // 4 * 4 + (2 if bits == 4 and len(es) % 2 else 0)
        cur = codes_off + packed.size
        es.append(dict(rows=rows, channels=channels, inner=inner, qmin=qmin, bits=bits, codes_off=codes_off, y_off=y_off, p_off=p_off,
                       nbytes=packed.size))
        codes.append((codes_off, packed))
        ref.append((y_off, y.reshape(-1)))
        scales.append(s)
        zps.append(z)
        y_off += (n + 3) // 4 * 4 + 4
        p_off += channels
    return es, codes, ref, np.concatenate(scales), np.concatenate(zps), cur + 8, y_off


@pytest.mark.parametrize("name", list(TABLES))
def test_dequantize_codes_multi_table(name, dev):
    from outlier_suppression_amd import _hip
    lib = _hip.load()
    es, codes, ref, scales, zps, codes_len, y_len = build_table(name)
    host_codes = np.zeros(codes_len, np.uint8)
    for off, packed in codes:
        host_codes[off:off + packed.size] = packed
    cb = torch.from_numpy(host_codes).to(dev)
    st, zt = torch.from_numpy(scales).to(dev), torch.from_numpy(zps).to(dev)
    y = torch.full((y_len,), SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)
    single = torch.full((y_len,), SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)
    descs = (_hip.CodesDesc * len(es))()
    row_end, total = [], 0
    for d, e in zip(descs, es):
        assert (cb.data_ptr() + e["codes_off"]) % (4 if e["bits"] == 8 else 2) == 0 and (y.data_ptr() + 4 * e["y_off"]) % 16 == 0
        d.codes, d.y = cb.data_ptr() + e["codes_off"], y.data_ptr() + 4 * e["y_off"]
        d.scale_eff, d.zp_eff = st.data_ptr() + 4 * e["p_off"], zt.data_ptr() + 4 * e["p_off"]
        d.rows, d.channels, d.inner, d.quant_min, d.code_bits = e["rows"], e["channels"], e["inner"], e["qmin"], e["bits"]
        total += e["rows"]
        row_end.append(total)
    if name == "beyond-the-grid":
        assert total > MULTI_WAVE_CAP
    table = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(dev)
    ends = torch.tensor(row_end, dtype=torch.int64, device=dev)
    before = cb.clone()
    _hip.check(lib.osq_dequantize_codes_multi(table.data_ptr(), ends.data_ptr(), len(es), total, _hip.stream_ptr(dev)), "dequantize_codes_multi")
    for e in es:                                        # the same entries one by one
        if e["rows"]:
            _hip.check(lib.osq_dequantize_codes(cb.data_ptr() + e["codes_off"], single.data_ptr() + 4 * e["y_off"], e["rows"] // e["channels"],
                                                e["channels"], e["inner"], st.data_ptr() + 4 * e["p_off"], zt.data_ptr() + 4 * e["p_off"],
                                                e["qmin"], e["bits"], _hip.stream_ptr(dev)), "dequantize_codes")
    torch.cuda.synchronize()
    got = y.view(torch.int32).cpu().numpy()
    want = np.full(y_len, SENTINEL, np.int32)
    for off, vals in ref:
        want[off:off + vals.size] = vals.view(np.int32)
    if not np.array_equal(got, want):
        k = int(np.nonzero(got != want)[0][0])
        entry = max(i for i, e in enumerate(es) if e["y_off"] <= k)
        raise AssertionError((name, "first wrong word", k, "entry", entry, es[entry], "wrong words", int((got != want).sum())))
    assert np.array_equal(single.view(torch.int32).cpu().numpy(), want), "the single-tensor entry point differs from the oracle"
    assert torch.equal(cb, before), "the codes were written"

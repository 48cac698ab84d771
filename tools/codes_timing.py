"""Time the integer-code kernels on the BERT-base weight table (77 tensors, 110 M parameters, per-channel symmetric):

    osq_fake_quant_weights_multi      the one-launch weight refresh, 8 B per element -- the yardstick
    osq_dequantize_codes_multi        at 8 and at 4 code bits, 5 and 4.5 B per element
    osq_quantize_codes                over the same tensors, one launch each (export is not one launch), 5 / 4.5 B per element

all in one process, interleaved, after a warm-up: median with min / max of REPS device-event timings each, bytes moved as
the algorithm needs them (computed from the shapes) and the rate they give.  The dequantised weights are compared with the
yardstick's output word for word before anything is timed.  Writes profiles/codes_timing.txt (--out).  Needs the GPU."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARMUP, REPS = 3, 15


def weight_shapes():
    """[rows, inner] of every weight-quantized operator of BERT-base (the model benchlib's quantized forward builds), in
    module order: Linear and Embedding weights."""
    from transformers import BertConfig, BertForSequenceClassification
    with torch.device("meta"):
        model = BertForSequenceClassification(BertConfig(num_labels=2))
    return [tuple(m.weight.shape) for m in model.modules() if isinstance(m, (torch.nn.Linear, torch.nn.Embedding))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "codes_timing.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("codes_timing: needs the GPU (a CPU run cannot give a time)")
    from outlier_suppression_amd import _hip, ops
    lib = _hip.load()
    dev = torch.device("cuda:0")
    st = _hip.stream_ptr(dev)
    shapes = weight_shapes()
    elems = sum(r * c for r, c in shapes)
    gen = torch.Generator(device=dev).manual_seed(0)
    xs = [torch.randn(s, device=dev, generator=gen) * 0.05 for s in shapes]
    total_rows = sum(r for r, _ in shapes)
    ends = torch.tensor([sum(r for r, _ in shapes[:i + 1]) for i in range(len(shapes))], dtype=torch.int64, device=dev)
    y_ref = torch.empty(elems, device=dev)
    y_out = torch.empty(elems, device=dev)

    def slices(flat, unit=1):
        out, off = [], 0
        for r, c in shapes:
            out.append(flat[off // unit:(off + r * c) // unit])
            off += r * c
        return out

    setups = {}
    for bits, (qmin, qmax) in ((8, (-128, 127)), (4, (-8, 7))):
        scales = [(x.abs().amax(dim=1) / qmax).clamp_min(1e-8).contiguous() for x in xs]
        zps = [torch.zeros(x.shape[0], dtype=torch.int32, device=dev) for x in xs]
        codes = torch.empty(elems * bits // 8, dtype=torch.uint8, device=dev)
        s_eff = [torch.empty_like(s) for s in scales]
        z_eff = [torch.empty_like(s) for s in scales]
        rejected = torch.zeros(1, dtype=torch.int32, device=dev)
        wd = (_hip.WeightDesc * len(xs))()
        cd = (_hip.CodesDesc * len(xs))()
        for i, (x, yr, yo, c) in enumerate(zip(xs, slices(y_ref), slices(y_out), slices(codes, 8 // bits))):
            w = wd[i]
            w.x, w.y, w.scale, w.zero_point = x.data_ptr(), yr.data_ptr(), scales[i].data_ptr(), zps[i].data_ptr()
            w.rows, w.channels, w.inner = x.shape[0], x.shape[0], x.shape[1]
            w.zp_type, w.mode, w.grad_factor, w.quant_min, w.quant_max = _hip.ZP_INT32, _hip.PARAM_FIXED, 1.0, qmin, qmax
            d = cd[i]
            d.codes, d.y, d.scale_eff, d.zp_eff = c.data_ptr(), yo.data_ptr(), s_eff[i].data_ptr(), z_eff[i].data_ptr()
            d.rows, d.channels, d.inner, d.quant_min, d.code_bits = x.shape[0], x.shape[0], x.shape[1], qmin, bits
        setups[bits] = dict(qmin=qmin, qmax=qmax, scales=scales, zps=zps, codes=codes, code_slices=slices(codes, 8 // bits), s_eff=s_eff,
                            z_eff=z_eff, rejected=rejected, keep=(wd, cd),
                            wtable=torch.frombuffer(bytearray(bytes(wd)), dtype=torch.uint8).to(dev),
                            ctable=torch.frombuffer(bytearray(bytes(cd)), dtype=torch.uint8).to(dev))

    def fake_quant_multi(bits):
        s = setups[bits]
        _hip.check(lib.osq_fake_quant_weights_multi(s["wtable"].data_ptr(), ends.data_ptr(), len(xs), total_rows, st), "weights_multi")

    def quantize(bits):
        s = setups[bits]
        for i, x in enumerate(xs):
            _hip.check(lib.osq_quantize_codes(_hip.DTYPE_F32, x.data_ptr(), s["code_slices"][i].data_ptr(), 1, x.shape[0], x.shape[1],
                                              s["scales"][i].data_ptr(), s["zps"][i].data_ptr(), _hip.ZP_INT32, _hip.PARAM_FIXED, 1.0,
                                              s["qmin"], s["qmax"], bits, s["s_eff"][i].data_ptr(), s["z_eff"][i].data_ptr(),
                                              s["rejected"].data_ptr(), st), "quantize_codes")

    def dequantize_multi(bits):
        s = setups[bits]
        _hip.check(lib.osq_dequantize_codes_multi(s["ctable"].data_ptr(), ends.data_ptr(), len(xs), total_rows, st), "dequantize_codes_multi")

    # results first: the codes carry the yardstick's output word for word
    for bits in (8, 4):
        fake_quant_multi(bits)
        quantize(bits)
        y_out.fill_(float("nan"))
        dequantize_multi(bits)
        torch.cuda.synchronize()
        assert int(setups[bits]["rejected"].item()) == 0
        assert torch.equal(y_out.view(torch.int32), y_ref.view(torch.int32)), f"dequantised weights differ from the fake-quant at {bits} bits"

    runs = [("osq_fake_quant_weights_multi (yardstick, 1 launch)", lambda: fake_quant_multi(8), 8.0),
            ("osq_dequantize_codes_multi, 8 code bits (1 launch)", lambda: dequantize_multi(8), 5.0),
            ("osq_dequantize_codes_multi, 4 code bits (1 launch)", lambda: dequantize_multi(4), 4.5),
            (f"osq_quantize_codes, 8 code bits ({len(xs)} launches)", lambda: quantize(8), 5.0),
            (f"osq_quantize_codes, 4 code bits ({len(xs)} launches)", lambda: quantize(4), 4.5)]
    times = {name: [] for name, _, _ in runs}
    for rep in range(WARMUP + REPS):
        for name, fn, _ in runs:                       # interleaved: every kind sees the same neighbours and the same drift
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            if rep >= WARMUP:
                times[name].append(a.elapsed_time(b) * 1e3)
    lines = [f"BERT-base weight table: {len(xs)} tensors, {total_rows} rows, {elems} elements; {torch.cuda.get_device_name(0)}",
             f"device-event time around the call(s), {REPS} repetitions after {WARMUP} warm-up rounds, kinds interleaved",
             "", f"{'kernel':58s} {'median us':>10s} {'min':>9s} {'max':>9s} {'MB moved':>9s} {'GB/s':>8s}  B/elem"]
    med = {}
    for name, _, per_elem in runs:
        t = sorted(times[name])
        med[name] = t[len(t) // 2]
        mb = per_elem * elems / 1e6
        lines.append(f"{name:58s} {med[name]:10.1f} {t[0]:9.1f} {t[-1]:9.1f} {mb:9.1f} {mb * 1e6 / med[name] / 1e3:8.0f}  {per_elem}")
    yard = med[runs[0][0]]
    lines += ["", "dequantise / yardstick time: " + ", ".join(f"{runs[i][0].split(',')[1].split('(')[0].strip()} {med[runs[i][0]] / yard:.3f}" for i in (1, 2))
              + "   (bytes: 0.625 and 0.5625)"]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()

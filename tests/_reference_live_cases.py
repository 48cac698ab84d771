"""The seeded random cases of tests/test_oracle_vs_reference_live.py, drawn in one place: the test runs the oracle on them,
tests/golden/make_golden_reference_live.py runs the REFERENCE on them and stores what it returned
(tests/golden/reference_live.npz).  CPU torch generators: the same draws on every machine."""
import numpy as np
import torch


def fake_quant_cases():
    """60 per-tensor cases (and a per-channel one wherever x has 2+ dims): shapes, bit widths, scales over five decades."""
    gen = torch.Generator().manual_seed(20260930)
    for trial in range(60):
        bit = int(torch.randint(2, 9, (1,), generator=gen))
        sym = bool(torch.randint(0, 2, (1,), generator=gen))
        qmin, qmax = (-(1 << (bit - 1)), (1 << (bit - 1)) - 1) if sym else (0, (1 << bit) - 1)
        shape = tuple(int(v) for v in torch.randint(1, 9, (int(torch.randint(1, 4, (1,), generator=gen)),), generator=gen))
        x = torch.randn(*shape, generator=gen) * float(10 ** torch.empty(1).uniform_(-3, 2, generator=gen))
        scale = float(torch.empty(1).uniform_(1e-4, 2.0, generator=gen))
        zp = 0 if sym else int(torch.randint(qmin, qmax + 1, (1,), generator=gen))
        case = dict(trial=trial, bit=bit, sym=sym, qmin=qmin, qmax=qmax, shape=shape, x=x, scale=scale, zp=zp)
        if x.dim() >= 2:
            C = x.shape[0]
            case["s"] = torch.empty(C).uniform_(1e-3, 1.0, generator=gen)
            case["z"] = torch.zeros(C, dtype=torch.int32) if sym else torch.randint(qmin, qmax + 1, (C,), generator=gen).int()
        yield case


OBSERVERS = ("MinMaxObserver", "AvgMinMaxObserver", "AvgPruneMinMaxObserver")


def observer_cases():
    """45 observers, three batches each: layouts, masks, percentiles, one-sided ranges."""
    gen = torch.Generator().manual_seed(77001)
    for trial in range(45):
        cls_name = OBSERVERS[trial % 3]
        bit = int(torch.randint(3, 9, (1,), generator=gen))
        sym = bool(torch.randint(0, 2, (1,), generator=gen))
        B, T, H = (int(torch.randint(lo, hi, (1,), generator=gen)) for lo, hi in ((1, 7), (2, 12), (2, 10)))
        layout = trial % 4
        name = "m.attention_probs_x" if trial % 9 == 8 else "m.x_post_act_fake_quantize"
        pct = float(torch.empty(1).uniform_(0.05, 1.0, generator=gen))
        batches = []
        for it in range(3):
            shift = float(torch.empty(1).uniform_(-3, 3, generator=gen)) if trial % 5 == 0 else 0.0
            if layout == 0:
                x, sp = torch.randn(B, T, H, generator=gen) + shift, 1
            elif layout == 1:
                x, sp = torch.randn(B, 2, T, H, generator=gen) + shift, 2
            elif layout == 2:
                x, sp = (torch.randn(B, T, 2, H, generator=gen) + shift).permute(0, 2, 3, 1), 3
            else:
                x, sp = torch.randn(B, T, H, generator=gen).abs() + 0.1, 1       # one-sided range
            L = torch.randint(1, T + 1, (B,), generator=gen)
            batches.append((x, L, sp))
        yield dict(trial=trial, cls_name=cls_name, bit=bit, sym=sym, name=name, pct=pct, batches=batches,
                   masked=trial % 7 != 6)


def lsqplus_cases():
    """40 LSQ+ forward / backward cases."""
    from oracle import fake_quant_oracle as FQ
    gen = torch.Generator().manual_seed(424242)
    for trial in range(40):
        bit = int(torch.randint(3, 9, (1,), generator=gen))
        qmin, qmax = 0, (1 << bit) - 1
        shape = (int(torch.randint(1, 6, (1,), generator=gen)), int(torch.randint(1, 40, (1,), generator=gen)))
        x = torch.randn(*shape, generator=gen) * 2
        scale = torch.empty(1).uniform_(0.01, 0.5, generator=gen)
        zp = torch.empty(1).uniform_(qmin, qmax, generator=gen)
        g = float(FQ.lsqplus_grad_factor(x.numel(), qmax))
        gy = torch.randn(*shape, generator=gen)
        yield dict(trial=trial, qmin=qmin, qmax=qmax, x=x, scale=scale, zp=zp, g=g, gy=gy)


def msefast_cases():
    """MSEFast per-channel weights, per-tensor averaged activations, and four one-sided batches per (class, side)."""
    gen = torch.Generator().manual_seed(77)
    weights = [(cols, bit, torch.randn(24, cols, generator=gen) * 0.05) for cols, bit in ((768, 4), (3072, 4), (96, 6))]
    acts = []
    for sym, shape in ((True, (4, 16, 32)), (False, (4, 16, 32)), (False, (2, 8, 64))):
        x = torch.randn(*shape, generator=gen)
        x[..., 1] *= 9.0
        acts.append((sym, shape, x))
    one_sided = []
    for avg in (False, True):
        for side in ("pos", "neg"):
            xs = []
            for it in range(4):
                x = torch.randn(3, 7, 16, generator=gen).abs() * (1.0 + 0.3 * it) + 1e-3
                xs.append(x if side == "pos" else -x)
            one_sided.append((avg, side, xs))
    return weights, acts, one_sided


MIXED_DTYPES = ((np.float32, np.float64), (np.float64, np.float32), (np.float32, np.float32), (np.float64, np.float64))


def mixed_dtype_cases():
    """(symmetric, k, min_val, max_val): 2 x 2000 statistics of every float32 / float64 combination."""
    rng = np.random.default_rng(0)
    for sym in (False, True):
        for k in range(2000):
            dts = MIXED_DTYPES[k % 4]
            yield sym, k, dts[0](-rng.random() * 2), dts[1](rng.random() * 3)

"""CPU-only: the host checks of the two whole-sequence attention entry points (osq_attention_fake_quant,
osq_attention_fake_quant_int; csrc/attention_seq.h) -- every class of refusal, the outcome and the text of osq_last_error(),
and which refusal wins where two apply.  Every call returns before a launch: the pointers are dummy integers, and no case has
wholly valid, non-empty arguments."""
import pytest

OK, INVALID, UNSUPPORTED = 0, -1, -3
P = 0x1000                                     # an aligned, non-null "pointer"
NONE = (None, None, 0, 0, 1.0, 0, 1)           # no quantizer: scale, zero_point, zp_type, mode, grad_factor, quant_min, quant_max
Q8 = (P, P, 0, 0, 1.0, 0, 255)                 # a per-tensor quantizer of 256 codes


def _group(**kw):
    g = dict(zip(("scale", "zero_point", "zp_type", "mode", "grad_factor", "quant_min", "quant_max"), Q8))
    g.update(kw)
    return tuple(g.values())


# wholly valid arguments of a [2, 2, 4, 16] q over 8 keys; never passed as they are
BASE = dict(q=P, k=P, v=P, mask=None, out=P, probs_out=None, batch=2, heads=2, tokens=4, kv_len=8, head_dim=16,
            q_strides=(128, 64, 16), k_strides=(256, 128, 16), v_strides=(256, 128, 16), mask_strides=(0, 0, 0),
            alpha=1.0, divisor=1.0, q_quant=Q8, k_quant=Q8, v_quant=Q8, probs_quant=Q8, ctx_quant=NONE)

FP32, INT = "attention_fake_quant", "attention_fake_quant_int"
BOTH = (FP32, INT)

# (forms, the arguments that differ from BASE, return code, message after the entry's prefix -- None: no error was recorded)
CASES = [
    (BOTH, dict(batch=-1), INVALID, "bad shape"),
    (BOTH, dict(heads=-1), INVALID, "bad shape"),
    (BOTH, dict(tokens=2 ** 31), INVALID, "bad shape"),
    (BOTH, dict(head_dim=0), INVALID, "bad shape"),
    (BOTH, dict(q_strides=(128, -64, 16)), INVALID, "negative stride"),
    (BOTH, dict(k_strides=(-256, 128, 16)), INVALID, "negative stride"),
    (BOTH, dict(v_strides=(256, 128, -16)), INVALID, "negative stride"),
    (BOTH, dict(mask=P, mask_strides=(8, 0, -8)), INVALID, "negative mask stride"),
    (BOTH, dict(mask_strides=(0, -4, 0), tokens=0), OK, None),                  # without a mask its strides are not read
    (BOTH, dict(alpha=0.125, divisor=8.0), INVALID, "give alpha or divisor, not both"),
    ((FP32,), dict(probs_quant=_group(zero_point=None)), INVALID, "probs scale without zero_point"),
    (BOTH, dict(ctx_quant=_group(zero_point=None)), INVALID, "ctx scale without zero_point"),
    ((FP32,), dict(probs_quant=_group(mode=3)), INVALID, "bad probs mode"),
    ((FP32,), dict(probs_quant=_group(mode=64)), INVALID, "bad probs mode"),
    (BOTH, dict(ctx_quant=_group(mode=3)), INVALID, "bad ctx mode"),
    (BOTH, dict(ctx_quant=_group(mode=16 | 64)), INVALID, "bad ctx mode"),
    (BOTH, dict(head_dim=24), UNSUPPORTED, None),
    (BOTH, dict(head_dim=256), UNSUPPORTED, None),
    (BOTH, dict(kv_len=0), UNSUPPORTED, None),
    ((FP32,), dict(kv_len=1025), UNSUPPORTED, None),
    ((INT,), dict(kv_len=16385), UNSUPPORTED, None),
    (BOTH, dict(q_strides=(128, 64, 18)), UNSUPPORTED, None),
    (BOTH, dict(k_strides=(258, 128, 16)), UNSUPPORTED, None),
    (BOTH, dict(v_strides=(256, 129, 16)), UNSUPPORTED, None),
    (BOTH, dict(batch=65536, heads=65536), INVALID, "bad shape"),               # batch * heads * tiles over INT32_MAX
    (BOTH, dict(batch=2 ** 31), INVALID, "bad shape"),
    (BOTH, dict(batch=2 ** 20, heads=2 ** 9, tokens=4097), INVALID, "bad shape"),   # 2**29 (b, head) pairs of 129 / 33 tiles
    (BOTH, dict(tokens=0), OK, None),
    (BOTH, dict(batch=0), OK, None),
    (BOTH, dict(heads=0, q=None, out=None), OK, None),
    (BOTH, dict(q=None), INVALID, "null tensor"),
    (BOTH, dict(v=None), INVALID, "null tensor"),
    (BOTH, dict(out=None), INVALID, "null tensor"),
    (BOTH, dict(q=P + 4), UNSUPPORTED, None),
    (BOTH, dict(k=P + 8), UNSUPPORTED, None),
    (BOTH, dict(out=P + 4), UNSUPPORTED, None),
    (BOTH, dict(mask=P + 2), UNSUPPORTED, None),
    (BOTH, dict(probs_out=P + 2), UNSUPPORTED, None),
    # the integer form: its four product quantizers are required, per-tensor records of at most 256 codes
    ((INT,), dict(q_quant=NONE), UNSUPPORTED, None),
    ((INT,), dict(k_quant=NONE), UNSUPPORTED, None),
    ((INT,), dict(v_quant=NONE), UNSUPPORTED, None),
    ((INT,), dict(probs_quant=NONE), UNSUPPORTED, None),
    ((INT,), dict(k_quant=_group(zero_point=None)), UNSUPPORTED, None),
    ((INT,), dict(v_quant=_group(mode=3)), UNSUPPORTED, None),
    ((INT,), dict(q_quant=_group(quant_max=256)), UNSUPPORTED, None),
    ((INT,), dict(probs_quant=_group(quant_min=-128, quant_max=128)), UNSUPPORTED, None),
    ((INT,), dict(v_quant=_group(quant_min=1, quant_max=0)), UNSUPPORTED, None),
    # two refusals at once: the earlier check wins
    (BOTH, dict(batch=-1, q_strides=(-128, 64, 16)), INVALID, "bad shape"),
    (BOTH, dict(q_strides=(-128, 64, 16), mask=P, mask_strides=(-8, 0, 0)), INVALID, "negative stride"),
    (BOTH, dict(mask=P, mask_strides=(-8, 0, 0), alpha=0.5, divisor=2.0), INVALID, "negative mask stride"),
    (BOTH, dict(alpha=0.5, divisor=2.0, ctx_quant=_group(zero_point=None)), INVALID, "give alpha or divisor, not both"),
    ((FP32,), dict(probs_quant=_group(mode=3), ctx_quant=_group(zero_point=None)), INVALID, "ctx scale without zero_point"),
    ((FP32,), dict(probs_quant=_group(zero_point=None, mode=3), ctx_quant=_group(mode=3)), INVALID, "probs scale without zero_point"),
    ((FP32,), dict(probs_quant=_group(mode=3), ctx_quant=_group(mode=3)), INVALID, "bad probs mode"),
    (BOTH, dict(ctx_quant=_group(mode=3), head_dim=24), INVALID, "bad ctx mode"),
    ((INT,), dict(q_quant=NONE, ctx_quant=_group(mode=3)), INVALID, "bad ctx mode"),
    ((INT,), dict(q_quant=NONE, alpha=0.5, divisor=2.0), INVALID, "give alpha or divisor, not both"),
    ((INT,), dict(q_quant=_group(quant_max=256), batch=65536, heads=65536), UNSUPPORTED, None),
    (BOTH, dict(head_dim=24, q=None), UNSUPPORTED, None),
    (BOTH, dict(kv_len=0, batch=65536, heads=65536), UNSUPPORTED, None),
    (BOTH, dict(q_strides=(130, 64, 16), batch=65536, heads=65536), UNSUPPORTED, None),
    (BOTH, dict(batch=65536, heads=65536, tokens=0), INVALID, "bad shape"),     # the grid bound is asked before the empty case
    (BOTH, dict(batch=65536, heads=65536, q=None), INVALID, "bad shape"),
    (BOTH, dict(tokens=0, q=None, k=P + 4), OK, None),                          # an empty call reads no pointer
    (BOTH, dict(tokens=0, head_dim=24), UNSUPPORTED, None),
    (BOTH, dict(q=None, k=P + 4), INVALID, "null tensor"),
    (BOTH, dict(q=P + 4, mask=P + 2), UNSUPPORTED, None),
]


def _call(lib, form, changes):
    a = dict(BASE, **changes)
    groups = [a["probs_quant"], a["ctx_quant"]] if form == FP32 else [a[x + "_quant"] for x in ("q", "k", "v", "probs", "ctx")]
    return getattr(lib, "osq_" + form)(a["q"], a["k"], a["v"], a["mask"], a["out"], a["probs_out"], a["batch"], a["heads"],
                                       a["tokens"], a["kv_len"], a["head_dim"], *a["q_strides"], *a["k_strides"],
                                       *a["v_strides"], *a["mask_strides"], a["alpha"], a["divisor"],
                                       *[x for g in groups for x in g], None)


@pytest.mark.parametrize("form", BOTH)
def test_every_refusal_of_the_shared_launch_check(form):
    from outlier_suppression_amd import _hip
    lib = _hip.load()
    ran = 0
    for forms, changes, rc, message in CASES:
        if form not in forms:
            continue
        assert changes and (rc != OK or not all(dict(BASE, **changes)[x] for x in ("batch", "heads", "tokens"))), changes
        assert lib.osq_set_tuning(b"no_such_key", 1) == INVALID            # a known text: a call that records none leaves it
        got = _call(lib, form, changes)
        text = lib.osq_last_error().decode()
        print(form, changes, got, text)
        assert got == rc, (form, changes, text)
        if message is None:
            assert "unknown key" in text, (form, changes, text)
        else:
            assert text == f"{form}: {message}", (form, changes)
        ran += 1
    assert ran > 50

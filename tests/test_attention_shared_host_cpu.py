"""CPU-only: the host checks of the two SHARED whole-sequence attention entry points (osq_attention_fake_quant_shared,
osq_attention_fake_quant_int_shared; csrc/attention_seq.h) -- what `group` adds to the refusals of the unshared entry points
(tests/test_attention_host_checks.py, whose table and dummy arguments are reused here), and that with group = 1 every case of
that table is refused with the code and the text of the unshared entry point.  Every call returns before a launch."""
import pytest

import test_attention_host_checks as HC
from test_attention_host_checks import BASE, BOTH, FP32, INVALID, OK, UNSUPPORTED

TILE_Q = {FP32: 32, HC.INT: 128}             # kBlkTQ / kIntTQ: the query rows of a workgroup

# (the arguments that differ from BASE, group, return code, message after the entry's prefix -- None: no error was recorded)
GROUP_CASES = [
    (dict(), 0, INVALID, "bad shape"),
    (dict(), -1, INVALID, "bad shape"),
    (dict(tokens=0), 0, INVALID, "bad shape"),                                   # before the empty call
    (dict(batch=2 ** 16), 2 ** 15, INVALID, "bad shape"),                        # batch * group = 2**31
    (dict(batch=2 ** 16, tokens=0), 2 ** 15, INVALID, "bad shape"),
    (dict(batch=1, tokens=2 ** 16), 2 ** 15, INVALID, "bad shape"),              # group * tokens = 2**31
    (dict(batch=0, tokens=1), 2 ** 31, INVALID, "bad shape"),
    (dict(batch=1, tokens=2), 2 ** 62, INVALID, "bad shape"),                    # a product that wraps in 64 bits is refused too
    (dict(tokens=0), 3, OK, None),
    (dict(tokens=0, q=None, k=HC.P + 4), 3, OK, None),                           # an empty call reads no pointer
    (dict(head_dim=24), 3, UNSUPPORTED, None),
    (dict(head_dim=24, tokens=0), 3, UNSUPPORTED, None),
    (dict(kv_len=0), 3, UNSUPPORTED, None),
    (dict(q=None), 3, INVALID, "null tensor"),
    (dict(q=HC.P + 4), 3, UNSUPPORTED, None),
    # the earlier check wins, as in the unshared table
    (dict(q_strides=(-128, 64, 16)), 0, INVALID, "bad shape"),
    (dict(q_strides=(-128, 64, 16)), 3, INVALID, "negative stride"),
    (dict(head_dim=24, batch=2 ** 16), 2 ** 15, UNSUPPORTED, None),              # the batch * group bound sits with the grid bound
    (dict(head_dim=24, batch=1, tokens=2 ** 16), 2 ** 15, INVALID, "bad shape"),     # the group * tokens bound with tokens'
]


def _call(lib, form, changes, group):
    a = dict(BASE, **changes)
    groups = [a["probs_quant"], a["ctx_quant"]] if form == FP32 else [a[x + "_quant"] for x in ("q", "k", "v", "probs", "ctx")]
    return getattr(lib, f"osq_{form}_shared")(a["q"], a["k"], a["v"], a["mask"], a["out"], a["probs_out"], a["batch"], group,
                                             a["heads"], a["tokens"], a["kv_len"], a["head_dim"], *a["q_strides"],
                                             *a["k_strides"], *a["v_strides"], *a["mask_strides"], a["alpha"], a["divisor"],
                                             *[x for g in groups for x in g], None)


def _outcome(lib, call):
    """(return code, text of osq_last_error() -- None when the call recorded none)."""
    assert lib.osq_set_tuning(b"no_such_key", 1) == INVALID                # a known text: a call that records none leaves it
    got = call()
    text = lib.osq_last_error().decode()
    return got, None if "unknown key" in text else text


@pytest.fixture(scope="module")
def lib():
    from outlier_suppression_amd import _hip
    return _hip.load()


@pytest.mark.parametrize("form", BOTH)
def test_what_group_adds_to_the_refusals(lib, form):
    for changes, group, rc, message in GROUP_CASES:
        assert rc != OK or not all(dict(BASE, **changes)[x] for x in ("batch", "heads", "tokens")), changes     # nothing launches
        got, text = _outcome(lib, lambda: _call(lib, form, changes, group))
        print(form, changes, group, got, text)
        assert got == rc, (form, changes, group, text)
        assert text == (None if message is None else f"{form}: {message}"), (form, changes, group)


@pytest.mark.parametrize("form", BOTH)
def test_a_grid_over_int32_that_group_alone_causes(lib, form):
    """batch * heads * tiles: 2**20 * 2**9 (b, head) pairs take three tiles at most without a group; the group that brings a
    fifth tile brings the grid over INT32_MAX.  The last group under the bound passes that check (and is then refused for
    its null q, the next check but one)."""
    tq = TILE_Q[form]
    shape = dict(batch=2 ** 20, heads=2 ** 9, tokens=tq)
    for group, rc, message in ((1, INVALID, "null tensor"), (3, INVALID, "null tensor"), (4, INVALID, "bad shape"),
                               (5, INVALID, "bad shape")):
        # 2**29 pairs: 1, 3 tiles fit (3 * 2**29 < 2**31 - 1), 4 tiles are 2**31
        got, text = _outcome(lib, lambda: _call(lib, form, dict(shape, q=None), group))
        assert (got, text) == (rc, f"{form}: {message}"), (form, group, got, text)
    # the tiles are those of group * tokens rows, not group times those of tokens: 4 groups of a quarter tile are one tile
    got, text = _outcome(lib, lambda: _call(lib, form, dict(shape, tokens=tq // 4, q=None), 4))
    assert (got, text) == (INVALID, f"{form}: null tensor"), (form, got, text)
    got, text = _outcome(lib, lambda: _call(lib, form, dict(shape, tokens=tq // 4 + 1, q=None), 12))       # 3 tiles + 12 rows
    assert (got, text) == (INVALID, f"{form}: bad shape"), (form, got, text)


@pytest.mark.parametrize("form", BOTH)
def test_group_one_is_the_unshared_entry_point(lib, form):
    ran = 0
    for forms, changes, rc, message in HC.CASES:
        if form not in forms:
            continue
        want = _outcome(lib, lambda: HC._call(lib, form, changes))
        got = _outcome(lib, lambda: _call(lib, form, changes, 1))
        assert got == want, (form, changes, got, want)
        assert want == (rc, None if message is None else f"{form}: {message}"), (form, changes, want)      # the table's own
        ran += 1
    assert ran > 50


def test_the_header_and_the_host_name_both_entry_points():
    import os
    from outlier_suppression_amd import _hip
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "osq_hip.h")).read()
    for name in ("osq_attention_fake_quant_shared", "osq_attention_fake_quant_int_shared"):
        assert name in header.split("#define OSQ_ABI_VERSION")[0], f"{name} missing from the 'Added within 10' list"
        assert f"int {name}(" in header
        unshared = _hip.SIGNATURES[name[:-len("_shared")]][1]
        assert _hip.SIGNATURES[name][1] == unshared[:7] + [unshared[6]] + unshared[7:]          # an int64 after batch

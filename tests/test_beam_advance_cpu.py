"""CPU: what advancing the beams (csrc/beam_advance.hip, ops.beam_advance, generate(beam_advance=True)) needs where no GPU is
involved: the numpy restatement of tests/_beam_advance.py against the torch lines it restates
(generation._advance_beams_torch, on CPU tensors, whose division by the scalar is the correctly rounded one); the entry point in
the header's list and in ``_hip.SIGNATURES``; the switch and its environment variable; and generate(beam_advance=True) on CPU
tensors: the tokens of the torch lines, and a reason.

What is compared with the torch lines: the sentinel entries tie (x - 1e9 rounds to -1e9 for |x| < 32, and scores starts at
-1e9) and torch.topk's choice among ties is unspecified, so running, running_scores, beam_idx, improvable, go_on, scores and
done are compared word for word, finished and finished_len only in the slots where done_out is true.
The kernel runs on the GPU (tests/test_gpu_beam_advance.py, tests/test_gpu_beam_advance_model.py)."""
import itertools
import os
import re

import numpy as np
import pytest
import torch

import _beam_advance as BA

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BSZ, L, VOCAB = 3, 9, 50
EOS = {0: (), 1: (2,), 2: (2, 7)}
KINDS = ("nothing", "some", "all", "stale")


def torch_step(state, top_lp, top_idx, cur, vocab, eos, early_stopping, length_penalty, device="cpu"):
    """generation._advance_beams_torch on ``device`` from numpy inputs: the dict of its outputs as numpy arrays."""
    from outlier_suppression_amd.model import generation as G
    bsz, nb, max_length = state["running"].shape
    keep = top_lp.shape[1]
    t = {k: torch.from_numpy(v.copy()).to(device) for k, v in state.items()}
    t["improvable"] = t["improvable"].view(bsz, 1)
    top_mask = torch.cat((torch.ones(nb, dtype=torch.bool), torch.zeros(keep - nb, dtype=torch.bool))).to(device)
    offsets = torch.arange(bsz, device=device).view(-1, 1) * nb
    eos_t = torch.tensor(list(eos), device=device) if len(eos) else None
    new, beam_idx, go_on = G._advance_beams_torch(G._BeamState(**{k: t[k] for k in G._BeamState.FIELDS}),
                                                  torch.from_numpy(top_lp).to(device), torch.from_numpy(top_idx).to(device), cur,
                                                  vocab, eos_t, top_mask, offsets, max_length, length_penalty, early_stopping)
    out = {k: getattr(new, k).cpu().numpy() for k in G._BeamState.FIELDS}
    out["improvable"] = out["improvable"].reshape(bsz)
    out["beam_idx"] = beam_idx.cpu().numpy()
    out["next_tokens"] = out["running"][:, :, cur].reshape(-1)
    out["go_on"] = np.array([bool(go_on)], dtype=np.int32)
    return out


def words(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def compare_with_torch(got, want, label):
    """Word equality where the torch lines have no ties; returns the number of finished rows compared."""
    for name in ("running", "running_scores", "beam_idx", "next_tokens", "improvable", "go_on", "scores", "done"):
        assert np.array_equal(words(got[name]), words(want[name])), (label, name, got[name], want[name])
    done = want["done"]
    assert np.array_equal(got["finished"][done], want["finished"][done]), (label, "finished")
    assert np.array_equal(got["finished_len"][done], want["finished_len"][done]), (label, "finished_len")
    return int(done.sum())


def tie_free(state, top_lp, top_idx, cur, vocab, eos, early_stopping, length_penalty, nb, reciprocal=False):
    """What entitles a case to word equality: the first nb of top_running_lp are pairwise distinct and above the rest, and the
    real entries of scores | cand are pairwise distinct."""
    ref = BA.reference(top_lp, top_idx, state, cur, vocab, eos, early_stopping, length_penalty, reciprocal)
    for b in range(top_lp.shape[0]):
        token = top_idx[b] % vocab
        hits = np.full(top_lp.shape[1], cur + 1 >= state["running"].shape[2]) | np.isin(token, np.asarray(eos, dtype=np.int64))
        trl = np.sort(top_lp[b] + hits.astype(np.float32) * BA.BIG)[::-1]
        assert len(set(trl[:nb + 1].tolist())) == min(nb + 1, len(trl)), "top_running_lp ties among the kept"
        real = ref["_cat"][b][ref["_cat"][b] > -5e8]
        assert len(set(real.tolist())) == len(real), "real scores tie"
    return ref


@pytest.mark.parametrize("nb, n_eos, early_stopping, length_penalty",
                         list(itertools.product((1, 2, 6), (0, 1, 2), (False, True, "never"), (0, 0.8, 1, 2))))
def test_reference_restates_the_torch_lines(nb, n_eos, early_stopping, length_penalty):
    eos = EOS[n_eos]
    keep = max(2, 1 + n_eos) * nb
    rng = np.random.default_rng(1000 * nb + 100 * n_eos + 7)
    compared = 0
    for kind, last in itertools.product(KINDS, (False, True)):
        cur = L - 1 if last else 4
        state = BA.random_state(rng, BSZ, nb, L, cur, VOCAB, kind, eos)
        top_lp, top_idx = BA.random_selection(rng, BSZ, nb, keep, VOCAB, eos, wide=last)
        if not last:        # an ordinary step: at least nb candidates are no hit, the kept ones tie with nothing
            token = top_idx % VOCAB
            assert ((~np.isin(token, np.asarray(eos, dtype=np.int64))).sum(axis=1) >= nb).all()
        got = tie_free(state, top_lp, top_idx, cur, VOCAB, eos, early_stopping, length_penalty, nb)
        want = torch_step(state, top_lp, top_idx, cur, VOCAB, eos, early_stopping, length_penalty)
        compared += compare_with_torch(got, want, (kind, last))
        assert not (last and got["go_on"][0])                # the last step always stops
    assert compared >= 1


def test_reference_order_rule():
    """Ties by smaller index, NaN first, -0.0 equal to +0.0: the part torch.topk leaves open."""
    v = np.array([1.0, 3.0, -np.inf, 3.0, np.nan, -0.0, 0.0, np.nan, -np.inf], dtype=np.float32)
    assert BA.order(v) == [4, 7, 1, 3, 0, 5, 6, 2, 8]


def test_reference_division_forms_differ():
    """The two forms of the division are different words somewhere: the flag is not idle."""
    v = -(np.arange(1, 65, dtype=np.float32)) / np.float32(64)
    assert (BA._divide(v, 3 ** 0.8, True).view(np.uint32) != BA._divide(v, 3 ** 0.8, False).view(np.uint32)).any()


def test_entry_point_is_listed_and_bound():
    from outlier_suppression_amd import _hip
    header = open(os.path.join(ROOT, "include", "osq_hip.h")).read()
    above = header[:header.index("#define OSQ_ABI_VERSION")]
    added = re.search(r"Added within 10 \(no existing signature changed\):(.*?)\*/", above, re.S).group(1)
    assert "osq_beam_advance" in set(re.findall(r"osq_\w+", added))
    decl = re.search(r"^int osq_beam_advance\((.*?)\);", header, re.M | re.S)
    assert decl, "osq_beam_advance is not declared"
    assert len(decl.group(1).split(",")) == len(_hip.SIGNATURES["osq_beam_advance"][1]) == 34
    assert re.search(r"#define OSQ_ABI_VERSION 10\b", header) and _hip.ABI_VERSION == 10
    makefile = open(os.path.join(ROOT, "outlier_suppression_amd", "csrc", "Makefile")).read()
    assert makefile.count("beam_advance.hip") == 2          # the library and its development build


@pytest.fixture()
def switch():
    from outlier_suppression_amd import util_layernorm as UL
    old = UL.BEAM_ADVANCE
    yield UL
    UL.BEAM_ADVANCE = old


@pytest.mark.parametrize("value, want", [(None, False), ("", False), ("0", False), ("1", True), ("yes", True)])
def test_environment_variable(value, want):
    import outlier_suppression_amd as osq
    env = {} if value is None else {"OSQ_BEAM_ADVANCE": value}
    assert osq.beam_advance_from_environment(env) is want


def test_switch_and_environment_reach_reset_tier(switch, monkeypatch):
    import outlier_suppression_amd as osq
    from outlier_suppression_amd import ops
    assert switch.BEAM_ADVANCE is False or os.environ.get("OSQ_BEAM_ADVANCE", "") not in ("", "0")
    osq.set_beam_advance()
    assert switch.BEAM_ADVANCE is True
    osq.set_beam_advance(False)
    assert switch.BEAM_ADVANCE is False
    monkeypatch.setattr(ops, "set_tuning", lambda key, value, lib=None: None)
    monkeypatch.setenv("OSQ_BEAM_ADVANCE", "1")
    osq.reset_tier()
    assert switch.BEAM_ADVANCE is True
    monkeypatch.delenv("OSQ_BEAM_ADVANCE")
    osq.reset_tier()
    assert switch.BEAM_ADVANCE is False


def test_generate_on_the_cpu_takes_the_torch_lines_and_says_why(switch):
    from test_bart_decode_cpu import batch, tiny_bart, wrapped
    q = wrapped(tiny_bart())
    ids, mask = batch()
    kw = dict(attention_mask=mask, max_length=12, num_beams=3, min_length=5, no_repeat_ngram_size=2)
    with torch.no_grad():
        want = q.generate(ids, beam_advance=False, **kw)
        info = q.last_beam_advance
        assert (info.advanced, info.reason) == (0, "not asked for") and info.eager >= 4
        got = q.generate(ids, beam_advance=True, **kw)
        assert torch.equal(got, want)
        info = q.last_beam_advance
        assert info.advanced == 0 and info.eager >= 4 and "CPU" in info.reason, info
        switch.BEAM_ADVANCE = True                     # the package switch asks as the argument does
        assert torch.equal(q.generate(ids, **kw), want) and "CPU" in q.last_beam_advance.reason
        q.generate(ids, attention_mask=mask, max_length=6, num_beams=1)
        assert q.last_beam_advance.advanced == 0 and "greedy" in q.last_beam_advance.reason

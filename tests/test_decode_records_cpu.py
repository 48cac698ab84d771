"""CPU: the host layer under generate() and sample() where no GPU and no built library is involved -- the nine outcome
records (graph_decode.Outcome) and their "asked for?" constructor, the reasons of every ``*_why_not`` and of the two kernel
plans in their order of precedence, what the plans make of transformers' own logits processors (_read_processors), and the
twelve on / off environment switches with reset_tier.

Every expected value here is a literal, and every literal was recorded by running the same expression at the commit before
the host layer was folded (nine hand-written record classes, five copies of the device guard, two walks over the processors,
twelve copies of the environment rule), not read off the code under test: this file pins what that fold must not move.  The
plans meet their processors on ``torch.device("cuda:0")``, a name only, with id tensors that stay on the CPU when they are
sent there (_Stay), so that the walk runs behind the real device guard on a machine without a GPU.  The rows of a reason
table differ from the row before by the one condition that took precedence there.  At that older commit all of this file
passes but the five tests that name what the fold added: ``Outcome.asked`` and ``_read_processors``."""
from types import SimpleNamespace as NS

import pytest
import torch

CPU, GPU = torch.device("cpu"), torch.device("cuda:0")           # GPU: a name only; nothing is ever moved to it
RECORDS = [("generation", "BeamSelectInfo", ("selected", "eager")), ("generation", "ShareCrossKvInfo", ("shared", "eager")),
           ("generation", "BeamAdvanceInfo", ("advanced", "eager")), ("generation", "GreedyAdvanceInfo", ("advanced", "eager")),
           ("generation", "SampleAdvanceInfo", ("advanced", "eager")), ("graph_decode", "DecodeGraphInfo", ("captured", "replays")),
           ("graph_decode", "BeamGraphInfo", ("captured", "replays", "issued")),
           ("graph_decode", "GreedyGraphInfo", ("captured", "replays")), ("graph_decode", "SampleGraphInfo", ("captured", "replays"))]
REPRS = {"BeamSelectInfo": ("BeamSelectInfo(selected=0, eager=0, reason=None)", "BeamSelectInfo(selected=1, eager=2, reason='why')"),
         "ShareCrossKvInfo": ("ShareCrossKvInfo(shared=0, eager=0, reason=None)", "ShareCrossKvInfo(shared=1, eager=2, reason='why')"),
         "BeamAdvanceInfo": ("BeamAdvanceInfo(advanced=0, eager=0, reason=None)", "BeamAdvanceInfo(advanced=1, eager=2, reason='why')"),
         "GreedyAdvanceInfo": ("GreedyAdvanceInfo(advanced=0, eager=0, reason=None)",
                               "GreedyAdvanceInfo(advanced=1, eager=2, reason='why')"),
         "SampleAdvanceInfo": ("SampleAdvanceInfo(advanced=0, eager=0, reason=None)",
                               "SampleAdvanceInfo(advanced=1, eager=2, reason='why')"),
         "DecodeGraphInfo": ("DecodeGraphInfo(captured=0, replays=0, reason=None)",
                             "DecodeGraphInfo(captured=1, replays=2, reason='why')"),
         "BeamGraphInfo": ("BeamGraphInfo(captured=0, replays=0, issued=0, reason=None)",
                           "BeamGraphInfo(captured=1, replays=2, issued=3, reason='why')"),
         "GreedyGraphInfo": ("GreedyGraphInfo(captured=0, replays=0, reason=None)",
                             "GreedyGraphInfo(captured=1, replays=2, reason='why')"),
         "SampleGraphInfo": ("SampleGraphInfo(captured=0, replays=0, reason=None)",
                             "SampleGraphInfo(captured=1, replays=2, reason='why')")}


def _modules():
    from outlier_suppression_amd.model import generation, graph_decode
    return {"generation": generation, "graph_decode": graph_decode}


@pytest.mark.parametrize("module, name, counters", RECORDS)
def test_record_repr_fresh_and_counted(module, name, counters):
    record = getattr(_modules()[module], name)()
    assert repr(record) == REPRS[name][0]
    assert [getattr(record, c) for c in counters] == [0] * len(counters) and record.reason is None
    for i, c in enumerate(counters):
        setattr(record, c, getattr(record, c) + i + 1)
    record.reason = "why"
    timed = module == "graph_decode"                 # capture_seconds: on the four graph records, never in a repr
    assert hasattr(record, "capture_seconds") is timed
    if timed:
        assert record.capture_seconds == 0.0
        record.capture_seconds += 0.5
    assert repr(record) == REPRS[name][1]
    assert type(record)("given").reason == "given"


def test_the_two_sampling_records_are_the_greedy_ones():
    m = _modules()
    assert isinstance(m["generation"].SampleAdvanceInfo(), m["generation"].GreedyAdvanceInfo)
    assert isinstance(m["graph_decode"].SampleGraphInfo(), m["graph_decode"].GreedyGraphInfo)


@pytest.mark.parametrize("flag, given, reason", [(False, None, "not asked for"), (True, None, None), (True, False, "not asked for"),
                                                 (False, True, None)])
def test_asked_reads_the_flag_when_called(flag, given, reason):
    from outlier_suppression_amd import util_layernorm as UL
    m = _modules()
    old = UL.BEAM_SELECT, UL.SAMPLE_GRAPH
    try:
        UL.BEAM_SELECT = UL.SAMPLE_GRAPH = flag
        for cls, name in ((m["generation"].BeamSelectInfo, "BEAM_SELECT"), (m["graph_decode"].SampleGraphInfo, "SAMPLE_GRAPH")):
            record = cls.asked(given, name)
            assert type(record) is cls and record.reason == reason
            assert repr(record) == REPRS[cls.__name__][0].replace("reason=None", f"reason={reason!r}")
    finally:
        UL.BEAM_SELECT, UL.SAMPLE_GRAPH = old


def _under(grad, fn, *args):
    with (torch.enable_grad() if grad else torch.no_grad()):
        return fn(*args)


def _model(training=False, head_dim=8, plain=True):
    """As much of a wrapped BART as _share_why_not looks at: one decoder layer's cross-attention and its five quantizers."""
    attn = NS(head_dim=head_dim, num_heads=2, embed_dim=2 * head_dim, dropout=0.1)
    for site in ("query", "key", "value", "attention_probs", "context"):
        setattr(attn, site + "_post_act_fake_quantize", NS(fake_quant_enabled=1, observer_enabled=0, ch_axis=-1,
                                                           scale=NS(is_cuda=plain)))
    return NS(model=NS(decoder=NS(training=training, layers=[NS(dropout=0.1, encoder_attn=attn)])))


def _ids(n):
    return torch.arange(n)


# (autograd on, model(training, head_dim, plain quantizers), device, use_cache, beams, source length) -> reason
SHARE = [((True, (True, 6, False), CPU, False, 1, 1025), "one beam per batch row (num_beams == 1): there is nothing to share"),
         ((True, (True, 6, False), CPU, False, 65, 1025), "num_beams above 64"),
         ((True, (True, 6, False), CPU, False, 3, 1025), "use_cache=False: there is no cache"),
         ((True, (True, 6, False), CPU, True, 3, 1025), "the tensors are on the CPU"),
         ((True, (True, 6, False), GPU, True, 3, 1025), "autograd is on"),
         ((False, (True, 6, False), GPU, True, 3, 1025), "dropout is active"),
         ((False, (False, 6, False), GPU, True, 3, 1025), "the source is longer than 1024"),
         ((False, (False, 6, False), GPU, True, 3, 14), "the shared cross-attention does not take head_dim 6"),
         ((False, (False, 8, False), GPU, True, 3, 14),
          "a cross-attention quantizer is not in the plain quantising state (decoder layer 0, query)"),
         ((False, (False, 8, True), GPU, True, 3, 14), None)]


@pytest.mark.parametrize("row, reason", SHARE)
def test_share_why_not(row, reason):
    grad, model, rest = row[0], _model(*row[1]), row[2:]
    assert _under(grad, _modules()["generation"]._share_why_not, model, *rest) == reason


GEOMETRY = "the kernel takes keep <= 64, num_beams <= 64 and max_length in [2, 4096]"
# (autograd on, device, beams, keep, max_length, number of eos ids or None) -> reason
ADVANCE = [((True, CPU, 65, 130, 1, 17), "the tensors are on the CPU"), ((True, GPU, 65, 130, 1, 17), "autograd is on"),
           ((False, GPU, 65, 130, 1, 17), GEOMETRY), ((False, GPU, 64, 130, 1, 17), GEOMETRY), ((False, GPU, 64, 64, 1, 17), GEOMETRY),
           ((False, GPU, 64, 64, 4097, 17), GEOMETRY), ((False, GPU, 64, 64, 4096, 17), "more than 16 eos ids"),
           ((False, GPU, 64, 64, 4096, 16), None), ((False, GPU, 64, 64, 2, None), None)]


@pytest.mark.parametrize("row, reason", ADVANCE)
def test_advance_why_not(row, reason):
    grad, device, nb, keep, max_length, n_eos = row
    eos = None if n_eos is None else _ids(n_eos)
    assert _under(grad, _modules()["generation"]._advance_why_not, device, nb, keep, max_length, eos) == reason


# (the plan's reason, top_k, top_p, sample_nucleus, vocab) -> reason
SAMPLE = [(("a plan's reason", 0, 0.5, True, 60000), "a plan's reason"), ((None, 0, 0.5, True, 60000), "vocab above 51200"),
          ((None, 0, 0.5, True, 51200), None), ((None, 0, 0.5, False, 51200), "top_p below 1 without top_k"),
          ((None, 65, 0.5, False, 51200), "top_k above 64"), ((None, 64, 0.5, False, 51200), None),
          ((None, 0, 1.0, False, 51200), None), ((None, 0, 1.0, True, 60000), None)]


@pytest.mark.parametrize("row, reason", SAMPLE)
def test_sample_why_not_over_a_stub_plan(row, reason):
    assert _modules()["generation"]._sample_why_not(NS(reason=row[0]), *row[1:]) == reason


# (autograd on, device, use_cache, FUSE_KV_APPEND) -> reason, all of them without a model
GRAPH = [((True, CPU, False, False), "the tensors are on the CPU"), ((True, GPU, False, False), "use_cache=False: there is no cached step"),
         ((True, GPU, True, False), "autograd is on"),
         ((False, GPU, True, False), "the one-launch KV append is off (util_layernorm.FUSE_KV_APPEND)")]


@pytest.mark.parametrize("row, reason", GRAPH)
def test_graph_why_not_answers_without_the_model(row, reason):
    from outlier_suppression_amd import util_layernorm as UL
    grad, device, use_cache, fuse = row
    old = UL.FUSE_KV_APPEND
    try:
        UL.FUSE_KV_APPEND = fuse
        assert _under(grad, _modules()["graph_decode"].why_not, None, device, use_cache, 12) == reason
    finally:
        UL.FUSE_KV_APPEND = old
    assert _under(False, _modules()["graph_decode"].why_not, None, CPU) == "the tensors are on the CPU"


def _no_processors():
    from transformers.generation.logits_process import LogitsProcessorList
    return LogitsProcessorList()


SELECT_GEOMETRY = "the kernel takes keep <= min(vocab, 64), num_beams <= 64 and max_length <= 4096"
# (autograd on, device, beams, vocab, keep, max_length) -> _BeamSelectPlan(...).reason
BEAM_PLAN = [((True, CPU, 65, 70, 71, 4097), "the tensors are on the CPU"), ((True, GPU, 65, 70, 71, 4097), "autograd is on"),
             ((False, GPU, 65, 70, 71, 4097), SELECT_GEOMETRY), ((False, GPU, 65, 70, 65, 4097), SELECT_GEOMETRY),
             ((False, GPU, 65, 70, 64, 4097), SELECT_GEOMETRY), ((False, GPU, 64, 70, 64, 4097), SELECT_GEOMETRY),
             ((False, GPU, 64, 70, 64, 4096), None)]
# (autograd on, device, vocab, max_length) -> _GreedyPlan(..., eos=None, pad=None).reason
GREEDY_PLAN = [((True, CPU, 70, 1), "the tensors are on the CPU"), ((True, GPU, 70, 1), "autograd is on"),
               ((False, GPU, 70, 1), "the kernel takes max_length in [2, 4096]"),
               ((False, GPU, 70, 4097), "the kernel takes max_length in [2, 4096]"), ((False, GPU, 70, 4096), None)]


@pytest.mark.parametrize("row, reason", BEAM_PLAN)
def test_beam_select_plan_guards(row, reason):
    plan = _under(row[0], _modules()["generation"]._BeamSelectPlan, _no_processors(), *row[1:])
    assert plan.reason == reason and (plan.ngram, plan.min_length, plan.eos, plan.forced_at) == (0, 0, None, set())


@pytest.mark.parametrize("row, reason", GREEDY_PLAN)
def test_greedy_plan_guards(row, reason):
    plan = _under(row[0], _modules()["generation"]._GreedyPlan, _no_processors(), *row[1:], None, None)
    assert plan.reason == reason
    assert (plan.ngram, plan.min_length, plan.ban, plan.forced_bos, plan.forced_eos, plan.eos, plan.pad) == (0, 0, None, None, None, None, 0)


class _Stay(torch.Tensor):
    """Ids that stay where they are: ``.to(device=...)`` converts the dtype and moves nothing."""

    def to(self, *args, **kwargs):
        kwargs.pop("device", None)
        return self.as_subclass(torch.Tensor).to(*args, **kwargs)


def _case(name):
    from transformers.generation.logits_process import (ForcedBOSTokenLogitsProcessor, ForcedEOSTokenLogitsProcessor,
                                                        LogitsProcessorList, MinLengthLogitsProcessor,
                                                        NoRepeatNGramLogitsProcessor, TemperatureLogitsWarper)
    ngram, bos = NoRepeatNGramLogitsProcessor, ForcedBOSTokenLogitsProcessor

    def staying(proc):
        proc.eos_token_id = proc.eos_token_id.as_subclass(_Stay)
        return proc

    def min_len(n, ids):
        return staying(MinLengthLogitsProcessor(n, ids))

    def eos(max_length, ids):
        return staying(ForcedEOSTokenLogitsProcessor(max_length, ids))
    return LogitsProcessorList({
        "ngram": lambda: [ngram(3)], "min1": lambda: [min_len(5, [2])], "min17": lambda: [min_len(5, list(range(17)))],
        "bos": lambda: [bos(7)], "eos1": lambda: [eos(12, [2])], "eos2": lambda: [eos(12, [2, 3])],
        "eos_other": lambda: [eos(9, [2])], "unknown": lambda: [TemperatureLogitsWarper(0.5)],
        "all": lambda: [ngram(2), min_len(4, [2, 3]), bos(0), eos(12, [2])],
        "ngram_twice": lambda: [ngram(2), ngram(3)],
        "bos_twice_unknown": lambda: [bos(7), bos(8), TemperatureLogitsWarper(0.5)],
        "bos_outside": lambda: [bos(70)]}[name]())


def _restate(name):
    return f"a logits processor the kernel does not restate ({name})"


IDS17 = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
# Both plans at 2 beams, vocab 70, keep 4, max_length 12, no eos and no pad of the call's own:
#   name -> (_BeamSelectPlan: ngram, min_length, eos, sorted forced_at, reason), (_GreedyPlan: ngram, min_length, ban,
#           forced_bos, forced_eos, reason)
PLANS = {
    "ngram": ((3, 0, None, [], None), (3, 0, None, None, None, None)),
    "min1": ((0, 5, [2], [], None), (0, 5, [2], None, None, None)),
    "min17": ((0, 5, IDS17, [], "more than 16 eos ids"), (0, 5, IDS17, None, None, "more than 16 eos ids")),
    "bos": ((0, 0, None, [1], None), (0, 0, None, 7, None, None)),
    "eos1": ((0, 0, None, [11], None), (0, 0, None, None, 2, None)),
    "eos2": ((0, 0, None, [11], None), (0, 0, None, None, None, _restate("ForcedEOSTokenLogitsProcessor"))),
    "eos_other": ((0, 0, None, [8], None), (0, 0, None, None, None, _restate("ForcedEOSTokenLogitsProcessor"))),
    "unknown": ((0, 0, None, [], _restate("TemperatureLogitsWarper")), (0, 0, None, None, None, _restate("TemperatureLogitsWarper"))),
    "all": ((2, 4, [2, 3], [1, 11], None), (2, 4, [2, 3], 0, 2, None)),
    "ngram_twice": ((2, 0, None, [], _restate("NoRepeatNGramLogitsProcessor")),
                    (2, 0, None, None, None, _restate("NoRepeatNGramLogitsProcessor"))),
    "bos_twice_unknown": ((0, 0, None, [1], _restate("TemperatureLogitsWarper")),
                          (0, 0, None, 7, None, _restate("ForcedBOSTokenLogitsProcessor"))),
    "bos_outside": ((0, 0, None, [1], None), (0, 0, None, 70, None, "a forced token is outside the vocabulary")),
}


def _listed(t):
    return None if t is None else t.tolist()


@pytest.mark.parametrize("name", sorted(PLANS))
def test_what_each_plan_makes_of_the_processors(name):
    G = _modules()["generation"]
    with torch.no_grad():
        b = G._BeamSelectPlan(_case(name), GPU, 2, 70, 4, 12)
        g = G._GreedyPlan(_case(name), GPU, 70, 12, None, None)
    assert (b.ngram, b.min_length, _listed(b.eos), sorted(b.forced_at), b.reason) == PLANS[name][0]
    assert (g.ngram, g.min_length, _listed(g.ban), g.forced_bos, g.forced_eos, g.reason) == PLANS[name][1]
    for ids in (b.eos, g.ban):
        assert ids is None or (ids.dtype == torch.int64 and ids.dim() == 1 and ids.is_contiguous())
    if name == "all":
        assert [g.forced(cur) for cur in (1, 2, 10, 11)] == [0, None, None, 2]
        assert b.takes(2, torch.zeros(4, 70)) is False                  # CPU logits: the torch lines


def test_the_reader_walks_the_list_once_and_in_order():
    G = _modules()["generation"]
    items = list(G._read_processors(_case("all"), CPU))
    assert [kind for kind, _ in items] == ["ngram", "min_length", "forced_bos", "forced_eos"]
    assert items[0][1] == 2 and items[1][1][0] == 4 and items[1][1][1].tolist() == [2, 3]
    assert int(items[2][1].bos_token_id) == 0 and int(items[3][1].max_length) == 12
    assert [kind for kind, _ in G._read_processors(_case("min17"), CPU)] == ["min_length", "reason"]
    assert list(G._read_processors(_case("bos_twice_unknown"), CPU))[-1] == ("reason", _restate("TemperatureLogitsWarper"))
    assert list(G._read_processors(_no_processors(), CPU)) == []


SWITCHES = ["CACHE_CODES", "GRAPH_DECODE", "BEAM_SELECT", "BEAM_ADVANCE", "BEAM_GRAPH", "GREEDY_ADVANCE", "GREEDY_GRAPH",
            "SAMPLE_ADVANCE", "SAMPLE_GRAPH", "SAMPLE_NUCLEUS", "SHARE_CROSS_KV", "FAST_LM_LOSS"]


@pytest.mark.parametrize("name", SWITCHES)
def test_environment_readers(name):
    import outlier_suppression_amd as osq
    read = getattr(osq, name.lower() + "_from_environment")
    got = [read({} if value is None else {"OSQ_" + name: value}) for value in (None, "", "0", "1", "no")]
    assert got == [False, False, False, True, True]
    assert read({"OSQ_OTHER": "1"}) is False and read.__doc__.startswith(f"What OSQ_{name} asks for")


@pytest.mark.parametrize("on", [None] + SWITCHES)
def test_reset_tier_leaves_each_flag_at_its_variable(on, monkeypatch):
    import outlier_suppression_amd as osq
    from outlier_suppression_amd import ops, util_layernorm as UL
    for name in SWITCHES + ["FUSE_LAYERNORM", "FUSE_SOFTMAX", "FUSE_DECODE_ATTENTION"]:
        monkeypatch.setattr(UL, name, getattr(UL, name))               # put back after the test
    monkeypatch.setattr(ops, "set_tuning", lambda key, value, lib=None: None)
    for name in SWITCHES:
        monkeypatch.delenv("OSQ_" + name, raising=False)
        setattr(UL, name, name != on)                                   # every flag starts at the opposite
    if on is not None:
        monkeypatch.setenv("OSQ_" + on, "1")
    osq.reset_tier()
    assert {name: getattr(UL, name) for name in SWITCHES} == {name: name == on for name in SWITCHES}

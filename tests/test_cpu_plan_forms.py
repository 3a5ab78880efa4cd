"""Host: engine.decide_forms — every launch-form decision of a ForwardPlan, made from host
metadata before any buffer exists — on the cases of _plan_cases.py, with the device graph
built on the CPU device.  The expected forms are literals read off the plans the commit before
the decision was split out built on the GPU (their flags and sets as golden/plan_forms.json
records them; a layer's kind and table from its launch classes and kernel names there).
"""
import dataclasses

import pytest

import _plan_cases as pc

torch = pytest.importorskip("torch")

ALL = [(0, 0), (0, 1), (1, 0), (1, 1)]
P_REASSOC = [(0, 0), (0, 1), (1, 0)]
PARTIAL = ("partial", "", False)
TAB = ("fused_seg", "tab", False)
ROWS = ("seg_rows", "tab", False)

# case -> (true flags, {set name: members}, (kind, table, peer_red) of layer 1, of layer 2)
EXPECTED = {
    "S": ({"fused_seg", "tab_weighted"}, {"fused": [0, 1], "preproj": ALL}, TAB, ("fused_seg", "narrow", False)),
    "S-no-preproject": ({"fused_seg", "tab_weighted"}, {"fused": [0, 1], "seg_proj": ALL}, TAB, TAB),
    "S-no-wave-table": ({"fused_seg"}, {"fused": [0, 1], "seg_proj": ALL},
                        ("fused_seg", "", False), ("fused_seg", "", False)),
    "S-no-fused-seg": (set(), {"fused": [0, 1]}, ("fused", "", False), ("fused", "", False)),
    "S-partial": (set(), {}, PARTIAL, PARTIAL),
    "S-keep-sums": ({"flat_mode"}, {}, PARTIAL, PARTIAL),
    "S-keep-sums-dropout": ({"flat_mode"}, {}, PARTIAL, PARTIAL),
    "P-small": (set(), {"staged_proj": [(1, 1)]}, PARTIAL, PARTIAL),
    "P-small-keep-sums": ({"sums_mode"}, {"staged_proj": [(1, 1)]}, PARTIAL, PARTIAL),
    "S-sets-2-seg": ({"flat_mode", "seg_mode"}, {"seg_proj": ALL}, ROWS, ROWS),
    "S-sets-8-seg": ({"flat_mode", "seg_mode"}, {"seg_proj": ALL}, PARTIAL, PARTIAL),
    "S-sets-2-fused": ({"flat_mode"}, {"fused": [0, 1]}, ("fused", "", False), ("fused", "", False)),
    "S-lpt-2": ({"flat_mode"}, {"seg_proj": [(0, 0), (0, 1), (1, 1)]}, PARTIAL, PARTIAL),
    "P-small-split-3": ({"flat_mode"}, {"seg_proj": P_REASSOC, "staged_proj": [(1, 1)]}, PARTIAL, PARTIAL),
    "P-small-split-2-keep-sums": ({"flat_mode"}, {"staged_proj": [(1, 1)]}, PARTIAL, PARTIAL),
    "S-sets-2-seg-peer-fused": ({"flat_mode", "seg_mode"}, {"seg_proj": ALL}, ROWS, ROWS),
    "S-sets-2-seg-peer-kernel": ({"flat_mode", "seg_mode"}, {"seg_proj": ALL}, ROWS, ROWS),
    "P-small-split-3-peer-fused": ({"flat_mode", "peer_reduce"}, {"seg_proj": P_REASSOC, "staged_proj": [(1, 1)]},
                                   ("partial", "", True), ("partial", "", True)),
    "P-small-split-3-peer-kernel": ({"flat_mode"}, {"seg_proj": P_REASSOC, "staged_proj": [(1, 1)]},
                                    PARTIAL, PARTIAL),
    "S-sparse-features": ({"fused_seg", "tab_weighted"}, {"fused": [0, 1], "preproj": ALL}, TAB,
                          ("fused_seg", "narrow", False)),
}
CASES = {c.name: c for c in pc.cases()}


def _decide(case):
    from decagon_amd import engine

    with pc.policy(case):
        dg, args, kw = pc.plan_args(case, torch.device("cpu"))
        return dg, kw, engine.decide_forms(dg, pc.H1, pc.H2, **kw)


def test_every_case_has_its_literals():
    assert sorted(EXPECTED) == sorted(CASES)


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_decided_forms(name):
    flags, sets, l1, l2 = EXPECTED[name]
    _, _, f = _decide(CASES[name])
    assert {k for k in pc.FLAGS if getattr(f, k)} == flags
    for k in pc.SETS:
        assert sorted(getattr(f, k)) == sets.get(k, []), k
    for layer, want in ((1, l1), (2, l2)):
        lf = f.layers[layer]
        assert (lf.kind, lf.table, lf.peer_red) == want, layer
        assert (lf.layer, lf.d, lf.relu) == (layer, (pc.H1, pc.H2)[layer - 1], layer == 1)
        assert lf.d_in == (pc.H1 if layer == 1 or f.seg_proj else pc.H2)


def test_peer_reduce_that_does_not_fit(monkeypatch):
    """Targets that do not fit one epilogue launch keep the flat buffer and the all-reduce; a
    record that has the peer reduce on over targets that do not fit raises (no assert: python -O
    would strip it and leave the relation-sharded sums unreduced)."""
    from decagon_amd import engine

    case = CASES["P-small-split-3-peer-fused"]
    dg, kw, f = _decide(case)
    assert f.peer_reduce and f.peer_fit
    bad = dataclasses.replace(f, peer_fit=False)
    with pytest.raises(RuntimeError, match="peer all-reduce"):
        engine._layer_forms(bad, dg, 1, pc.H1, pc.H2)
    calls = []
    monkeypatch.setattr(engine, "_peer_reduce_fits", lambda *a: calls.append(a) or False)
    f = engine.decide_forms(dg, pc.H1, pc.H2, **kw)
    assert len(calls) == 1  # computed once
    assert not f.peer_reduce and not f.peer_fit
    assert not f.layers[1].peer_red and not f.layers[2].peer_red


def test_decision_reads_no_device_data(monkeypatch):
    """The decision runs on host metadata: the group tensors may be absent altogether."""
    from decagon_amd import engine

    case = CASES["P-small-split-3"]
    dg, kw, want = _decide(case)
    for g in dg.groups.values():
        for k in ("rowptr", "vcol", "val"):
            setattr(g, k, None)
    assert engine.decide_forms(dg, pc.H1, pc.H2, **kw) == want

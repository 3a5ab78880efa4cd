"""GPU: the ForwardPlan built for every case of _plan_cases.py — its forms, its launches by
class and order with their groups, its wave tables' parameters, its byte accounting
(_plan_cases.manifest) — equals golden/plan_forms.json, written by golden/make_plan_forms.py
at the commit before the plan builder was split by launch form; and the unsharded plans' one
forward equals the float64 oracle within 1e-4 relative (test_gpu_model.py's tolerance).
Sharded cases are one rank's share with no-op collectives: held to the manifest alone.
"""
import json
from pathlib import Path

import pytest

import _plan_cases as pc
from conftest import rel_err

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TOL = 1e-4
GOLDEN = json.loads((Path(__file__).parent / "golden" / "plan_forms.json").read_text())
CASES = pc.cases()


def test_golden_lists_the_cases():
    assert sorted(GOLDEN) == sorted(c.name for c in CASES)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_plan_matches_parent_manifest(case):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    plan = pc.build_plan(case, torch.device("cuda", 0))
    try:
        got = json.loads(json.dumps(pc.manifest(plan)))
        want = GOLDEN[case.name]
        assert sorted(got) == sorted(want)
        for key in want:
            assert got[key] == want[key], key
        if case.sharded:
            return
        plan.run()
        torch.cuda.synchronize()
        h1, emb = pc.oracle(case)
        for t in plan.hidden1:
            print(case.name, t, rel_err(plan.hidden1[t].cpu().numpy(), h1[t]),
                  rel_err(plan.embeddings[t].cpu().numpy(), emb[t]))
            assert rel_err(plan.hidden1[t].cpu().numpy(), h1[t]) <= TOL, ("hidden1", t)
            assert rel_err(plan.embeddings[t].cpu().numpy(), emb[t]) <= TOL, ("embeddings", t)
    finally:
        if plan.peer is not None:
            plan.peer.close()

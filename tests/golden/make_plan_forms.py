"""Writes tests/golden/plan_forms.json: the manifest (tests/_plan_cases.manifest) of the
ForwardPlan built for every case of tests/_plan_cases.py, on the GPU.

    python tests/golden/make_plan_forms.py [--out FILE] [--hashes FILE]

The committed file was written at the commit before ForwardPlan was split into a form
decision and per-form builders; tests/test_gpu_plan_forms.py holds every later plan to it.
--hashes FILE also runs each plan once and writes the SHA-256 of its outputs
(_plan_cases.output_hashes) to FILE — for comparing two commits bit for bit, not committed.
"""
import argparse
import json
import sys
import time
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path[:0] = [str(HERE.parents[1]), str(HERE.parent)]


def main():
    import torch

    import _plan_cases as pc

    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(HERE / "plan_forms.json"))
    ap.add_argument("--hashes", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    forms, hashes = {}, {}
    for case in pc.cases():
        t0 = time.perf_counter()
        plan = pc.build_plan(case, dev)
        forms[case.name] = pc.manifest(plan)
        if args.hashes:
            plan.run()
            torch.cuda.synchronize()
            if plan.peer is not None:
                plan.peer.check()
            hashes[case.name] = pc.output_hashes(plan)
        if plan.peer is not None:
            plan.peer.close()
        print(f"{case.name}: {time.perf_counter() - t0:.2f} s", flush=True)
    Path(args.out).write_text(json.dumps(forms, indent=1, sort_keys=True) + "\n")
    if args.hashes:
        Path(args.hashes).write_text(json.dumps(hashes, indent=1, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""Batches of every relation served from device-resident edges, measured on the polypharmacy-shaped
synthetic graph (config P: 1,932 relations), batch 512, device-drawn negatives.

  (a) kernel   dg_epoch_batch_i32 alone for the drug×drug edge type (1,928 relations × 512 pairs):
               device time between events over --reps launches, --rounds rounds; the gather rate is
               the 8-byte edge pairs read plus the two 4-byte index arrays written, per second.
  (b) step     one trainall.train_step_all fed by EdgeBatches.batch (formed inside the timed pass)
               against the same step fed by EdgeBatches.host_batch — the host dicts: pack_batches and
               one upload per edge type (trainall.type_batch) before the run, then the device-fed
               step's path.  The host dicts are built before the clock starts.
  (c) stages   the device-fed step with a device synchronise after every stage (trainall.stage_log):
               batch formation, forward and plan, operands, sampler, scorer and hinge, gradient set-up,
               backward (decoder gradient, occurrence lists, row sums, GCN backward), update; the rest
               of the pass is the session's share (feeds, the cost's copy back) and, for the host-fed
               step, whose stages are taken the same way, pack_batches.
  (d) epoch    one whole epoch of each kind (EdgeBatches.steps steps; the edge types the reference
               wraps — (0,0), (0,1), (1,0) — wrap here too).

Whole passes are warmed up, then timed with a host clock around passes that end in a device
synchronise, alternating; medians and min..max spreads are reported.  Prints one JSON line and writes
it to --out (default profiles/epoch_bench.json).  Needs a HIP device: there is no CPU fallback."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms)),
            "all_ms": [round(float(x), 4) for x in ms]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=str, default="P", choices=["P", "S"])
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20, help="kernel launches between two events in (a)")
    ap.add_argument("--steps-per-round", type=int, default=3)
    ap.add_argument("--epoch-steps", type=int, default=0, help="cap on the steps of (d); 0: the whole epoch")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", type=str, default=str(ROOT / "profiles" / "epoch_bench.json"))
    a = ap.parse_args()

    import torch

    from decagon_amd import epochs, kernels, synthetic, trainall
    from train_all_bench import build_model

    if not torch.cuda.is_available():
        raise SystemExit("epoch_bench: no HIP device (timings are taken on the GPU only)")
    dev = torch.device("cuda")
    B = a.batch
    graph = synthetic.make_P(seed=0) if a.config == "P" else synthetic.load_S()
    dg, ph, model, opt, feed = build_model(graph, B)
    train = {et: {k: np.asarray(coo[0]) for k, coo in enumerate(rels)} for et, rels in graph.adj.items()}
    shapes = {et: tuple(int(s) for s in rels[0][2]) for et, rels in graph.adj.items()}
    wrap = [et for et in ((0, 0), (0, 1), (1, 0)) if et in graph.edge_types]
    t0 = time.perf_counter()
    eb = epochs.EdgeBatches(train, graph.edge_types, shapes, B, a.seed, dev, wrap=wrap)
    torch.cuda.synchronize()
    build_s = time.perf_counter() - t0
    steps = eb.steps(0)
    n_edges = {str(et): int(te.ptr[-1]) for et, te in eb.types.items()}
    log(f"EdgeBatches: {sum(n_edges.values())} edges uploaded in {build_s:.2f} s; {steps} steps an epoch; "
        f"{len(eb.skipped)} relations skipped")
    res = {"bench": "epoch", "config": a.config, "batch": B, "rounds": a.rounds, "steps_per_epoch": steps,
           "edges": n_edges, "skipped_relations": len(eb.skipped), "wrapping": [list(et) for et in wrap],
           "edge_batches_build_s": build_s}
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)

    # ---------------------------------------------------------------- (a) the kernel alone
    et = (1, 1)
    te = eb.types[et]
    rel, seg2, rel2 = eb._meta(te, 0)
    n_seg = len(rel)
    edges_d, ptr_d, mask_d = te.dev
    rows = torch.empty(n_seg * B, device=dev, dtype=torch.int32)
    cols = torch.empty_like(rows)

    def launch(t):
        kernels.epoch_batch(edges_d, ptr_d, rel2[:n_seg], mask_d, B, t, 0, eb.seed, te.first_slot, te.shape[0],
                            rows=rows, cols=cols)

    for t in range(3):
        launch(t)
    torch.cuda.synchronize()
    ker = []
    for r in range(a.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for q in range(a.reps):
            launch(q % 3)  # (steps every relation still has a batch in)
        e1.record()
        torch.cuda.synchronize()
        ker.append(e0.elapsed_time(e1) / a.reps)
    pairs = n_seg * B
    res["kernel"] = {"edge_type": list(et), "segments": n_seg, "pairs": pairs, "launches_per_round": a.reps,
                     **stats(ker), "bytes_per_pair": 16,
                     "gather_GB_per_s": float(pairs * 16 / (np.median(ker) * 1e-3) / 1e9),
                     "pairs_per_s": float(pairs / (np.median(ker) * 1e-3))}
    log(f"(a) kernel: {np.median(ker) * 1e3:.1f} us for {pairs} pairs")
    out.write_text(json.dumps(res) + "\n")

    # ---------------------------------------------------------------- (b) the step, device-fed against host-fed
    sess = dg.Session()
    n_timed = a.rounds * a.steps_per_round
    ts = [q % max(1, min(steps, 3)) for q in range(n_timed + 1)]
    t0 = time.perf_counter()
    host_batches = {t: eb.host_batch(0, t) for t in sorted(set(ts))}
    host_batch_ms = 1e3 * (time.perf_counter() - t0) / len(host_batches)
    n_rel = sum(len(v) for v in host_batches[0].values())

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    dev_step = lambda t: trainall.train_step_all(sess, opt, ph, feed, eb.batch(0, t))  # noqa: E731
    host_step = lambda t: trainall.train_step_all(sess, opt, ph, feed, host_batches[t])  # noqa: E731
    t0 = time.perf_counter()
    c0 = dev_step(ts[-1])
    log(f"(b) first device-fed step {time.perf_counter() - t0:.1f} s (builds the plans), cost {c0:.4f}")
    host_step(ts[-1])
    tt = {"device_fed": [], "host_fed": []}
    q = 0
    for r in range(a.rounds):
        for _ in range(a.steps_per_round):
            t = ts[q]
            q += 1
            tt["device_fed"].append(timed(lambda: dev_step(t)))
            tt["host_fed"].append(timed(lambda: host_step(t)))
        log(f"(b) round {r}: {tt['device_fed'][-1]:.2f} ms against {tt['host_fed'][-1]:.2f} ms")
    d_med, h_med = np.median(tt["device_fed"]), np.median(tt["host_fed"])
    res["step"] = {"relations": n_rel, "pairs": n_rel * B, "device_fed": stats(tt["device_fed"]),
                   "host_fed": stats(tt["host_fed"]), "ratio": float(h_med / d_med),
                   "outside_host_spread": bool(max(tt["device_fed"]) < min(tt["host_fed"])),
                   "host_batch_build_ms_not_timed": host_batch_ms,
                   "negatives": "device-drawn on both sides", "adam_updates_per_step": 1}
    out.write_text(json.dumps(res) + "\n")

    # ---------------------------------------------------------------- (c) the stages of the device-fed step
    # (the host-fed step's too: its stages are the device-fed step's; pack_batches and the upload precede the
    # run and fall to the remainder)
    for kind in ("device_fed", "host_fed"):
        acc, totals, form = {}, [], []
        for r in range(a.rounds):
            t = ts[r]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            b = eb.batch(0, t) if kind == "device_fed" else host_batches[t]
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            trainall.stage_log = {}
            trainall.train_step_all(sess, opt, ph, feed, b)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            log_, trainall.stage_log = trainall.stage_log, None
            form.append(1e3 * (t1 - t0))
            totals.append(1e3 * (t2 - t0))
            for k, v in log_.items():
                acc.setdefault(k, []).append(v)
        st = {k: float(np.median(v)) for k, v in acc.items()}
        if kind == "device_fed":
            st["batch_formation"] = float(np.median(form))
        st["packing_session_and_cost_readback"] = float(np.median(totals) - sum(st.values()))
        key = "stages_ms" if kind == "device_fed" else "stages_host_fed_ms"
        res[key] = {"synchronised_pass_ms": float(np.median(totals)), **st}
        log(f"(c) stages, {kind}: " + ", ".join(f"{k} {v:.2f}" for k, v in res[key].items()))
    out.write_text(json.dumps(res) + "\n")

    # ---------------------------------------------------------------- (d) one epoch of each kind
    n_ep = steps if a.epoch_steps <= 0 else min(steps, a.epoch_steps)
    t0 = time.perf_counter()
    ep_host = [eb.host_batch(1, t) for t in range(n_ep)]
    ep_build_s = time.perf_counter() - t0

    def dev_epoch():
        for t in range(n_ep):
            trainall.train_step_all(sess, opt, ph, feed, eb.batch(1, t))

    def host_epoch():
        for t in range(n_ep):
            trainall.train_step_all(sess, opt, ph, feed, ep_host[t])

    trained = sum(len(b) for hb in ep_host for per in hb.values() for b in per.values())
    e_dev, e_host = timed(dev_epoch), timed(host_epoch)
    res["epoch"] = {"steps": n_ep, "whole_epoch": bool(n_ep == steps), "trained_edges": int(trained),
                    "device_fed_ms": e_dev, "host_fed_ms": e_host, "ratio": float(e_host / e_dev),
                    "device_fed_edges_per_s": float(trained / (e_dev * 1e-3)),
                    "host_fed_edges_per_s": float(trained / (e_host * 1e-3)),
                    "host_batches_build_s_not_timed": ep_build_s}
    log(f"(d) epoch of {n_ep} steps: {e_dev:.0f} ms against {e_host:.0f} ms")
    out.write_text(json.dumps(res) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

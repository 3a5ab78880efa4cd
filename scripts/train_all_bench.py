#!/usr/bin/env python
"""Training on every relation's batch in one step, measured against one step per relation.

  (a) decoder  the decoder backward alone at config P's drug×drug shape (645 drugs, 1,928 DEDICOM
               relations, 512 pairs each, d = 32; synthetic l2-normalised embeddings):
                 segmented  kernels.PreparedDecoderGradSeg + the two node-major occurrence lists
                            (stable device sorts) + two kernels.segment_rows_sum into dE
                 loop       what the package offered before, to the same accumulated dE and
                            decoder gradients: per relation kernels.PreparedDecoderGrad + two
                            kernels.scatter_rows, the shared R's gradient added up
               Both sides get the same fed negatives and the same scores; their results are
               compared at the timed size.  The segmented side's stages are timed too, and its
               kernels are set against two floors: the derived traffic (3 gathered rows read and 3
               gradient-row passes written or re-read per pair, P·d·4 bytes each) at the measured
               HBM rate, and the MFMA count (d/2 v_mfma_f32_32x32x2_f32 of 64 cycles per product
               and 32-pair tile; 1,024 SIMDs at 2.4 GHz).
  (b) step     through the drop-in surface (Session, DecagonModel, DecagonOptimizer), config P and
               config S: one trainall.train_step_all over a batch of EVERY relation of every edge
               type, against one `opt_op` step per relation over the same batches, both with
               device-drawn negatives.  Reported as trained edges per second.  The two differ in
               the number of Adam updates: 1 against one per relation.

Whole passes are warmed up, then timed with a host clock around passes that end in a device
synchronise, alternating, --rounds rounds; medians and min..max spreads are reported.  Prints one
JSON line and writes it to --out (default profiles/train_all_bench.json).  Needs a HIP device:
there is no CPU fallback."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

HBM_BYTES_PER_S = 6.29e12   # measured float4 copy rate of the MI355X
MFMA_CYCLES, SIMDS, CLOCK = 64.0, 1024, 2.4e9


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms)),
            "all_ms": [round(float(x), 4) for x in ms]}


def decoder_part(a, torch, kernels, dev):
    N, K, d, B = a.drugs, a.relations, a.d, a.batch
    rng = np.random.default_rng(a.seed)
    E = torch.from_numpy(rng.uniform(-1, 1, (N, d)).astype(np.float32)).to(dev)
    E = (E / E.norm(dim=1, keepdim=True)).contiguous()
    lim = np.sqrt(6.0 / (2 * d))
    G = torch.from_numpy(rng.uniform(-lim, lim, (d, d)).astype(np.float32)).to(dev)
    L = torch.from_numpy(rng.uniform(-1, 1, (K, d)).astype(np.float32)).to(dev)
    P = K * B
    host = rng.integers(0, N, (3, P)).astype(np.int32)
    buf = torch.from_numpy(host).to(dev)
    rows, cols, negs = buf[0], buf[1], buf[2]
    seg_ptr = torch.arange(0, P + 1, B, dtype=torch.int32, device=dev)
    seg2 = torch.arange(0, 2 * P + 1, B, dtype=torch.int32, device=dev)
    rel2 = torch.arange(K, dtype=torch.int32, device=dev).repeat(2)
    scores = kernels.decoder_score_seg(E, E, torch.cat([rows, negs]), torch.cat([cols, cols]), seg2, G, L, seg_rel=rel2)
    pos, neg = scores[:P].contiguous(), scores[P:].contiguous()
    margin = 0.1
    active = float(((neg - (pos - margin)) > 0).float().mean())

    dE = torch.zeros((N, d), device=dev)
    dG, dl = torch.zeros(d * d, device=dev), torch.zeros(K * d, device=dev)

    def segmented(marks=None):
        def mark():
            if marks is not None:
                e = torch.cuda.Event(enable_timing=True)
                e.record()
                marks.append(e)
        dE.zero_(), dG.zero_(), dl.zero_()
        mark()
        op = kernels.PreparedDecoderGradSeg(E, E, rows, cols, negs, seg_ptr, None, pos, neg, G, L, margin, dG=dG, dl=dl)
        op()
        mark()
        node_ptr, order = kernels.occurrence_list(torch.cat([rows, negs]), N)
        sign = torch.where(order < P, -1.0, 1.0).to(torch.float32)
        item = torch.remainder(order, P).to(torch.int32)
        cptr, corder = kernels.occurrence_list(cols, N)
        mark()
        kernels.segment_rows_sum(node_ptr, item, op.mv, dE, sign=sign)
        kernels.segment_rows_sum(cptr, corder, op.grad_cols, dE)
        mark()
        return dE, dG, dl

    bE = torch.zeros((N, d), device=dev)
    bG, bGk, bl = torch.zeros(d * d, device=dev), torch.zeros(d * d, device=dev), torch.zeros(K * d, device=dev)

    def loop():
        bE.zero_(), bG.zero_(), bl.zero_()
        for k in range(K):
            s = slice(k * B, (k + 1) * B)
            op = kernels.PreparedDecoderGrad(E, E, rows[s], cols[s], negs[s], pos[s], neg[s], G, L[k], margin,
                                             dG=bGk, dl=bl[k * d:(k + 1) * d])
            op()
            kernels.scatter_rows(op.row_idx, op.grad_rows, bE)
            kernels.scatter_rows(cols[s], op.grad_cols, bE)
            bG.add_(bGk)
        return bE, bG, bl

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    log("decoder part: warm-up")
    x, y = segmented(), loop()
    torch.cuda.synchronize()
    err = {nm: float((u.double() - v.double()).abs().max() / v.double().abs().max())
           for nm, u, v in zip(("dE", "dG", "dl"), x, y)}
    t = {"segmented": [], "loop": []}
    stages = []
    for r in range(a.rounds):
        t["segmented"].append(timed(segmented))
        t["loop"].append(timed(loop))
        marks = []
        segmented(marks)
        torch.cuda.synchronize()
        stages.append([marks[i].elapsed_time(marks[i + 1]) for i in range(3)])
        log(f"decoder part: round {r}: {t['segmented'][-1]:.3f} ms against {t['loop'][-1]:.1f} ms")
    st = np.median(np.array(stages), axis=0)
    tiles = -(-B // 32) * K
    mfma = tiles * ((d // 32) * (d // 2) * 2 + (d // 32) ** 2 * 16)
    floor_mfma = 1e3 * mfma * MFMA_CYCLES / (SIMDS * CLOCK)
    unit = P * d * 4
    floor_bytes = 1e3 * 6 * unit / HBM_BYTES_PER_S
    chunk, waves = kernels.segment_rows_chunk()
    return {
        "drugs": N, "relations": K, "batch": B, "d": d, "pairs": P, "active_fraction": active,
        "segmented": stats(t["segmented"]), "loop": stats(t["loop"]),
        "speedup": float(np.median(t["loop"]) / np.median(t["segmented"])),
        "segmented_stage_ms": {"gradient_launches": float(st[0]), "occurrence_lists": float(st[1]),
                               "row_sums": float(st[2])},
        "row_sum_chunk": chunk, "row_sum_waves": waves,
        "traffic_bytes_derived": 6 * unit, "traffic_floor_ms": floor_bytes,
        "mfma_count": int(mfma), "mfma_floor_ms": floor_mfma,
        "kernels_over_floor": float((st[0] + st[2]) / max(floor_bytes, floor_mfma)),
        "max_rel_difference_against_loop": err,
    }


def build_model(graph, batch):
    import decagon_amd as dg

    n = graph.n_nodes
    ph = dg.construct_placeholders(graph.edge_types)
    model = dg.DecagonModel(placeholders=ph, num_feat=n, nonzero_feat=n, edge_types=graph.edge_types,
                            decoders=graph.decoders)
    dims = {et: [tuple(int(s) for s in c[2]) for c in rels] for et, rels in graph.adj.items()}
    opt = dg.DecagonOptimizer(embeddings=model.embeddings, latent_inters=model.latent_inters,
                              latent_varies=model.latent_varies, degrees=graph.degrees, edge_types=graph.edge_types,
                              edge_type2dim=dims, placeholders=ph, batch_size=batch, margin=0.1)
    feed = {}
    for (i, j), rels in graph.adj.items():
        for k, coo in enumerate(rels):
            feed[ph["adj_mats_%d,%d,%d" % (i, j, k)]] = (coo[0], coo[1], tuple(int(s) for s in coo[2]))
    for t in n:
        feed[ph["feat_%d" % t]] = (np.stack([np.arange(n[t])] * 2, 1), np.ones(n[t]), (n[t], n[t]))
    feed[ph["dropout"]] = 0.0
    return dg, ph, model, opt, feed


def step_part(a, torch, config):
    from decagon_amd import synthetic
    from decagon_amd.trainall import train_step_all

    graph = synthetic.make_P(seed=0) if config == "P" else synthetic.load_S()
    B = a.batch
    dg, ph, model, opt, feed = build_model(graph, B)
    rng = np.random.default_rng(a.seed)
    batches = {}
    for et, rels in graph.adj.items():
        batches[et] = {}
        for k, coo in enumerate(rels):
            c = np.asarray(coo[0])
            batches[et][k] = c[rng.choice(len(c), B, replace=len(c) < B)].astype(np.int64)
    n_rel = sum(len(v) for v in batches.values())
    sess = dg.Session()

    def all_step():
        return train_step_all(sess, opt, ph, feed, batches)

    def sweep():
        e = 0
        for (i, j), per in batches.items():
            for k, b in per.items():
                f = dict(feed)
                f.update({ph["batch"]: b, ph["batch_edge_type_idx"]: e, ph["batch_row_edge_type"]: i,
                          ph["batch_col_edge_type"]: j})
                sess.run(opt.opt_op, feed_dict=f)
                e += 1

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    log(f"step part {config}: {n_rel} relations; warm-up (builds the plans)")
    t0 = time.perf_counter()
    cost0 = all_step()
    log(f"step part {config}: first all-relation step {time.perf_counter() - t0:.1f} s, cost {cost0:.4f}")
    t0 = time.perf_counter()
    sweep()
    log(f"step part {config}: first sweep {time.perf_counter() - t0:.1f} s")
    t = {"all_relations_step": [], "per_relation_sweep": []}
    for r in range(a.rounds if config == "S" else a.step_rounds):
        for _ in range(a.steps_per_round):
            t["all_relations_step"].append(timed(all_step))
        t["per_relation_sweep"].append(timed(sweep))
        log(f"step part {config}: round {r}: {t['all_relations_step'][-1]:.2f} ms against "
            f"{t['per_relation_sweep'][-1]:.1f} ms")
    edges = n_rel * B
    one, many = np.median(t["all_relations_step"]), np.median(t["per_relation_sweep"])
    return {
        "config": config, "relations": n_rel, "batch": B, "trained_edges_per_pass": edges,
        "all_relations_step": stats(t["all_relations_step"]), "per_relation_sweep": stats(t["per_relation_sweep"]),
        "all_relations_edges_per_s": float(edges / (one * 1e-3)),
        "per_relation_edges_per_s": float(edges / (many * 1e-3)),
        "ratio": float(many / one),
        "adam_updates": {"all_relations_step": 1, "per_relation_sweep": n_rel},
        "negatives": "device-drawn on both sides",
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--drugs", type=int, default=645)
    ap.add_argument("--relations", type=int, default=1928)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--d", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--step-rounds", type=int, default=3, help="rounds of the config P step comparison")
    ap.add_argument("--steps-per-round", type=int, default=3, help="all-relation steps timed per round")
    ap.add_argument("--parts", type=str, default="decoder,S,P")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", type=str, default=str(ROOT / "profiles" / "train_all_bench.json"))
    a = ap.parse_args()

    import torch

    from decagon_amd import kernels

    if not torch.cuda.is_available():
        raise SystemExit("train_all_bench: no HIP device (timings are taken on the GPU only)")
    dev = torch.device("cuda")
    res = {"bench": "train_all", "rounds": a.rounds}
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    for part in a.parts.split(","):
        if part == "decoder":
            res["decoder_backward"] = decoder_part(a, torch, kernels, dev)
        else:
            res["step_" + part] = step_part(a, torch, part)
        out.write_text(json.dumps(res) + "\n")  # (kept after every part)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

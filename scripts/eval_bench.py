#!/usr/bin/env python
"""Link-prediction evaluation of every relation of config P's drug×drug edge type
(decagon_amd/synthetic.py: 645 drugs, 964 Zipf-sized symmetric relations + their transposes =
1,928 relation slots, DEDICOM), d = 32, k = 50.  Per relation 10 % of its edges are the positives
and as many uniform pairs the negatives.

  fused     what evaluate.accuracy_scores_all runs after its forward pass: one upload of the
            packed indices, kernels.decoder_score_seg over the 2·K segments,
            evaluate.rank_metrics_seg_device, one copy back
  baseline  the per-relation loop the package offered before (evaluate.accuracy_scores after its
            forward pass), per relation: four index uploads, two kernels.decoder_score,
            evaluate.rank_metrics_device, .cpu()

Whole passes are warmed up, timed with device events around passes that end with the results on
the host, alternating, and the two results are compared for equality (bit for bit) at the timed
size.  The fused pass's stages are timed as well (events between them).  Prints one JSON line (and
writes it to --out).  Needs a HIP device: there is no CPU fallback."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--drugs", type=int, default=645)
    ap.add_argument("--side-effects", type=int, default=964)
    ap.add_argument("--d", type=int, default=32)
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--fraction", type=float, default=0.1, help="share of a relation's edges sampled as positives")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--fused-reps", type=int, default=10, help="fused passes per round")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()

    import torch

    from decagon_amd import evaluate, kernels, synthetic

    N, d, k = a.drugs, a.d, a.k
    rng = np.random.default_rng(a.seed)
    rels = [synthetic._sym_relation(rng, N, max(500, int(28568 * r ** -0.31))) for r in range(1, a.side_effects + 1)]
    rels = rels + rels  # the transposed copies of symmetric relations (synthetic.make_P)
    K = len(rels)
    pos, neg = {}, {}
    for r, m in enumerate(rels):
        co = m.tocoo()
        n = max(1, int(a.fraction * co.nnz))
        pick = rng.choice(co.nnz, n, replace=False)
        pos[r] = np.stack([co.row[pick], co.col[pick]], 1).astype(np.int64)
        neg[r] = rng.integers(0, N, (n, 2))
    edges_pos, edges_neg = {(1, 1): pos}, {(1, 1): neg}
    if not torch.cuda.is_available():
        raise SystemExit("eval_bench: no HIP device (timings are taken on the GPU only)")
    dev = torch.device("cuda")
    lim = np.sqrt(6.0 / (N + d))
    E = torch.from_numpy(rng.uniform(-1, 1, (N, d)).astype(np.float32)).to(dev)
    E = E / E.norm(dim=1, keepdim=True)  # the model's embeddings are l2-normalised rows
    G = torch.from_numpy(rng.uniform(-lim, lim, (d, d)).astype(np.float32)).to(dev)
    L = torch.from_numpy(rng.uniform(-1, 1, (K, d)).astype(np.float32)).to(dev)

    ri, ci, pos_ptr, neg_ptr, rel = evaluate.pack_edge_samples(edges_pos, edges_neg, (1, 1), K, (N, N))
    P, Nn = int(pos_ptr[-1]), int(neg_ptr[-1])
    host = np.concatenate([ri, ci, pos_ptr, P + neg_ptr[1:], rel, rel, neg_ptr]).astype(np.int32)

    def fused(marks=None):
        def mark():
            if marks is not None:
                e = torch.cuda.Event(enable_timing=True)
                e.record()
                marks.append(e)

        mark()
        buf = torch.from_numpy(host).to(dev)
        n = P + Nn
        o = 2 * n
        d_seg, d_rel, d_neg = buf[o:o + 2 * K + 1], buf[o + 2 * K + 1:o + 4 * K + 1], buf[o + 4 * K + 1:]
        mark()
        s = kernels.decoder_score_seg(E, E, buf[:n], buf[n:o], d_seg, G, L, seg_rel=d_rel)
        mark()
        m = evaluate.rank_metrics_seg_device(s[:P], d_seg[:K + 1], s[P:], d_neg, k, "main")
        mark()
        out = m.cpu().numpy()
        mark()
        return out

    def baseline():
        out = np.empty((K, 3))
        for r in range(K):
            sc = []
            for e in (pos[r], neg[r]):
                rd = torch.from_numpy(e[:, 0].astype(np.int32)).to(dev)
                cd = torch.from_numpy(e[:, 1].astype(np.int32)).to(dev)
                sc.append(kernels.decoder_score(E, E, rd, cd, G, L[r]))
            out[r] = evaluate.rank_metrics_device(sc[0], sc[1], k, "main").cpu().numpy()
        return out

    def timed(fn, reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(reps):
            out = fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / reps, out

    # warm-up of both, and the comparison at the timed size
    for _ in range(2):
        f = fused()
    b = baseline()
    torch.cuda.synchronize()
    identical = bool(np.array_equal(f.view(np.uint64), b.view(np.uint64)))
    assert identical, "fused and per-relation metrics differ"

    t_f, t_b, stages = [], [], []
    for _ in range(a.rounds):  # alternate the variants
        t_f.append(timed(fused, a.fused_reps)[0])
        t_b.append(timed(baseline, 1)[0])
        marks = []
        fused(marks)
        torch.cuda.synchronize()
        stages.append([marks[i].elapsed_time(marks[i + 1]) for i in range(4)])
    st = np.median(np.array(stages), axis=0)
    res = {
        "bench": "eval", "drugs": N, "relations": K, "d": d, "k": k, "positives": P, "negatives": Nn,
        "largest_relation_positives": int(np.diff(pos_ptr).max()),
        "fused_ms": float(np.median(t_f)), "fused_ms_all": [round(x, 4) for x in t_f],
        "baseline_ms": float(np.median(t_b)), "baseline_ms_all": [round(x, 3) for x in t_b],
        "speedup": float(np.median(t_b) / np.median(t_f)),
        "fused_stage_ms": {"upload": float(st[0]), "scorer": float(st[1]), "metrics": float(st[2]),
                           "copy_back": float(st[3])},
        "identical_bits": identical, "mean_auroc": float(np.nanmean(f[:, 0])),
        "pooled_measured": False,
    }
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""Top-k candidate ranking at config P's drug×drug shape (decagon_amd/synthetic.py: 645 drugs,
964 Zipf-sized symmetric relations + their transposes = 1,928 relation slots, DEDICOM), d = 32,
k = 50, all relations:

  fused     kernels.decoder_topk — one call, no N×N matrix (with and without the training
            adjacency as the exclusion set)
  baseline  what the package offered before: per relation runtime.full_scores (two fp32 GEMMs,
            the 645×645 matrix written to memory) + torch.topk on the flattened matrix

Both are warmed up, timed with device events around whole passes that end in a synchronise,
alternating, and the fused result is compared with the baseline's at the timed size.  Prints one
JSON line (and writes it to --out).  Needs a HIP device: there is no CPU fallback."""
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
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--fused-reps", type=int, default=20, help="fused calls per round")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()

    import torch

    from decagon_amd import _lib, kernels, runtime, synthetic
    from decagon_amd.sparse import exclusion_csr

    N, d, k = a.drugs, a.d, a.k
    rng = np.random.default_rng(a.seed)
    rels = [synthetic._sym_relation(rng, N, max(500, int(28568 * r ** -0.31))) for r in range(1, a.side_effects + 1)]
    rels = rels + rels  # the transposed copies of symmetric relations (synthetic.make_P)
    K = len(rels)
    ex = exclusion_csr(rels, (N, N))
    if not torch.cuda.is_available():
        raise SystemExit("topk_bench: no HIP device (timings are taken on the GPU only)")
    dev = torch.device("cuda")
    ex_dev = (torch.from_numpy(ex.rowptr).to(dev), torch.from_numpy(ex.col).to(dev))
    lim = np.sqrt(6.0 / (N + d))
    E = torch.from_numpy(rng.uniform(-1, 1, (N, d)).astype(np.float32)).to(dev)
    E = E / E.norm(dim=1, keepdim=True)  # the model's embeddings are l2-normalised rows
    G = torch.from_numpy(rng.uniform(-lim, lim, (d, d)).astype(np.float32)).to(dev)
    L = torch.from_numpy(rng.uniform(-1, 1, (K, d)).astype(np.float32)).to(dev)

    def fused(exclude=None):
        return kernels.decoder_topk(E, E, G, L, k, exclude=exclude)

    def baseline():
        vals = torch.empty((K, k), device=dev)
        idx = torch.empty((K, k), device=dev, dtype=torch.int64)
        for r in range(K):
            S = runtime.full_scores(E, E, G, L[r])
            v, i = torch.topk(S.view(-1), k)
            vals[r], idx[r] = v, i
        return vals, idx

    def timed(fn, reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(reps):
            out = fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / reps, out

    # warm-up of every timed shape, and the comparison at the timed size
    for _ in range(2):
        f = fused()
        fx = fused(ex_dev)
    bv, bi = baseline()
    torch.cuda.synchronize()
    fs = f[0].cpu().numpy().astype(np.float64)
    bs = bv.cpu().numpy().astype(np.float64)
    worst = float(np.max(np.abs(fs - bs) - (1e-4 * np.abs(bs) + 1e-6)))
    same_pairs = float(np.mean((f[1].long() * N + f[2].long()).cpu().numpy() == bi.cpu().numpy()))
    assert int(f[3].min()) == k and worst <= 0, f"fused and baseline top-k scores differ: {worst}"

    t_f, t_fx, t_b = [], [], []
    for _ in range(a.rounds):  # alternate the variants
        t_f.append(timed(fused, a.fused_reps)[0])
        t_fx.append(timed(lambda: fused(ex_dev), a.fused_reps)[0])
        t_b.append(timed(baseline, 1)[0])

    ws = int(_lib.load().dg_decoder_topk_workspace(K, N, N, k))  # the per-wave lists: written, then merged
    fused_bytes = 2 * N * d * 4 + d * d * 4 + K * d * 4 + 2 * ws + K * (3 * k + 1) * 4
    # per relation: T = (E∘l)·G written and read back, the N×N scores written, then read by topk
    base_bytes = K * (2 * N * d * 4 + d * d * 4 + d * 4 + 2 * N * d * 4 + 2 * N * N * 4 + k * 12)
    flops = K * (2.0 * N * N * d + 2.0 * N * d * d)
    res = {
        "bench": "topk", "drugs": N, "relations": K, "d": d, "k": k, "exclusion_nnz": ex.nnz,
        "fused_ms": float(np.median(t_f)), "fused_ms_all": [round(x, 4) for x in t_f],
        "fused_excl_ms": float(np.median(t_fx)), "fused_excl_ms_all": [round(x, 4) for x in t_fx],
        "baseline_ms": float(np.median(t_b)), "baseline_ms_all": [round(x, 3) for x in t_b],
        "speedup": float(np.median(t_b) / np.median(t_f)),
        "fused_algorithmic_bytes": int(fused_bytes), "baseline_algorithmic_bytes": int(base_bytes),
        "score_flops": flops, "fused_tflops": flops / (np.median(t_f) * 1e-3) / 1e12,
        "fused_vs_baseline_worst_excess_over_tol": worst, "identical_pair_fraction": same_pairs,
    }
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()

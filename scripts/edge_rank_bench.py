#!/usr/bin/env python
"""The filtered rank of held-out edges (kernels.decoder_edge_rank / dg_decoder_edge_rank_f32), d = 32,
at two shapes:

  drug_drug   config P's drug×drug (decagon_amd/synthetic.py: 645 drugs, 1,928 DEDICOM relation
              slots): a held-out tenth of every relation's edges, both directions, ranked among the
              row's columns outside the relation's adjacency
  long_walk   one relation over 19,081 nodes (P's protein×protein size; its adjacency the
              exclusion) with 4,096 queries: few query tiles against a long column range — the
              case that decides whether the column range is split over workgroups

  fused     what evaluate.edge_ranks runs after its forward pass, per side: one upload of
            [row_idx | col_idx | seg_ptr | seg_rel], one launch, one copy back of rank, score, cand
  no_split  (long_walk) the same with every query tile's columns in one workgroup
  route     what a caller had before, on the device in torch: per relation the N_i×N_j fp32 score
            matrix by matmul, a dense mask from the exclusion, a gather of the true scores, then
            compare and count; one copy back at the end
  mask      the route's dense masks alone (they are part of `route`)

Whole passes are warmed up, then timed (host clock around passes that end with the results on the
host and the device idle), the variants alternating and each round starting with another,
--rounds rounds: median and min – max.  The exclusion's host build and its upload are paid once per
training set and are reported apart.  The kernel alone (device events) is set against its MFMA
floor: ⌈queries/32⌉·⌈N_j/32⌉·d/2 v_mfma_f32_32x32x2_f32 of 64 cycles each on 1,024 SIMDs at 2.4 GHz.
Prints one JSON line (and writes it to --out).  Needs a HIP device: there is no CPU fallback."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

SIMDS, CLOCK_HZ, MFMA_CYCLES = 1024, 2.4e9, 64  # the floor's yardstick: the MI355X's specified figures


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--nodes", type=int, default=19081)
    ap.add_argument("--queries", type=int, default=4096)
    ap.add_argument("--shapes", type=str, default="drug_drug,long_walk")
    ap.add_argument("--out", type=str, default=str(Path(__file__).resolve().parents[1] / "profiles" / "edge_rank_bench.json"))
    a = ap.parse_args()

    import torch

    from decagon_amd import kernels, sparse, synthetic

    if not torch.cuda.is_available():
        raise SystemExit("edge_rank_bench: no HIP device (timings are taken on the GPU only)")
    d = a.d
    rng = np.random.default_rng(a.seed)
    dev = torch.device("cuda")
    t0 = time.perf_counter()
    P = synthetic.make_P(a.seed)
    graph_s = time.perf_counter() - t0

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t), out

    def event_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def stats(v):
        return {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v)),
                "all_ms": [round(float(x), 4) for x in v]}

    def shape(name, N, rel_edges, G, L, with_no_split):
        """rel_edges: per relation the [nnz, 2] edges (the exclusion); the queries are drawn from them."""
        K = len(rel_edges)
        lim = np.sqrt(6.0 / (N + d))
        E = torch.from_numpy(rng.uniform(-1, 1, (N, d)).astype(np.float32)).to(dev)
        E = E / E.norm(dim=1, keepdim=True)  # the model's embeddings are l2-normalised rows
        Gd = torch.from_numpy(rng.uniform(-lim, lim, G).astype(np.float32)).to(dev)
        Ld = torch.from_numpy(rng.uniform(-1, 1, L).astype(np.float32)).to(dev) if L else None
        t0 = time.perf_counter()
        csr = sparse.exclusion_csr(rel_edges, (N, N))
        csr_s = time.perf_counter() - t0
        upload_ms, ex = timed(lambda: (torch.from_numpy(csr.rowptr).to(dev), torch.from_numpy(csr.col).to(dev)))
        # the route's view of the same sets: the stacked row of every entry, for the dense masks
        ex_row = torch.repeat_interleave(torch.arange(K * N, device=dev), (ex[0][1:] - ex[0][:-1]).long()) % N
        ex_col = ex[1].long()
        rel_lo = csr.rowptr[::N].astype(np.int64)  # entries [rel_lo[k], rel_lo[k+1]) are relation k's
        return dict(name=name, N=N, K=K, E=E, G=Gd, L=Ld, ex=ex, ex_row=ex_row, ex_col=ex_col, rel_lo=rel_lo,
                    csr_s=csr_s, upload_ms=upload_ms, nnz=int(csr.nnz), with_no_split=with_no_split)

    def queries_tenth(rel_edges):
        """A tenth of every relation's undirected edges (r < c), both directions, packed by relation."""
        parts, lens = [], []
        for e in rel_edges:
            und = e[e[:, 0] < e[:, 1]]
            pick = und[rng.choice(len(und), max(1, len(und) // 10), replace=False)]
            parts.append(np.concatenate([pick, pick[:, ::-1]]))
            lens.append(2 * len(pick))
        return np.concatenate(parts).astype(np.int32), np.asarray(lens, np.int64)

    def measure(s, q, lens):
        N, K, E, G, L, ex = s["N"], s["K"], s["E"], s["G"], s["L"], s["ex"]
        n = q.shape[0]
        ptr = np.zeros(K + 1, np.int64)
        np.cumsum(lens, out=ptr[1:])
        host = np.concatenate([q[:, 0], q[:, 1], ptr, np.arange(K)]).astype(np.int32)
        col = torch.arange(N, device=dev)

        def fused(split=True):
            buf = torch.from_numpy(host).to(dev)
            rank, score, cand = kernels.decoder_edge_rank(E, E, buf[:n], buf[n:2 * n], buf[2 * n:2 * n + K + 1], G, L,
                                                          seg_rel=buf[2 * n + K + 1:], exclude=ex, column_split=split)
            return torch.cat([rank, score.view(torch.int32), cand]).cpu().numpy().reshape(3, n)

        def route(mask_only=False):
            buf = torch.from_numpy(host).to(dev).long()
            mask = torch.empty((N, N), dtype=torch.bool, device=dev)
            out = []
            for k in range(K):
                lo, hi = s["rel_lo"][k], s["rel_lo"][k + 1]
                mask.zero_()
                mask[s["ex_row"][lo:hi], s["ex_col"][lo:hi]] = True
                if mask_only or ptr[k] == ptr[k + 1]:
                    continue
                rq, cq = buf[ptr[k]:ptr[k + 1]], buf[n + ptr[k]:n + ptr[k + 1]]
                Gk = G[k] if G.dim() == 3 else G
                A = E * L[k] if L is not None else E
                S = (A @ Gk) @ A.T
                rows, others = S[rq], ~mask[rq]
                others.scatter_(1, cq[:, None], False)
                true = rows.gather(1, cq[:, None])
                before = (rows > true) | ((rows == true) & (col[None, :] < cq[:, None]))
                out.append(torch.stack([1 + (before & others).sum(1), 1 + others.sum(1)]))
            return None if mask_only else torch.cat(out, 1).cpu().numpy()

        variants = [("fused", fused), ("route", route), ("mask", lambda: route(True))]
        if s["with_no_split"]:
            variants.insert(1, ("no_split", lambda: fused(False)))
        f, r = fused(), route()  # a warm pass of each, and the comparison
        route(True)
        assert np.array_equal(f[2], r[1]), "the fused call and the route count different candidates"
        same = float(np.mean(f[0] == r[0]))  # (the route's matmul rounds differently: near-ties may swap)
        within_1 = float(np.mean(np.abs(f[0] - r[0]) <= 1))
        if s["with_no_split"]:
            assert fused(False).tobytes() == f.tobytes(), "the split changes the result"
        t = {nm: [] for nm, _ in variants}
        for rnd in range(a.rounds):  # alternate the variants, each round starting with another
            m = rnd % len(variants)
            for nm, fn in variants[m:] + variants[:m]:
                t[nm].append(timed(fn)[0])

        # the kernel alone, on device-resident indices
        buf = torch.from_numpy(host).to(dev)
        call = lambda split: kernels.decoder_edge_rank(E, E, buf[:n], buf[n:2 * n], buf[2 * n:2 * n + K + 1], G, L,  # noqa: E731
                                                       seg_rel=buf[2 * n + K + 1:], exclude=ex, column_split=split)
        kern = {nm: [] for nm in (("split", "no_split") if s["with_no_split"] else ("split",))}
        for nm in kern:
            call(nm == "split")
        for _ in range(a.rounds):
            for nm in kern:
                kern[nm].append(event_ms(lambda: call(nm == "split")))
        tiles = int(sum(-(-int(x) // 32) for x in lens))
        mfma = tiles * -(-N // 32) * (d // 2)
        floor_ms = 1e3 * mfma * MFMA_CYCLES / SIMDS / CLOCK_HZ
        med = {nm: float(np.median(v)) for nm, v in t.items()}
        return {"shape": s["name"], "nodes": N, "relations": K, "queries": int(n), "query_tiles": tiles,
                "column_tiles": -(-N // 32), "exclusion_entries": s["nnz"], "exclusion_csr_host_s": s["csr_s"],
                "exclusion_upload_ms": s["upload_ms"], "mean_rank": float(f[0].mean()), "mean_candidates": float(f[1 + 1].mean()),
                "ranks_equal_to_route": same, "ranks_within_1_of_route": within_1,
                **{nm: stats(v) for nm, v in t.items()}, "route_over_fused": med["route"] / med["fused"],
                "kernel": {nm: stats(v) for nm, v in kern.items()}, "mfma_instructions": mfma, "mfma_floor_ms": floor_ms,
                "kernel_fraction_of_floor": floor_ms / float(np.median(kern["split"]))}

    shapes = []
    for nm in a.shapes.split(","):
        if nm == "drug_drug":
            adj = P.adj[1, 1]
            rel_edges = [np.asarray(c[0], np.int64) for c in adj]
            N, K = int(adj[0][2][0]), len(adj)
            s = shape(nm, N, rel_edges, (d, d), (K, d), False)  # DEDICOM: a shared R, one diagonal per relation
            q, lens = queries_tenth(rel_edges)
        elif nm == "long_walk":
            e = np.asarray(P.adj[0, 0][0][0], np.int64)
            e = e[(e[:, 0] < a.nodes) & (e[:, 1] < a.nodes)]
            s = shape(nm, a.nodes, [e], (1, d, d), None, True)  # Bilinear: one dense G, no diagonal
            und = e[e[:, 0] != e[:, 1]]
            q = und[rng.choice(len(und), a.queries, replace=False)].astype(np.int32)
            lens = np.asarray([a.queries], np.int64)
        else:
            raise SystemExit(f"edge_rank_bench: unknown shape {nm}")
        shapes.append(measure(s, q, lens))
        del s
        torch.cuda.empty_cache()

    res = {"bench": "edge_rank", "d": d, "rounds": a.rounds, "synthetic_graph_s": graph_s,
           "floor": {"simds": SIMDS, "clock_hz": CLOCK_HZ, "cycles_per_mfma": MFMA_CYCLES}, "shapes": shapes}
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()

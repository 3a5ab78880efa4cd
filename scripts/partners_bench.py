#!/usr/bin/env python
"""A node's best partners per relation (kernels.decoder_node_topk / dg_decoder_node_topk_f32), d = 32,
at three shapes:

  drug_drug   config P's drug×drug (decagon_amd/synthetic.py: 645 drugs, 1,928 DEDICOM relation
              slots): every drug a query of every relation, k = 10, outside the relation's
              adjacency and without the drug itself
  one_rel     one relation over 19,081 nodes (P's protein×protein size; its adjacency the
              exclusion), every node a query, k = 50
  one_node    one drug against all 1,928 relations, k = 10 — the interactive query: every query
              tile holds one live row of 32

  fused     what evaluate.top_partners runs after its forward pass, per side: one upload of
            [node_idx | seg_ptr | seg_rel], one launch pair, one copy back of scores, partners, counts
  no_split  (one_rel) the same with every query tile's columns in one workgroup
  route     what a caller had before, on the device in torch: per relation the N_i×N_j fp32 score
            matrix by matmul, −inf where the exclusion says so, torch.topk of the wanted rows; one
            copy back at the end

Whole passes are warmed up, then timed (host clock around passes that end with the results on the
host and the device idle), the variants alternating and each round starting with another,
--rounds rounds: median and min – max.  The exclusion's host build and its upload are paid once per
training set and are reported apart.  The kernels alone (device events around the launch pair) are
set against the MFMA floor: ⌈queries/32⌉ per segment ·⌈N_j/32⌉·d/2 v_mfma_f32_32x32x2_f32 of 64
cycles each on 1,024 SIMDs at 2.4 GHz.  Prints one JSON line (and writes it to --out).  Needs a HIP
device: there is no CPU fallback."""
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
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--nodes", type=int, default=19081)
    ap.add_argument("--shapes", type=str, default="drug_drug,one_rel,one_node")
    ap.add_argument("--out", type=str, default=str(Path(__file__).resolve().parents[1] / "profiles" / "partners_bench.json"))
    a = ap.parse_args()

    import torch

    from decagon_amd import kernels, sparse, synthetic

    if not torch.cuda.is_available():
        raise SystemExit("partners_bench: no HIP device (timings are taken on the GPU only)")
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

    def shape(name, N, rel_edges, G, L):
        """rel_edges: per relation the [nnz, 2] edges (the exclusion)."""
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
        # the route's view of the same sets: the row of every entry, for the dense masks
        ex_row = torch.repeat_interleave(torch.arange(K * N, device=dev), (ex[0][1:] - ex[0][:-1]).long()) % N
        ex_col = ex[1].long()
        rel_lo = csr.rowptr[::N].astype(np.int64)  # entries [rel_lo[k], rel_lo[k+1]) are relation k's
        return dict(name=name, N=N, K=K, E=E, G=Gd, L=Ld, ex=ex, ex_row=ex_row, ex_col=ex_col, rel_lo=rel_lo,
                    csr_s=csr_s, upload_ms=upload_ms, nnz=int(csr.nnz))

    def measure(s, nodes, k, no_self, with_no_split):
        """nodes: the query nodes, the same for every relation."""
        N, K, E, G, L, ex = s["N"], s["K"], s["E"], s["G"], s["L"], s["ex"]
        m = nodes.size
        n = m * K
        ptr = m * np.arange(K + 1, dtype=np.int64)
        host = np.concatenate([np.tile(nodes, K), ptr, np.arange(K)]).astype(np.int32)
        diag = torch.arange(N, device=dev)

        def call(buf, split=True):
            return kernels.decoder_node_topk(E, E, buf[:n], buf[n:n + K + 1], G, L, k, seg_rel=buf[n + K + 1:],
                                             exclude=ex, no_self=no_self, column_split=split)

        def fused(split=True):
            score, col, count = call(torch.from_numpy(host).to(dev), split)
            return torch.cat([score.view(torch.int32).reshape(-1), col.reshape(-1), count]).cpu().numpy()

        def route():
            rows = torch.from_numpy(host[:m]).to(dev).long()
            out = []
            for r in range(K):
                lo, hi = s["rel_lo"][r], s["rel_lo"][r + 1]
                Gk = G[r] if G.dim() == 3 else G
                A = E * L[r] if L is not None else E
                S = (A @ Gk) @ A.T
                S[s["ex_row"][lo:hi], s["ex_col"][lo:hi]] = -np.inf
                if no_self:
                    S[diag, diag] = -np.inf
                v, c = torch.topk(S if m == N else S[rows], k, dim=1)
                out.append(torch.cat([v.view(torch.int32), c.int()], 1))
            return torch.cat(out).cpu().numpy()

        variants = [("fused", fused), ("route", route)]
        if with_no_split:
            variants.insert(1, ("no_split", lambda: fused(False)))
        f, r = fused(), route()  # a warm pass of each, and the comparison
        f_col, f_cnt = f[n * k:2 * n * k].reshape(n, k), f[2 * n * k:]
        r_val, r_col = r[:, :k].view(np.float32), r[:, k:]
        if m == N:  # (the route took all rows in order)
            r_col, r_val = r_col.reshape(K, N, k)[:, nodes].reshape(n, k), r_val.reshape(K, N, k)[:, nodes].reshape(n, k)
        valid = np.arange(k)[None, :] < f_cnt[:, None]
        assert np.array_equal(np.isfinite(r_val).sum(1), f_cnt), "the fused call and the route count different partners"
        # (the route's matmul rounds differently: near-ties may swap)
        lists_equal = float(np.mean(np.all((f_col == r_col) | ~valid, axis=1)))
        sets_equal = float(np.mean([np.array_equal(np.sort(x[v]), np.sort(y[v])) for x, y, v in
                                    zip(f_col[::max(1, n // 20000)], r_col[::max(1, n // 20000)], valid[::max(1, n // 20000)])]))
        if with_no_split:
            assert fused(False).tobytes() == f.tobytes(), "the split changes the result"
        t = {nm: [] for nm, _ in variants}
        for rnd in range(a.rounds):  # alternate the variants, each round starting with another
            at = rnd % len(variants)
            for nm, fn in variants[at:] + variants[:at]:
                t[nm].append(timed(fn)[0])

        # the kernels alone, on device-resident indices
        buf = torch.from_numpy(host).to(dev)
        kern = {nm: [] for nm in (("split", "no_split") if with_no_split else ("split",))}
        for nm in kern:
            call(buf, nm == "split")
        for _ in range(a.rounds):
            for nm in kern:
                kern[nm].append(event_ms(lambda: call(buf, nm == "split")))
        tiles = K * -(-m // 32)
        mfma = tiles * -(-N // 32) * (d // 2)
        floor_ms = 1e3 * mfma * MFMA_CYCLES / SIMDS / CLOCK_HZ
        med = {nm: float(np.median(v)) for nm, v in t.items()}
        spread = {nm: float(max(v) - min(v)) for nm, v in t.items()}
        return {"shape": s["name"], "nodes": N, "relations": K, "k": k, "no_self": bool(no_self), "queries": int(n),
                "query_tiles": tiles, "live_rows_per_tile": m / -(-m // 32), "column_tiles": -(-N // 32),  # (live rows: of 32)
                "exclusion_entries": s["nnz"], "exclusion_csr_host_s": s["csr_s"], "exclusion_upload_ms": s["upload_ms"],
                "workspace_bytes": int(kernels._lib.load().dg_decoder_node_topk_workspace(n, K, N, k)),
                "copy_back_bytes": int(f.nbytes), "mean_count": float(f_cnt.mean()),
                "lists_equal_to_route": lists_equal, "sets_equal_to_route_sampled": sets_equal,
                **{nm: stats(v) for nm, v in t.items()}, "route_over_fused": med["route"] / med["fused"],
                "fused_beats_route_by_more_than_the_spread": bool(med["route"] - med["fused"] > spread["route"] + spread["fused"]),
                "kernel": {nm: stats(v) for nm, v in kern.items()}, "mfma_instructions": mfma, "mfma_floor_ms": floor_ms,
                "kernel_fraction_of_floor": floor_ms / float(np.median(kern["split"]))}

    shapes = []
    for nm in a.shapes.split(","):
        if nm in ("drug_drug", "one_node"):
            adj = P.adj[1, 1]
            rel_edges = [np.asarray(c[0], np.int64) for c in adj]
            N, K = int(adj[0][2][0]), len(adj)
            s = shape(nm, N, rel_edges, (d, d), (K, d))  # DEDICOM: a shared R, one diagonal per relation
            nodes = np.arange(N) if nm == "drug_drug" else rng.integers(0, N, 1)
            shapes.append(measure(s, nodes, 10, True, False))
        elif nm == "one_rel":
            e = np.asarray(P.adj[0, 0][0][0], np.int64)
            e = e[(e[:, 0] < a.nodes) & (e[:, 1] < a.nodes)]
            s = shape(nm, a.nodes, [e], (1, d, d), None)  # Bilinear: one dense G, no diagonal
            shapes.append(measure(s, np.arange(a.nodes), 50, False, True))
        else:
            raise SystemExit(f"partners_bench: unknown shape {nm}")
        del s
        torch.cuda.empty_cache()

    res = {"bench": "partners", "d": d, "rounds": a.rounds, "synthetic_graph_s": graph_s,
           "floor": {"simds": SIMDS, "clock_hz": CLOCK_HZ, "cycles_per_mfma": MFMA_CYCLES}, "shapes": shapes}
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""Ranking each drug pair's relations OUTSIDE its known ones at config P's drug×drug shape
(decagon_amd/synthetic.py: 645 drugs, 1,928 DEDICOM relation slots), d = 32, k = 10, for 4,096
pairs and all 207,690 unordered pairs.  The exclusion is synthetic.make_P's drug×drug adjacencies.

  masked    what evaluate.top_relations(exclude=) runs after its forward pass: one upload of the
            2·P indices, kernels.decoder_top_relations(k, exclude=lists on the device), one copy back
  route     what a caller had to do before: decoder_top_relations with
            k' = min(DG_TOPK_MAX_K, k + the most known relations of a queried pair), the copy
            back of the [P, k'] arrays, and a filter on the host (a sorted lookup of every returned
            (pair, slot) in the known ones, then the first k that remain).  The pairs whose known
            relations exceed k' − k it cannot be sure to serve are counted.
  unmasked  decoder_top_relations(k) of the same build, no exclusion: what the exclusion costs

Whole passes are warmed up, then timed (host clock around passes that end with the results on the
host and the device idle), alternating and each round starting with another variant (so that no
variant always follows the route's host filter), --rounds rounds: median and min – max.  The host build of
the lists (sparse.pair_exclusion; sparse.exclusion_csr of the 1,928 adjacencies apart) and their
upload are paid once per (pairs, training set) and are reported apart.  The selection kernel alone
(kernels.row_topk on one chunk of scores, device events) is set against its traffic floor: the
[chunk, n_sel] scores read once plus 4·nnz bytes of lists.  Prints one JSON line (and writes it to
--out).  Needs a HIP device: there is no CPU fallback."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

HBM_BYTES_PER_S = 8.0e12  # the MI355X's specified HBM3E bandwidth: the floor's yardstick


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", type=int, default=32)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--sizes", type=str, default="4096,all", help="pair counts; 'all' = every unordered pair")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()

    import torch

    from decagon_amd import _lib, kernels, sparse, synthetic

    if not torch.cuda.is_available():
        raise SystemExit("exclusion_bench: no HIP device (timings are taken on the GPU only)")
    d, k = a.d, a.k
    t0 = time.perf_counter()
    adj = synthetic.make_P(a.seed).adj[1, 1]
    graph_s = time.perf_counter() - t0
    N, K = adj[0][2][0], len(adj)
    rng = np.random.default_rng(a.seed)
    dev = torch.device("cuda")
    lim = np.sqrt(6.0 / (N + d))
    E = torch.from_numpy(rng.uniform(-1, 1, (N, d)).astype(np.float32)).to(dev)
    E = E / E.norm(dim=1, keepdim=True)  # the model's embeddings are l2-normalised rows
    G = torch.from_numpy(rng.uniform(-lim, lim, (d, d)).astype(np.float32)).to(dev)
    L = torch.from_numpy(rng.uniform(-1, 1, (K, d)).astype(np.float32)).to(dev)
    all_pairs = np.stack(np.triu_indices(N, 1), 1).astype(np.int32)
    t0 = time.perf_counter()
    csr = sparse.exclusion_csr(adj, (N, N))
    csr_s = time.perf_counter() - t0

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t), out

    def event_ms(fn, rounds):
        ts = []
        for _ in range(rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        return ts

    def stats(v):
        return {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v)),
                "all_ms": [round(float(x), 4) for x in v]}

    sizes = []
    for tok in a.sizes.split(","):
        P = all_pairs.shape[0] if tok == "all" else int(tok)
        pr = all_pairs if tok == "all" else all_pairs[rng.choice(all_pairs.shape[0], P, replace=False)]
        host = np.ascontiguousarray(pr.T).reshape(-1)  # [row_idx | col_idx]

        t0 = time.perf_counter()
        pe = sparse.pair_exclusion(pr, csr, (N, N))
        build_s = time.perf_counter() - t0
        upload_ms, lists = timed(lambda: pe.device(dev))
        known = np.diff(pe.ptr)
        k_route = min(_lib.DG_TOPK_MAX_K, k + int(known.max()))
        beyond = int(np.count_nonzero(known > k_route - k))
        lin = pe.slot.astype(np.int64) + np.repeat(np.arange(P, dtype=np.int64), known) * K  # sorted (pair, slot)

        def top(kk, exclude=None):
            buf = torch.from_numpy(host).to(dev)
            s, i, n = kernels.decoder_top_relations(E, E, buf[:P], buf[P:], G, L, kk, exclude=exclude)
            return s.cpu().numpy(), i.cpu().numpy(), n.cpu().numpy()

        def masked():
            return top(k, lists)

        def unmasked():
            return top(k)

        def route():
            s, i, _ = top(k_route)
            q = i.astype(np.int64) + np.arange(P, dtype=np.int64)[:, None] * K
            pos = np.minimum(np.searchsorted(lin, q), max(lin.size - 1, 0))
            is_known = (lin[pos] == q) if lin.size else np.zeros(q.shape, bool)
            first = np.argsort(is_known, axis=1, kind="stable")[:, :k]  # the permitted ones, in order
            left = np.minimum(k, k_route - is_known.sum(axis=1)).astype(np.int32)
            live = np.arange(k)[None, :] < left[:, None]
            return (np.where(live, np.take_along_axis(s, first, 1), -np.inf).astype(np.float32),
                    np.where(live, np.take_along_axis(i, first, 1), -1).astype(np.int32), left)

        # a warm pass of each, and the comparison at the timed size
        m, r, u = masked(), route(), unmasked()
        served = known <= k_route - k
        route_equal = bool(all(np.array_equal(x[served], y[served]) for x, y in zip(m, r)))
        assert route_equal, "the masked selection and the filtered route differ on pairs the route can serve"
        assert np.array_equal(m[2], np.minimum(k, K - known))
        changed = int(np.count_nonzero(np.any(m[1] != u[1], axis=1)))
        del m, r, u

        t = {"masked": [], "route": [], "unmasked": []}
        variants = [("masked", masked), ("route", route), ("unmasked", unmasked)]
        for rnd in range(a.rounds):  # alternate the variants, each round starting with another
            for nm, fn in variants[rnd % 3:] + variants[:rnd % 3]:
                t[nm].append(timed(fn)[0])

        # the selection alone, on one chunk of scores as decoder_top_relations forms them
        p0, p1 = kernels.top_relations_chunks(P, K, 64 << 20)[0]
        buf = torch.from_numpy(host).to(dev)
        scores = kernels.decoder_score_cross(E, E, buf[:P][p0:p1].contiguous(), buf[P:][p0:p1].contiguous(), G, L)
        part = (lists[0][p0:p1 + 1].contiguous(), lists[1])
        nnz_chunk = int(pe.ptr[p1] - pe.ptr[p0])
        kernels.row_topk(scores, k)
        kernels.row_topk(scores, k, exclude=part)
        sel_u, sel_m = [], []
        for _ in range(a.rounds):
            sel_u += event_ms(lambda: kernels.row_topk(scores, k), 1)
            sel_m += event_ms(lambda: kernels.row_topk(scores, k, exclude=part), 1)
        floor_bytes = 4 * (p1 - p0) * K + 4 * nnz_chunk
        floor_ms = 1e3 * floor_bytes / HBM_BYTES_PER_S
        med = {nm: float(np.median(v)) for nm, v in t.items()}
        sizes.append({
            "pairs": P, "list_entries": int(pe.nnz), "known_per_pair_mean": float(known.mean()),
            "known_per_pair_max": int(known.max()), "route_k": k_route, "route_pairs_beyond_k": beyond,
            "route_equals_masked_on_served_pairs": route_equal, "pairs_whose_answer_the_exclusion_changes": changed,
            "pair_chunks": len(kernels.top_relations_chunks(P, K, 64 << 20)),
            **{nm: stats(v) for nm, v in t.items()},
            "route_over_masked": med["route"] / med["masked"],
            "masked_minus_unmasked_ms": med["masked"] - med["unmasked"],
            "unmasked_spread_ms": float(max(t["unmasked"]) - min(t["unmasked"])),
            "pair_exclusion_host_s": build_s, "lists_upload_ms": upload_ms, "lists_bytes": int(4 * (pe.nnz + P + 1)),
            "selection_chunk": {"pairs": p1 - p0, "list_entries": nnz_chunk, "unmasked": stats(sel_u),
                                "masked": stats(sel_m), "floor_bytes": floor_bytes, "floor_ms": floor_ms,
                                "masked_fraction_of_floor": floor_ms / float(np.median(sel_m)),
                                "unmasked_fraction_of_floor": 1e3 * 4 * (p1 - p0) * K / HBM_BYTES_PER_S
                                / float(np.median(sel_u))},
        })

    res = {"bench": "exclusion", "drugs": N, "relations": K, "d": d, "k": k, "rounds": a.rounds,
           "topk_max_k": _lib.DG_TOPK_MAX_K, "synthetic_graph_s": graph_s, "exclusion_csr_host_s": csr_s,
           "floor_bandwidth_bytes_per_s": HBM_BYTES_PER_S, "sizes": sizes}
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()

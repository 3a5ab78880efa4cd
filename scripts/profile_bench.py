#!/usr/bin/env python
"""The profile of drug pairs at config P's drug×drug shape (decagon_amd/synthetic.py: 645 drugs,
1,928 DEDICOM relation slots), d = 32: every relation's score of P pairs, and each pair's k = 10
best relations, for P = 32, 4,096 and all 207,690 unordered pairs.

  fused     what evaluate.pair_profiles / top_relations run after their forward pass: one upload
            of the 2·P indices, kernels.decoder_score_cross (scores) or
            kernels.decoder_top_relations (ranking), one copy back
  baseline  what the package offered before: the K-times-repeated index arrays built on the host
            and uploaded, kernels.decoder_score_seg over K segments that each hold the same P
            pairs, for the ranking torch.topk on the reshaped scores, then the copy back.  Above
            --baseline-chunk pairs the baseline runs in chunks of that many pairs (its index
            arrays are 2·K·P int32: 3.2 GB for all pairs at once).

Whole passes are warmed up, then timed with device events around passes that end with the results
on the host, alternating, --rounds rounds; the two score matrices are compared for equality, bit
for bit, at every timed size.  The fused passes' stages are timed as well (events between them).
The scorer's time is set against the MFMA floor: d/2 v_mfma_f32_32x32x2_f32 of 64 cycles per 32
scores and SIMD, 1,024 SIMDs at 2.4 GHz.  Prints one JSON line (and writes it to --out).  Needs a
HIP device: there is no CPU fallback."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--drugs", type=int, default=645)
    ap.add_argument("--relations", type=int, default=1928)
    ap.add_argument("--d", type=int, default=32)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--sizes", type=str, default="32,4096,all", help="pair counts; 'all' = every unordered pair")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--baseline-chunk", type=int, default=8192)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()

    import torch

    from decagon_amd import kernels

    if not torch.cuda.is_available():
        raise SystemExit("profile_bench: no HIP device (timings are taken on the GPU only)")
    N, K, d, k = a.drugs, a.relations, a.d, a.k
    rng = np.random.default_rng(a.seed)
    dev = torch.device("cuda")
    lim = np.sqrt(6.0 / (N + d))
    E = torch.from_numpy(rng.uniform(-1, 1, (N, d)).astype(np.float32)).to(dev)
    E = E / E.norm(dim=1, keepdim=True)  # the model's embeddings are l2-normalised rows
    G = torch.from_numpy(rng.uniform(-lim, lim, (d, d)).astype(np.float32)).to(dev)
    L = torch.from_numpy(rng.uniform(-1, 1, (K, d)).astype(np.float32)).to(dev)
    iu = np.triu_indices(N, 1)
    all_pairs = np.stack(iu, 1).astype(np.int32)
    floor_rate = 1024 * 2.4e9 * 32 / (64.0 * d / 2)  # scores per second

    def marker(marks):
        def mark():
            if marks is not None:
                e = torch.cuda.Event(enable_timing=True)
                e.record()
                marks.append(e)
        return mark

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        out = fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1), out

    sizes = []
    for tok in a.sizes.split(","):
        n = all_pairs.shape[0] if tok == "all" else int(tok)
        pr = all_pairs if tok == "all" else all_pairs[rng.choice(all_pairs.shape[0], n, replace=False)]
        host = np.ascontiguousarray(pr.T).reshape(-1)  # [row_idx | col_idx]
        P = n
        bc = min(P, a.baseline_chunk)

        def fused_scores(marks=None, host=host, P=P):
            mark = marker(marks)
            mark()
            buf = torch.from_numpy(host).to(dev)
            mark()
            s = kernels.decoder_score_cross(E, E, buf[:P], buf[P:], G, L)
            mark()
            out = s.cpu().numpy()
            mark()
            return out

        def fused_top(marks=None, host=host, P=P):
            mark = marker(marks)
            mark()
            buf = torch.from_numpy(host).to(dev)
            mark()
            s, i, n_ = kernels.decoder_top_relations(E, E, buf[:P], buf[P:], G, L, k)
            mark()
            out = s.cpu().numpy(), i.cpu().numpy(), n_.cpu().numpy()
            mark()
            return out

        def baseline_chunks(pr=pr, P=P, bc=bc):
            for p0 in range(0, P, bc):
                c = pr[p0:p0 + bc]
                m = c.shape[0]
                idx = np.concatenate([np.tile(c[:, 0], K), np.tile(c[:, 1], K), np.arange(K + 1, dtype=np.int32) * m])
                buf = torch.from_numpy(idx.astype(np.int32)).to(dev)
                s = kernels.decoder_score_seg(E, E, buf[:K * m], buf[K * m:2 * K * m], buf[2 * K * m:], G, L)
                yield p0, m, s.view(K, m)

        def baseline_scores(P=P):
            out = np.empty((P, K), np.float32)
            for p0, m, s in baseline_chunks():
                out[p0:p0 + m] = s.cpu().numpy().T
            return out

        def baseline_top(P=P):
            vs, ix = np.empty((P, k), np.float32), np.empty((P, k), np.int64)
            for p0, m, s in baseline_chunks():
                v, i = torch.topk(s.t(), k, dim=1)
                vs[p0:p0 + m], ix[p0:p0 + m] = v.cpu().numpy(), i.cpu().numpy()
            return vs, ix

        # warm-up of all four, and the comparison at the timed size
        f = fused_scores()
        ft = fused_top()
        b = baseline_scores()
        bt = baseline_top()
        torch.cuda.synchronize()
        identical = bool(np.array_equal(f.view(np.uint32), b.view(np.uint32)))
        assert identical, "fused and per-segment score matrices differ"
        top_values_equal = bool(np.array_equal(ft[0], bt[0]))  # (indices may differ inside exact ties)
        del f, b, ft, bt

        t = {nm: [] for nm in ("fused_scores", "baseline_scores", "fused_top", "baseline_top")}
        st_s, st_t = [], []
        for _ in range(a.rounds):  # alternate the variants
            for nm, fn in (("fused_scores", fused_scores), ("baseline_scores", baseline_scores),
                           ("fused_top", fused_top), ("baseline_top", baseline_top)):
                t[nm].append(timed(fn)[0])
            for fn, st in ((fused_scores, st_s), (fused_top, st_t)):
                marks = []
                fn(marks)
                torch.cuda.synchronize()
                st.append([marks[i].elapsed_time(marks[i + 1]) for i in range(3)])
        ss, tt = np.median(np.array(st_s), axis=0), np.median(np.array(st_t), axis=0)
        med = {nm: float(np.median(v)) for nm, v in t.items()}
        sizes.append({
            "pairs": P, "baseline_chunk_pairs": bc, "baseline_chunked": bool(P > bc),
            "slot_chunk": kernels.cross_slot_chunk(P, K),
            "pair_chunks_top": len(kernels.top_relations_chunks(P, K, 64 << 20)),
            **{nm + "_ms": med[nm] for nm in t},
            **{nm + "_ms_all": [round(x, 4) for x in v] for nm, v in t.items()},
            "baseline_scores_spread_ms": float(max(t["baseline_scores"]) - min(t["baseline_scores"])),
            "baseline_top_spread_ms": float(max(t["baseline_top"]) - min(t["baseline_top"])),
            "speedup_scores": med["baseline_scores"] / med["fused_scores"],
            "speedup_top": med["baseline_top"] / med["fused_top"],
            "fused_scores_stage_ms": {"upload": float(ss[0]), "scorer": float(ss[1]), "copy_back": float(ss[2])},
            "fused_top_stage_ms": {"upload": float(tt[0]), "score_and_select": float(tt[1]),
                                   "copy_back": float(tt[2])},
            "mfma_floor_ms": 1e3 * P * K / floor_rate,
            "scorer_fraction_of_mfma_floor": float(1e3 * P * K / floor_rate / ss[1]),
            "identical_bits": identical, "top_values_equal": top_values_equal,
        })

    res = {"bench": "profile", "drugs": N, "relations": K, "d": d, "k": k, "rounds": a.rounds, "sizes": sizes}
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()

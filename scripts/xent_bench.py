#!/usr/bin/env python
"""Training on the cross-entropy cost, measured against the hinge in the same run.

At config P's drug×drug shape (645 drugs, 1,928 DEDICOM relations, 512 pairs each, d = 32;
synthetic l2-normalised embeddings, as scripts/train_all_bench.py's decoder part):

  (a) sum       the cost over the 987,136 pairs of one all-relation step: dg_xent_loss_ws_f32 (up to
                256 workgroups, fp32 terms) against the single-workgroup dg_xent_loss_f32, and the
                hinge's dg_hinge_loss_ws_f32 beside them; --inner calls per timed pass
  (b) decoder   the segmented decoder backward into dE (kernels.PreparedDecoderGradSeg, the two
                occurrence lists, two kernels.segment_rows_sum), loss="xent" against loss="hinge" on the
                same indices and scores; the gradient launches alone are timed with device events.
                The xent form reads the same operands, writes 8 bytes a pair of coefficients and
                takes two expf a pair; its row reduction gathers its weights from `coef`.
  (c) step      through the drop-in surface at config P: one trainall.train_step_all over a batch of
                every relation, an optimizer with loss="xent" against one with loss="hinge" on the
                same model, device-drawn negatives
  (d) opt_op    one ordinary `opt_op` step through Session.run on one drug×drug relation's batch,
                xent against hinge

Whole passes are warmed up, then timed with a host clock around passes that end in a device
synchronise, the two sides alternating, --rounds rounds; medians and min..max spreads are
reported.  Prints one JSON line and writes it to --out (default profiles/xent_bench.json).  Needs a
HIP device: there is no CPU fallback.

The condition on the hinge — that making the kernels templates over the cost cost the default path
nothing — is checked with scripts/train_all_bench.py run at the parent commit and at this one on the
same machine, alternating.  `--attach label=path` (repeatable) files such a run's JSON under
"train_all_bench_runs" in --out, beside the numbers above; with `--parts none` nothing is measured
and the existing --out is only extended (no device needed)."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))

from train_all_bench import log, stats  # noqa: E402


def timed(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def alternate(torch, sides, rounds, what):
    """{name: [ms per round]}: every side warmed up once, then the sides in turn, `rounds` times."""
    for fn in sides.values():
        fn()
    torch.cuda.synchronize()
    t = {name: [] for name in sides}
    for r in range(rounds):
        for name, fn in sides.items():
            t[name].append(timed(torch, fn))
        log(f"{what}: round {r}: " + ", ".join(f"{name} {ms[-1]:.4f} ms" for name, ms in t.items()))
    return t


def operands(a, torch, kernels, dev):
    N, K, d, B = a.drugs, a.relations, a.d, a.batch
    rng = np.random.default_rng(a.seed)
    E = torch.from_numpy(rng.uniform(-1, 1, (N, d)).astype(np.float32)).to(dev)
    E = (E / E.norm(dim=1, keepdim=True)).contiguous()
    lim = np.sqrt(6.0 / (2 * d))
    G = torch.from_numpy(rng.uniform(-lim, lim, (d, d)).astype(np.float32)).to(dev)
    L = torch.from_numpy(rng.uniform(-1, 1, (K, d)).astype(np.float32)).to(dev)
    P = K * B
    buf = torch.from_numpy(rng.integers(0, N, (3, P)).astype(np.int32)).to(dev)
    rows, cols, negs = buf[0], buf[1], buf[2]
    seg_ptr = torch.arange(0, P + 1, B, dtype=torch.int32, device=dev)
    seg2 = torch.arange(0, 2 * P + 1, B, dtype=torch.int32, device=dev)
    rel2 = torch.arange(K, dtype=torch.int32, device=dev).repeat(2)
    scores = kernels.decoder_score_seg(E, E, torch.cat([rows, negs]), torch.cat([cols, cols]), seg2, G, L, seg_rel=rel2)
    return E, G, L, rows, cols, negs, seg_ptr, scores[:P].contiguous(), scores[P:].contiguous()


def sum_part(a, torch, kernels, dev, ops):
    pos, neg = ops[-2], ops[-1]
    ws = kernels.hinge_workspace(dev)
    out = torch.empty(1, device=dev)
    w = a.neg_weight

    def many(fn):
        def run():
            for _ in range(a.inner):
                fn()
        return run

    sides = {"xent_ws": many(lambda: kernels.xent_loss(pos, neg, w, out=out, workspace=ws)),
             "xent_single_block": many(lambda: kernels.xent_loss(pos, neg, w, out=out)),
             "hinge_ws": many(lambda: kernels.hinge_loss(pos, neg, 0.1, out=out, workspace=ws))}
    t = alternate(torch, sides, a.rounds, "sum part")
    one = float(kernels.xent_loss(pos, neg, w).cpu()[0])
    multi = float(kernels.xent_loss(pos, neg, w, workspace=ws).cpu()[0])
    p64, n64 = pos.double().cpu().numpy(), neg.double().cpu().numpy()
    sce = lambda x, z: np.maximum(x, 0) - x * z + np.log1p(np.exp(-np.abs(x)))  # noqa: E731
    ref = float(np.sum(sce(p64, 1.0)) + w * np.sum(sce(n64, 0.0)))
    res = {"pairs": int(pos.numel()), "calls_per_pass": a.inner, "neg_weight": w}
    for name, ms in t.items():
        res[name] = stats([x / a.inner for x in ms])
    res["single_block_over_ws"] = float(np.median(t["xent_single_block"]) / np.median(t["xent_ws"]))
    res["bytes_read"] = int(8 * pos.numel())
    res["xent_ws_bytes_per_s"] = float(8 * pos.numel() / (1e-3 * res["xent_ws"]["median_ms"]))
    res["rel_error_against_float64"] = {"xent_ws": abs(multi - ref) / ref, "xent_single_block": abs(one - ref) / ref}
    return res


def decoder_part(a, torch, kernels, dev, ops):
    E, G, L, rows, cols, negs, seg_ptr, pos, neg = ops
    N, K, d, P = a.drugs, a.relations, a.d, rows.numel()
    state = {}
    for loss in ("hinge", "xent"):
        state[loss] = (torch.zeros((N, d), device=dev), torch.zeros(d * d, device=dev), torch.zeros(K * d, device=dev))

    def backward(loss, marks=None):
        dE, dG, dl = state[loss]

        def mark():
            if marks is not None:
                e = torch.cuda.Event(enable_timing=True)
                e.record()
                marks.append(e)
        dE.zero_(), dG.zero_(), dl.zero_()
        mark()
        op = kernels.PreparedDecoderGradSeg(E, E, rows, cols, negs, seg_ptr, None, pos, neg, G, L, 0.1, dG=dG, dl=dl,
                                            loss=loss, neg_weight=a.neg_weight)
        op()
        mark()
        node_ptr, order = kernels.occurrence_list(torch.cat([rows, negs]), N)
        if loss == "hinge":
            sign = torch.where(order < P, -1.0, 1.0).to(torch.float32)
        else:
            sign = op.coef.index_select(0, order.long())
        item = torch.remainder(order, P).to(torch.int32)
        cptr, corder = kernels.occurrence_list(cols, N)
        mark()
        kernels.segment_rows_sum(node_ptr, item, op.mv, dE, sign=sign)
        kernels.segment_rows_sum(cptr, corder, op.grad_cols, dE)
        mark()

    sides = {loss: (lambda loss=loss: backward(loss)) for loss in ("hinge", "xent")}
    t = alternate(torch, sides, a.rounds, "decoder part")
    stages = {loss: [] for loss in sides}
    for _ in range(a.rounds):
        for loss in sides:
            marks = []
            backward(loss, marks)
            torch.cuda.synchronize()
            stages[loss].append([marks[i].elapsed_time(marks[i + 1]) for i in range(3)])
    res = {"drugs": N, "relations": K, "batch": a.batch, "d": d, "pairs": int(P), "neg_weight": a.neg_weight,
           "hinge_active_fraction": float(((neg - (pos - 0.1)) > 0).float().mean())}
    for loss in sides:
        st = np.array(stages[loss])
        res[loss] = stats(t[loss])
        res[loss + "_stage_ms"] = {
            name: {"median": float(np.median(st[:, q])), "min": float(st[:, q].min()), "max": float(st[:, q].max())}
            for q, name in enumerate(("gradient_launches", "occurrence_lists", "row_sums"))}
    res["xent_over_hinge"] = float(np.median(t["xent"]) / np.median(t["hinge"]))
    res["xent_over_hinge_gradient_launches"] = float(res["xent_stage_ms"]["gradient_launches"]["median"] /
                                                     res["hinge_stage_ms"]["gradient_launches"]["median"])
    res["all_gradients_finite"] = bool(all(torch.isfinite(x).all() for x in state["xent"]))
    return res


def step_part(a, torch):
    import decagon_amd as dg
    from decagon_amd import synthetic
    from decagon_amd.trainall import train_step_all
    from train_all_bench import build_model

    graph = synthetic.make_P(seed=0)
    B = a.batch
    dg_, ph, model, hinge, feed = build_model(graph, B)
    dims = {et: [tuple(int(s) for s in c[2]) for c in rels] for et, rels in graph.adj.items()}
    xent = dg.DecagonOptimizer(embeddings=model.embeddings, latent_inters=model.latent_inters,
                               latent_varies=model.latent_varies, degrees=graph.degrees, edge_types=graph.edge_types,
                               edge_type2dim=dims, placeholders=ph, batch_size=B, margin=0.1,
                               neg_sample_weights=a.neg_weight, loss="xent")
    opts = {"hinge": hinge, "xent": xent}
    rng = np.random.default_rng(a.seed)
    batches = {}
    for et, rels in graph.adj.items():
        batches[et] = {}
        for k, coo in enumerate(rels):
            c = np.asarray(coo[0])
            batches[et][k] = c[rng.choice(len(c), B, replace=len(c) < B)].astype(np.int64)
    n_rel = sum(len(v) for v in batches.values())
    sess = dg.Session()
    ets = list(graph.adj)
    e = sum(len(graph.adj[et]) for et in ets[:ets.index((1, 1))])  # the first drug×drug relation
    f = dict(feed)
    f.update({ph["batch"]: batches[1, 1][0], ph["batch_edge_type_idx"]: e, ph["batch_row_edge_type"]: 1,
              ph["batch_col_edge_type"]: 1})

    log(f"step part: {n_rel} relations; warm-up (builds the plans)")
    costs = {}
    all_sides = {}
    one_sides = {}
    for name, opt in opts.items():
        all_sides[name] = (lambda opt=opt: costs.__setitem__(opt.loss, train_step_all(sess, opt, ph, feed, batches)))
        one_sides[name] = (lambda opt=opt: sess.run(opt.opt_op, feed_dict=f))
    t_all = alternate(torch, all_sides, a.step_rounds, "all-relation step")
    t_one = alternate(torch, one_sides, a.rounds, "opt_op step")
    res = {"config": "P", "relations": n_rel, "batch": B, "trained_edges_per_step": n_rel * B,
           "neg_weight": a.neg_weight, "negatives": "device-drawn",
           "last_costs": {k: float(v) for k, v in costs.items()}}
    res["train_step_all"] = {name: stats(ms) for name, ms in t_all.items()}
    res["train_step_all"]["xent_over_hinge"] = float(np.median(t_all["xent"]) / np.median(t_all["hinge"]))
    res["opt_op"] = {name: stats(ms) for name, ms in t_one.items()}
    res["opt_op"]["xent_over_hinge"] = float(np.median(t_one["xent"]) / np.median(t_one["hinge"]))
    return res


def attach(a, res):
    """File the --attach results (train_all_bench.py's decoder and step numbers, in the order given)."""
    for item in a.attach:
        label, path = item.split("=", 1)
        run = json.loads(Path(path).read_text())
        dec = run["decoder_backward"]
        keep = {"decoder_backward": {k: dec[k] for k in ("segmented", "loop", "segmented_stage_ms")}}
        for part in ("step_S", "step_P"):
            if part in run:
                keep[part] = {k: run[part][k] for k in ("all_relations_step", "per_relation_sweep")}
        res.setdefault("train_all_bench_runs", {})[label] = keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--drugs", type=int, default=645)
    ap.add_argument("--relations", type=int, default=1928)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--d", type=int, default=32)
    ap.add_argument("--neg-weight", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--step-rounds", type=int, default=7, help="rounds of the all-relation step comparison")
    ap.add_argument("--inner", type=int, default=50, help="cost-sum calls per timed pass")
    ap.add_argument("--parts", type=str, default="sum,decoder,step")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--attach", action="append", default=[], metavar="LABEL=PATH",
                    help="a scripts/train_all_bench.py result to file under train_all_bench_runs")
    ap.add_argument("--out", type=str, default=str(ROOT / "profiles" / "xent_bench.json"))
    a = ap.parse_args()
    out = Path(a.out)
    if a.parts == "none":
        res = json.loads(out.read_text())
        attach(a, res)
        out.write_text(json.dumps(res) + "\n")
        print(json.dumps(res))
        return

    import torch

    from decagon_amd import kernels

    if not torch.cuda.is_available():
        raise SystemExit("xent_bench: no HIP device (timings are taken on the GPU only)")
    dev = torch.device("cuda")
    res = {"bench": "xent", "rounds": a.rounds}
    out.parent.mkdir(parents=True, exist_ok=True)
    ops = operands(a, torch, kernels, dev)
    for part in a.parts.split(","):
        if part == "sum":
            res["cost_sum"] = sum_part(a, torch, kernels, dev, ops)
        elif part == "decoder":
            res["decoder_backward"] = decoder_part(a, torch, kernels, dev, ops)
        else:
            res["step_P"] = step_part(a, torch)
        out.write_text(json.dumps(res) + "\n")  # (kept after every part)
    attach(a, res)
    out.write_text(json.dumps(res) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

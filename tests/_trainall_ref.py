"""The float64 reference of the all-relation training step on the golden S model, shared by the
tests of test_gpu_trainall.py: a batch and fed negatives for every relation of every edge type,
and the sum over (edge type, relation) of oracle.train_grads on them.

SEED was picked on the CPU with the oracle so that every pair's hinge argument z = neg − (pos −
margin) has |z| >= 1e-3 in float64, with and without the dropout masks of step 1: fp32 cannot
flip a relu mask.  The tests assert that condition; no pair is dropped to meet it."""
import numpy as np

from oracle import decagon_oracle as orc

SEED = 2
MARGIN = 0.1
# pairs per relation, in edge-type order: sub-tile, full tile, full + ragged, several tiles
SIZES = [33, 40, 7, 64, 32, 50, 45, 38, 36, 41]


def edge_types_of(z):
    return {(int(i), int(j)): int(k) for i, j, k in z["edge_types"]}


def make_batches(z, seed=SEED, sizes=SIZES):
    """({(i, j): {k: [n, 2]}}, {(i, j): {k: [n]}}): pairs drawn from each relation's training
    edges, negative rows uniform over the row type's nodes."""
    rng = np.random.default_rng(seed)
    n = [int(x) for x in z["n_nodes"]]
    batches, negs, r = {}, {}, 0
    for (i, j), K in edge_types_of(z).items():
        batches[i, j], negs[i, j] = {}, {}
        for k in range(K):
            edges = z[f"train_{i}_{j}_{k}"]
            batches[i, j][k] = edges[rng.choice(len(edges), sizes[r], replace=False)].astype(np.int64)
            negs[i, j][k] = rng.integers(0, n[i], sizes[r]).astype(np.int64)
            r += 1
    return batches, negs


def oracle_inputs(z):
    ets = edge_types_of(z)
    decoders = {et: str(d) for et, d in zip(ets, z["decoders"])}
    f64 = lambda a: np.asarray(a, np.float64)  # noqa: E731
    w1 = {(i, j): [f64(z[f"w1_{i}_{j}_{k}"]) for k in range(K)] for (i, j), K in ets.items()}
    w2 = {(i, j): [f64(z[f"w2_{i}_{j}_{k}"]) for k in range(K)] for (i, j), K in ets.items()}
    dec = {}
    for (i, j) in ets:
        pre = f"dec_{i}_{j}_"
        dec[i, j] = {name[len(pre):]: f64(z[name]) for name in z.files if name.startswith(pre)}
    adj = {(i, j): [(z[f"adj_{i}_{j}_{k}_coords"], z[f"adj_{i}_{j}_{k}_values"],
                     tuple(int(s) for s in z[f"adj_{i}_{j}_{k}_shape"])) for k in range(K)]
           for (i, j), K in ets.items()}
    return ets, decoders, w1, w2, dec, adj


def embeddings(ets, adj, w1, w2, drop1=None, drop2=None):
    """The forward of oracle.train_grads (identity features), for the pairs' hinge arguments."""
    S1, pre1 = {}, {}
    for (i, j) in ets:
        xs = [w if drop1 is None else w * drop1[i, j][k][:, None] for k, w in enumerate(w1[i, j])]
        S1[i, j] = np.sum([orc.sparse_dense_matmul(a, x) for a, x in zip(adj[i, j], xs)], axis=0)
        pre1[i] = pre1.get(i, 0.0) + orc.l2_normalize_rows(S1[i, j])
    H1 = {i: np.maximum(v, 0.0) for i, v in pre1.items()}
    E = {}
    for (i, j) in ets:
        ps = [(H1[j] if drop2 is None else H1[j] * drop2[i, j][k]) @ w for k, w in enumerate(w2[i, j])]
        E[i] = E.get(i, 0.0) + orc.l2_normalize_rows(
            np.sum([orc.sparse_dense_matmul(a, p) for a, p in zip(adj[i, j], ps)], axis=0))
    return E


def reference(z, batches, negs, drop1=None, drop2=None):
    """(cost, grads, zs): Σ over every (edge type, relation) of oracle.train_grads' cost and
    gradients ({"w1", "w2", "dec"} as the oracle returns them), and every pair's hinge argument."""
    ets, decoders, w1, w2, dec, adj = oracle_inputs(z)
    E = embeddings(ets, adj, w1, w2, drop1, drop2)
    inters, varies = orc.latent_matrices(ets, decoders, dec, 32)
    total, cost, zs, e = None, 0.0, [], 0
    for (i, j), K in ets.items():
        for k in range(K):
            if k in batches.get((i, j), {}):
                b, ng = batches[i, j][k], negs[i, j][k]
                c, g = orc.train_grads(ets, adj, {0: None, 1: None}, w1, w2, decoders, dec, 32, b, ng, e, i, j,
                                       MARGIN, drop1=drop1, drop2=drop2)
                M = varies[e] @ inters[e] @ varies[e]
                v = E[j][b[:, 1]]
                zs.append(np.sum((E[i][ng] @ M) * v, 1) - (np.sum((E[i][b[:, 0]] @ M) * v, 1) - MARGIN))
                cost += c
                if total is None:
                    total = g
                else:
                    for et in ets:
                        for kk in range(ets[et]):
                            total["w1"][et][kk] = total["w1"][et][kk] + g["w1"][et][kk]
                            total["w2"][et][kk] = total["w2"][et][kk] + g["w2"][et][kk]
                        for name in total["dec"][et]:
                            total["dec"][et][name] = total["dec"][et][name] + g["dec"][et][name]
            e += 1
    return cost, total, np.concatenate(zs)


def wanted(ets, decoder_vars, ref):
    """The reference gradients in grads_vars' order (layers 1, layers 2, decoders)."""
    want = []
    for et, K in ets.items():
        want += [ref["w1"][et][k] for k in range(K)]
    for et, K in ets.items():
        want += [ref["w2"][et][k] for k in range(K)]
    for et in ets:
        want += [ref["dec"][et][n] for n in decoder_vars[et]]
    return want

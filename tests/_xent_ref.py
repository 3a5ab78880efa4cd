"""The float64 reference of training on either cost, by autograd: the golden S forward rebuilt in
torch float64 on the CPU (identity features, l2_normalize, relu, the decoders' matrices from
oracle.latent_matrices, optional dropout masks from oracle.dropout_scale) with a `loss` switch,
and its gradients taken by torch.autograd — independent of the hand-derived backward formulas of
the kernels (decagon_amd/csrc/loss_policy.h) and of oracle.train_grads, which is hinge-only.

test_cpu_xent.py first holds this reference, in hinge mode, to oracle.train_grads; the xent
tests are then held to it.  Batches, negatives and the gradients' order come from _trainall_ref.
"""
import numpy as np
import torch

import _trainall_ref as R
from oracle import decagon_oracle as orc

MARGIN = R.MARGIN
D2 = 32


def _spmm(coo, x):
    coords, values, shape = coo
    a = torch.sparse_coo_tensor(torch.from_numpy(np.asarray(coords, np.int64).reshape(-1, 2).T.copy()),
                                torch.from_numpy(np.asarray(values, np.float64)), tuple(int(s) for s in shape))
    return torch.sparse.mm(a, x)


def _l2n(x):
    """tf.nn.l2_normalize(x, dim=1) (oracle.l2_normalize_rows)."""
    ss = torch.sum(x * x, dim=1, keepdim=True)
    return x * torch.rsqrt(torch.clamp(ss, min=orc.EPS_L2))


def cost_of(pos, neg, loss, w=1.0, margin=MARGIN):
    """The cost of optimizer.py:116-120 (hinge) or :122-127 (xent) on torch score vectors."""
    if loss == "hinge":
        return torch.sum(torch.relu(neg - (pos - margin)))
    if loss == "xent":
        return torch.sum(torch.nn.functional.softplus(-pos)) + w * torch.sum(torch.nn.functional.softplus(neg))
    raise ValueError(loss)


def reference(z, batches, negs, loss, w=1.0, margin=MARGIN, drop1=None, drop2=None):
    """(cost, grads, scores): the cost summed over every (edge type, relation) listed in `batches`
    ({(i, j): {k: [n, 2]}}, negatives {(i, j): {k: [n]}}), its gradients as oracle.train_grads
    returns them ({"w1", "w2", "dec"}; zeros where the cost does not reach a variable), and
    scores = {(i, j, k): (pos, neg)} as float64 arrays."""
    ets, decoders, w1, w2, dec, adj = R.oracle_inputs(z)
    leaf = lambda a: torch.tensor(np.asarray(a, np.float64), requires_grad=True)  # noqa: E731
    const = lambda a: torch.from_numpy(np.asarray(a, np.float64))  # noqa: E731
    tw1 = {et: [leaf(x) for x in w1[et]] for et in ets}
    tw2 = {et: [leaf(x) for x in w2[et]] for et in ets}
    inters, varies = orc.latent_matrices(ets, decoders, dec, D2)
    tG, tL = [leaf(g) for g in inters], [leaf(l) for l in varies]

    pre1 = {}
    for (i, j) in ets:
        xs = [x if drop1 is None else x * const(drop1[i, j][k])[:, None] for k, x in enumerate(tw1[i, j])]
        s1 = sum(_spmm(a, x) for a, x in zip(adj[i, j], xs))
        pre1[i] = pre1[i] + _l2n(s1) if i in pre1 else _l2n(s1)
    H1 = {i: torch.relu(v) for i, v in pre1.items()}
    E = {}
    for (i, j) in ets:
        ps = [(H1[j] if drop2 is None else H1[j] * const(drop2[i, j][k])) @ x for k, x in enumerate(tw2[i, j])]
        s2 = _l2n(sum(_spmm(a, p) for a, p in zip(adj[i, j], ps)))
        E[i] = E[i] + s2 if i in E else s2

    cost, scores, e = 0.0, {}, 0
    for (i, j), K in ets.items():
        for k in range(K):
            if k in batches.get((i, j), {}):
                b, ng = np.asarray(batches[i, j][k]), np.asarray(negs[i, j][k])
                M = tL[e] @ tG[e] @ tL[e]
                v = E[j][b[:, 1]]
                pos = torch.sum((E[i][b[:, 0]] @ M) * v, dim=1)
                neg = torch.sum((E[i][ng] @ M) * v, dim=1)
                cost = cost + cost_of(pos, neg, loss, w, margin)
                scores[i, j, k] = (pos.detach().numpy().copy(), neg.detach().numpy().copy())
            e += 1
    cost.backward()

    g = lambda t: np.zeros(tuple(t.shape)) if t.grad is None else t.grad.numpy().copy()  # noqa: E731
    grads = {"w1": {et: [g(x) for x in tw1[et]] for et in ets}, "w2": {et: [g(x) for x in tw2[et]] for et in ets},
             "dec": {}}
    e = 0
    for et, K in ets.items():
        kind = decoders[et]
        out = {name: np.zeros_like(np.asarray(val, np.float64)) for name, val in dec.get(et, {}).items()}
        for k in range(K):
            dG, dL = g(tG[e]), g(tL[e])
            if kind == "distmult":
                out["relation_%d" % k] += np.diag(dG)
            elif kind == "bilinear":
                out["relation_%d" % k] += dG
            elif kind == "dedicom":
                out["global_interaction"] += dG
                out["local_variation_%d" % k] += np.diag(dL)
            e += 1
        grads["dec"][et] = out
    return float(cost.detach()), grads, scores


def one_per_decoder_kind(z):
    """[(i, j, k, flat index e)]: the first relation of each decoder kind that has variables or not."""
    ets = R.edge_types_of(z)
    seen, out, e = set(), [], 0
    for (et, K), kind in zip(ets.items(), z["decoders"]):
        if str(kind) not in seen:
            seen.add(str(kind))
            out.append((et[0], et[1], 0, e))
        e += K
    return out


def closed_form(U, V, rows, cols, negs, pos, neg, G, l, w):
    """A numpy float64 restatement of the closed formulas of the kernels' header comments for the
    xent cost: a = σ(−pos), b = w·σ(neg), M = L·G·L →
    (a, b, grad_rows [2n, d], grad_cols [n, d], dM, dG, dl, dG_diag)."""
    f = lambda x: np.asarray(x, np.float64)  # noqa: E731
    U, V, pos, neg, G = f(U), f(V), f(pos), f(neg), f(G)

    def sig(x):
        e = np.exp(-np.abs(x))
        return np.where(x >= 0, 1.0, e) / (1.0 + e)

    a, b = sig(-pos), w * sig(neg)
    d = G.shape[0]
    lv = f(l) if l is not None else np.ones(d)
    L = np.diag(lv)
    M = L @ G @ L
    u, un, v = U[rows], U[negs], V[cols]
    mv = v @ M.T
    grad_rows = np.concatenate([-a[:, None] * mv, b[:, None] * mv])
    x = b[:, None] * un - a[:, None] * u
    grad_cols = x @ M
    dM = x.T @ v
    dG = L @ dM @ L
    dl = np.sum(dM * G * lv[None, :], axis=1) + np.sum(dM * G * lv[:, None], axis=0)
    return a, b, grad_rows, grad_cols, dM, dG, dl, np.diag(dG).copy()

"""The evaluation path: link-prediction accuracy on the device.

Reference: `get_accuracy_scores(edges_pos, edges_neg, edge_type)` (main.py:38-80) runs
`sess.run(opt.predictions)` — the full N_i×N_j score matrix of the edge type — then, on the
host, takes sigmoid(rec[u, v]) of the sampled positive and negative edges and calls sklearn's
roc_auc_score / average_precision_score and rank_metrics.apk(k=50)
(decagon/utility/rank_metrics.py:4-40); DecagonAccuracyEvaluator (main/AccuracyEvaluators/
Tensorflow/DecagonAccuracyEvaluator.py:58-150) does the same over the drug×drug relations.

Here only the sampled pairs are scored (dg_decoder_score_f32: u·L·G·L·v per pair, no
N_i×N_j matrix) and the three metrics come from dg_rank_metrics_ex_f32, which ranks the scores
the reference ranks — not the logits: the sigmoid is monotonic but it saturates, and the
resulting ties move AUROC, AUPRC and AP@k.  `sigmoid` selects the reference's form:

  "main"       get_accuracy_scores (main.py:51-52,60,70,81) under numpy 1.14
               (requirements.txt:14): float32 exp of TF's float32 logit, float64 1/(1+e),
               nan_to_num — logits > ≈36.7 score exactly 1.0, < ≈-88.7 exactly 0.0
  "evaluator"  DecagonAccuracyEvaluator (MathUtils.sigmoid on the float32 decoder output,
               DecagonAccuracyEvaluator.py:123): all float32, logits > ≈16.6 score 1.0
  None         the raw logits

accuracy_scores serves one relation per call.  accuracy_scores_all evaluates every relation of
an edge type — the reference's loop over edge_type2idx, DecagonAccuracyEvaluator.evaluateAll —
in one pass: the sampled pairs of all relations packed into segments (pack_edge_samples), one
scorer launch (dg_decoder_score_seg_f32) and one segmented metrics call
(dg_rank_metrics_seg_f32), row for row the bits of the per-relation call.

pair_profiles and top_relations answer the query the other way round — for given node pairs, the
score of every relation of the edge type and each pair's best relations (NpPredictor._predictEdges
per relation id, main/Predictor/NpPredictor.py:293-313): one launch over pairs × relations
(dg_decoder_score_cross_f32) and a per-pair selection on the device (dg_row_topk_f32), with
top_relations(exclude=) outside each pair's known relations (dg_row_topk_excl_f32) — the reference's
drop of the known edges on the host after _predictEdges.

edge_ranks and ranking_scores_all answer "given drug u and side effect k, where does the held-out
partner v stand among all partners u could have?" — the filtered rank of link prediction, and from
it mean reciprocal rank, mean rank and Hits@h per relation (ranking_metrics).  One launch per side
(dg_decoder_edge_rank_f32) walks every query's candidates and keeps a count; the reference's route is
_predictEdges' whole matrix per relation, a dense mask and a count on the host.

top_partners answers the question asked first — "given drug u and side effect k, which drugs are u's
likeliest partners outside the known ones?": the same walk with one running top-k list per query row in
place of the count (dg_decoder_node_topk_f32, one launch pair per side; pack_node_queries packs the
query nodes by relation on the host).
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib, kernels
from ._lib import check
from .graph import Node, RunContext


SIGMOID_MODES = {"main": _lib.DG_RANK_SIGMOID64, "evaluator": _lib.DG_RANK_SIGMOID32, None: _lib.DG_RANK_LOGIT}


def rank_metrics_device(pos: torch.Tensor, neg: torch.Tensor, k: int = 50,
                        sigmoid: Optional[str] = "main") -> torch.Tensor:
    """float64 device tensor [AUROC, AUPRC, AP@k] of device LOGIT vectors, ranked by the
    reference's sigmoid scores (module docstring; asynchronous)."""
    for t, nm in ((pos, "pos"), (neg, "neg")):
        kernels._dev(t, torch.float32, nm)
    if sigmoid not in SIGMOID_MODES:
        raise ValueError(f"sigmoid must be one of {list(SIGMOID_MODES)}")
    lib = _lib.load()
    P, N = pos.numel(), neg.numel()
    nbytes = int(lib.dg_rank_metrics_ex_workspace(P, N))
    ws = torch.empty(-(-nbytes // 8), dtype=torch.float64, device=pos.device)
    out = torch.empty(3, dtype=torch.float64, device=pos.device)
    check(lib.dg_rank_metrics_ex_f32(pos.data_ptr() if P else None, P, neg.data_ptr() if N else None, N, int(k),
                                     SIGMOID_MODES[sigmoid], out.data_ptr(), ws.data_ptr(), ws.numel() * 8,
                                     kernels._stream_ptr(None)), "dg_rank_metrics_ex_f32")
    return out


def rank_metrics(pos: torch.Tensor, neg: torch.Tensor, k: int = 50,
                 sigmoid: Optional[str] = "main") -> Tuple[float, float, float]:
    """(AUROC, AUPRC, AP@k) of device logit vectors, as roc_auc_score,
    average_precision_score and rank_metrics.apk(range(P), order of all scores) compute them
    on the reference's sigmoid scores."""
    au, ap, apk = rank_metrics_device(pos, neg, k, sigmoid).cpu().tolist()
    return au, ap, apk


def _stacked_latents(ctx: RunContext, dec, d: int):
    """(G, l) of ALL relations of one decoder for kernels.decoder_topk, as views of its flat
    parameter buffer: DEDICOM the shared R [d, d] and local_variation_k at stride d ([K, d]);
    Bilinear relation_k at stride d·d ([K, d, d]); DistMult's diagonals and InnerProduct's
    identity expanded once per run to dense G, as runtime.latent_operands does."""
    lay = dec.layout
    if lay.g_kind == "dense":
        G = lay.stacked(dec.flat, "G")
        G = G.view(d, d) if lay.G[3] == 1 else G.view(-1, d, d)
    else:
        key = ("topk_G", lay.g_kind, id(dec), d)
        if key not in ctx.cache:
            ctx.cache[key] = (torch.eye(d, device=ctx.session.device) if lay.g_kind == "eye"
                              else torch.diag_embed(lay.stacked(dec.flat, "G")).contiguous())
        G = ctx.cache[key]
    l = lay.stacked(dec.flat, "l") if lay.l_kind == "diag" else None
    return G, l


def first_relation(model, edge_type_ij) -> int:
    """The flat index (over all edge types, in model.edge_types' order) of relation 0 of an edge type."""
    ets = list(model.edge_types)
    return sum(model.edge_types[et] for et in ets[:ets.index(tuple(edge_type_ij))])


def _edge_type_record(ctx: RunContext, opt, model, edge_type_ij) -> dict:
    """What a run derives from an edge type's unchanging place among the optimizer's relations, per
    (optimizer, edge type) in the session caches: "first", its first_relation, and "latents", the
    set of its relations' latent nodes."""
    et = tuple(edge_type_ij)
    key = ("edge_type_record", id(opt), et)
    cache = ctx.session.caches
    if key not in cache:
        first = first_relation(model, et)
        rels = slice(first, first + model.edge_types[et])
        cache[key] = {"first": first, "latents": frozenset(opt.latent_inters[rels]) | frozenset(opt.latent_varies[rels])}
    return cache[key]


def latent_fed(ctx: RunContext, opt, model, edge_type_ij) -> bool:
    """Whether a latent matrix of any relation of the edge type is fed in this run."""
    return not _edge_type_record(ctx, opt, model, edge_type_ij)["latents"].isdisjoint(ctx.feeds)


def _edge_type_decoder(model, edge_type_ij, sigmoid):
    """The checks of an all-relation query that precede its sess.run; the edge type's decoder."""
    if sigmoid not in SIGMOID_MODES:
        raise ValueError(f"sigmoid must be one of {list(SIGMOID_MODES)}")
    if tuple(edge_type_ij) not in model.edge_type2decoder:
        raise ValueError(f"unknown edge type {tuple(edge_type_ij)}")
    return model.edge_type2decoder[tuple(edge_type_ij)]


def _edge_type_operands(name, ctx: RunContext, opt, model, edge_type_ij):
    """All relations of edge type (i, j) inside a run: (K, row table, column table, G, l), G and l
    as _stacked_latents gives them.  The decoder's variables are read in place, so a fed latent
    matrix is refused."""
    i, j = edge_type_ij
    dec = model.edge_type2decoder[i, j]
    if latent_fed(ctx, opt, model, (i, j)):
        raise ValueError(f"{name} reads the decoder's variables; a latent matrix is fed")
    row_t, col_t = opt._tables(ctx, i, j)
    G, l = _stacked_latents(ctx, dec, row_t.shape[1])
    return dec.num_types, row_t, col_t, G, l


def _sigmoid_host(x: np.ndarray, mode: Optional[str]) -> np.ndarray:
    """The reference's score of a float32 logit array (module docstring), on the host."""
    if mode is None:
        return x
    with np.errstate(over="ignore"):
        e = np.exp(-x.astype(np.float32))  # float32 exp, as both reference forms
        if mode == "main":
            return np.nan_to_num(1.0 / (1.0 + e.astype(np.float64)))
        return (np.float32(1.0) / (np.float32(1.0) + e)).astype(np.float32)


def top_candidates(sess, opt, placeholders, feed_dict, edge_type_ij, k: int, exclude=None, upper: bool = False,
                   no_diag: bool = False, sigmoid: Optional[str] = None):
    """For every relation of edge type (i, j), the k highest-scoring permitted pairs: numpy
    (scores [K, k], rows [K, k], cols [K, k], counts [K]); slots past counts[r] hold −inf / −1.

    What GreedyActiveLearner (main/ActiveLearner/GreedyActiveLearner.py:66-96) gets from
    session.run(predictions) → sigmoid → np.take(candidates) → argsort()[::-1][:n], one relation
    per run, here in one fused launch over all relations (dg_decoder_topk_f32): the model runs
    forward at dropout 0 and no N_i×N_j matrix is formed.  `exclude`: None, a
    sparse.ExclusionCSR, or one entry per relation as sparse.exclusion_csr takes them (e.g. the
    training adjacencies); `upper` keeps r < c, `no_diag` drops r == c.

    The ranking is by LOGIT (ties by smaller r·N_j + c).  `sigmoid` (a key of SIGMOID_MODES)
    only transforms the returned scores.  The sigmoid is monotonic, so this is the reference's
    ranking except inside saturated ties (logits the sigmoid maps to the same float, e.g. all
    above ≈36.7 under "main"), where the reference's own order is whatever numpy's unstable
    argsort leaves — unspecified."""
    model = opt._model()
    _edge_type_decoder(model, edge_type_ij, sigmoid)
    fd = dict(feed_dict)
    fd[placeholders["dropout"]] = 0.0

    def fn(ctx: RunContext):
        K, row_t, col_t, G, l = _edge_type_operands("top_candidates", ctx, opt, model, edge_type_ij)
        if G.dim() == 2 and l is None and K > 1:  # no per-relation parameter
            G = G.unsqueeze(0).expand(K, -1, -1).contiguous()
        ex = exclude
        if ex is not None and not hasattr(ex, "rowptr"):
            from .sparse import exclusion_csr
            ex = exclusion_csr(ex, (row_t.shape[0], col_t.shape[0]))
        return kernels.decoder_topk(row_t, col_t, G, l, k, exclude=ex, upper=upper, no_diag=no_diag)

    s, r, c, n = (np.asarray(t) for t in sess.run(Node("evaluate/top_candidates", fn), feed_dict=fd))
    if sigmoid is not None:
        valid = np.arange(s.shape[1])[None, :] < n[:, None]
        out = np.full(s.shape, -np.inf, np.float64 if sigmoid == "main" else np.float32)
        out[valid] = _sigmoid_host(s[valid], sigmoid)
        s = out
    return s, r, c, n


def _pairs(edges) -> Tuple[np.ndarray, np.ndarray]:
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    return e[:, 0].astype(np.int32), e[:, 1].astype(np.int32)


def accuracy_scores(sess, opt, placeholders, feed_dict, edges_pos, edges_neg, edge_type, edge_type2idx,
                    k: int = 50, sigmoid: Optional[str] = "main") -> Tuple[float, float, float]:
    """get_accuracy_scores (main.py:38-80) on the device: (roc, auprc, apk@k) of the edge
    type's sampled positive edges `edges_pos[edge_type[:2]][edge_type[2]]` against the sampled
    negatives, scored with the optimizer's decoder for that relation (dropout 0)."""
    fd = dict(feed_dict)
    fd[placeholders["dropout"]] = 0.0
    fd[placeholders["batch_edge_type_idx"]] = edge_type2idx[edge_type]
    fd[placeholders["batch_row_edge_type"]] = edge_type[0]
    fd[placeholders["batch_col_edge_type"]] = edge_type[1]
    pr, pc = _pairs(edges_pos[edge_type[:2]][edge_type[2]])
    nr, nc = _pairs(edges_neg[edge_type[:2]][edge_type[2]])

    def fn(ctx: RunContext):
        e, rt, ct = opt._edge(ctx)
        row_t, col_t = opt._tables(ctx, rt, ct)
        G, l = opt._latent(ctx, e)
        dev = ctx.session.device
        out = []
        for r, c in ((pr, pc), (nr, nc)):
            if r.size and (r.min() < 0 or r.max() >= row_t.shape[0] or c.min() < 0 or c.max() >= col_t.shape[0]):
                raise ValueError("edge sample outside the embedding tables")
            rd, cd = torch.from_numpy(r).to(dev), torch.from_numpy(c).to(dev)
            out.append(kernels.decoder_score(row_t, col_t, rd, cd, G, l) if r.size
                       else torch.empty(0, device=dev))
        return rank_metrics_device(out[0], out[1], k, sigmoid)

    au, ap, apk = sess.run(Node("evaluate/accuracy", fn), feed_dict=fd).tolist()
    return au, ap, apk


def rank_metrics_seg_device(pos: torch.Tensor, pos_ptr: torch.Tensor, neg: torch.Tensor, neg_ptr: torch.Tensor,
                            k: int = 50, sigmoid: Optional[str] = "main") -> torch.Tensor:
    """float64 device tensor [n_seg, 3]: row s = [AUROC, AUPRC, AP@k] of the positive logits
    pos[pos_ptr[s]:pos_ptr[s+1]] against the negative logits neg[neg_ptr[s]:neg_ptr[s+1]]
    (dg_rank_metrics_seg_f32) — bit for bit rank_metrics_device on that segment alone, for all
    segments in three launches.  pos_ptr / neg_ptr: device int32 [n_seg + 1], ascending from 0 to
    the length of pos / neg; they are not read on the host (asynchronous, graph-capturable)."""
    if sigmoid not in SIGMOID_MODES:
        raise ValueError(f"sigmoid must be one of {list(SIGMOID_MODES)}")
    if int(k) < 1:
        raise ValueError("k must be at least 1")
    for t, nm in ((pos, "pos"), (neg, "neg")):
        kernels._dev(t, torch.float32, nm)
    for t, nm in ((pos_ptr, "pos_ptr"), (neg_ptr, "neg_ptr")):
        kernels._dev(t, torch.int32, nm)
    n_seg = pos_ptr.numel() - 1
    if n_seg < 1 or neg_ptr.numel() != n_seg + 1:
        raise ValueError("pos_ptr and neg_ptr must both have n_seg + 1 >= 2 entries")
    lib = _lib.load()
    P, N = pos.numel(), neg.numel()
    nbytes = int(lib.dg_rank_metrics_seg_workspace(P, N, n_seg))
    ws = torch.empty(-(-nbytes // 8), dtype=torch.float64, device=pos_ptr.device)
    out = torch.empty((n_seg, 3), dtype=torch.float64, device=pos_ptr.device)
    check(lib.dg_rank_metrics_seg_f32(pos.data_ptr() if P else None, pos_ptr.data_ptr(), P,
                                      neg.data_ptr() if N else None, neg_ptr.data_ptr(), N, n_seg, int(k),
                                      SIGMOID_MODES[sigmoid], out.data_ptr(), ws.data_ptr(), ws.numel() * 8,
                                      kernels._stream_ptr(None)), "dg_rank_metrics_seg_f32")
    return out


def _relation_samples(edges, ij, r) -> np.ndarray:
    """The [n, 2] int64 samples of relation r in edges[ij] (a sequence or a mapping by relation);
    a missing relation, None or an empty array give [0, 2]."""
    per = edges.get(ij) if hasattr(edges, "get") else edges[ij]
    e = None
    if per is not None:
        if hasattr(per, "get"):
            e = per.get(r)
        elif 0 <= r < len(per):
            e = per[r]
    if e is None:
        return np.zeros((0, 2), np.int64)
    return np.asarray(e, dtype=np.int64).reshape(-1, 2)


def pack_edge_samples(edges_pos, edges_neg, edge_type_ij, num_relations: int, shape, relations=None):
    """The sampled edges of the relations of edge type (i, j), packed for one fused evaluation
    (host only): (row_idx, col_idx, pos_ptr, neg_ptr, relations), all numpy int32.

    row_idx / col_idx hold the positives of every listed relation, relation by relation in the
    order of `relations` (default: 0 .. num_relations − 1), then the negatives in the same order;
    relation relations[s]'s positives are row_idx[pos_ptr[s]:pos_ptr[s+1]] and its negatives
    row_idx[P + neg_ptr[s] : P + neg_ptr[s+1]] with P = pos_ptr[-1].  edges_pos / edges_neg are
    get_accuracy_scores' (main.py:38-80): edges[(i, j)][r] = an [n, 2] array; a relation that is
    missing, None or empty gives an empty segment.  An index outside `shape` = (N_i, N_j), or a
    relation outside [0, num_relations), raises ValueError."""
    ij = tuple(edge_type_ij)
    rels = np.arange(num_relations, dtype=np.int64) if relations is None else np.asarray(relations, np.int64).reshape(-1)
    if rels.size < 1:
        raise ValueError("no relations to evaluate")
    if rels.min() < 0 or rels.max() >= num_relations:
        raise ValueError(f"relation outside [0, {num_relations})")
    parts, ptrs = [], []
    for edges in (edges_pos, edges_neg):
        chunks = [_relation_samples(edges, ij, int(r)) for r in rels]
        ptr = np.zeros(rels.size + 1, np.int64)
        np.cumsum([len(c) for c in chunks], out=ptr[1:])
        parts.append(np.concatenate(chunks) if chunks else np.zeros((0, 2), np.int64))
        ptrs.append(ptr)
    allp = np.concatenate(parts)
    if allp.shape[0] >= 2**31 - 64 * (2 * rels.size + 1):
        raise ValueError("too many samples for 32-bit offsets")
    if allp.size and (allp.min() < 0 or allp[:, 0].max() >= shape[0] or allp[:, 1].max() >= shape[1]):
        raise ValueError("edge sample outside the embedding tables")
    return (np.ascontiguousarray(allp[:, 0], np.int32), np.ascontiguousarray(allp[:, 1], np.int32),
            ptrs[0].astype(np.int32), ptrs[1].astype(np.int32), rels.astype(np.int32))


def pack_node_queries(nodes, num_relations: int, n_nodes: int, relations=None):
    """The query nodes of the relations of an edge type, packed for one fused top_partners call
    (host only): (node_idx, seg_ptr, relations), all numpy int32.

    node_idx holds the nodes of every listed relation, relation by relation in the order of
    `relations` (default: 0 .. num_relations − 1); relation relations[s]'s are
    node_idx[seg_ptr[s]:seg_ptr[s+1]], in the order given.  `nodes` is a 1-D integer array (the same
    nodes for every listed relation) or a mapping {relation: array}; there a relation that is
    missing, None or empty gives an empty segment.  A node outside [0, n_nodes), a relation (listed,
    or a key of the mapping) outside [0, num_relations), a key of the mapping that is not among
    the listed relations and an array that is not 1-D raise ValueError."""
    rels = np.arange(num_relations, dtype=np.int64) if relations is None else np.asarray(relations, np.int64).reshape(-1)
    if rels.size < 1:
        raise ValueError("no relations to query")
    if rels.min() < 0 or rels.max() >= num_relations:
        raise ValueError(f"relation outside [0, {num_relations})")

    def one(a):
        a = np.zeros(0, np.int64) if a is None else np.asarray(a)
        if a.ndim != 1 or (a.size and not np.issubdtype(a.dtype, np.integer)):
            raise ValueError("nodes must be 1-D integer arrays")
        return a.astype(np.int64)

    if hasattr(nodes, "keys"):
        if any(not 0 <= int(r) < num_relations for r in nodes.keys()):
            raise ValueError(f"relation outside [0, {num_relations})")
        unlisted = sorted({int(r) for r in nodes.keys()} - set(rels.tolist()))
        if unlisted:
            raise ValueError(f"nodes given for relations {unlisted}, which are not among those listed")
        per = {int(r): one(a) for r, a in nodes.items()}
        chunks = [per.get(int(r), np.zeros(0, np.int64)) for r in rels]
    else:
        chunks = [one(nodes)] * rels.size
    ptr = np.zeros(rels.size + 1, np.int64)
    np.cumsum([c.size for c in chunks], out=ptr[1:])
    idx = np.concatenate(chunks)
    if idx.size + 32 * rels.size >= 2**31:
        raise ValueError("too many queries for 32-bit offsets")
    if idx.size and (idx.min() < 0 or idx.max() >= n_nodes):
        raise ValueError("query node outside the embedding table")
    return idx.astype(np.int32), ptr.astype(np.int32), rels.astype(np.int32)


def accuracy_scores_all(sess, opt, placeholders, feed_dict, edges_pos, edges_neg, edge_type_ij, relations=None,
                        k: int = 50, sigmoid: Optional[str] = "main", pooled: bool = False):
    """get_accuracy_scores (main.py:38-80) for ALL relations of edge type (i, j) in one fused pass:
    numpy float64 [K, 3], row s = (roc, auprc, apk@k) of relation relations[s] (default: every
    relation of the edge type, in order) — exactly what accuracy_scores returns for it.

    What the reference's final loop over edge_type2idx and DecagonAccuracyEvaluator.evaluateAll
    (DecagonAccuracyEvaluator.py:57-91) do one relation at a time: here one sess.run at dropout 0,
    one upload of the packed sample indices (pack_edge_samples), one scorer launch over the 2·K
    segments (dg_decoder_score_seg_f32: positives, then negatives), one segmented metrics call
    (dg_rank_metrics_seg_f32) and one copy back.  The decoder's variables are read in place for
    all four decoder types, so a fed latent matrix is refused, as in top_candidates.

    pooled=True also returns (auroc, auprc) of the samples of all listed relations concatenated —
    evaluateAll's pooled figures (DecagonAccuracyEvaluator.py:73-91) — as a second value:
    (scores [K, 3], (auroc, auprc)).  It is the same entry point with a single segment over the
    already contiguous score arrays, and it is off by default: its cost grows with
    P_total·(P_total + N_total), and it has NOT been measured at the polypharmacy shape."""
    model = opt._model()
    _edge_type_decoder(model, edge_type_ij, sigmoid)
    fd = dict(feed_dict)
    fd[placeholders["dropout"]] = 0.0

    def fn(ctx: RunContext):
        K, row_t, col_t, G, l = _edge_type_operands("accuracy_scores_all", ctx, opt, model, edge_type_ij)
        ri, ci, pos_ptr, neg_ptr, rels = pack_edge_samples(edges_pos, edges_neg, tuple(edge_type_ij), K,
                                                           (row_t.shape[0], col_t.shape[0]), relations)
        n_seg, P, N = rels.size, int(pos_ptr[-1]), int(neg_ptr[-1])
        # one upload: [row_idx | col_idx | seg_ptr (2·n_seg + 1) | seg_rel (2·n_seg) | neg_ptr | 0, P | 0, N]
        seg_ptr = np.concatenate([pos_ptr, P + neg_ptr[1:]])
        host = np.concatenate([ri, ci, seg_ptr, rels, rels, neg_ptr, [0, P], [0, N]]).astype(np.int32)
        buf = torch.from_numpy(host).to(ctx.session.device)
        n = P + N
        o = 2 * n
        d_ri, d_ci = buf[:n], buf[n:o]
        d_seg, o = buf[o:o + 2 * n_seg + 1], o + 2 * n_seg + 1
        d_rel, o = buf[o:o + 2 * n_seg], o + 2 * n_seg
        d_neg, o = buf[o:o + n_seg + 1], o + n_seg + 1
        d_pos = d_seg[:n_seg + 1]
        scores = kernels.decoder_score_seg(row_t, col_t, d_ri, d_ci, d_seg, G, l, seg_rel=d_rel)
        per = rank_metrics_seg_device(scores[:P], d_pos, scores[P:], d_neg, k, sigmoid)
        if not pooled:
            return per
        allm = rank_metrics_seg_device(scores[:P], buf[o:o + 2], scores[P:], buf[o + 2:o + 4], k, sigmoid)
        return torch.cat([per, allm])

    res = np.asarray(sess.run(Node("evaluate/accuracy_all", fn), feed_dict=fd), np.float64)
    if not pooled:
        return res
    return res[:-1], (float(res[-1, 0]), float(res[-1, 1]))


def _profile_query(name, sess, opt, placeholders, feed_dict, pairs, edge_type_ij, relations, sigmoid, run):
    """The part pair_profiles and top_relations share: checks, one sess.run at dropout 0 of a Node
    that uploads [row_idx | col_idx | rel_idx] once and returns run(row_t, col_t, ri, ci, G, l, rel_idx)."""
    model = opt._model()
    K = _edge_type_decoder(model, edge_type_ij, sigmoid).num_types
    pr = np.asarray(pairs, dtype=np.int64)
    if pr.ndim != 2 or pr.shape[1] != 2:
        raise ValueError("pairs must be an [n, 2] array")
    rels = np.arange(K, dtype=np.int64) if relations is None else np.asarray(relations, np.int64).reshape(-1)
    if rels.size < 1:
        raise ValueError("no relations to score")
    if rels.min() < 0 or rels.max() >= K:
        raise ValueError(f"relation outside [0, {K})")
    fd = dict(feed_dict)
    fd[placeholders["dropout"]] = 0.0

    def fn(ctx: RunContext):
        _, row_t, col_t, G, l = _edge_type_operands(name, ctx, opt, model, edge_type_ij)
        if pr.size and (pr.min() < 0 or pr[:, 0].max() >= row_t.shape[0] or pr[:, 1].max() >= col_t.shape[0]):
            raise ValueError("pair outside the embedding tables")
        n = pr.shape[0]
        host = np.concatenate([pr[:, 0], pr[:, 1], rels]).astype(np.int32)
        buf = torch.from_numpy(host).to(ctx.session.device)
        return run(row_t, col_t, buf[:n], buf[n:2 * n], G, l, buf[2 * n:])

    return sess.run(Node(f"evaluate/{name}", fn), feed_dict=fd), rels


def pair_profiles(sess, opt, placeholders, feed_dict, pairs, edge_type_ij, relations=None,
                  sigmoid: Optional[str] = None) -> np.ndarray:
    """The profile of node pairs: numpy [P, n_sel], entry [p, s] the score of relation
    relations[s] (default: every relation of edge type (i, j), in order; repeats allowed) for
    pair pairs[p] = (row node, column node).

    What the reference gets from NpPredictor(relationId)._predictEdges
    (main/Predictor/NpPredictor.py:293-313: E·D·R·D·Eᵀ of one relation, then the wanted entries)
    run per relation id, and from the per-relation session.run(predictions) of
    DecagonAccuracyEvaluator._computePredictions — here one sess.run at dropout 0, one upload of
    the indices, one launch over pairs × relations (dg_decoder_score_cross_f32) and one copy back.
    The decoder's variables are read in place for all four decoder types, so a fed latent matrix
    is refused, as in top_candidates.  `pairs` is checked on the host against the table sizes
    (ValueError).  `sigmoid` (a key of SIGMOID_MODES) transforms the returned logits."""
    def run(row_t, col_t, ri, ci, G, l, rel):
        return kernels.decoder_score_cross(row_t, col_t, ri, ci, G, l, rel_idx=rel)

    res, _ = _profile_query("pair_profiles", sess, opt, placeholders, feed_dict, pairs, edge_type_ij, relations,
                            sigmoid, run)
    return _sigmoid_host(np.asarray(res), sigmoid)


def _pair_exclusion(exclude, pairs, relations, num_relations: int, shape):
    """top_relations' `exclude` as a sparse.PairExclusion of this query (None stays None): a
    prebuilt one is checked against the query's pair and slot counts, anything else is built on
    the host against `pairs` and `relations` with the edge type's table sizes `shape`."""
    from .sparse import PairExclusion, pair_exclusion

    if exclude is None:
        return None
    n_pairs = int(np.asarray(pairs).reshape(-1, 2).shape[0])
    n_sel = int(num_relations) if relations is None else int(np.asarray(relations).size)
    if isinstance(exclude, PairExclusion):
        if (int(exclude.n_pairs), int(exclude.n_sel)) != (n_pairs, n_sel):
            raise ValueError(f"exclude: lists of {exclude.n_pairs} pairs × {exclude.n_sel} slots, "
                             f"the query has {n_pairs} × {n_sel}")
        if exclude.ptr.shape[0] != n_pairs + 1:
            raise ValueError("exclude: ptr must have one entry per pair and one more")
        return exclude
    return pair_exclusion(pairs, exclude, shape, relations, num_relations=num_relations)


def top_relations(sess, opt, placeholders, feed_dict, pairs, edge_type_ij, k: int, relations=None,
                  sigmoid: Optional[str] = None, exclude=None):
    """For every pair its k highest-scoring relations of edge type (i, j) — "for this pair of
    drugs, which side effects?": numpy (scores [P, k], relations [P, k] int32, counts [P] int32),
    descending; slots past counts[p] hold −inf / −1.

    Replaces the same reference paths as pair_profiles (NpPredictor.py:293-313 run per relation
    id; the per-relation session.run(predictions) of DecagonAccuracyEvaluator._computePredictions)
    followed by a sort of each pair's row on the host: here the pairs are scored in chunks and
    each chunk selected on the device (kernels.decoder_top_relations), so no P×K matrix is formed
    or copied.  `relations` restricts and orders the candidates (default: all, in order); the
    returned array holds relation numbers, not positions.

    The ranking is by LOGIT, ties by the earlier position in `relations`; `sigmoid` (a key of
    SIGMOID_MODES) only transforms the returned scores, as in top_candidates.

    `exclude` ranks every pair among the relations it is NOT yet known to have — the query for new
    side effects.  It replaces NpPredictor._predictEdges per relation id followed by dropping the
    known edges of each pair on the host (or, here, asking for k + known relations and filtering,
    which copies the widest pair's columns back for every pair and ends at DG_TOPK_MAX_K): the
    selection itself skips them (dg_row_topk_excl_f32).  None; a sparse.PairExclusion built for
    these `pairs` and `relations` (sparse.pair_exclusion: kept across calls it is uploaded once per
    device; its n_pairs and n_sel must match, ValueError); or what pair_exclusion takes — a
    sparse.ExclusionCSR, or one entry per relation of the edge type as sparse.exclusion_csr takes
    them (e.g. the training adjacencies), checked against the table sizes and turned into lists
    on the host.  counts[p] becomes min(k, candidates − excluded candidates of pair p)."""
    k = int(k)
    K = opt._model().edge_type2decoder.get(tuple(edge_type_ij))
    K = K.num_types if K is not None else 0  # (an unknown edge type is refused below)

    def run(row_t, col_t, ri, ci, G, l, rel):
        pe = _pair_exclusion(exclude, pairs, relations, K, (row_t.shape[0], col_t.shape[0]))
        lists = pe.device(ri.device) if pe is not None else None
        s, idx, n = kernels.decoder_top_relations(row_t, col_t, ri, ci, G, l, k, rel_idx=rel, exclude=lists)
        return torch.cat([s.view(torch.int32).reshape(-1), idx.reshape(-1), n])  # one copy back

    flat, rels = _profile_query("top_relations", sess, opt, placeholders, feed_dict, pairs, edge_type_ij,
                                relations, sigmoid, run)
    flat = np.asarray(flat, np.int32)
    P = flat.size // (2 * int(k) + 1)
    s = flat[:P * k].view(np.float32).reshape(P, k)
    idx, n = flat[P * k:2 * P * k].reshape(P, k), flat[2 * P * k:]
    rel = np.where(idx >= 0, rels.astype(np.int32)[np.maximum(idx, 0)], np.int32(-1)).astype(np.int32)
    if sigmoid is not None:
        valid = np.arange(s.shape[1])[None, :] < n[:, None]
        out = np.full(s.shape, -np.inf, np.float64 if sigmoid == "main" else np.float32)
        out[valid] = _sigmoid_host(s[valid], sigmoid)
        s = out
    return s, rel, n


RANK_SIDES = ("col", "row", "both")


def _side_query(name, sess, opt, placeholders, feed_dict, edge_type_ij, *, exclude, side, sigmoid, pack, call,
                own_checks=None):
    """The part edge_ranks and top_partners share: (packed, sides, flat).  Checks the side, the edge
    type and `sigmoid`, refuses a sharded session and a fed latent; then one sess.run at dropout 0
    of a Node that packs the query on the host — pack(K, shape) gives (queries, seg_ptr, relations,
    packed): the per-query index arrays (the row table's first), and what the result dictionary
    opens with — uploads [queries | seg_ptr | relations] once, and for every side returns the
    tensors of call(row_t, col_t, queries, seg_ptr, G, l, relations, exclude), all concatenated as
    int32 for one copy back.  Side "row" is the same call with the tables and the queries swapped,
    G transposed per relation and the exclusion transposed: `queries` is (row-table index,
    column-table index) for a query that is a pair — so it is reversed with the tables — or one
    array for a query that is a node of whichever table is the row table.  `own_checks()` raises
    the caller's own ValueErrors where they always stood: after the edge type's."""
    from .graph import InvalidArgumentError
    from .sparse import exclusion_csr

    if side not in RANK_SIDES:
        raise ValueError(f"side must be one of {list(RANK_SIDES)}")
    model = opt._model()
    _edge_type_decoder(model, edge_type_ij, sigmoid)
    if own_checks is not None:
        own_checks()
    if getattr(sess, "shard", None) is not None:
        raise NotImplementedError(f"{name} runs on one GPU (the session is sharded)")
    et = tuple(edge_type_ij)
    sides = ("col", "row") if side == "both" else (side,)
    fd = dict(feed_dict)
    fd[placeholders["dropout"]] = 0.0
    packed = {}

    def fn(ctx: RunContext):
        if latent_fed(ctx, opt, model, et):
            raise InvalidArgumentError(f"{name} reads the decoder's variables; a latent matrix is fed")
        K, row_t, col_t, G, l = _edge_type_operands(name, ctx, opt, model, et)
        shape = (row_t.shape[0], col_t.shape[0])
        queries, seg_ptr, rels, head = pack(K, shape)
        packed.update(head)
        ex = exclude
        if ex is not None and not hasattr(ex, "rowptr"):
            ex = exclusion_csr(ex, shape)
        if ex is not None and (int(ex.n_rels), int(ex.n_rows), int(ex.n_cols)) != (K,) + shape:
            raise ValueError(f"{name}: exclusion of {ex.n_rels} relations, {ex.n_rows} × {ex.n_cols}; "
                             f"the edge type has {K}, {shape[0]} × {shape[1]}")
        n, n_seg = queries[0].size, rels.size
        buf = torch.from_numpy(np.concatenate([*queries, seg_ptr, rels]).astype(np.int32)).to(ctx.session.device)
        d_q = [buf[n * t:n * (t + 1)] for t in range(len(queries))]
        d_seg, d_rel = buf[n * len(d_q):n * len(d_q) + n_seg + 1], buf[n * len(d_q) + n_seg + 1:]
        out = []
        for sd in sides:
            if sd == "col":
                out += call(row_t, col_t, d_q, d_seg, G, l, d_rel, ex)
            else:
                out += call(col_t, row_t, d_q[::-1], d_seg, G.transpose(-1, -2).contiguous(), l, d_rel,
                            ex.transposed() if ex is not None else None)
        return torch.cat([t.view(torch.int32).reshape(-1) for t in out])  # one copy back

    flat = np.asarray(sess.run(Node(f"evaluate/{name}", fn), feed_dict=fd), np.int32)
    return packed, sides, flat


def edge_ranks(sess, opt, placeholders, feed_dict, edges, edge_type_ij, relations=None, exclude=None,
               side: str = "col", no_self: bool = False) -> dict:
    """The filtered rank of held-out edges of edge type (i, j) — "given drug u and side effect k,
    where does the held-out partner v stand among all partners u could have?" — for every listed
    relation in one launch per side (dg_decoder_edge_rank_f32).

    What the reference offers is NpPredictor._predictEdges (main/Predictor/NpPredictor.py:293-313)
    per relation id: the whole N_i×N_j matrix, then a dense mask of the known edges and a count on
    the host.  Here: one sess.run at dropout 0, one upload of the packed indices, one launch per
    side and one copy back; no N_i×N_j matrix is formed.  The decoder's variables are read in
    place, so a fed latent matrix is refused (InvalidArgumentError), as is a sharded session.

    edges: the held-out positives as accuracy_scores_all takes them, edges[(i, j)][r] = [n, 2]
    (row node, column node); an index outside the tables raises ValueError (pack_edge_samples).
    relations: the relations to rank, in order (default: all).  exclude: None, a
    sparse.ExclusionCSR over all relations of the edge type, or one entry per relation as
    sparse.exclusion_csr takes them (e.g. the adjacencies): the known partners a query does not
    compete with — the query's own partner always stays a candidate.  side="col" ranks edge
    (u, v)'s column v among the columns of row u; "row" ranks u among the rows of column v (the
    same call with the tables swapped, G transposed per relation and the exclusion transposed;
    ties then go to the smaller row); "both" does both.  no_self drops the candidate that is the
    query node itself (square edge types).

    Returns {"relations": int32 [n_sel], "seg_ptr": int32 [n_sel + 1], and per side ("col" / "row")
    {"rank": int32 [n], "cand": int32 [n], "score": float32 [n]}}: query q of relation relations[s]
    lies in [seg_ptr[s], seg_ptr[s+1]), in the order of `edges`; 1 <= rank <= cand."""
    def pack(K, shape):
        ri, ci, seg_ptr, _, rels = pack_edge_samples(edges, {}, tuple(edge_type_ij), K, shape, relations)
        return [ri, ci], seg_ptr, rels, {"relations": rels, "seg_ptr": seg_ptr}

    def call(row_t, col_t, q, seg, G, l, rel, ex):
        return kernels.decoder_edge_rank(row_t, col_t, q[0], q[1], seg, G, l, seg_rel=rel, exclude=ex, no_self=no_self)

    res, sides, flat = _side_query("edge_ranks", sess, opt, placeholders, feed_dict, edge_type_ij, exclude=exclude,
                                   side=side, sigmoid=None, pack=pack, call=call)
    n = flat.size // (3 * len(sides))
    for t, sd in enumerate(sides):
        part = flat[3 * n * t:3 * n * (t + 1)]
        res[sd] = {"rank": part[:n].copy(), "score": part[n:2 * n].view(np.float32).copy(), "cand": part[2 * n:].copy()}
    return res


def ranking_metrics(rank, seg_ptr, hits=(1, 3, 10)) -> np.ndarray:
    """float64 [n_seg, 2 + len(hits)]: per segment s of `rank` (ranks >= 1 of queries
    [seg_ptr[s], seg_ptr[s+1])) the row [MRR, mean rank, Hits@h for h in hits] — the mean of
    1/rank, of rank and of (rank <= h).  An empty segment gives a row of NaN.  Host only."""
    rank = np.asarray(rank, np.float64).reshape(-1)
    ptr = np.asarray(seg_ptr, np.int64).reshape(-1)
    hits = tuple(int(h) for h in hits)
    if ptr.size < 1 or ptr[0] < 0 or np.any(np.diff(ptr) < 0) or ptr[-1] > rank.size:
        raise ValueError("seg_ptr must ascend within the ranks")
    if rank.size and rank[ptr[0]:ptr[-1]].min(initial=1.0) < 1:
        raise ValueError("ranks start at 1")
    out = np.full((ptr.size - 1, 2 + len(hits)), np.nan)
    for s in range(ptr.size - 1):
        r = rank[ptr[s]:ptr[s + 1]]
        if r.size:
            out[s] = [np.mean(1.0 / r), np.mean(r)] + [np.mean(r <= h) for h in hits]
    return out


def ranking_scores_all(sess, opt, placeholders, feed_dict, edges, edge_type_ij, relations=None, exclude=None,
                       side: str = "col", no_self: bool = False, hits=(1, 3, 10), pooled: bool = False):
    """Filtered MRR, mean rank and Hits@h of the held-out edges of every listed relation of edge
    type (i, j): numpy float64 [n_sel, 2 + len(hits)], row s = ranking_metrics of relation
    relations[s]'s ranks from edge_ranks (same arguments); with side="both" over the concatenation
    of both sides' ranks.  A relation without edges gives a row of NaN.  pooled=True also returns
    the same metrics over the queries of all listed relations, as a second value."""
    res = edge_ranks(sess, opt, placeholders, feed_dict, edges, edge_type_ij, relations, exclude, side, no_self)
    sides = ("col", "row") if side == "both" else (side,)
    ptr = res["seg_ptr"].astype(np.int64)
    per = [np.concatenate([res[sd]["rank"][ptr[s]:ptr[s + 1]] for sd in sides]) for s in range(ptr.size - 1)]
    lens = np.zeros(len(per) + 1, np.int64)
    np.cumsum([p.size for p in per], out=lens[1:])
    ranks = np.concatenate(per) if per else np.zeros(0, np.int32)
    rows = ranking_metrics(ranks, lens, hits)
    if not pooled:
        return rows
    return rows, ranking_metrics(ranks, [0, ranks.size], hits)[0]


def top_partners(sess, opt, placeholders, feed_dict, nodes, edge_type_ij, k: int, relations=None, exclude=None,
                 side: str = "col", no_self: bool = False, sigmoid: Optional[str] = None) -> dict:
    """For given nodes and every listed relation of edge type (i, j), each node's k best permitted
    partners — "given drug u and side effect k, which drugs are u's likeliest partners outside the
    known ones?" — in one launch pair per side (dg_decoder_node_topk_f32).

    What the reference offers is NpPredictor._predictEdges (main/Predictor/NpPredictor.py:293-313)
    per relation id: the whole N_i×N_j matrix, a dense mask of the known edges and a sort of each
    wanted row on the host.  Here: one sess.run at dropout 0, one upload of the packed indices
    (pack_node_queries), one launch pair per side and one copy back; no N_i×N_j matrix is formed.
    The decoder's variables are read in place, so a fed latent matrix is refused
    (InvalidArgumentError), as is a sharded session.

    nodes: a 1-D integer array (the same nodes for every listed relation) or {relation: array}; a
    node outside the table raises ValueError.  relations: the relations to query, in order
    (default: all).  exclude: as edge_ranks takes it — None, a sparse.ExclusionCSR over all
    relations of the edge type, or one entry per relation as sparse.exclusion_csr takes them (e.g.
    the adjacencies): the known partners, which are not listed.  side="col" lists the best column
    nodes of a row node; "row" the best row nodes of a column node (the same call with the tables
    swapped, G transposed per relation and the exclusion transposed; ties then go to the smaller
    row); "both" does both, and then a node must lie in both tables.  no_self drops the query node
    itself (square edge types).  k in [1, DG_NODE_TOPK_MAX_K].

    The ranking is by LOGIT (ties by the smaller partner); `sigmoid` (a key of SIGMOID_MODES) only
    transforms the returned scores, as in top_candidates.

    Returns {"relations": int32 [n_sel], "seg_ptr": int32 [n_sel + 1], "nodes": int32 [n], and per
    side ("col" / "row") {"partner": int32 [n, k], "score": [n, k], "count": int32 [n]}}: query q
    of relation relations[s] lies in [seg_ptr[s], seg_ptr[s+1]), in the order of `nodes`;
    count = min(k, permitted partners), slots past it hold −1 / −inf."""
    def k_in_range():
        if not 1 <= int(k) <= _lib.DG_NODE_TOPK_MAX_K:
            raise ValueError(f"top_partners: k must be in [1, {_lib.DG_NODE_TOPK_MAX_K}]")

    def pack(K, shape):
        n_nodes = min(shape) if side == "both" else shape[0] if side == "col" else shape[1]
        idx, seg_ptr, rels = pack_node_queries(nodes, K, n_nodes, relations)
        return [idx], seg_ptr, rels, {"relations": rels, "seg_ptr": seg_ptr, "nodes": idx}

    def call(row_t, col_t, q, seg, G, l, rel, ex):
        return kernels.decoder_node_topk(row_t, col_t, q[0], seg, G, l, k, seg_rel=rel, exclude=ex, no_self=no_self)

    res, sides, flat = _side_query("top_partners", sess, opt, placeholders, feed_dict, edge_type_ij, exclude=exclude,
                                   side=side, sigmoid=sigmoid, pack=pack, call=call, own_checks=k_in_range)
    k = int(k)
    n = flat.size // ((2 * k + 1) * len(sides))
    for t, sd in enumerate(sides):
        part = flat[(2 * k + 1) * n * t:(2 * k + 1) * n * (t + 1)]
        s = part[:n * k].view(np.float32).reshape(n, k).copy()
        count = part[2 * n * k:].copy()
        if sigmoid is not None:
            valid = np.arange(k)[None, :] < count[:, None]
            out = np.full(s.shape, -np.inf, np.float64 if sigmoid == "main" else np.float32)
            out[valid] = _sigmoid_host(s[valid], sigmoid)
            s = out
        res[sd] = {"partner": part[n * k:2 * n * k].reshape(n, k).copy(), "score": s, "count": count}
    return res

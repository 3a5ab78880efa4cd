"""One training step on a batch of EVERY relation: the summed cost Σ_(i,j) Σ_k cost_ijk (the hinge,
or the cross-entropy of an optimizer built with loss="xent").

The reference trains one (relation, batch) at a time (decagon/deep/optimizer.py:108-114 driven by
decagon/deep/minibatch.py:278-313): every step pays the whole two-layer forward, the whole
backward through both GCN layers over every relation and Adam on every variable, for the 512
edges of one side effect.  Neither GCN pass depends on the relation the batch came from — only
the decoder's gradient and its scatter into dE do — and the gradient of a sum of costs is the
sum of the gradients.  `train_step_all` therefore takes a batch of every relation, fills ONE dE
and runs one GCN backward and one Adam update: gradient accumulation over relations.

Per edge type: one sampler call (dg_unigram_sample_slots, unless the negatives are fed), one
scorer launch over the positive and negative pairs (dg_decoder_score_seg_f32), one cost sum
(dg_hinge_loss_ws_f32 / dg_xent_loss_ws_f32), one segmented decoder gradient
(dg_decoder_grad_seg_f32 / dg_decoder_grad_seg_xent_f32) and two row reductions into dE
(dg_segment_rows_sum_f32 over node-major occurrence lists, built by one stable device sort
each; the row side's weights are −1 / +1 for the hinge and the kernel's `coef` for the
cross-entropy).  The forward, the TrainPlan, the dropout masks, the embeddings
tables and the Adam slots are those of `opt_op`, so all-relation steps and ordinary steps mix.

The batches are host dicts, packed and uploaded per step, or an epochs.DeviceBatches formed on the
device from resident edges (epochs.EdgeBatches), which the step uses as it is; `train_epoch_all`
runs an epoch of the latter.
"""
from __future__ import annotations

import time
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import kernels
from .epochs import DeviceBatches, TypeBatch, _items
from .evaluate import _edge_type_record, _stacked_latents, latent_fed
from .graph import InvalidArgumentError, Node, RunContext

EdgeType = Tuple[int, int]


def pack_batches(batches, edge_types, shapes) -> Dict[EdgeType, Dict[str, np.ndarray]]:
    """Pack {edge type (i, j): {relation k: int array [n_k, 2] of (row, col)}} for the segmented
    kernels (host): per edge type int32 `rows`, `cols` [Σ n_k], `seg_ptr` [n_seg + 1] and
    `seg_rel` [n_seg], one segment per listed relation in the order given.  Empty batches are
    allowed (an empty segment).  A relation's batches may also be given as a sequence of
    (k, array) pairs.

    edge_types: {(i, j): number of relations}; shapes: {(i, j): (rows of type i, rows of type j)}.
    ValueError: an unknown edge type or relation, a relation listed twice, an index outside the
    edge type's shape, an array that is not [n, 2]."""
    out = {}
    for et, per_rel in _items(batches):
        et = tuple(int(x) for x in et) if isinstance(et, (tuple, list)) else et
        if et not in edge_types:
            raise ValueError(f"unknown edge type {et}")
        K = int(edge_types[et])
        n_r, n_c = (int(x) for x in shapes[et])
        arrs, rels, seen = [], [], set()
        for k, b in _items(per_rel):
            if int(k) != k or not 0 <= int(k) < K:
                raise ValueError(f"edge type {et}: unknown relation {k!r} (it has {K})")
            k = int(k)
            if k in seen:
                raise ValueError(f"edge type {et}: relation {k} listed twice")
            seen.add(k)
            b = np.asarray(b)
            if b.size == 0:
                b = np.zeros((0, 2), np.int64)
            if b.ndim != 2 or b.shape[1] != 2 or b.dtype.kind not in "iu":
                raise ValueError(f"edge type {et}, relation {k}: a batch is an integer array [n, 2]")
            arrs.append(b)
            rels.append(k)
        ptr = np.zeros(len(arrs) + 1, np.int64)
        np.cumsum([b.shape[0] for b in arrs], out=ptr[1:])
        cat = np.concatenate(arrs).astype(np.int64, copy=False) if arrs else np.zeros((0, 2), np.int64)
        # (the indices of all relations are checked at once; the culprit is looked up only on failure)
        bad = (cat < 0) | (cat >= np.asarray([n_r, n_c]))
        if bad.any():
            k = rels[int(np.searchsorted(ptr, int(np.nonzero(bad.any(axis=1))[0][0]), side="right")) - 1]
            raise ValueError(f"edge type {et}, relation {k}: index outside {(n_r, n_c)}")
        if ptr[-1] >= 2**31:
            raise ValueError(f"edge type {et}: too many pairs")
        out[et] = {"rows": np.ascontiguousarray(cat[:, 0], np.int32), "cols": np.ascontiguousarray(cat[:, 1], np.int32),
                   "seg_ptr": ptr.astype(np.int32), "seg_rel": np.asarray(rels, np.int32)}
    return out


def occurrence_list(idx: np.ndarray, n_out_rows: int):
    """The node-major occurrence list of an index array, on the host (what
    kernels.occurrence_list builds on the device): (node_ptr [n_out_rows + 1], order) with
    order[node_ptr[r] : node_ptr[r+1]] the positions of r in idx, ascending; indices outside
    [0, n_out_rows) are in no list."""
    idx = np.asarray(idx, np.int64)
    order = np.argsort(idx, kind="stable")
    node_ptr = np.searchsorted(idx[order], np.arange(n_out_rows + 1))
    return node_ptr.astype(np.int32), order.astype(np.int32)


def row_occurrences(rows: np.ndarray, neg_rows: np.ndarray, n_out_rows: int):
    """The row side's list for dg_segment_rows_sum_f32 over `mv` (stored once per pair): the
    occurrences of a node among the positive rows (sign −1) and the negative rows (sign +1),
    positives first: (node_ptr, item = the pair, sign)."""
    n = len(rows)
    node_ptr, order = occurrence_list(np.concatenate([rows, neg_rows]), n_out_rows)
    return node_ptr, (order % max(n, 1)).astype(np.int32), np.where(order < n, -1.0, 1.0).astype(np.float32)


def _negatives(neg_samples, packed, shapes) -> Dict[EdgeType, np.ndarray]:
    """Fed negatives, packed in the batches' segment order (one negative row per pair)."""
    out = {}
    for et, p in packed.items():
        if et not in neg_samples:
            raise ValueError(f"neg_samples has no entry for edge type {et}")
        per = dict(_items(neg_samples[et]))
        segs = []
        for s, k in enumerate(p["seg_rel"]):
            n = int(p["seg_ptr"][s + 1] - p["seg_ptr"][s])
            a = np.asarray(per.get(int(k), np.zeros(0, np.int64))).reshape(-1)
            if a.size != n:
                raise ValueError(f"edge type {et}, relation {int(k)}: {a.size} negatives for {n} pairs")
            if n and (a.min() < 0 or a.max() >= shapes[et][0]):
                raise ValueError(f"edge type {et}, relation {int(k)}: negative row outside [0, {shapes[et][0]})")
            segs.append(a)
        out[et] = (np.concatenate(segs) if segs else np.zeros(0)).astype(np.int32)
    return out


def _alias_stack(ctx: RunContext, opt, et: EdgeType, first: int, K: int) -> torch.Tensor:
    """The alias tables of an edge type's K relations as one [K, range, 2] tensor (session cache)."""
    key = ("sampler_stack", id(opt), et)
    cache = ctx.session.caches
    if key not in cache:
        cache[key] = torch.stack(opt._sampler(ctx).tables[first:first + K]).contiguous()
    return cache[key]


stage_log: Optional[dict] = None  # a dict here collects the step's stages in ms (scripts/epoch_bench.py)


def _stage(name: str, t0: float) -> float:
    """With `stage_log` set: synchronise, add the host time since t0 to stage `name`, return now."""
    if stage_log is None:
        return t0
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    stage_log[name] = stage_log.get(name, 0.0) + 1e3 * (t1 - t0)
    return t1


def type_batch(p: Dict[str, np.ndarray], negs: Optional[np.ndarray], device):
    """One edge type's packed host batches (pack_batches) as an epochs.TypeBatch on `device`, and
    its fed negatives there (`negs`, in segment order; None stays None) — one upload:
    [rows | cols | (negatives) | seg_ptr | seg_ptr[1:] + n | seg_rel | seg_rel]."""
    n, n_seg = int(p["seg_ptr"][-1]), len(p["seg_rel"])
    host = np.concatenate([p["rows"], p["cols"]] + ([negs] if negs is not None else []) +
                          [p["seg_ptr"], p["seg_ptr"][1:] + n, p["seg_rel"], p["seg_rel"]]).astype(np.int32)
    buf = torch.from_numpy(host).to(device)
    o = buf.numel() - (4 * n_seg + 1)
    seg2, rel2 = buf[o:o + 2 * n_seg + 1], buf[o + 2 * n_seg + 1:]
    tb = TypeBatch(buf[:n], buf[n:2 * n], seg2[:n_seg + 1], rel2[:n_seg], n, n_seg, seg2, rel2, p["seg_rel"])
    return tb, (buf[2 * n:3 * n] if negs is not None else None)


def _device_types(batches: DeviceBatches, edge_types, neg_samples, shapes, device):
    """A DeviceBatches' TypeBatches as they are, each with its fed negatives on `device` (or None)."""
    for et, tb in batches.items():
        if et not in edge_types:
            raise ValueError(f"unknown edge type {et}")
        if tb.n_seg > edge_types[et] or (tb.n_seg and int(tb.rel_host.max()) >= edge_types[et]):
            raise ValueError(f"edge type {et}: the batches list relations it does not have")
    if neg_samples is None:
        return {et: (tb, None) for et, tb in batches.items()}
    segs = {et: {"seg_ptr": np.arange(tb.n_seg + 1, dtype=np.int64) * batches.batch_size, "seg_rel": tb.rel_host}
            for et, tb in batches.items()}
    negs = _negatives(neg_samples, segs, shapes)
    return {et: (tb, torch.from_numpy(negs[et]).to(device)) for et, tb in batches.items()}


def _cached_latents(ctx: RunContext, rec: dict, dec, d: int):
    """_stacked_latents, kept across steps (in the edge type's record) where (G, l) are views of the
    decoder's flat buffer (DEDICOM, Bilinear: the optimizer updates it in place); the expanded forms
    depend on the variables' values and are rebuilt per run."""
    if dec.layout.g_kind != "dense":
        return _stacked_latents(ctx, dec, d)
    if rec.get("Gl_d") != d:
        rec["Gl"], rec["Gl_d"] = _stacked_latents(ctx, dec, d), d
    return rec["Gl"]


def train_step_all(sess, opt, placeholders, feed_dict, batches, neg_samples=None, apply: bool = True):
    """One step on Σ_(i,j) Σ_k cost of relation k's batch, the cost being opt.loss's (module docstring).

    batches: {(i, j): {k: int array [n_k, 2]}} (pack_batches' input).  neg_samples, in the same
    nesting ({(i, j): {k: int array [n_k]}}), feeds the negative rows; None draws relation k's
    from its own degree table on the device (dg_unigram_sample_slots with the optimizer's seed:
    the relations' tables gathered in segment order, draw c of the call's stream numbered
    slot0·n + c with n the common batch size and slot0 = ⌈draw counter / n⌉; the counter then
    stands after the last draw, so it advances by the number of draws whenever it was a multiple
    of n).  Drawing needs equal n_k within an edge type; otherwise feed the negatives.

    apply=True: one Adam update of every variable, with the slots `opt_op` uses (Adam's t advances
    once); returns the cost (float, before the update).  apply=False: (cost, grads_vars) with
    grads_vars exactly as `opt.grads_vars` returns it, nothing updated.

    batches may also be an epochs.DeviceBatches (EdgeBatches.batch): the step then uses its device
    arrays as they are — nothing is packed, no index array is uploaded (fed negatives apart) and
    nothing is read back before the cost.  Host batches are packed and uploaded once per edge type
    into the same form (type_batch) before the run; from there both forms take one path.  It takes
    the edge type's latent nodes and first relation from a per-(optimizer, edge type) record in the
    session caches, the operand views of DEDICOM and Bilinear from the same record, and the
    gradient slices from the decoder's layout — no walk over every relation's variables.  The same
    kernels run on the same indices: cost and gradients of the device form equal the host form's
    on EdgeBatches.host_batch bit for bit.

    NotImplementedError for a sharded session; InvalidArgumentError when a decoder latent of a
    trained edge type, or `outputs` / `neg_outputs` / `cost`, is fed."""
    model = opt._model()
    if getattr(sess, "shard", None) is not None:
        raise NotImplementedError("train_step_all runs on one GPU (the session is sharded)")
    shapes = {et: tuple(int(x) for x in opt.edge_type2dim[et][0]) for et in model.edge_types}
    if isinstance(batches, DeviceBatches):
        types = _device_types(batches, model.edge_types, neg_samples, shapes, sess.device)
    else:
        packed = pack_batches(batches, model.edge_types, shapes)
        if neg_samples is None:
            for et, p in packed.items():
                if len(set(np.diff(p["seg_ptr"]).tolist())) > 1:
                    raise ValueError(f"edge type {et}: batch sizes differ between relations; feed neg_samples")
        negs_host = _negatives(neg_samples, packed, shapes) if neg_samples is not None else {}
        types = {et: type_batch(p, negs_host.get(et), sess.device) for et, p in packed.items()}

    def fn(ctx: RunContext):
        opt._check_training(ctx)
        t0 = time.perf_counter()
        for et in types:
            if latent_fed(ctx, opt, model, et):
                raise InvalidArgumentError("train_step_all trains the decoder's variables; a latent matrix is fed")
        fwd, tp = opt._train_plan(ctx, model)
        if tp.sharded:
            raise NotImplementedError("train_step_all runs on one GPU (the plan is sharded)")
        dev = ctx.session.device
        dec_grads = opt._decoder_grad_buffers(ctx, model)
        t0 = _stage("forward", t0)
        costs, work = [], []
        for et, (tb, negs) in types.items():
            i, j = et
            n, n_seg, rows, cols = tb.n, tb.n_seg, tb.rows, tb.cols
            if n == 0:
                continue
            dec = model.edge_type2decoder[et]
            row_t, col_t = opt._tables(ctx, i, j)
            rec = _edge_type_record(ctx, opt, model, et)
            G, l = _cached_latents(ctx, rec, dec, row_t.shape[1])
            t0 = _stage("operands", t0)
            if negs is None:
                s = opt._sampler(ctx)
                stack = _alias_stack(ctx, opt, et, rec["first"], model.edge_types[et])
                if stack.shape[1] > row_t.shape[0]:
                    raise InvalidArgumentError("degrees list longer than the row embedding table")
                nk = n // n_seg  # (equal batch sizes, and n > 0: every segment holds nk >= 1 pairs)
                slot0 = -(-s.counter // nk)
                tabs = stack.index_select(0, tb.seg_rel.long()).contiguous()
                negs = kernels.unigram_sample_slots(tabs, slot0, nk, n, opt.seed, first_slot=slot0)
                s.counter = (slot0 + n_seg) * nk
            t0 = _stage("sampler", t0)
            # positives, then negatives (the positive batch's columns: optimizer.py:51-57)
            scores = kernels.decoder_score_seg(row_t, col_t, torch.cat([rows, negs]), torch.cat([cols, cols]), tb.seg2,
                                               G, l, seg_rel=tb.rel2)
            pos, neg = scores[:n], scores[n:]
            if opt.loss == "hinge":
                costs.append(kernels.hinge_loss(pos, neg, opt.margin, workspace=kernels.hinge_workspace(dev)))
            else:
                costs.append(kernels.xent_loss(pos, neg, opt.neg_sample_weights,
                                               workspace=kernels.hinge_workspace(dev)))
            t0 = _stage("score_hinge", t0)
            op = kernels.PreparedDecoderGradSeg(row_t, col_t, rows, cols, negs, tb.seg_ptr, tb.seg_rel, pos, neg, G, l,
                                                opt.margin, **dec.layout.grad_outputs(dec_grads[et]),
                                                loss=opt.loss, neg_weight=opt.neg_sample_weights)
            work.append((i, j, n, rows, cols, negs, op))
            t0 = _stage("gradient_setup", t0)

        def decoder_grad(dE):
            for i, j, n, rows, cols, negs, op in work:
                op()
                node_ptr, order = kernels.occurrence_list(torch.cat([rows, negs]), dE[i].shape[0])
                if opt.loss == "hinge":
                    sign = torch.where(order < n, -1.0, 1.0).to(torch.float32)
                else:  # (−a_p for a positive row's occurrence, +b_p for a negative row's)
                    sign = op.coef.index_select(0, order.long())
                kernels.segment_rows_sum(node_ptr, torch.remainder(order, n).to(torch.int32), op.mv, dE[i], sign=sign)
                node_ptr, order = kernels.occurrence_list(cols, dE[j].shape[0])
                kernels.segment_rows_sum(node_ptr, order, op.grad_cols, dE[j])

        tp.backward(decoder_grad)
        t0 = _stage("backward", t0)
        # (the edge types' sums are added on the host, in float64)
        cost = torch.cat([c.reshape(1) for c in costs]) if costs else torch.zeros(1, device=dev)
        out = cost, opt._finish_step(ctx, model, tp, dec_grads, apply)
        _stage("update", t0)
        return out

    node = Node("trainall/step", fn)
    node.training = True
    cost, gv = sess.run(node, feed_dict=dict(feed_dict))
    cost = float(np.asarray(cost, np.float64).sum())
    return cost if apply else (cost, gv)


def train_epoch_all(sess, opt, placeholders, feed_dict, eb, epoch: int, neg_samples=None) -> np.ndarray:
    """One epoch of all-relation steps from an epochs.EdgeBatches: steps 0 .. eb.steps(epoch) − 1,
    each `train_step_all` on `eb.batch(epoch, t)` (applied).  neg_samples: None (device-drawn
    negatives), or a callable (t, DeviceBatches) → the step's fed negatives.  Returns the steps'
    costs as a float64 array."""
    costs = []
    for t in range(eb.steps(epoch)):
        db = eb.batch(epoch, t)
        negs = neg_samples(t, db) if neg_samples is not None else None
        costs.append(train_step_all(sess, opt, placeholders, feed_dict, db, neg_samples=negs))
    return np.asarray(costs, np.float64)

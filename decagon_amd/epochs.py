"""Epochs of all-relation training: the train/validation split, the per-epoch shuffle and batch
serving — the counterpart of the reference's EdgeMinibatchIterator (decagon/deep/minibatch.py) for
`trainall.train_step_all`.

The shuffle is stateless.  `perm(n, key, x)` is a keyed bijection of [0, n) (an 8-round Feistel
network with cycle walking; csrc/permute.h defines it for the device and the host, this module
restates it in numpy, tests/test_cpu_epochs.py holds the two to the same integers), and relation
k's order in epoch e is x → perm(n_k, epoch_key(seed, e, global slot of k), x).  `EdgeBatches`
uploads the training edges once; `batch(epoch, t)` forms step t's batches of every relation that
still has one on the device (dg_epoch_batch_i32: one launch per edge type) and returns a
`DeviceBatches` that `train_step_all` consumes without packing or uploading index arrays.
`host_batch(epoch, t)` gives the same batches as numpy dicts.

`split_edges` is the host-side train/validation split with validation negatives.
"""
from __future__ import annotations

import bisect
from dataclasses import dataclass
from typing import Dict, List, Mapping, Optional, Tuple

import numpy as np

EdgeType = Tuple[int, int]

_M32 = np.uint64(0xFFFFFFFF)
PERM_ROUNDS = 8  # csrc/permute.h: kPermRounds
_SPLIT_EPOCH = 0x53504C54  # the "epoch" of the split's keys: no training epoch reaches it
_FALSE_TAG = 0x46414C53    # … and the tag of the false-edge candidate stream


def _items(per_rel):
    """(relation, array) pairs of a mapping, or of a sequence of such pairs."""
    return list(per_rel.items()) if isinstance(per_rel, Mapping) else [(k, v) for k, v in per_rel]


# ------------------------------------------------------------------ the permutation (numpy twin of permute.h)
def lowbias32(x):
    """csrc/dropout.h's lowbias32 on uint32 values (array or int), exact."""
    x = np.asarray(x, np.uint64) & _M32
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & _M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & _M32
    x = x ^ (x >> np.uint64(16))
    return x


def epoch_key(seed: int, epoch: int, slot: int) -> int:
    """permute.h's epoch_key: the key of global relation slot `slot` in epoch `epoch`."""
    seed = int(seed) & (2**64 - 1)
    a = int(lowbias32((seed & 0xFFFFFFFF) ^ ((int(slot) * 0x9E3779B9) & 0xFFFFFFFF)))
    b = ((seed >> 32) + int(epoch) * 0x85EBCA6B) & 0xFFFFFFFF
    return int(lowbias32(a ^ b))


def perm(n: int, key: int, x) -> np.ndarray:
    """permute.h's perm, vectorised over x (integers in [0, n)): int64 array of the images."""
    n = int(n)
    if not 1 <= n < 2**31:
        raise ValueError(f"perm: n = {n} outside [1, 2^31)")
    x = np.asarray(x, np.int64)
    if x.size and (x.min() < 0 or x.max() >= n):
        raise ValueError("perm: x outside [0, n)")
    if n == 1:
        return np.zeros(x.shape, np.int64)
    w = (n - 1).bit_length()
    lw = w >> 1
    hw = w - lw
    lmask, hmask = np.uint64((1 << lw) - 1), np.uint64((1 << hw) - 1)
    rk = [lowbias32((int(key) + (r + 1) * 0x9E3779B9) & 0xFFFFFFFF) for r in range(PERM_ROUNDS)]

    def encrypt(y):
        lo, hi = y & lmask, y >> np.uint64(lw)
        for r in range(PERM_ROUNDS):
            if r % 2 == 0:
                hi = hi ^ (lowbias32(lo ^ rk[r]) & hmask)
            else:
                lo = lo ^ (lowbias32(hi ^ rk[r]) & lmask)
        return (hi << np.uint64(lw)) | lo

    y = encrypt(x.astype(np.uint64).reshape(-1))
    while True:  # cycle walking: the elements that left [0, n) are encrypted again
        out = np.nonzero(y >= np.uint64(n))[0]
        if out.size == 0:
            break
        y[out] = encrypt(y[out])
    return y.astype(np.int64).reshape(x.shape)


# ------------------------------------------------------------------ batches
@dataclass
class TypeBatch:
    """One edge type's batches of a step, in the segmented kernels' layout: device int32 `rows`,
    `cols` [n], `seg_ptr` [n_seg + 1] (= arange·B) and `seg_rel` [n_seg] (the active relations,
    ascending), host ints `n`, `n_seg`.  `seg2` = [seg_ptr | seg_ptr[1:] + n] and `rel2` =
    [seg_rel | seg_rel] are the doubled forms the scorer takes over positives and negatives (seg_ptr
    and seg_rel are views of them); `rel_host` is seg_rel on the host."""
    rows: "object"
    cols: "object"
    seg_ptr: "object"
    seg_rel: "object"
    n: int
    n_seg: int
    seg2: "object"
    rel2: "object"
    rel_host: np.ndarray


class DeviceBatches:
    """Step t of epoch `epoch`: a TypeBatch per edge type that has an active relation
    (`db[(i, j)]`, `db.items()`); every segment holds exactly `batch_size` pairs."""

    def __init__(self, types: Dict[EdgeType, TypeBatch], batch_size: int, epoch: int, t: int):
        self.types, self.batch_size, self.epoch, self.t = types, batch_size, epoch, t

    def __getitem__(self, et):
        return self.types[et]

    def __contains__(self, et):
        return et in self.types

    def __len__(self):
        return len(self.types)

    def items(self):
        return self.types.items()

    def to_host(self) -> Dict[EdgeType, Dict[int, np.ndarray]]:
        """Downloaded, in host_batch's form: {(i, j): {k: int64 [B, 2]}} (synchronises)."""
        out = {}
        B = self.batch_size
        for et, tb in self.types.items():
            rc = np.stack([tb.rows.cpu().numpy(), tb.cols.cpu().numpy()], 1).astype(np.int64)
            out[et] = {int(k): rc[s * B:(s + 1) * B] for s, k in enumerate(tb.rel_host)}
        return out


class _TypeEdges:
    """One edge type's training edges (host), and its per-threshold device metadata."""

    def __init__(self, et, K, shape, first_slot, wraps, edges, ptr, B):
        self.et, self.K, self.shape, self.first_slot, self.wraps = et, K, shape, first_slot, wraps
        self.edges, self.ptr = edges, ptr  # int32 [N, 2] relation-major; int64 [K + 1]
        self.counts = np.diff(ptr)
        self.nb = self.counts // B
        self.levels = sorted(set(int(x) for x in self.nb))  # the distinct batch counts
        self.dev = None      # (edges, edge_ptr, wrap_mask) on the device
        self.meta = {}       # threshold level -> (rel_host, seg2, rel2)

    def level(self, t: int) -> int:
        """The index of t among the thresholds: the active list is the same for every t of a level."""
        return 0 if self.wraps else bisect.bisect_right(self.levels, t)

    def active(self, t: int) -> np.ndarray:
        return np.nonzero(self.nb >= 1 if self.wraps else self.nb > t)[0].astype(np.int32)


class EdgeBatches:
    """Serves every relation's shuffled batches of `batch_size` edges from device-resident edges.

    train_edges: {(i, j): {k: int array [n_k, 2] of (row, col)}} (pack_batches' nesting; a relation's
    edges may also be given as a sequence of (k, array) pairs; relations and edge types not listed
    have no edges).  edge_types: {(i, j): number of relations}, in the model's order (it numbers the
    global relation slots that key the permutations); shapes: {(i, j): (rows of type i, rows of type
    j)}.  device: a torch device, or None for a host-only object (`batch` then raises).

    Relation k takes part in step t of an epoch while t < ⌊n_k / B⌋ — it leaves the epoch when fewer
    than a full batch remains (minibatch.py:300-307), so the last n_k mod B edges of the epoch's order
    go unused.  The relations of the edge types in `wrap` wrap round instead (batch t mod ⌊n_k/B⌋ of
    the same order) and do not count toward the epoch's length, as the reference treats (0,0), (0,1)
    and (1,0) (minibatch.py:304-305).  Relations with n_k < B never take part: `skipped` lists them
    as ((i, j), k) (the reference would spin forever on a wrapping one).

    ValueError: as pack_batches — an unknown edge type or relation, a relation listed twice, an array
    that is not an integer [n, 2], an index outside the edge type's shape, too many pairs — and a
    batch size below 1 or an unknown edge type in `wrap`.  Indices are checked once, here, in one
    pass per edge type."""

    def __init__(self, train_edges, edge_types, shapes, batch_size, seed, device, wrap=()):
        if int(batch_size) != batch_size or int(batch_size) < 1:
            raise ValueError(f"batch_size must be a positive integer, got {batch_size!r}")
        self.batch_size = B = int(batch_size)
        self.seed = int(seed) & (2**64 - 1)
        self.edge_types = {tuple(et): int(K) for et, K in edge_types.items()}
        self.wrap = set()
        for et in wrap:
            et = tuple(int(x) for x in et)
            if et not in self.edge_types:
                raise ValueError(f"wrap: unknown edge type {et}")
            self.wrap.add(et)
        given = {}
        for et, per_rel in _items(train_edges):
            et = tuple(int(x) for x in et) if isinstance(et, (tuple, list)) else et
            if et not in self.edge_types:
                raise ValueError(f"unknown edge type {et}")
            if et in given:
                raise ValueError(f"edge type {et} listed twice")
            given[et] = per_rel
        self.types: Dict[EdgeType, _TypeEdges] = {}
        self.skipped: List[Tuple[EdgeType, int]] = []
        first = 0
        for et, K in self.edge_types.items():
            n_r, n_c = (int(x) for x in shapes[et])
            per = {}
            for k, b in _items(given.get(et, {})):
                if int(k) != k or not 0 <= int(k) < K:
                    raise ValueError(f"edge type {et}: unknown relation {k!r} (it has {K})")
                k = int(k)
                if k in per:
                    raise ValueError(f"edge type {et}: relation {k} listed twice")
                b = np.asarray(b)
                if b.size == 0:
                    b = np.zeros((0, 2), np.int64)
                if b.ndim != 2 or b.shape[1] != 2 or b.dtype.kind not in "iu":
                    raise ValueError(f"edge type {et}, relation {k}: the edges are an integer array [n, 2]")
                per[k] = b
            ptr = np.zeros(K + 1, np.int64)
            np.cumsum([per[k].shape[0] if k in per else 0 for k in range(K)], out=ptr[1:])
            arrs = [per[k] for k in range(K) if k in per]
            cat = np.concatenate(arrs).astype(np.int64, copy=False) if arrs else np.zeros((0, 2), np.int64)
            bad = (cat < 0) | (cat >= np.asarray([n_r, n_c]))
            if bad.any():
                k = int(np.searchsorted(ptr, int(np.nonzero(bad.any(axis=1))[0][0]), side="right")) - 1
                raise ValueError(f"edge type {et}, relation {k}: index outside {(n_r, n_c)}")
            if ptr[-1] >= 2**31 or 2 * K * B >= 2**31 - 512:
                raise ValueError(f"edge type {et}: too many pairs")
            te = _TypeEdges(et, K, (n_r, n_c), first, et in self.wrap, np.ascontiguousarray(cat, np.int32), ptr, B)
            self.types[et] = te
            self.skipped += [(et, int(k)) for k in np.nonzero(te.counts < B)[0]]
            first += K
        self.device = device
        if device is not None:
            import torch

            for te in self.types.values():
                mask = np.zeros(-(-te.K // 32), np.uint32)
                if te.wraps:
                    for k in range(te.K):
                        mask[k >> 5] |= np.uint32(1 << (k & 31))
                te.dev = (torch.from_numpy(te.edges).to(device), torch.from_numpy(te.ptr).to(device),
                          torch.from_numpy(mask.view(np.int32)).to(device) if te.wraps else None)

    # -------------------------------------------------------------- host logic
    def steps(self, epoch: int = 0) -> int:
        """Steps of an epoch: the largest ⌊n_k / B⌋ over the relations of the edge types that do
        not wrap (the same for every epoch).  ValueError when every edge type wraps."""
        tes = [te for te in self.types.values() if not te.wraps]
        if not tes:
            raise ValueError("every edge type wraps: the epoch has no length")
        return max([int(te.nb.max()) if te.K else 0 for te in tes])

    def active(self, et, t: int) -> np.ndarray:
        """The relations of edge type `et` that have a batch in step t (ascending, int32)."""
        if int(t) != t or t < 0:
            raise ValueError(f"step {t!r} is not a non-negative integer")
        return self.types[tuple(et)].active(int(t))

    def _key(self, te: _TypeEdges, epoch: int, k: int) -> int:
        return epoch_key(self.seed, epoch, te.first_slot + k)

    @staticmethod
    def _check_step(epoch, t):
        if int(epoch) != epoch or not 0 <= int(epoch) < 2**32:
            raise ValueError(f"epoch {epoch!r} outside [0, 2^32)")
        if int(t) != t or not 0 <= int(t) < 2**31:
            raise ValueError(f"step {t!r} outside [0, 2^31)")
        return int(epoch), int(t)

    def host_batch(self, epoch: int, t: int) -> Dict[EdgeType, Dict[int, np.ndarray]]:
        """Step t's batches on the host, by the numpy `perm`: {(i, j): {k: int64 [B, 2]}} over the
        edge types with an active relation — train_step_all's host input, and what `batch` holds."""
        epoch, t = self._check_step(epoch, t)
        B = self.batch_size
        out = {}
        for et, te in self.types.items():
            per = {}
            for k in te.active(t):
                k = int(k)
                n = int(te.counts[k])
                tb = t % int(te.nb[k]) if te.wraps else t
                q = perm(n, self._key(te, epoch, k), np.arange(tb * B, (tb + 1) * B))
                per[k] = te.edges[te.ptr[k] + q].astype(np.int64)
            if per:
                out[et] = per
        return out

    # -------------------------------------------------------------- device
    def _meta(self, te: _TypeEdges, t: int):
        lv = te.level(t)
        if lv not in te.meta:
            import torch

            rel = te.active(t)
            n_seg = len(rel)
            rel2 = torch.from_numpy(np.concatenate([rel, rel])).to(self.device)
            seg2 = torch.arange(2 * n_seg + 1, device=self.device, dtype=torch.int32) * self.batch_size
            te.meta[lv] = (rel, seg2, rel2)
        return te.meta[lv]

    def batch(self, epoch: int, t: int, stream=None) -> DeviceBatches:
        """Step t's batches on the device (asynchronous; no device→host synchronisation).  The
        active lists and their segment arrays are cached per threshold of t, so most steps upload
        nothing."""
        from . import kernels

        if self.device is None:
            raise RuntimeError("EdgeBatches was built without a device: only host_batch is available")
        epoch, t = self._check_step(epoch, t)
        B = self.batch_size
        types = {}
        for et, te in self.types.items():
            rel, seg2, rel2 = self._meta(te, t)
            n_seg = len(rel)
            if n_seg == 0:
                continue
            edges, edge_ptr, mask = te.dev
            seg_rel = rel2[:n_seg]
            rows, cols = kernels.epoch_batch(edges, edge_ptr, seg_rel, mask, B, t, epoch, self.seed, te.first_slot,
                                             bad_row=te.shape[0], stream=stream)
            types[et] = TypeBatch(rows, cols, seg2[:n_seg + 1], seg_rel, n_seg * B, n_seg, seg2, rel2, rel)
        return DeviceBatches(types, B, epoch, t)


# ------------------------------------------------------------------ the split
def _mulhi(h: np.ndarray, n: int) -> np.ndarray:
    return ((h * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def _false_edges(key: int, shape, edge_keys: np.ndarray, want: int) -> np.ndarray:
    """The first `want` distinct non-edges of the candidate stream c → (mulhi(lowbias32(key ^ 2c),
    n_r), mulhi(lowbias32(key ^ (2c + 1)), n_c)); edge_keys: the sorted row·n_c + col of the edges."""
    n_r, n_c = shape
    found = np.zeros(0, np.int64)
    c0, chunk = 0, max(64, 2 * want)
    while found.size < want:
        if c0 + chunk > 2**31:
            raise ValueError("split_edges: the candidate stream is exhausted")
        c = np.arange(c0, c0 + chunk, dtype=np.uint64)
        r = _mulhi(lowbias32(np.uint64(key) ^ (np.uint64(2) * c)), n_r)
        q = _mulhi(lowbias32(np.uint64(key) ^ (np.uint64(2) * c + np.uint64(1))), n_c)
        cand = r * n_c + q
        pos = np.searchsorted(edge_keys, cand)
        is_edge = (pos < edge_keys.size) & (edge_keys[np.minimum(pos, max(edge_keys.size - 1, 0))] == cand) \
            if edge_keys.size else np.zeros(cand.shape, bool)
        cand = cand[~is_edge & ~np.isin(cand, found)]
        _, firsts = np.unique(cand, return_index=True)  # first occurrences, back in stream order
        found = np.concatenate([found, cand[np.sort(firsts)]])
        c0, chunk = c0 + chunk, 2 * chunk
    found = found[:want]
    return np.stack([found // n_c, found % n_c], 1)


def split_edges(adj_mats, val_fraction: float = 0.01, min_val: int = 50, seed: int = 0, mirror=None):
    """The train/validation split of every relation (host, numpy):
    (train_edges, val_edges, val_edges_false, adj_train).

    adj_mats: {(i, j): [scipy sparse matrix per relation]}.  Per relation, sparse_to_tuple's n edges
    are ordered by `perm` under a key of the split (seed and the relation's global slot); the first
    num_val = min(max(min_val, ⌊n·val_fraction⌋), n // 2) are validation edges, the rest training
    edges.  val_edges_false are the first num_val distinct pairs that are not edges of the relation in
    a counter-based candidate stream (lowbias32 of (key, 2c) and (key, 2c + 1), scaled to the shape by
    multiply-high), found by membership in the sorted row·N_j + col keys; ValueError when the relation
    has fewer than num_val non-edges.  The first three results are {(i, j): {k: int64 [n, 2]}} —
    EdgeBatches' and accuracy_scores_all's inputs — and adj_train is {(i, j): [COO tuple per
    relation]}: sparse.preprocess_graph of the training edges.

    mirror: {(j, i): (i, j)} gives edge type (j, i) the flipped split of (i, j), relation by relation
    (the reference's _mask_test_edges_from_tpose).

    A deliberate departure from the reference: its _mask_test_edges_new leaves the false-edge loop
    after ONE false edge (a `break`, minibatch.py:202,216), so its validation negatives are a single
    pair per relation; this function builds the num_val false edges that code evidently intends.  The
    reference's test split is not built (the reference itself sets its size to zero)."""
    import scipy.sparse as sp

    from .sparse import preprocess_graph, sparse_to_tuple

    mirror = {tuple(a): tuple(b) for a, b in (mirror or {}).items()}
    ets = list(adj_mats)
    for a, b in mirror.items():
        if a not in adj_mats or b not in adj_mats or b in mirror:
            raise ValueError(f"mirror: {a} -> {b} does not name two edge types, the second split on its own")
        if len(adj_mats[a]) != len(adj_mats[b]):
            raise ValueError(f"mirror: {a} and {b} differ in their number of relations")
    if not 0 <= val_fraction <= 1 or int(min_val) != min_val or min_val < 0:
        raise ValueError("split_edges: val_fraction in [0, 1] and an integer min_val >= 0")
    train, val, false, adj_train = {}, {}, {}, {}
    first = {}
    slot = 0
    for et in ets:
        first[et] = slot
        slot += len(adj_mats[et])
    for et in [e for e in ets if e not in mirror]:
        train[et], val[et], false[et], adj_train[et] = {}, {}, {}, []
        for k, adj in enumerate(adj_mats[et]):
            m = sp.csr_matrix(adj)
            m.sum_duplicates()
            m.eliminate_zeros()
            coords, _, shape = sparse_to_tuple(m)
            coords = np.asarray(coords, np.int64)
            n = coords.shape[0]
            num_val = min(max(int(min_val), int(n * val_fraction)), n // 2)
            key = epoch_key(seed, _SPLIT_EPOCH, first[et] + k)
            order = coords[perm(n, key, np.arange(n))] if n else coords
            keys = np.sort(coords[:, 0] * shape[1] + coords[:, 1])
            if shape[0] * shape[1] - n < num_val:
                raise ValueError(f"edge type {et}, relation {k}: fewer than {num_val} pairs are not edges")
            val[et][k], train[et][k] = order[:num_val], order[num_val:]
            fkey = int(lowbias32(key ^ _FALSE_TAG))
            false[et][k] = _false_edges(fkey, shape, keys, num_val) if num_val else np.zeros((0, 2), np.int64)
            t = train[et][k]
            adj_train[et].append(preprocess_graph(sp.csr_matrix((np.ones(len(t)), (t[:, 0], t[:, 1])), shape=shape)))
    for a, b in mirror.items():
        flip = lambda d: {k: np.ascontiguousarray(v[:, ::-1]) for k, v in d.items()}  # noqa: E731
        train[a], val[a], false[a] = flip(train[b]), flip(val[b]), flip(false[b])
        adj_train[a] = []
        for k, adj in enumerate(adj_mats[a]):
            t = train[a][k]
            shape = tuple(int(s) for s in adj.shape)
            adj_train[a].append(preprocess_graph(sp.csr_matrix((np.ones(len(t)), (t[:, 0], t[:, 1])), shape=shape)))
    order = lambda d: {et: d[et] for et in ets}  # noqa: E731  (the caller's edge-type order)
    return order(train), order(val), order(false), order(adj_train)

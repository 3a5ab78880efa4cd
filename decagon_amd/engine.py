"""Device-resident relation graph and the fused two-layer GCN forward plan.

The reference rebuilds the full-graph forward inside every `sess.run` and re-feeds every
COO adjacency from the host each step (decagon/deep/minibatch.py:259-267, main.py:315).
Here the adjacencies are converted once to the chunk-merged CSR of dg_rel_group and uploaded
(`DeviceGraph`), all buffers are allocated once (`ForwardPlan`), and one forward is a fixed
sequence of launches — capturable into a hipGraph.  Per layer, per node type i:

  fused   (every group (i,j) is one chunk, single GPU)   dg_gcn_fused_f32
          Σ_k Â_k·X_k, l2norm per group, Σ_j, relu            layers.py:90-93, model.py:74-75
          (+ layer 1: the next layer's P_k = H1_i·W2_k)        layers.py:113
  partial (many relations, or sharded)                   dg_spmm_groups_f32 + dg_gcn_epilogue_f32
  projections not fused                                  dg_gemm_f32, all groups in one launch

With a relation shard (multi-GPU, sharding.py) each rank runs its relations only, writes or
reduces its chunk partials into one pre-normalisation sum per group, all-reduces those sums
(RCCL) and runs the same epilogue: the normalisation must follow the full Σ_k
(layers.py:92-93).  Every relation-indexed buffer (W1, the projections P, sparse-feature
products X·W1) is indexed by the GLOBAL relation id, so one merged layout serves both layers.
"""
from __future__ import annotations

import heapq
import math
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import kernels, wavetable
from ._lib import DG_EPI_L2NORM, DG_EPI_RELU, DG_MAX_GROUPS
from .peer import SLOT_FUSED, SLOT_KERNEL, SLOT_PROBE, PeerExchange, device_tensor
from .sparse import HostCSR, MergedCSR, chunk_segments, merge_chunks, merge_windows, staged_layout
from .tuning import knob

EdgeType = Tuple[int, int]


# LDS-staged groups (staged.hip): many relations over a column space narrow enough that one
# relation's 16-float column slice and the output rows' accumulators fit LDS.
STAGED_MIN_RELS = knob("DG_STAGED_MIN_RELS", 32)
STAGED_MAX_COLS = 1024
STAGED_MAX_ROWS = 1022
STAGED_BINS = knob("DG_STAGED_BINS", 128)


def drop_tag(layer: int, group: int) -> int:
    """The dropout mask stream of (layer, edge-type index): layer 1 masks rows of the
    relation-stacked W1 of the group, layer 2 masks elements of H1_j per relation."""
    return (layer << 16) | group


def stageable(n_rels: int, n_rows: int, n_cols: int) -> bool:
    return (knob("DG_STAGED", True) and n_rels >= STAGED_MIN_RELS
            and 0 < n_cols <= STAGED_MAX_COLS and 0 < n_rows <= STAGED_MAX_ROWS
            and kernels.staged_lds_bytes(n_rows, n_cols) <= kernels.STAGED_LDS_BYTES)


STAGED_TARGET_BLOCKS = knob("DG_STAGED_BLOCKS", 256)  # one round: a workgroup per CU

# Large groups whose relations fit one chunk (PPI: 2 x 19,085^2) are laid out in column
# windows (sparse.merge_windows): each window's gathers stay in its XCDs' L2.  Measured on
# config P's PPI (scripts/exp_window.py): d=64 63.6 us merged -> 40.0 us with 2 windows
# (+5.6 us epilogue); 4 windows 40.8, 8 windows 53.7 (the window partials start to cost).
# A rank's row block of such a group at N = 8 (2,386 protein rows) is windowed too, in twice
# as many windows (its launch is short of waves, not of L2): config P's N = 8 rank share
# (--simulate-world 8, max over ranks) 110.7 us without windows, 106.5 with 2, 106.0 with 4,
# 109.9 with 8 (round 5).
WINDOW_MIN_ROWS = knob("DG_WINDOW_MIN_ROWS", 1024)
WINDOW_FULL_ROWS = 4096  # below this many rows: 2 x N_WINDOWS windows
N_WINDOWS = knob("DG_WINDOWS", 2)
# node types with at most this many rows finish in the fused row-per-workgroup kernel; larger
# ones run partial mode + epilogue (one wave per row keeps more gathers in flight)
FUSED_MAX_ROWS = knob("DG_FUSED_MAX_ROWS", 4096)
# layer 2 of staged groups makes its slabs H1_j·W2_k on the MFMA inside the SpMM kernel
STAGED_PROJ = knob("DG_STAGED_PROJ", True)
# one-GPU plans whose node types all fit dg_gcn_fused_seg_f32 (config S) use it, layer 2
# reassociated; DG_FUSED_SEG=0 keeps dg_gcn_fused_f32 with the projection epilogue + P
FUSED_SEG = knob("DG_FUSED_SEG", True)
# config S's N-GPU rank share (seg mode): each row of the rank's block finished by one
# dg_gcn_fused_seg_f32 workgroup, one wave per relation of the row's N relation sets
# (DG_SEG_FUSED=0, or more relations a row: dg_spmm_seg_f32 partials + the epilogue launch)
SEG_FUSED = knob("DG_SEG_FUSED", True)
# ... when a row has at most 16 relations (one wave each: N <= 2 for config S).  A form whose 16
# waves looped over more relations measured 25.2 µs a rank share at N = 4 (seg + epilogue 25.1)
# and 35.6 at N = 8 (25.6), so it was not kept
SEG_FUSED_MAX_ITEMS = 16
# fused-seg and seg launches (config S on one GPU and its N-GPU row blocks) through their
# wave-table forms, dg_gcn_fused_tab_f32 / dg_spmm_seg_tab_f32 (host-built: each wave's segment
# bounds, gather base and finishing roles precomputed, its first pairs at a fixed slot; bitwise
# the same rows): config S's step 18.14 -> 15.56 us at 200 steps (round 5)
WAVE_TABLE = knob("DG_WAVE_TABLE", True)
# the wave-table fused launches deal each row's pairs over every wave slot of its workgroup
# (PreparedFusedTab balance, round 6) instead of one wave per relation: 0 never, 1 layer 1 only
# (d_in == d_out), 2 both layers
TAB_BALANCE = knob("DG_TAB_BALANCE", 1)
# one-GPU forward plans in the wave-table fused form (config S): layer 1's workgroups also make
# layer 2's operands P_k = H1_j·W2_k from the rows they finish (dg_gcn_fused_tab_post_f32: the
# reference's own order, layers.py:113-114), and layer 2 is a plain 32-wide gather-sum over the P
# stacks — half the gather bytes of the reassociated form, no W slab per (row, relation) wave, and
# free to deal a row's pairs over every wave as layer 1 does.  DG_L2_PREPROJECT=0, training,
# dropout, sharded plans, and plans whose projection jobs do not fit a workgroup's waves keep the
# reassociated layer 2
L2_PREPROJECT = knob("DG_L2_PREPROJECT", True)
# ... one wave projecting every row of its workgroup onto a relation (the W slab read once a
# workgroup: config S's layer 1 5.46 -> 5.31 us); 0: one (row, relation) a wave
L2_PREPROJECT_SHARE = knob("DG_L2_PREPROJECT_SHARE", True)
# ... with a launch's wave slots dealt in proportion to pairs (PreparedFusedTab weighted): a wave
# for every T pairs of a row's group in 16-slot workgroups, rows packed while their slots fit,
# instead of an equal share of the workgroup a row — a wave then runs one gather round (at most T
# pairs) whatever its row's length.  Only where _tab_balance holds (TAB_BALANCE = 0 keeps the
# per-relation tables); 0: the equal-share tables in both layers
TAB_WEIGHTED = knob("DG_TAB_WEIGHTED", 1)
# ... T per layer, 0 = that layer keeps its equal shares.  Layer 2 (32 floats a row): 48, one
# overlapped round of the gather ring — config S's step 13.22-13.29 -> 12.85-13.04 us, against
# 13.09 at 64 and 13.80-13.99 at 32 with layer 1 at 24.  Layer 1 (64 floats): off — weighted at
# 16 / 20 / 24 / 32 it measured slower than its equal shares at every T (24: +0.35 us), DESIGN §5
TAB_WEIGHTED_T64 = knob("DG_TAB_WEIGHTED_T64", 0)
TAB_WEIGHTED_T32 = knob("DG_TAB_WEIGHTED_T32", 48)
# ... and layer 2's launch in turn makes the DEDICOM decoder's row operands
# Q[r] = l ∘ ((E[r] ∘ l)·G) from the embedding rows it finishes (dg_gcn_fused_tab_dec_f32), for a
# decoder that attaches (ForwardPlan.attach_decoder_rows; kernels.PreparedDecoderHinge does): a
# score is then a 32-float dot product.  Read per attachment: DG_DEC_PREPROJECT=0 never attaches.
# sharded forward plans: layer 2 of the non-staged groups reassociated over the rank's own rows
# and relations, Σ_k (Â_k·H1_j)·W2_k in dg_spmm_seg_f32, instead of every rank projecting all of
# H1_j·W2_k (config P's PPI: 19,085 rows x 2 relations, 9.4 µs on every rank at N = 8)
REASSOC_ROWS = knob("DG_REASSOC_ROWS", True)


def _epilogue(targets, d: int, flags: int, peer=None, push=None):
    """An epilogue launch in its row-table form when the targets allow it (WAVE_TABLE), else
    dg_gcn_epilogue_multi_f32 / _peer_f32 — bitwise the same rows either way."""
    if WAVE_TABLE:
        try:
            return kernels.PreparedEpilogueTab(targets, d, flags, peer=peer, push=push)
        except ValueError:
            pass
    return kernels.PreparedEpilogueMulti(targets, d, flags, peer=peer, push=push)


# staged groups in variable-size output chunks (dg_staged_group.chunk_start): the relations are
# dealt LPT into about STAGED_TARGET_BLOCKS / 4 chunks (a 64-wide layer's), each split LPT in two
# for a 32-wide layer — instead of fixed runs of snake-binned relations, which at a rank's share
# (config P at N = 8: ~241 relations, 4 a chunk) put a 43 k-nonzero relation beside three others
STAGED_VAR = knob("DG_STAGED_VAR", True)


def _lpt_bins(costs: np.ndarray, items: np.ndarray, n_bins: int, cap: int) -> List[List[int]]:
    """items dealt largest first to the least-loaded bin that has room (< cap items); ties to the
    lower bin index (deterministic).  Every bin gets an item when len(items) >= n_bins."""
    order = items[np.argsort(-costs[items], kind="stable")]
    bins: List[List[int]] = [[] for _ in range(n_bins)]
    heap = [(0.0, b) for b in range(n_bins)]
    for it in order:
        full = []
        while True:
            load, b = heapq.heappop(heap)
            if len(bins[b]) < cap:
                break
            full.append((load, b))
        bins[b].append(int(it))
        heapq.heappush(heap, (load + float(costs[it]), b))
        for f in full:
            heapq.heappush(heap, f)
    return bins


def staged_var_chunks(costs: Sequence[float], n_top: int, split: int = 2, cap: int = 64):
    """Variable output chunks of a staged group: (device order of the relations, top-level chunk
    starts, sub-chunk starts).  The relations are dealt LPT into n_top chunks of <= cap, each
    chunk's relations LPT into <= split sub-chunks; the device order lists the chunks heaviest,
    lightest, second heaviest, ... (so runs of two merge evenly), sub-chunk by sub-chunk."""
    c = np.asarray(costs, np.float64)
    n = len(c)
    n_top = max(1, min(n_top, n))
    if n > n_top * cap:
        raise ValueError("more relations than chunks x cap")
    top = _lpt_bins(c, np.arange(n), n_top, cap)
    loads = np.array([c[b].sum() for b in top])
    by = list(np.argsort(-loads, kind="stable"))
    seq = []
    while by:
        seq.append(by.pop(0))
        if by:
            seq.append(by.pop())
    order, tops, subs = [], [0], [0]
    for b in seq:
        items = np.asarray(top[b], np.int64)
        for sb in _lpt_bins(c, items, min(split, len(items)), cap):
            order += sb
            subs.append(len(order))
        tops.append(len(order))
    return np.asarray(order, np.int64), np.asarray(tops, np.int32), np.asarray(subs, np.int32)


# ... and a relation costing more than STAGED_PIECE x a chunk's mean (a 32-wide layer's chunks are
# halves) is cut by rows into pieces of at most that (each piece its own staged "relation" reading
# the same slab): config P's N = 8 rank share holds 58 k-nonzero relations against chunks of ~45 k
STAGED_PIECE = knob("DG_STAGED_PIECE", 0.5)


def staged_pieces(loc: Sequence[HostCSR], costs: Sequence[float], n_top: int, frac: float):
    """Row pieces of the relations that cost more than frac x sum(costs) / n_top: a list of
    (relation index, HostCSR) — whole relations as themselves, heavy ones as pieces of consecutive
    rows of about equal nonzeros, at most that cost each (every row in exactly one piece, so a
    row's sum over a relation is the same arithmetic)."""
    mean = float(sum(costs)) / max(1, n_top)
    out = []
    for i, (c, cost) in enumerate(zip(loc, costs)):
        n_p = int(math.ceil(cost / (frac * mean))) if frac > 0 and cost > frac * mean else 1
        if n_p <= 1:
            out.append((i, c))
            continue
        rp = c.rowptr.astype(np.int64)
        cuts = np.searchsorted(rp, np.arange(1, n_p) * (c.nnz / n_p), side="left")
        bounds = np.unique(np.concatenate([[0], np.clip(cuts, 0, c.shape[0]), [c.shape[0]]]))
        for ra, rb in zip(bounds[:-1], bounds[1:]):
            p0, p1 = int(rp[ra]), int(rp[rb])
            if p1 == p0:
                continue
            prow = (np.clip(rp, p0, p1) - p0).astype(np.int32)
            out.append((i, HostCSR(prow, c.col[p0:p1], c.val[p0:p1], tuple(c.shape))))
    return out


def staged_chunk_starts(grp, d: int) -> Optional[np.ndarray]:
    """The variable output chunks of a staged group for a layer of width d (None: fixed runs of
    staged_out_chunk relations): the sub-chunks when the layer wants at least twice the top-level
    chunks of workgroups' worth (STAGED_TARGET_BLOCKS / slices), the top-level chunks when it
    wants at least as many, else runs of consecutive top-level chunks (heavy-light pairs)."""
    if grp.var_chunks is None:
        return None
    tops, subs = grp.var_chunks
    want = max(1, STAGED_TARGET_BLOCKS // -(-d // 16))
    n_top = len(tops) - 1
    if want >= 2 * n_top and len(subs) - 1 <= kernels.STAGED_MAX_CHUNKS:
        return subs
    if want >= n_top:
        return tops
    f = -(-n_top // want)
    st = tops[::f] if (n_top % f == 0) else np.concatenate([tops[::f], tops[-1:]])
    if np.diff(st).max() > 64:
        return None
    return st.astype(np.int32)


def _staged_n(grp) -> int:
    """Relations of a staged group's layout (row pieces counted one by one)."""
    lay = getattr(grp, "layout", None)
    return lay.n_rels if lay is not None else grp.n_rels


def staged_out_chunk(grp, d: int) -> int:
    """Relations per output chunk of a staged group for a layer of width d: a multiple of the
    group's snake-bin size (so chunks stay balanced) giving about STAGED_TARGET_BLOCKS
    workgroups of (chunk, 16-float slice) — one round on the chip, one LDS-full workgroup per CU.
    (With variable chunks, staged_chunk_starts: the largest chunk.)"""
    st = staged_chunk_starts(grp, d)
    if st is not None:
        return int(np.diff(st).max())
    n_slices = -(-d // 16)
    want = max(1, STAGED_TARGET_BLOCKS // n_slices)        # output chunks
    per = max(1, -(-_staged_n(grp) // want))
    oc = grp.out_chunk * max(1, -(-per // grp.out_chunk))
    return min(oc, 64)


# a staged relation's cost in "nonzeros": its nonzeros plus the per-relation overhead (slab
# copy, tables, barrier) of the staged kernel
STAGED_REL_OVERHEAD = 1500


def snake_bins(costs: Sequence[float], bin_size: int, max_swaps: int = 4000) -> np.ndarray:
    """An order of the items in which every run of `bin_size` consecutive items has about
    the same total cost (a staged launch's output chunk is one or more such runs).  The
    relation sizes are Zipf-skewed (P: 7.5 k - 58 k nonzeros), so dealing in snake order
    leaves the bin with the largest relation 10-50 % over the mean, and that bin's workgroup
    sets the launch time.  Here: rounds of n_bins items (largest first), each round's items
    to the bins in increasing load order; then pairwise swaps between the heaviest bin and
    any other that lower the heaviest load, until none does (deterministic).  Bins are
    emitted heaviest-with-lightest so that runs of two bins balance as well."""
    n = len(costs)
    n_bins = max(1, -(-n // bin_size))
    c = np.asarray(costs, np.float64)
    order = np.argsort(-c, kind="stable")
    B = np.full((n_bins, bin_size), -1, np.int64)     # item ids per bin (-1: empty slot)
    cap = np.full(n_bins, bin_size, np.int64)
    cap[-1] = n - (n_bins - 1) * bin_size               # only the last bin may be short
    fill = np.zeros(n_bins, np.int64)
    load = np.zeros(n_bins)
    r0 = 0
    while r0 < n:
        open_ = np.nonzero(fill < cap)[0]
        items = order[r0:r0 + len(open_)]
        tgt = open_[np.argsort(load[open_], kind="stable")[:len(items)]]
        B[tgt, fill[tgt]] = items
        fill[tgt] += 1
        load[tgt] += c[items]
        r0 += len(items)
    cost = np.where(B >= 0, c[np.maximum(B, 0)], np.nan)
    for _ in range(max_swaps):
        h = int(np.argmax(load))
        ch = cost[h]                                    # [bs]
        d = ch[None, :, None] - cost[:, None, :]        # [bins, bs_h, bs_l]: swap h's i with l's j
        with np.errstate(invalid="ignore"):
            new_max = np.maximum(load[h] - d, load[:, None, None] + d)
            gain = np.where((d > 0) & np.isfinite(d), load[h] - new_max, -np.inf)
        gain[h] = -np.inf
        k = int(np.argmax(gain))
        if not gain.flat[k] > 1e-9:
            break
        l, i, j = np.unravel_index(k, gain.shape)
        dd = d[l, i, j]
        B[h, i], B[l, j] = B[l, j], B[h, i]
        cost[h, i], cost[l, j] = cost[l, j], cost[h, i]
        load[h] -= dd
        load[l] += dd
    full = n_bins - 1 if cap[-1] < bin_size else n_bins
    by = list(np.argsort(-load[:full], kind="stable"))
    seq = []
    while by:
        seq.append(by.pop(0))
        if by:
            seq.append(by.pop())
    seq += list(range(full, n_bins))                     # the short bin last
    out = [int(i) for b in seq for i in B[b] if i >= 0]
    return np.asarray(out, np.int64)


def _tab_balance(d_in: int, d_out: int) -> bool:
    """TAB_BALANCE's choice for a wave-table fused launch (layer 1: d_in == d_out)."""
    return TAB_BALANCE >= 2 or (TAB_BALANCE == 1 and d_in == d_out)


def _tab_weighted(d_in: int, d_out: int) -> int:
    """TAB_WEIGHTED's T for a launch of the pre-projected plan (plain sums, d_in == d_out): 0 =
    the equal-share table."""
    if not (TAB_WEIGHTED and d_in == d_out and _tab_balance(d_in, d_out)):
        return 0
    return max(0, TAB_WEIGHTED_T64 if d_in == 64 else TAB_WEIGHTED_T32)  # (T = 0: this layer's equal shares)


def _tab_groups_fit(n_groups: Sequence[int], d: int) -> bool:
    """The wave-table fused form finishes a row in one wave, one lane set of d/4 lanes per group
    (PreparedFusedTab): at most 64 / (d/4) groups a target (n_groups: each target's count);
    otherwise the fused-seg form."""
    return all(k <= 64 // (d // 4) for k in n_groups)


def choose_chunk(n_rels: int, n_rows: int, nnz: int, d: int, target_waves: int = 32768) -> int:
    """Relations per chunk.  Partials cost 8·d bytes per (chunk, row) against ≈8 bytes per
    nonzero of CSR reads; keep them under a quarter of it, but keep at least `target_waves`
    waves (one per (chunk, row)) to fill 256 CUs when the group is big.  Small groups end
    up as one chunk, which is what lets the fused kernel finish the layer."""
    if n_rels <= 1 or n_rows == 0:
        return max(1, n_rels)
    avg = nnz / float(n_rels * n_rows)
    chunk_traffic = max(1, math.ceil(4.0 * d / max(avg, 1e-9)))
    chunk_par = max(1, (n_rels * n_rows) // target_waves)
    chunk = chunk_par if chunk_traffic <= chunk_par else chunk_traffic
    return int(min(max(1, chunk), n_rels))


def row_slice(c: HostCSR, a: int, b: int) -> HostCSR:
    """Rows [a, b) of a CSR relation (a row-split rank's block), columns unchanged."""
    p0, p1 = int(c.rowptr[a]), int(c.rowptr[b])
    return HostCSR((c.rowptr[a:b + 1] - p0).astype(np.int32), c.col[p0:p1], c.val[p0:p1], (b - a, c.shape[1]))


@dataclass
class DeviceGroup:
    """One (i,j) group's (local) relations on the device, chunk-merged."""

    edge_type: EdgeType
    n_rows: int
    n_cols: int
    K: int                         # relations of the group in the whole graph (slab count)
    rel_ids: np.ndarray            # global relation id of each local relation
    chunk: int
    n_chunks: int
    rowptr: torch.Tensor
    vcol: torch.Tensor
    val: torch.Tensor
    nnz: int
    vcol_max: int
    rel_map: Optional[torch.Tensor] = None   # device rel_ids, when not 0..K-1
    staged: bool = False           # runs through dg_spmm_staged_f32 (layout: chunk = 1)
    out_chunk: int = 1             # staged: snake-bin size (a layer's output chunk is a multiple)
    # staged, variable chunks (STAGED_VAR): (top-level chunk starts, sub-chunk starts), device order
    var_chunks: Optional[Tuple[np.ndarray, np.ndarray]] = None
    # staged, heavy relations in row pieces (staged_pieces): the layout's slab per piece (global
    # relation id; the layout then lists pieces, not rel_ids' relations); None: rel_map
    staged_slab: Optional[torch.Tensor] = None
    layout: Optional["kernels.StagedDevice"] = None  # staged: the diagonal-major layout
    host: Optional[List[HostCSR]] = None  # the local relations (host CSR), device order
    seg: Optional[torch.Tensor] = None    # dg_spmm_seg_f32's segment starts (sparse.chunk_segments)
    # a windowed row-split group's second layout for the reassociated layer 2 (all its relations
    # in one chunk, with segment starts): (rowptr, vcol, val, seg, chunk, n_chunks, vcol_max)
    seg2: Optional[tuple] = None

    @property
    def n_rels(self) -> int:
        return int(self.rel_ids.shape[0])


class DeviceGraph:
    """Every (i,j) group's relations, chunk-merged and uploaded once.

    adj[(i,j)] lists the K_ij relations (HostCSR, or None for relations another rank owns);
    `local` restricts each group to a subset (a rank's shard); `chunk` overrides the
    relations-per-chunk policy (an int for every group, or a dict per edge type)."""

    def __init__(self, edge_types: Dict[EdgeType, int], adj: Dict[EdgeType, Sequence[Optional[HostCSR]]],
                 device: torch.device, local: Optional[Dict[EdgeType, Sequence[int]]] = None,
                 chunk=None, target_waves: int = 32768, d_policy: int = 64,
                 row_block: Optional[Dict[int, Tuple[int, int, int]]] = None, segments: bool = True):
        """segments: also upload each chunk-merged group's segment starts (sparse.chunk_segments)
        for dg_spmm_seg_f32 — groups of at most 16 relations per chunk."""
        self.edge_types = dict(edge_types)
        self.device = device
        self.groups: Dict[EdgeType, DeviceGroup] = {}
        self.n_nodes: Dict[int, int] = {}
        self.sharded = local is not None
        # row-split node types (sharding.py): this rank holds rows [a, b) of every relation
        # into them; their groups' output rows are local row indices
        self.row_block = dict(row_block or {})
        for et, K in self.edge_types.items():
            rels = list(adj[et])
            if len(rels) != K:
                raise ValueError(f"edge type {et}: {len(rels)} matrices fed, {K} expected")
            known = [r for r in rels if r is not None]
            if not known:
                raise ValueError(f"edge type {et}: no relation given")
            n_r, n_c = known[0].shape
            for t, n in ((et[0], n_r), (et[1], n_c)):
                if self.n_nodes.setdefault(t, n) != n:
                    raise ValueError(f"node type {t}: inconsistent sizes {self.n_nodes[t]} vs {n}")
            ids = np.arange(K, dtype=np.int32) if local is None else np.asarray(local[et], np.int32)
            if any(rels[k] is None for k in ids):
                raise ValueError(f"edge type {et}: a local relation was not given")
            loc = [rels[k] for k in ids]
            if et[0] in self.row_block:
                a, b, _ = self.row_block[et[0]]
                loc = [row_slice(c, a, b) for c in loc]
                n_r = b - a
            nnz = int(sum(c.nnz for c in loc))
            ch = chunk.get(et) if isinstance(chunk, dict) else chunk
            staged = ch is None and stageable(len(loc), n_r, n_c)
            out_chunk = 1
            if staged:
                # one chunk per relation; output chunks of out_chunk relations with balanced
                # nonzero counts (relation sizes are Zipf-skewed)
                out_chunk = max(1, -(-len(loc) // STAGED_BINS))
                costs = [c.nnz + STAGED_REL_OVERHEAD for c in loc]
                var, pieces = None, None
                n_top = max(1, STAGED_TARGET_BLOCKS // -(-d_policy // 16))
                if STAGED_VAR:
                    pieces = staged_pieces(loc, costs, n_top, STAGED_PIECE)
                    if len(pieces) == len(loc):
                        pieces = None
                n_v = len(pieces) if pieces is not None else len(loc)
                if STAGED_VAR and n_v <= 65535 and n_v <= 64 * n_top:
                    vcosts = costs if pieces is None else [c.nnz + STAGED_REL_OVERHEAD for _, c in pieces]
                    perm, tops, subs = staged_var_chunks(vcosts, n_top)
                    var = (tops, subs)
                else:
                    pieces = None
                    perm = snake_bins(costs, out_chunk)
                if pieces is None:
                    ids = ids[perm]
                    loc = [loc[i] for i in perm]
                    stage_loc, stage_slab = loc, None
                else:  # the pieces in device order; the group's relations keep their order
                    stage_loc = [pieces[i][1] for i in perm]
                    stage_slab = ids[np.asarray([pieces[i][0] for i in perm], np.int64)].astype(np.int32)
                ch = 1
            if ch is None:
                ch = choose_chunk(len(loc), n_r, nnz, d_policy, target_waves)
            windows = (not staged and loc and ch >= len(loc) and n_r >= WINDOW_MIN_ROWS
                       and N_WINDOWS > 1 and (chunk is None))
            if windows:
                m = merge_windows(loc, ids, N_WINDOWS if n_r >= WINDOW_FULL_ROWS else 2 * N_WINDOWS, K)
            elif loc:
                m = merge_chunks(loc, ids, ch, K)
            else:
                m = MergedCSR(np.zeros(n_r + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32),
                              n_r, n_c, 1, 1, K * n_c)
            g = DeviceGroup(
                et, n_r, n_c, K, ids, m.chunk, m.n_chunks,
                torch.from_numpy(m.rowptr).to(device), torch.from_numpy(m.vcol).to(device),
                torch.from_numpy(m.val).to(device), m.nnz,
                int(m.vcol.max()) if m.nnz else -1)
            if ids.size and not np.array_equal(ids, np.arange(K)):
                g.rel_map = torch.from_numpy(ids).to(device)
            g.staged, g.out_chunk = staged, out_chunk
            if staged:
                g.var_chunks = var
                if stage_slab is not None:
                    g.staged_slab = torch.from_numpy(stage_slab).to(device)
            g.host = loc  # local relations in device order (the backward builds Âᵀ from them)
            if segments and loc and not staged and not windows and m.chunk <= 16:
                g.seg = torch.from_numpy(chunk_segments(loc, m)).to(device)
            elif windows and et[0] in self.row_block and len(loc) <= 16 and REASSOC_ROWS:
                # (sharded: layer 2 of this group reassociated over the rank's rows, ForwardPlan)
                m2 = merge_chunks(loc, ids, len(loc), K)
                up = lambda a: torch.from_numpy(a).to(device)  # noqa: E731
                g.seg2 = (up(m2.rowptr), up(m2.vcol), up(m2.val), up(chunk_segments(loc, m2)), m2.chunk, m2.n_chunks,
                          int(m2.vcol.max()) if m2.nnz else -1)
            if staged:
                lay = staged_layout(stage_loc, kernels.staged_block,
                                    lanes=knob("DG_STAGED_LANES", 1024),
                                    split=knob("DG_STAGED_SPLIT", True))
                g.layout = kernels.StagedDevice.upload(lay, device)
            self.groups[et] = g

    @property
    def total_nnz(self) -> int:
        return sum(g.nnz for g in self.groups.values())


@dataclass
class LayerWeights:
    """Weight stacks of one layer: per (i,j) group a tensor [K, d_in, d_out] (device)."""

    stacks: Dict[EdgeType, torch.Tensor]


@dataclass
class LayerForms:
    """The launch form of one layer of a plan (decide_forms)."""

    layer: int  # 1 or 2: the width, relu, outputs, padded buffers and peer slots follow from it
    d: int      # output width
    d_in: int   # operand width of its seg launches: h1 where layer 2 is reassociated, else d
    # "seg_rows": one launch finishes this rank's row block of every node type (seg mode);
    # "fused_seg": the one-GPU fused-seg / wave-table launch; "fused": dg_gcn_fused_f32 over
    # plan.fused, the other node types partial; "partial": SpMM launches and a finishing step
    kind: str = "partial"
    # seg_rows / fused_seg: "tab" the wave-table form, "narrow" its 32 -> 32 form over the P
    # stacks layer 1 made, "" dg_gcn_fused_seg_f32
    table: str = ""
    peer_red: bool = False  # the pushing epilogue launch carries the peer all-reduce

    @property
    def relu(self) -> bool:
        return self.layer == 1


@dataclass
class PlanForms:
    """Every launch-form decision of one ForwardPlan (decide_forms); the plan mirrors the
    fields of FORM_ATTRS as attributes of the same names."""

    flat_mode: bool = False
    sums_mode: bool = False  # partial mode whose epilogue also writes each S_ij
    seg_mode: bool = False
    fused_seg: bool = False
    peer_reduce: bool = False
    tab_weighted: bool = False
    fused: List[int] = field(default_factory=list)
    staged_proj: set = field(default_factory=set)
    preproj: set = field(default_factory=set)
    seg_proj: set = field(default_factory=set)
    proj_fused: List[EdgeType] = field(default_factory=list)  # projected by the launch finishing H1_j
    peer_fit: bool = True  # the peer all-reduce's targets fit ONE epilogue launch (_peer_reduce_fits)
    layers: Dict[int, LayerForms] = field(default_factory=dict)


FORM_ATTRS = ("flat_mode", "sums_mode", "seg_mode", "fused_seg", "peer_reduce", "tab_weighted", "fused",
              "staged_proj", "preproj", "seg_proj")


def _targets(dgraph: DeviceGraph) -> Dict[int, List[EdgeType]]:
    """Node type -> the edge types into it, in the graph's order."""
    targets: Dict[int, List[EdgeType]] = {}
    for et in dgraph.edge_types:
        targets.setdefault(et[0], []).append(et)
    if any(len(v) > DG_MAX_GROUPS for v in targets.values()):
        raise ValueError(f"more than {DG_MAX_GROUPS} edge types into one node type")
    return targets


def _local_rows(dgraph: DeviceGraph, i: int) -> int:
    """Rows of node type i this rank finishes (a row-split rank: its block)."""
    if i in dgraph.row_block:
        return dgraph.row_block[i][1] - dgraph.row_block[i][0]
    return dgraph.n_nodes[i]


def _fused_targets(dgraph: DeviceGraph, targets, sharded: bool, keep_sums: bool, fused_rows: bool) -> List[int]:
    """Node types one dg_gcn_fused_f32 launch finishes: at most FUSED_MAX_ROWS (local) rows,
    every group one chunk (and not staged).  Sharded plans finish only row-split node types
    this way, when the shard asks for it (`fused_rows`: their rows are complete on this
    rank; relation-sharded ones need the all-reduce first), and the sharded backward takes
    none."""
    row_block, groups = dgraph.row_block, dgraph.groups
    if sharded and (keep_sums or not row_block or not fused_rows):
        return []
    return [i for i, ets in targets.items()
            if (not sharded or i in row_block)
            and 0 < _local_rows(dgraph, i) <= FUSED_MAX_ROWS
            and all(groups[et].n_chunks == 1 and groups[et].n_rels > 0 and not groups[et].staged for et in ets)]


def _preproject_fit(targets, rels: Dict[EdgeType, int], h1: int) -> Tuple[bool, bool]:
    """(Layer 1's wave-table workgroups have a wave slot for every (row, sourced relation):
    L2_PREPROJECT can hold; so have TAB_WEIGHTED's weighted workgroups for a row's jobs)."""
    order = list(targets)
    if any(et[1] not in targets for et in rels):
        return False, False
    if not _tab_groups_fit([len(targets[i]) for i in order], h1):  # (layer 2's 32-wide bound is the looser)
        return False, False
    waves_t = [sum(rels[et] for et in targets[i]) for i in order]
    sourced_t = [sum(k for et, k in rels.items() if et[1] == i) for i in order]
    if not wavetable.tab_proj_fit(waves_t, sourced_t, _tab_balance(h1, h1), L2_PREPROJECT_SHARE):
        return False, False
    return True, wavetable.weighted_proj_fit(sourced_t, L2_PREPROJECT_SHARE)


def _epilogue_fits(n_targets: int, n_groups: int) -> bool:
    """Whether ONE epilogue launch takes these targets (dg_gcn_epilogue_multi_f32 / _peer_f32)."""
    return n_targets <= 8 and n_groups <= DG_MAX_GROUPS


def _peer_reduce_fits(dgraph: DeviceGraph, targets) -> bool:
    """Whether the pushing epilogue launch can carry the peer all-reduce: the row-split node
    types plus every relation-sharded node type with local relations as targets of ONE
    dg_gcn_epilogue_peer_f32 launch.  A larger graph keeps the flat buffer and the RCCL
    all-reduce instead (it used to raise)."""
    t = [i for i in targets if i in dgraph.row_block]
    t += [i for i in targets if i not in dgraph.row_block and any(dgraph.groups[et].n_rels for et in targets[i])]
    return _epilogue_fits(len(t), sum(len(targets[i]) for i in t))


def _layer_forms(f: PlanForms, dgraph: DeviceGraph, layer: int, h1: int, h2: int) -> LayerForms:
    """One layer's launch form under the plan-wide forms f."""
    targets = _targets(dgraph)
    d = h1 if layer == 1 else h2
    reassoc = layer == 2 and bool(f.seg_proj)
    lf = LayerForms(layer, d, h1 if reassoc else d)
    row_rels = [sum(dgraph.groups[et].n_rels for et in ets) for ets in targets.values()]
    if f.seg_mode and SEG_FUSED and all(r <= SEG_FUSED_MAX_ITEMS for r in row_rels):
        lf.kind = "seg_rows"
    elif f.fused_seg:
        lf.kind = "fused_seg"
    elif f.fused:
        lf.kind = "fused"
    if lf.kind in ("seg_rows", "fused_seg") and WAVE_TABLE and _tab_groups_fit([len(v) for v in targets.values()], d):
        if lf.d_in == 64 and (d == 64 or reassoc):
            lf.table = "tab"
        elif lf.kind == "fused_seg" and f.preproj and lf.d_in == d == 32:
            lf.table = "narrow"
    # the peer all-reduce rides where the layer has both relation-sharded sums and a pushing
    # epilogue over row-split blocks
    split_t = [i for i in targets if i in dgraph.row_block and i not in f.fused]
    red = [i for i in targets if i not in dgraph.row_block and i not in f.fused]
    lf.peer_red = f.peer_reduce and bool(red) and bool(split_t)
    if lf.peer_red and not f.peer_fit:
        # (not an assert: under python -O the relation-sharded sums would silently go unreduced)
        raise RuntimeError(f"layer {layer}: the peer all-reduce is on but its targets do not fit one epilogue launch")
    return lf


def decide_forms(dgraph: DeviceGraph, h1: int, h2: int, allreduce=None, keep_sums: bool = False,
                 dropout=None, shard=None) -> PlanForms:
    """The launch forms of ForwardPlan(dgraph, ..., h1, h2, allreduce, keep_sums, dropout, shard),
    decided once and before any buffer is allocated, from host metadata alone: the device
    graph's group records, the shard, the widths and this module's policy.  No device tensor's
    data is read."""
    if shard is not None:
        allreduce = shard.allreduce
    groups, row_block, edge_types = dgraph.groups, dgraph.row_block, list(dgraph.edge_types)
    targets = _targets(dgraph)
    rels = {et: groups[et].n_rels for et in edge_types}
    dropping = dropout is not None and float(dropout[0]) < 1.0
    plain = not keep_sums and not dropping  # forward only, no dropout
    wide = h1 == 64 and h2 == 32            # the shape of the seg kernels' reassociated layer 2
    # flat mode: every group's pre-normalisation sum S_ij lands in one flat buffer per
    # layer (all-reduced when sharded; kept for the backward when training), and one fused
    # launch over dense-rows groups (DG_GROUP_DENSE_ROWS) finishes every node type from it
    f = PlanForms(flat_mode=allreduce is not None or keep_sums)
    f.fused = _fused_targets(dgraph, targets, allreduce is not None, keep_sums, getattr(shard, "fused_rows", False))
    if keep_sums and allreduce is None:
        # one GPU, training: when no node type would take the fused path anyway (config P),
        # keep the partial-mode layers and let their one epilogue launch also write every
        # group's pre-normalisation sum S_ij — no flat reduces, no finishing launch
        f.sums_mode = not f.fused
        f.flat_mode, f.fused = bool(f.fused), []
    # config S's weak scaling (RelationShard.weak_sets form "seg"): every node type row-split,
    # its groups in dg_spmm_seg_f32 (one wave per (row, relation), one chunk per relation
    # set) + the epilogue, and layer 2 reassociated, Σ_k (Â_k·H1_j)·W2_k — no projection
    # GEMM over every relation on every rank (forward only: the backward keeps the sums)
    f.seg_mode = (shard is not None and getattr(shard, "seg_rows", False) and plain and wide
                  and all(et[0] in row_block for et in edge_types)
                  and all(g.seg is not None or not g.n_rels for g in groups.values()))
    # (otherwise such a shard runs the same chunks in dg_spmm_groups_f32 + the epilogue,
    # with the projection GEMM)
    # the peer all-reduce (config P's drug rows, peer mode "fused"): the relation-sharded
    # groups' pre-normalisation sums of layer L live in `world` slots of the region, slot r
    # written by rank r's epilogue launch into every rank's copy; the finishing launch adds
    # the slots in rank order (dense-rows groups with n_chunks = world) — no RCCL all-reduce
    pc = getattr(shard, "peer", None)
    if (pc is not None and pc.mode == "fused" and f.flat_mode and plain and not f.seg_mode and not f.fused
            and any(i in row_block for i in targets)):
        f.peer_fit = _peer_reduce_fits(dgraph, targets)
        f.peer_reduce = f.peer_fit
    # staged groups make their slabs H1_j·W2_k in the layer-2 kernel itself
    # (dg_spmm_staged_proj_f32): no P buffer, no GEMM for them (64-wide H1, no dropout)
    f.staged_proj = {et for et in edge_types
                     if groups[et].staged and rels[et] and h1 == 64 and not dropping and STAGED_PROJ}
    # one GPU (config S): every node type finished by dg_gcn_fused_seg_f32 — one workgroup
    # per row, one wave per relation — with layer 2 reassociated (no projection in layer 1,
    # no GEMM), when every group is one chunk of <= 16 relations per row in total
    f.fused_seg = (FUSED_SEG and not f.flat_mode and not row_block and not dropping and wide
                   and all(g.seg is not None and g.n_chunks == 1 and g.chunk == g.n_rels >= 1
                           and not g.staged for g in groups.values())
                   and all(sum(rels[et] for et in ets) <= 16 for ets in targets.values()))
    if f.fused_seg:
        f.fused = list(targets)
    # ... or, L2_PREPROJECT, layer 2's operands made by layer 1's launch (plan.proj), layer 2 a
    # plain gather-sum over them: a one-GPU forward-only plan in the wave-table fused form
    if f.fused_seg and WAVE_TABLE and plain and shard is None:
        # TAB_WEIGHTED: where a weighted workgroup also has the wave slots for a row's jobs.  (Read
        # by layer 1 with L2_PREPROJECT = 0 too: the plan's A/B fallback keeps layer 1's table, a
        # row's waves and so H1's bits, and differs in layer 2 alone.)
        fits, f.tab_weighted = _preproject_fit(targets, rels, h1)
        if fits and L2_PREPROJECT:
            f.preproj = set(edge_types)
    if wide and (f.seg_mode or f.fused_seg):
        f.seg_proj = {et for et in edge_types if rels[et] and et not in f.preproj}
    # sharded forward plans: every other non-staged group's layer 2 reassociated as well, over
    # the rank's own rows / relations (config P: PPI in its one-chunk layout, (0,1), (1,0)),
    # so no rank runs a projection GEMM over all of H1 (REASSOC_ROWS)
    if REASSOC_ROWS and shard is not None and plain and wide:
        f.seg_proj |= {et for et in edge_types if rels[et] and not groups[et].staged
                       and (groups[et].seg is not None or groups[et].seg2 is not None)}
    # layer-1 rows finished by a fused launch (the SpMM one, or — sharded — the one that
    # finishes the all-reduced sums) project themselves onto the layer-2 relations
    rels_from: Dict[int, int] = {}
    for et in edge_types:
        rels_from[et[1]] = rels_from.get(et[1], 0) + rels[et]
    finished = (set(targets) - set(row_block)) if f.flat_mode else set(f.fused)
    f.proj_fused = [et for et in edge_types
                    if rels[et] and et[1] in finished and et not in f.staged_proj | f.seg_proj | f.preproj
                    and rels_from[et[1]] <= ForwardPlan.FUSED_PROJ_MAX_RELS and not dropping]
    if len(f.proj_fused) > DG_MAX_GROUPS:
        f.proj_fused = []
    f.layers = {layer: _layer_forms(f, dgraph, layer, h1, h2) for layer in (1, 2)}
    return f


@dataclass
class _L2Tab:
    """Layer 2's 32 -> 32 wave-table launch as built (attach_decoder_rows rebuilds it with the
    decoder's row operands)."""

    targets: list
    nodes: List[int]  # the targets' node types
    plain: "kernels.PreparedFusedTab"  # the launch without a decoder: its widths, balance, weighted


class ForwardPlan:
    """All buffers and prepared launches of one two-layer forward on one device."""

    # a fused launch projects a row onto at most this many layer-2 relations (VALU epilogue);
    # beyond it the batched MFMA GEMM is used
    FUSED_PROJ_MAX_RELS = knob("DG_FUSED_PROJ_MAX", 64)

    def __init__(self, dgraph: DeviceGraph, features: Dict[int, Optional[HostCSR]],
                 w1: LayerWeights, w2: LayerWeights, h1: int, h2: int,
                 allreduce: Optional[Callable[[torch.Tensor], None]] = None, keep_sums: bool = False,
                 dropout: Optional[Tuple[float, torch.Tensor]] = None, shard=None):
        self.g = dgraph
        self.h1, self.h2 = h1, h2
        self._check_shard(shard, allreduce)
        # dropout (training): (keep probability, device state {seed, step}); every forward
        # draws new masks (the step advances first), the backward reuses them
        # (sharded: a relation's masks are keyed by its GLOBAL id, so every rank — and one GPU —
        # masks it identically; each rank masks its own relations only)
        self.keep, self.drop_state = 1.0, None
        if dropout is not None and float(dropout[0]) < 1.0:
            self.keep, self.drop_state = float(dropout[0]), dropout[1]
        self.keep_sums = keep_sums
        self.launch_groups: Dict[int, List[EdgeType]] = {}  # id(SpMM launch) -> its groups
        self.runs = 0     # run() calls so far (decoder_rows_valid)
        self._dec = None  # the attached decoder's row operands (attach_decoder_rows)
        self._dec_retired: list = []
        self._l2_tab: Optional[_L2Tab] = None
        self._f32 = dict(device=dgraph.device, dtype=torch.float32)
        self.edge_types = list(dgraph.edge_types)
        self.targets = _targets(dgraph)
        self.et_index = {et: n for n, et in enumerate(self.edge_types)}
        # every form decision, before the first buffer
        self.forms = decide_forms(dgraph, h1, h2, self.allreduce, keep_sums, dropout, shard)
        for name in FORM_ATTRS:  # (readable on the plan as before the decision was split out)
            setattr(self, name, getattr(self.forms, name))
        x1 = self._layer1_operands(features, w1)
        self._exchange_region()
        self._outputs()
        self._projection_buffers(w2)
        # ---- layer 1 (+ the layer-2 projections of rows it finishes) ----
        self._layer1 = self._build_layer(1, x1, self._fused_projections(w2),
                                         post={et: w2.stacks[et] for et in self.edge_types if et in self.preproj})
        # ---- layer 2: remaining projections in one batched MFMA GEMM launch, then SpMM ----
        self._layer2_operands(w2)
        self._layer2 = self._build_layer(2, self.proj,
                                         staged_proj={et: (self.hidden1[et[1]], w2.stacks[et])
                                                      for et in self.staged_proj},
                                         seg_w={et: (self.hidden1[et[1]], w2.stacks[et]) for et in self.seg_proj})

    # ------------------------------------------------------------------ buffers and operands
    def _check_shard(self, shard, allreduce) -> None:
        """multi-GPU (sharding.RelationShard): the collectives joining the ranks' shares —
        all-reduce of the relation-sharded node types' sums, all-gather of the row-split
        node types' finished row blocks"""
        self.shard = shard
        if shard is not None:
            allreduce = shard.allreduce
        self.allreduce = allreduce
        self.row_block = dict(self.g.row_block)
        self.world = shard.world_size if shard is not None else 1
        self.allgather = shard.allgather if shard is not None else None
        if self.row_block and (shard is None or shard.row_block != self.row_block
                               or (self.allgather is None and getattr(shard, "peer", None) is None)):
            raise ValueError("a row-split device graph needs its RelationShard (with an all-gather or a peer exchange)")
        if shard is not None and allreduce is None:
            raise ValueError("a RelationShard needs its all-reduce")

    def _layer1_operands(self, features, w1: LayerWeights) -> Dict[EdgeType, torch.Tensor]:
        """Layer 1's dense operand per group: W1 (identity features) or X_j·W1_k (sparse
        features), and the launches that make them each forward (self._pre)."""
        dgraph, n, dev, h1 = self.g, self.g.n_nodes, self.g.device, self.h1
        self._pre: List[Callable[[], None]] = []
        x1: Dict[EdgeType, torch.Tensor] = {}
        if self.drop_state is not None:
            self._pre.append(lambda st=self.drop_state: kernels.dropout_advance(st))
        for et in self.edge_types:
            i, j = et
            grp = dgraph.groups[et]
            W = w1.stacks[et]
            K, F, dh = W.shape
            if dh != h1 or K != grp.K:
                raise ValueError(f"layer-1 weights of {et} are {tuple(W.shape)}, expected ({grp.K}, *, {h1})")
            fj = features.get(j)
            if fj is None:  # identity features: X_j·W_k ≡ W_k (bit-exact), no kernel
                if F != n[j]:
                    raise ValueError(f"identity features of type {j} need {n[j]} weight rows, got {F}")
                x1[et] = W
                if self.drop_state is not None:
                    # dropout_sparse on the identity (layers.py:87-88): relation k's operand is W1_k
                    # with rows kept / scaled by 1/keep — a masked copy of the stack per forward
                    # (sharded: of the local relations' slabs only, at their global positions)
                    xd = torch.empty_like(W)
                    t = drop_tag(1, self.et_index[et])
                    if grp.rel_map is None:
                        self._pre.append(lambda W=W, xd=xd, t=t: kernels.dropout_rows(W, xd, self.drop_state, t,
                                                                                      self.keep))
                    elif grp.n_rels:
                        self._pre.append(lambda W=W, xd=xd, t=t, m=grp.rel_map, F=F, mx=int(grp.rel_ids.max()):
                                         kernels.dropout_rows_map(W, xd, m, F, self.drop_state, t, self.keep, True,
                                                                  True, rel_map_max=mx))
                    x1[et] = xd
                continue
            if fj.shape[0] != n[j] or fj.shape[1] != F:
                raise ValueError(f"features of type {j} have shape {fj.shape}, weights expect (*, {F})")
            # X_j·W1_k for every relation k of the group (global slabs; sharded ranks compute
            # all of them — sparse features are small next to the adjacency): one copy of X_j's
            # pattern shared by the K chunks, chunk k reading W1_k; with dropout, chunk k masks
            # X_j's values with its own draw (dropout_sparse per relation, layers.py:23-31, :88)
            xw = torch.empty((K, n[j], h1), **self._f32)
            drop = (None if self.drop_state is None
                    else (self.drop_state, drop_tag(1, self.et_index[et]), self.keep))
            spec = kernels.RelGroupSpec(torch.from_numpy(fj.rowptr).to(dev), torch.from_numpy(fj.col).to(dev),
                                        torch.from_numpy(fj.val).to(dev), W, xw, n[j], K, h1, F,
                                        vcol_max=int(fj.col.max()) if fj.nnz else -1, shared=True, drop=drop)
            self._pre.append(kernels.PreparedSpmm([spec], h1))
            x1[et] = xw
        return x1

    def _exchange_region(self) -> None:
        """Row-split node types: the full output rows live in a buffer padded to world × block
        rows (this rank finishes its block in place, the all-gather fills the rest), keyed by
        node type and layer: h1 == h2 must not share a buffer.  Every such buffer is carved from
        ONE exchange region with the same layout on every rank, which a peer exchange (peer.py)
        maps into every peer — with, for the peer all-reduce, the world slots of each layer's
        relation-sharded sums behind them."""
        n = self.g.n_nodes
        self._pad: Dict[Tuple[int, int], torch.Tensor] = {}
        self.xregion: Optional[torch.Tensor] = None
        self.peer = None
        self._red_slots: Dict[Tuple[int, EdgeType], torch.Tensor] = {}  # (layer, et) -> [world, n_i, d] view
        split_nodes = [i for i in self.targets if i in self.row_block]
        if not split_nodes:
            return
        pc = getattr(self.shard, "peer", None)
        layout, off = {}, 0
        for layer, d in ((1, self.h1), (2, self.h2)):
            for i in split_nodes:
                nb = self.world * self.row_block[i][2] * d
                layout[i, layer] = (off, nb, d)
                off += -(-nb // 64) * 64  # 256-byte aligned
        red_layout = {}
        if self.peer_reduce:
            for layer, d in ((1, self.h1), (2, self.h2)):
                red = [et for et in self.edge_types if et[0] not in self.row_block]
                per = sum(n[et[0]] * d for et in red)  # one slot: every group's rows, in order
                per = -(-per // 64) * 64
                o2 = 0
                for et in red:
                    red_layout[layer, et] = (off, o2, per, n[et[0]], d)
                    o2 += n[et[0]] * d
                off += self.world * per
        # zeros: a slot no rank ever pushes (a group without relations on that rank) reads as
        # zeros forever
        if pc is not None and pc.region_kind:  # (uncached by default: peer.PeerConfig)
            self.xregion = device_tensor(max(off, 64), pc.region_kind, self.g.device)
        else:
            self.xregion = torch.zeros(max(off, 64), **self._f32)
        for (i, layer), (o, nb, d) in layout.items():
            self._pad[i, layer] = self.xregion[o:o + nb].view(-1, d)
        for key, (base, o2, per, rows, d) in red_layout.items():
            self._red_slots[key] = torch.as_strided(self.xregion, (self.world, rows, d), (per, d, 1), base + o2)
        if pc is not None:
            self.peer = PeerExchange(self.xregion, self.shard.rank, self.world, pc)

    def _outputs(self) -> None:
        n = self.g.n_nodes

        def out_buf(i, d, layer):
            if i not in self.row_block:
                return torch.empty((n[i], d), **self._f32)
            return self._pad[i, layer][:n[i]]

        self.hidden1 = {i: out_buf(i, self.h1, 1) for i in self.targets}
        self.embeddings = {i: out_buf(i, self.h2, 2) for i in self.targets}
        self._outs = {1: self.hidden1, 2: self.embeddings}  # by layer
        for i, e in self.embeddings.items():  # (a decoder built on one finds this plan from the tensor)
            kernels.register_row_producer(e, self, i)

    def _projection_buffers(self, w2: LayerWeights) -> None:
        """Layer 2's operands P_k = H1_j·W2_k (global slabs) of the groups that are neither
        staged-projected nor reassociated."""
        h1, h2 = self.h1, self.h2
        self.proj: Dict[EdgeType, torch.Tensor] = {}
        for et in self.edge_types:
            grp = self.g.groups[et]
            K, din, dout = w2.stacks[et].shape
            if din != h1 or dout != h2 or K != grp.K:
                raise ValueError(f"layer-2 weights of {et} are {(K, din, dout)}, expected ({grp.K}, {h1}, {h2})")
            if et[1] not in self.hidden1:
                raise ValueError(f"node type {et[1]} has no incoming edge type; layer 2 needs hidden1[{et[1]}]")
            if et not in self.staged_proj and et not in self.seg_proj:
                self.proj[et] = torch.empty((K, self.g.n_nodes[et[1]], h2), **self._f32)

    def _fused_projections(self, w2: LayerWeights):
        """(source node type, ProjSpec) of forms.proj_fused: the launch that finishes H1_j aims
        each at its target (_retarget)."""
        projs = []
        for et in self.forms.proj_fused:
            grp = self.g.groups[et]
            projs.append((et[1], kernels.ProjSpec(
                w2.stacks[et], self.proj[et], grp.n_rels, -1, rel_map=grp.rel_map,
                rel_map_max=int(grp.rel_ids.max()) if grp.rel_map is not None else None)))
        return projs

    def _layer2_operands(self, w2: LayerWeights) -> None:
        """self._gemm2: the remaining projections in batched MFMA GEMM launches, after (training)
        the dropout of their operands."""
        n, dev, h1, h2 = self.g.n_nodes, self.g.device, self.h1, self.h2
        made = set(self.forms.proj_fused) | self.staged_proj | self.seg_proj | self.preproj
        gemms, drops = [], []
        self.hdrop: Dict[EdgeType, torch.Tensor] = {}
        for et in self.edge_types:
            grp = self.g.groups[et]
            if not grp.n_rels or et in made:
                continue
            j = et[1]
            W = w2.stacks[et]
            a, sa, b_map = self.hidden1[j], (0, h1, 1), grp.rel_map
            b_max = int(grp.rel_ids.max()) if b_map is not None else None
            if self.drop_state is not None:
                # tf.nn.dropout(H1_j) drawn per relation (layers.py:111-113): H_k = M_k∘H1_j/keep,
                # one slab per LOCAL relation in ascending relation id (the backward's dP order;
                # sharded: slab b is relation sorted_ids[b], its mask drawn under that global id),
                # projected into P's global slabs
                hd = torch.empty((grp.n_rels, n[j], h1), **self._f32)
                self.hdrop[et] = hd
                t = drop_tag(2, self.et_index[et])
                sids = np.sort(grp.rel_ids).astype(np.int32)
                smap = None if np.array_equal(sids, np.arange(grp.K)) else torch.from_numpy(sids).to(dev)
                if smap is None:
                    drops.append(lambda j=j, hd=hd, t=t: kernels.dropout_elems(self.hidden1[j], hd, self.drop_state,
                                                                               t, self.keep))
                else:
                    drops.append(lambda j=j, hd=hd, t=t, m=smap, mx=int(sids.max()): kernels.dropout_elems_map(
                        self.hidden1[j], hd, m, self.drop_state, t, self.keep, rel_map_max=mx))
                a, sa, b_map, b_max = hd, (n[j] * h1, h1, 1), smap, (int(sids.max()) if smap is not None else None)
            gemms.append(kernels.PreparedGemm(a, sa, W, (h1 * h2, h2, 1), self.proj[et], (n[j] * h2, h2, 1), n[j], h2, h1,
                                              grp.n_rels, b_map=b_map, b_batches=W.shape[0], b_map_max=b_max))
        self._gemm2 = drops + [kernels.PreparedGemmMulti(gemms[s:s + DG_MAX_GROUPS])
                               for s in range(0, len(gemms), DG_MAX_GROUPS)]

    # ------------------------------------------------------------------ layer builders
    def _spec(self, et, x: torch.Tensor, out, d) -> kernels.RelGroupSpec:
        grp = self.g.groups[et]
        return kernels.RelGroupSpec(grp.rowptr, grp.vcol, grp.val, x, out, grp.n_rows, grp.n_chunks, d,
                                    grp.K * grp.n_cols, vcol_max=grp.vcol_max)

    def _seg_spec(self, et, xs, seg_w, out=None) -> kernels.SegSpec:
        """A group's seg spec over its layer's operand: layer 2 reassociated (seg_w) reads H1_j
        and W2's stack, otherwise xs[et]."""
        grp = self.g.groups[et]
        x, w = seg_w[et] if et in seg_w else (xs[et], None)
        rp, vc, vv, sg, ch, nc, vmax = self._seg_layout(grp)
        return kernels.SegSpec(rp, sg, vc, vv, x, out, grp.n_rows, grp.n_cols, nc, ch, grp.n_rels, x.stride(-2),
                               grp.K * grp.n_cols, vcol_max=vmax, w=w, slab=grp.rel_map,
                               slab_max=int(grp.rel_ids.max()) if grp.n_rels else -1)

    @staticmethod
    def _seg_layout(grp: DeviceGroup) -> tuple:
        """(rowptr, vcol, val, seg, chunk, n_chunks, vcol_max) of a group's seg launches."""
        if grp.seg is None and grp.seg2 is not None:  # a windowed group's one-chunk layout
            return grp.seg2
        return grp.rowptr, grp.vcol, grp.val, grp.seg, grp.chunk, grp.n_chunks, grp.vcol_max

    def _seg_targets(self, rows: Dict[int, torch.Tensor], xs, seg_w, relu: bool) -> list:
        """The target list of a fused-seg / wave-table launch finishing rows[i] of node type i."""
        return [(out, out.shape[0], [self._seg_spec(et, xs, seg_w) for et in self.targets[i]], relu)
                for i, out in rows.items()]

    def _row_block_of(self, i: int, layer: int):
        """A row-split node type's (padded output, this rank's block of it — what the all-gather
        sends — and the block's finished rows, in place in the padded output)."""
        a, b, blk = self.row_block[i]
        pad = self._pad[i, layer]
        r0 = self.shard.rank * blk
        return pad, pad[r0:r0 + blk], pad[r0:r0 + (b - a)]

    @staticmethod
    def _retarget(projs, nodes: List[int]) -> list:
        """The projection specs whose source rows a launch over `nodes` finishes, aimed at their
        target's position in it (sharded: the finishing launch projects the others)."""
        out = []
        for tgt_node, pj in projs:
            if tgt_node in nodes:
                pj.target = nodes.index(tgt_node)
                out.append(pj)
        return out

    def _build_layer(self, layer: int, xs: Dict[EdgeType, torch.Tensor], projs=(), staged_proj=None, seg_w=None,
                     post=None) -> "_Layer":
        """Prepared launches of one layer, in the form decide_forms chose: fused targets in one
        launch; the other targets' groups in partial mode, then the finishing step — with, when
        sharded, the chunk reduce into the all-reduce buffer and the all-reduce before it."""
        lf = self.forms.layers[layer]
        seg_w = seg_w or {}
        if lf.kind == "seg_rows":
            return self._build_seg_rows(lf, xs, seg_w)
        L = _Layer(allreduce=self.allreduce, allgather=self.allgather, fused_targets=self.fused)
        if lf.kind == "fused_seg":
            self._build_fused_seg(L, lf, xs, seg_w, post or {})
        elif lf.kind == "fused":
            self._build_fused(L, lf, xs, projs)
        rest = [et for et in self.edge_types if et[0] not in self.fused]
        sviews = self._sum_buffers(L, lf, [et for et in rest if et[0] not in self.row_block])
        partials, reduces = self._build_partial(L, lf, rest, xs, staged_proj or {}, seg_w, sviews)
        # row-split node types (sharded) not finished by the fused launch: their groups run in
        # partial mode over this rank's row block and one epilogue finishes the block before
        # the exchange
        split_t = [i for i in self.targets if i in self.row_block and i not in self.fused]
        if split_t:
            reduces = self._finish_blocks(L, lf, split_t, partials, sviews, reduces)
        L.launches += reduces
        if lf.peer_red:
            # the relation-sharded rows finished from the world slots, added in rank order by
            # the dense-rows groups of ONE fused launch (l2norm, Σ_j, relu, layer-1 projections)
            self._finish_sums(L, lf, projs, self._slots_spec)
        elif L.flat is not None:
            # sharded: the all-reduced group sums S_ij are finished by ONE fused launch whose
            # groups are the dense rows S_ij[r] themselves (DG_GROUP_DENSE_ROWS), so the l2norm,
            # Σ_j, relu and (layer 1) the layer-2 projections of every node type run in one
            # kernel after the exchange
            self._finish_sums(L, lf, projs, lambda i, et, layer, d: self._identity_spec(i, L.views[et], d))
        elif not split_t:
            self._finish_plain(L, lf, rest, partials)
        L.gather_all = self._peer_gather_all(L.gathers, layer)
        return L

    def _build_seg_rows(self, lf: LayerForms, xs, seg_w) -> "_Layer":
        """Seg mode, every node type row-split: one launch finishes this rank's row block of each
        (its workgroups' waves loop over the N relation sets), then the all-gathers."""
        gathers, rows = [], {}
        for i in self.targets:
            pad, blk, rows[i] = self._row_block_of(i, lf.layer)
            gathers.append((pad, blk))
        tgts = self._seg_targets(rows, xs, seg_w, lf.relu)
        peer = self._peer_fused(lf.layer)
        if lf.table == "tab":
            # (one wave per relation here: dealing the pairs of N = 2's 14-relation rows over
            # 16 wave slots measured 16.45 / 23.04 µs a rank against 16.39 / 22.65, RCCL no-op /
            # peer loopback, round 6)
            launch = kernels.PreparedFusedTab(tgts, lf.d_in, lf.d, peer=peer, balance=False)  # (the wave-table form)
        else:
            launch = kernels.PreparedFusedSeg(tgts, lf.d_in, lf.d, peer=peer)
        self.launch_groups[id(launch)] = [et for i in self.targets for et in self.targets[i]]
        if peer is not None:
            gathers = []  # the launch itself ends with the exchange
        return _Layer(launches=[launch], allreduce=self.allreduce, gathers=gathers, allgather=self.allgather,
                      gather_all=self._peer_gather_all(gathers, lf.layer))

    def _build_fused_seg(self, L: "_Layer", lf: LayerForms, xs, seg_w, post) -> None:
        """One GPU: every node type finished by one fused-seg launch, in its wave-table form
        where decide_forms found it fits."""
        d_in, d = lf.d_in, lf.d
        tgts = self._seg_targets({i: self._outs[lf.layer][i] for i in self.fused}, xs, seg_w, lf.relu)
        weighted = _tab_weighted(d_in, d) if self.tab_weighted else 0
        if lf.table == "tab":
            # the wave-table form: the same rows bitwise, fewer dependent loads a wave
            # (post: layer 1 also projecting its rows onto layer 2's relations, L2_PREPROJECT)
            pj = []
            for et, W2 in post.items():
                grp = self.g.groups[et]
                pj.append(kernels.TabProjSpec(self.fused.index(et[1]), W2, self.proj[et], grp.n_rels,
                                              None if grp.rel_map is None else grp.rel_map.cpu().numpy()))
            launch = kernels.PreparedFusedTab(tgts, d_in, d, balance=_tab_balance(d_in, d), projs=pj,
                                              share_proj=L2_PREPROJECT_SHARE, weighted=weighted)
        elif lf.table == "narrow":
            # layer 2 over the P stacks layer 1 made: layer 1's shape at half the width
            launch = kernels.PreparedFusedTab(tgts, d_in, d, balance=_tab_balance(d_in, d), weighted=weighted)
            self._l2_tab = _L2Tab(tgts, list(self.fused), launch)
        else:
            launch = kernels.PreparedFusedSeg(tgts, d_in, d)
        L.launches.append(launch)
        self.launch_groups[id(launch)] = [et for i in self.fused for et in self.targets[i]]

    def _build_fused(self, L: "_Layer", lf: LayerForms, xs, projs) -> None:
        """self.fused finished by one dg_gcn_fused_f32 launch."""
        g, fused_t, d = self.g, self.fused, lf.d
        # waves per group: small launches (latency-bound) split the densest row group's
        # batches of 64 over up to two waves; big launches have parallelism to spare
        avg = max(g.groups[et].nnz / max(1, g.groups[et].n_rows) for i in fused_t for et in self.targets[i])
        max_groups = max(len(self.targets[i]) for i in fused_t)
        rows = sum(g.groups[self.targets[i][0]].n_rows for i in fused_t)
        # (row blocks of N relation sets — config S's weak scaling — have N times longer
        # rows over 1/N of the rows: up to 16 waves per row there; measured at N = 8, rank
        # 0's layer 1: 27.0 µs at 2 waves per group)
        cap = 16 // max_groups if self.row_block else 2
        wpg = 1 if rows >= 4096 else int(max(1, min(cap, 16 // max_groups, math.ceil(avg / 64.0))))
        tgts = []
        for i in fused_t:
            out = self._outs[lf.layer][i]
            if i in self.row_block:
                # a row-split node type (sharded): this rank's block, finished in place in the
                # padded output, then all-gathered
                pad, blk, out = self._row_block_of(i, lf.layer)
                L.gathers.append((pad, blk))
            tgts.append((out, out.shape[0], [self._spec(et, xs[et], None, d) for et in self.targets[i]], lf.relu))
        L.launches.append(kernels.PreparedFused(tgts, d, self._retarget(projs, fused_t), wpg))
        self.launch_groups[id(L.launches[-1])] = [et for i in fused_t for et in self.targets[i]]

    def _sum_buffers(self, L: "_Layer", lf: LayerForms, red: List[EdgeType]) -> Dict[EdgeType, torch.Tensor]:
        """Where each relation-sharded (or, training, every) group of `red` writes this rank's
        pre-normalisation sum: {et: tensor}, empty outside flat mode."""
        sviews: Dict[EdgeType, torch.Tensor] = {}
        if lf.peer_red:
            # the peer all-reduce: each relation-sharded group's sum goes to this rank's slot (and
            # every peer's copy of it) from the epilogue launch; no flat buffer, no RCCL all-reduce
            for et in red:
                sviews[et] = self._red_slots[lf.layer, et][self.shard.rank]
        elif self.flat_mode and red:
            # flat (the reduced sums, read by the finishing launch and the backward) and, when
            # sharded, send (this rank's partial sums, written by its SpMM / reduces): the
            # all-reduce runs out of place, so the regions of groups without local relations
            # stay zero from allocation on — no per-step fill
            sizes = [self.g.groups[et].n_rows * lf.d for et in red]
            L.flat = torch.zeros(int(sum(sizes)), **self._f32)
            L.send = torch.zeros_like(L.flat) if self.allreduce is not None else L.flat
            off = 0
            for et, sz in zip(red, sizes):
                L.views[et] = L.flat[off:off + sz]
                sviews[et] = L.send[off:off + sz]
                off += sz
            L.need_zero = L.send is L.flat and any(self.g.groups[et].n_rels == 0 for et in red)
        return sviews

    def _build_partial(self, L: "_Layer", lf: LayerForms, rest, xs, staged_proj, seg_w, sviews):
        """The partial-mode launches of the groups in `rest` — seg, staged, spmm, in that order,
        each in slices of DG_MAX_GROUPS — into chunk partials: ({et: (partials, chunks)}, the
        reduces of multi-chunk groups into their sums)."""
        g, d = self.g, lf.d
        partials, specs, staged, reduces, segs = {}, [], [], [], []
        # outside seg mode: layer 2 reassociated (seg_w), in dg_spmm_seg_f32
        reassoc = set(seg_w) if not self.seg_mode else set()
        for et in rest:
            grp = g.groups[et]
            cst = staged_chunk_starts(grp, d) if grp.staged else None
            n_out = ((len(cst) - 1 if cst is not None else -(-_staged_n(grp) // staged_out_chunk(grp, d)))
                     if grp.staged else grp.n_chunks)
            if et in reassoc:
                n_out = self._seg_layout(grp)[5]
            if L.flat is not None and et in L.views and n_out == 1:
                part = sviews[et]  # single chunk: the SpMM writes the group sum in place
            else:
                part = torch.zeros((max(1, n_out), grp.n_rows, d), **self._f32)
                if L.flat is not None and et in L.views and grp.n_rels:
                    reduces.append(kernels.PreparedEpilogue([(part, n_out)], sviews[et], grp.n_rows, d, 0))
            partials[et] = (part, max(1, n_out))
            if not grp.n_rels:
                continue
            if grp.staged:
                staged.append((et, kernels.StagedSpec(
                    grp.layout, grp.staged_slab if grp.staged_slab is not None else grp.rel_map, xs.get(et), part,
                    staged_out_chunk(grp, d), d, grp.K * grp.n_cols,
                    slab_max=int(grp.rel_ids.max()), proj=staged_proj.get(et), chunk_start=cst)))
            elif self.seg_mode or et in reassoc:
                segs.append((et, self._seg_spec(et, xs, seg_w, part)))
            else:
                specs.append((et, self._spec(et, xs[et], part, d)))

        def seg_launch(part):
            if WAVE_TABLE and wavetable._tab_shape(lf.d_in, d, part):
                return kernels.PreparedSegTab(part, lf.d_in, d)  # (the wave-table form)
            return kernels.PreparedSeg(part, lf.d_in, d)

        for items, make in ((segs, seg_launch), (staged, lambda part: kernels.PreparedStaged(part, d)),
                            (specs, lambda part: kernels.PreparedSpmm(part, d))):
            for s in range(0, len(items), DG_MAX_GROUPS):
                part = items[s:s + DG_MAX_GROUPS]
                L.launches.append(make([spec for _, spec in part]))
                self.launch_groups[id(L.launches[-1])] = [et for et, _ in part]
        return partials, reduces

    def _finish_blocks(self, L: "_Layer", lf: LayerForms, split_t, partials, sviews, reduces) -> list:
        """The local epilogue: one launch finishes this rank's row block of every node type of
        split_t before the exchange (pushing the rows itself with a fused peer exchange), the
        chunk reduces — or the peer all-reduce's sums — riding along where they fit.  Returns
        the reduces left to run as launches of their own."""
        g, n, d = self.g, self.g.n_nodes, lf.d
        epi_peer = self._peer_fused(lf.layer)
        blocks = []
        for i in split_t:
            pad, blk, out = self._row_block_of(i, lf.layer)
            parts = [partials[et] for et in self.targets[i]]
            if self.keep_sums:
                # training: the epilogue also keeps each group's pre-normalisation sum S_ij over
                # this rank's block rows (the backward's l2-norm gradient reads them)
                for n_, et in enumerate(self.targets[i]):
                    L.views[et] = torch.empty(out.shape[0] * d, **self._f32)
                    parts[n_] = (parts[n_][0], parts[n_][1], L.views[et])
            blocks.append((parts, out, out.shape[0]))
            if epi_peer is None:  # (else the epilogue launch itself ends with the exchange)
                L.gathers.append((pad, blk))
        n_push = len(blocks)
        # the relation-sharded node types' chunk reduces ride in the same launch: a target
        # whose groups write their pre-normalisation sums into the send buffer (its
        # finished rows go to a scratch buffer, unread) — one launch per layer instead of two
        # (the peer all-reduce: every relation-sharded group with local relations, its sum into
        # this rank's slot, pushed to every peer — the rest of the slot stays zero; decide_forms
        # turned it on only where these targets fit the launch)
        def summed(et):
            return bool(g.groups[et].n_rels) and (lf.peer_red or (et in L.views and partials[et][1] > 1))

        red_t = [i for i in self.targets if i not in self.row_block and any(summed(et) for et in self.targets[i])]
        if lf.peer_red or (reduces and _epilogue_fits(len(split_t) + len(red_t),
                                                      sum(len(self.targets[i]) for i in split_t + red_t))):
            for i in red_t:
                grp_parts = [partials[et][:2] + (sviews[et] if summed(et) else None,) + ((True,) if lf.peer_red else ())
                             for et in self.targets[i]]
                blocks.append((grp_parts, torch.empty((n[i], d), **self._f32), n[i]))
            reduces = []
        flags = DG_EPI_L2NORM | (DG_EPI_RELU if lf.relu else 0)
        L.local_epilogues.append(_epilogue(blocks, d, flags, peer=epi_peer,
                                           push=[t < n_push for t in range(len(blocks))]))
        return reduces

    def _finish_sums(self, L: "_Layer", lf: LayerForms, projs, spec) -> None:
        """The relation-sharded (or, training, all) node types finished from their groups' sums
        by ONE fused launch over dense-rows groups; spec(i, et, layer, d) is a group's."""
        n, tl = self.g.n_nodes, [i for i in self.targets if i not in self.row_block]
        L.epilogues.append(kernels.PreparedFused(
            [(self._outs[lf.layer][i], n[i], [spec(i, et, lf.layer, lf.d) for et in self.targets[i]], lf.relu)
             for i in tl], lf.d, self._retarget(projs, tl), 1))

    def _finish_plain(self, L: "_Layer", lf: LayerForms, rest, partials) -> None:
        """One GPU: every partial-mode node type finishes in ONE epilogue launch (side by side,
        no stream fork)."""
        n, d = self.g.n_nodes, lf.d
        if self.sums_mode:  # training: the epilogue also writes each group's S_ij
            for et in rest:
                L.views[et] = torch.empty(self.g.groups[et].n_rows * d, **self._f32)
                partials[et] = partials[et] + (L.views[et],)
        tl = [i for i in self.targets if i not in self.fused]
        # node types with the most chunk partials per row first: their long rows start early
        tl.sort(key=lambda i: -sum(partials[et][1] for et in self.targets[i]))
        if tl:
            flags = DG_EPI_L2NORM | (DG_EPI_RELU if lf.relu else 0)
            L.epilogues.append(_epilogue([([partials[et] for et in self.targets[i]], self._outs[lf.layer][i], n[i])
                                          for i in tl], d, flags))

    # ---- peer exchange (peer.py) ----
    def _peer_fused(self, layer: int):
        """(PeerExchange, slot) for a finishing launch that pushes its rows and exchanges, or None."""
        if self.peer is None or self.peer.cfg.mode != "fused":
            return None
        return self.peer, SLOT_FUSED + layer - 1

    def _peer_gather_all(self, gathers, layer: int):
        """With a peer exchange, the layer's remaining all-gathers as ONE stand-alone
        dg_peer_allgather launch (mode "kernel", or a finishing launch without a push form)."""
        if self.peer is None or not gathers:
            return None
        return self.peer.allgather_fn([blk for _, blk in gathers], SLOT_KERNEL + layer - 1)

    def peer_probe(self):
        """bench.py: each layer's stand-alone peer exchange of this rank's blocks (slots
        SLOT_PROBE + layer - 1), to time beside whatever exchange the plan runs."""
        out = []
        for layer in (1, 2):
            blks = [self._row_block_of(i, layer)[1] for i in self.targets if i in self.row_block]
            if blks:
                out.append(self.peer.allgather_fn(blks, SLOT_PROBE + layer - 1))
        return out

    def _slots_spec(self, i: int, et: EdgeType, layer: int, d: int) -> kernels.RelGroupSpec:
        """The peer all-reduce's dense-rows group: the world slots of (layer, et) as chunks."""
        sl = self._red_slots[layer, et]
        per, n_i = sl.stride(0), self.g.n_nodes[i]
        x = torch.as_strided(self.xregion, ((self.world - 1) * per + n_i * d,), (1,), sl.storage_offset())
        return kernels.RelGroupSpec(None, None, None, x, None, n_i, self.world, d, per // d, dense=True)

    def _identity_spec(self, i: int, x: torch.Tensor, d: int) -> kernels.RelGroupSpec:
        """A group spec with no adjacency (DG_GROUP_DENSE_ROWS): the fused kernel reads the dense
        rows x[r] as the group sums."""
        n_i = self.g.n_nodes[i]
        return kernels.RelGroupSpec(None, None, None, x, None, n_i, 1, d, n_i, dense=True)

    def run_layer1(self) -> None:
        for p in self._pre:
            p()
        self._layer1.run()

    def run_layer2(self) -> None:
        for gm in self._gemm2:
            gm()
        self._layer2.run()

    def run(self) -> None:
        if self.peer is not None:
            self.peer.ensure_ok()  # a timed-out exchange found by an earlier check poisons the plan
        self.run_layer1()
        self.run_layer2()
        self.runs += 1

    # ---- the decoder's row operands, made by layer 2's launch ----
    def attach_decoder_rows(self, node_type: int, G: torch.Tensor, l: Optional[torch.Tensor]):
        """Have layer 2's launch also store Q[r] = l ∘ ((E[r] ∘ l)·G) for every row of
        embeddings[node_type] (dg_gcn_fused_tab_dec_f32), and return Q [rows, 32] — or None when
        the plan cannot: anything but the one-GPU forward-only plan whose layer 2 is the 32 -> 32
        wave-table launch (self.preproj), h2 != 32, G / l not float32 [32, 32] / [32] and 16-byte
        aligned, DG_DEC_PREPROJECT=0, or another (G, l) attached already (one attachment a plan:
        the same pointers get the same Q).  Q holds the rows of a run() after this call
        (decoder_rows_valid), computed from G and l as they are when that run's launch executes.
        Only layer 2's table and launch are rebuilt; release_decoder_rows undoes it."""
        if not knob("DG_DEC_PREPROJECT", True):
            return None
        tab = self._l2_tab
        if not self.preproj or tab is None or self.h2 != 32 or node_type not in tab.nodes:
            return None
        if (G.dtype != torch.float32 or tuple(G.shape) != (32, 32) or not G.is_contiguous() or G.data_ptr() % 16
                or G.device != self.embeddings[node_type].device):
            return None
        if l is not None and (l.dtype != torch.float32 or tuple(l.shape) != (32,) or l.data_ptr() % 16
                              or l.device != G.device):
            return None
        key = (node_type, G.data_ptr(), None if l is None else l.data_ptr())
        if self._dec is not None:
            if self._dec["key"] != key:
                return None
            self._dec["users"] += 1
            return self._dec["Q"]
        E = self.embeddings[node_type]
        Q = torch.zeros((E.shape[0], 32), dtype=torch.float32, device=E.device)
        p = tab.plain
        launch = kernels.PreparedFusedTab(tab.targets, p.d_in, p.d_out, balance=p.balance, weighted=p.weighted,
                                          dec=kernels.TabDecSpec(tab.nodes.index(node_type), G, l, Q))
        self._swap_l2(tab.plain, launch)
        self._dec = {"key": key, "Q": Q, "G": G, "l": l, "launch": launch, "users": 1, "runs": self.runs}
        return Q

    def release_decoder_rows(self, Q: torch.Tensor) -> None:
        """Undo attach_decoder_rows for one holder of Q; the last one restores the plain layer-2
        launch (the same E bitwise)."""
        if self._dec is None or self._dec["Q"] is not Q:
            return
        self._dec["users"] -= 1
        if self._dec["users"] > 0:
            return
        self._swap_l2(self._dec["launch"], self._l2_tab.plain)
        # (kept alive with the plan: a graph captured while attached still replays that launch)
        self._dec_retired.append(self._dec)
        self._dec = None

    def decoder_rows_valid(self, Q: torch.Tensor) -> bool:
        """Whether Q (of attach_decoder_rows) holds the rows of this plan's last run: the plan has
        run since the attachment."""
        return self._dec is not None and self._dec["Q"] is Q and self.runs > self._dec["runs"]

    def _swap_l2(self, old, new) -> None:
        L = self._layer2.launches
        L[L.index(old)] = new
        self.launch_groups[id(new)] = self.launch_groups[id(old)]

    def phases(self) -> List[Tuple[str, Callable[[], None]]]:
        """The forward as alternating ("compute", fn) / ("exchange", fn) phases: the device
        launches between two collectives form one compute phase (capturable into one
        hipGraph), each layer's all-reduce of its pre-normalisation sums is an exchange."""
        out: List[Tuple[str, Callable[[], None]]] = []
        cur: List[Callable[[], None]] = []

        def close():
            if cur:
                fns = list(cur)
                out.append(("compute", lambda: [f() for f in fns]))
                cur.clear()

        cur.extend(self._pre)
        for layer, before in ((self._layer1, []), (self._layer2, self._gemm2)):
            cur.extend(before)
            if layer.need_zero:
                cur.append(layer.flat.zero_)
            cur.append(layer.run_spmm)
            cur.extend(layer.local_epilogues)
            if layer.has_exchange:
                close()
                out.append(("exchange", layer.exchange))
            cur.extend(layer.epilogues)
        close()
        return out

    def parallelism(self, backend: str = "nccl") -> str:
        return "1 GPU" if self.shard is None else self.shard.describe(backend)

    @property
    def spmm_launches(self):
        """(layer-1, layer-2) SpMM launches (fused or partial) — what the roofline times."""
        kinds = (kernels.PreparedSpmm, kernels.PreparedFused, kernels.PreparedStaged, kernels.PreparedSeg,
                 kernels.PreparedFusedSeg)
        pick = lambda L: [l for l in L.launches if isinstance(l, kinds)]
        return pick(self._layer1), pick(self._layer2)

    # ---- accounting (bench / DESIGN.md roofline) ----
    def group_bytes(self, et: EdgeType, d: int, fused: bool, layer: int = 1) -> int:
        """Algorithmic bytes of one group's SpMM: its CSR once (4 B per row of each
        relation + 8 B per nonzero), its dense operands once (4·d B per row of each X_k) and,
        in partial mode, its sum S_ij once (4·d B per output row)."""
        grp = self.g.groups[et]
        if not grp.n_rels:
            return 0
        tot = 4 * (grp.n_rels * grp.n_rows + 1) + 8 * grp.nnz
        if layer == 2 and (et in self.staged_proj or et in self.seg_proj):  # H1_j and W2 instead of P_k
            tot += 4 * self.h1 * (grp.n_cols + d * grp.n_rels)
        else:
            tot += 4 * d * grp.n_cols * grp.n_rels
        return tot if fused else tot + 4 * d * grp.n_rows

    def _extra_bytes(self, launch, layer: int) -> int:
        """What a launch moves beside its groups and rows: layer 1, W2 slabs read once and P rows
        written once by its projections (PreparedFused's epilogue, PreparedFusedTab's jobs);
        layer 2, G / l read once and Q rows written once where it makes the decoder's operands."""
        if layer == 1:
            return sum(4 * pj.n_rels * (pj.w.shape[1] * pj.w.shape[2] + pj.out.shape[1] * pj.w.shape[2])
                       for pj in getattr(launch, "projs", ()))
        dec = getattr(launch, "dec", None)
        if dec is None:
            return 0
        return 4 * (dec.G.numel() + (dec.l.numel() if dec.l is not None else 0) + dec.out.numel())

    def launch_bytes(self, launch, layer: int) -> int:
        """Algorithmic bytes of one SpMM launch of a layer (its groups; a fused launch also
        writes its targets' rows once, and in layer 1 reads W2 / writes P for its fused
        projections)."""
        L = self._layer1 if layer == 1 else self._layer2
        d = self.h1 if layer == 1 else self.h2
        ets = self.launch_groups.get(id(launch), [])
        fused = isinstance(launch, (kernels.PreparedFused, kernels.PreparedFusedSeg))
        tot = sum(self.group_bytes(et, d, fused, layer) for et in ets)
        if fused:
            tot += sum(4 * d * _local_rows(self.g, i) for i in L.fused_targets) + self._extra_bytes(launch, layer)
        return tot

    def layer_bytes(self, layer: int) -> int:
        """Algorithmic (compulsory) HBM bytes of one layer's SpMM launches: the CSR once
        (row pointers 4 B per row of each relation, vcol+val 8 B per nonzero), every distinct
        dense operand X_k once (4·d B per row of X_k), the output once — 4·d B per row of each
        group's sum S_ij in partial mode (chunk / window partials are the implementation's
        choice, not counted), per output row in fused mode — and, for layer 1, the fused
        projections' W2 reads and P writes."""
        L = self._layer1 if layer == 1 else self._layer2
        d = self.h1 if layer == 1 else self.h2
        tot = sum(self.group_bytes(et, d, et[0] in L.fused_targets, layer) for et in self.g.groups)
        tot += sum(4 * d * _local_rows(self.g, i) for i in L.fused_targets)
        return tot + sum(self._extra_bytes(f, layer) for f in L.launches)


@dataclass
class _Layer:
    """The prepared launches of one layer and how to run them."""

    launches: List[Callable[[], None]] = field(default_factory=list)
    flat: Optional[torch.Tensor] = None   # flat mode: the (reduced) sums of every group, one buffer
    send: Optional[torch.Tensor] = None   # this rank's partial sums (sharded: all-reduced into flat)
    views: Dict[EdgeType, torch.Tensor] = field(default_factory=dict)  # (i,j) -> that group's S_ij, [n_i * d]
    need_zero: bool = False
    allreduce: Optional[Callable[..., None]] = None
    epilogues: List[Callable[[], None]] = field(default_factory=list)
    fused_targets: Sequence[int] = ()
    local_epilogues: List[Callable[[], None]] = field(default_factory=list)  # row-split blocks, finished before the exchange
    gathers: list = field(default_factory=list)  # (padded out, this rank's block) per node type
    allgather: Optional[Callable[..., None]] = None
    gather_all: Optional[Callable[[], None]] = None  # all gathers in one peer-exchange launch

    @property
    def has_exchange(self) -> bool:
        return (self.flat is not None and self.allreduce is not None) or bool(self.gathers)

    def exchange(self) -> None:
        """The layer's collectives: all-reduce of the relation-sharded sums, then the
        all-gather of the row-split blocks."""
        if self.flat is not None and self.allreduce is not None:
            self.allreduce(self.send, self.flat)
        if self.gather_all is not None:
            self.gather_all()
            return
        for out, blk in self.gathers:
            self.allgather(out, blk)

    def run(self) -> None:
        if self.need_zero:
            self.flat.zero_()  # groups without local relations contribute zeros
        self.run_spmm()
        for e in self.local_epilogues:
            e()
        if self.has_exchange:
            self.exchange()
        for e in self.epilogues:
            e()

    def run_spmm(self) -> None:
        """The layer's SpMM launches (and chunk reduces), as the forward runs them: in order,
        on one stream."""
        for l in self.launches:
            l()

"""Host builder of the wave tables (dg_wave_table, include/decagon_hip.h) that
dg_gcn_fused_tab_*_f32 and dg_spmm_seg_tab_f32 run on.  numpy only: a table is built from host
arrays and integer device addresses, so its layout can be built and checked without a GPU.
kernels.PreparedFusedTab / PreparedSegTab validate their tensors, hand them over as SegData /
ProjData / DecData, and upload the HostTable that fused_table / seg_table return.

This file holds the numpy form of the 64-byte descriptor (DESC; tests/test_cpu_abi.py compares it
with the header's dg_tab_desc); the bit fields of its `role`, `wr` and `gwaves` words are the
header's DG_TAB_* macros, read from it by abi.py.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

# the bit fields of dg_tab_desc's role, wr and gwaves words (the header documents each beside its macro)
from .abi import (DG_TAB_GWAVES_BITS, DG_TAB_MAX_ROW_SLOTS, DG_TAB_ROLE_DEC_BIT, DG_TAB_ROLE_PROJ_BIT,  # noqa: F401
                  DG_TAB_ROLE_PROJ_SLOTS_BITS, DG_TAB_ROLE_PROJ_SLOTS_SHIFT, DG_TAB_ROLE_SEG_WAVES_BITS,
                  DG_TAB_ROLE_SEG_WAVES_SHIFT, DG_TAB_WR_GROUPS_BITS, DG_TAB_WR_RELU_BIT, DG_TAB_WR_SLOT_SHIFT)

# ---------------------------------------------------------------------------------------
# The descriptor contract (dg_tab_desc)
# ---------------------------------------------------------------------------------------
DESC = np.dtype([("x", "<u8"), ("w", "<u8"), ("orow", "<u8"), ("cnt", "<i4"), ("x_ld", "<i4"), ("ovf", "<i4"),
                 ("role", "<u4"), ("wr", "<u4"), ("aux_lo", "<i4"), ("aux_hi", "<i4"), ("gwaves", "<i4"),
                 ("first_wave", "<i4"), ("reserved", "<i4")])
assert DESC.itemsize == 64

PROJ_ROW_BYTES = 32 * 4            # a P or Q row: 32 floats
W_SLAB_BYTES = 64 * 32 * 4         # one relation's W slab


class Role(NamedTuple):
    proj_slots: Tuple[int, ...]    # row slots of the wave's projection job (() = no job)
    dec: bool
    seg_waves: int


class Wr(NamedTuple):
    groups: int
    relu: bool
    slot: int


def encode_role(proj_slots: Sequence[int] = (), dec: bool = False, seg_waves: int = 0) -> int:
    """dg_tab_desc.role.  A projection job names at least one row slot."""
    role = 0
    if proj_slots:
        assert all(0 <= s < DG_TAB_ROLE_PROJ_SLOTS_BITS for s in proj_slots)
        role |= (1 << DG_TAB_ROLE_PROJ_BIT) | (sum(1 << s for s in proj_slots) << DG_TAB_ROLE_PROJ_SLOTS_SHIFT)
    if dec:
        role |= 1 << DG_TAB_ROLE_DEC_BIT
    assert 0 <= seg_waves < 1 << DG_TAB_ROLE_SEG_WAVES_BITS
    return role | (seg_waves << DG_TAB_ROLE_SEG_WAVES_SHIFT)


def decode_role(role: int) -> Role:
    role = int(role)
    mask = (role >> DG_TAB_ROLE_PROJ_SLOTS_SHIFT) & ((1 << DG_TAB_ROLE_PROJ_SLOTS_BITS) - 1)
    proj = (role >> DG_TAB_ROLE_PROJ_BIT) & 1
    return Role(tuple(s for s in range(DG_TAB_ROLE_PROJ_SLOTS_BITS) if proj and (mask >> s) & 1),
                bool((role >> DG_TAB_ROLE_DEC_BIT) & 1),
                (role >> DG_TAB_ROLE_SEG_WAVES_SHIFT) & ((1 << DG_TAB_ROLE_SEG_WAVES_BITS) - 1))


def encode_wr(groups: int, relu: bool, slot: int) -> int:
    """dg_tab_desc.wr of a row's finishing wave."""
    assert 0 <= groups < 1 << DG_TAB_WR_GROUPS_BITS and 0 <= slot < DG_TAB_MAX_ROW_SLOTS
    return groups | (int(bool(relu)) << DG_TAB_WR_RELU_BIT) | (slot << DG_TAB_WR_SLOT_SHIFT)


def decode_wr(wr: int) -> Wr:
    wr = int(wr)
    return Wr(wr & ((1 << DG_TAB_WR_GROUPS_BITS) - 1), bool((wr >> DG_TAB_WR_RELU_BIT) & 1), wr >> DG_TAB_WR_SLOT_SHIFT)


def encode_gwaves(counts: Sequence[int]) -> int:
    """dg_tab_desc.gwaves (as the int32 stored): the wave count of each group of a row."""
    assert all(1 <= c <= 1 << DG_TAB_GWAVES_BITS for c in counts) and len(counts) * DG_TAB_GWAVES_BITS <= 32
    word = sum((c - 1) << (DG_TAB_GWAVES_BITS * u) for u, c in enumerate(counts))
    return int(np.uint32(word).astype(np.int32))


def decode_gwaves(word: int, n_groups: int) -> List[int]:
    word = int(word) & 0xffffffff
    return [((word >> (DG_TAB_GWAVES_BITS * u)) & ((1 << DG_TAB_GWAVES_BITS) - 1)) + 1 for u in range(n_groups)]


def split_addr(addr: int) -> Tuple[int, int]:
    """A 64-bit address as the descriptor's (aux_lo, aux_hi) int32 words."""
    return (int(np.uint32(addr & 0xffffffff).astype(np.int32)), int(np.uint32(addr >> 32).astype(np.int32)))


def join_addr(lo: int, hi: int) -> int:
    return ((int(hi) & 0xffffffff) << 32) | (int(lo) & 0xffffffff)


# ---------------------------------------------------------------------------------------
# Plain-data inputs and the built table
# ---------------------------------------------------------------------------------------
@dataclass
class SegData:
    """A kernels.SegSpec as the builder needs it: its CSR on the host, device addresses as
    integers (None = none)."""

    rowptr: np.ndarray            # int32 [n_chunks*n_rows + 1]
    seg: np.ndarray               # int32 [n_chunks*n_rows*chunk]
    vcol: np.ndarray              # int32 [nnz]
    val: np.ndarray               # float32 [nnz]
    slab: Optional[np.ndarray]    # int32 [n_rels] (None: relation k is slab k)
    x: int                        # address of the gather operand
    w: Optional[int]              # address of the weight stack [K, 64, 32], or None
    out: Optional[int]            # address of out [n_chunks, n_rows, d_out], or None (the fused form)
    x_ld: int
    n_rows: int
    n_cols: int
    chunk: int
    n_chunks: int
    n_rels: int


@dataclass
class ProjData:
    """A kernels.TabProjSpec: P[slab(k), r] = row r of target `target` times w[slab(k)]."""

    target: int
    w: int                        # address of [K, 64, 32]
    out: int                      # address of [K, target rows, 32]
    n_rels: int
    slab: Optional[Sequence[int]] = None


@dataclass
class DecData:
    """A kernels.TabDecSpec: Q[r] stored by the finishing wave of row r of target `target`."""

    target: int
    out: int                      # address of [target rows, 32]


@dataclass
class HostTable:
    """A wave table on the host, ready to upload (dg_wave_table's arrays and counts)."""

    desc: np.ndarray              # DESC [n_blocks * stride]
    pairs: np.ndarray             # int32 [n_blocks * stride * slot_pairs, 2]
    ovf: np.ndarray               # int32 [64 * batches (at least one), 2]
    n_blocks: int
    nw: int
    stride: int
    slot_pairs: int
    plan: list = field(default_factory=list)  # per workgroup, in launch order (see the builders)


class _WaveTable:
    """Builder of a dg_wave_table's arrays: per wave slot a 64-byte descriptor and
    the first S pairs of its segment (in the hand-out order of its gather form: pair m in lane
    16·(m & 3) + (m >> 2), stored compactly at (m & 3)·S/4 + (m >> 2); with 32-float rows, lp = 8,
    eight pairs are handed out at once: lane 8·(m & 7) + (m >> 3), stored at (m & 7)·S/8 + (m >> 3)),
    the rest in batches of 64 in an overflow array.  S (slot_pairs, round 6) is the smallest of 16 / 32 / 48 / 64
    holding the first batch of ≥ SLOT_COVER of the non-empty waves: a wave then fetches S·8 B
    where round 5 fetched 512 B whatever its length (a config-S wave holds 7–81 pairs)."""

    SLOT_COVER = 0.97

    def __init__(self, specs: Sequence[SegData], n_slots: int, proj: bool, lp: int = 16):
        assert lp in (8, 16) and not (proj and lp == 8)
        self.specs, self.proj = list(specs), proj
        self.G = 64 // lp  # pairs handed out at once
        self.n_slots = n_slots
        self.pv: dict = {}  # wave slot -> its pairs [cnt, 2] (laid out once S is known)
        self.desc = np.zeros(n_slots, DESC)
        # entry of pair m within a batch: its lane in the DPP hand-out (both layers since round 6)
        m = np.arange(64)
        self.lane_of = (64 // self.G) * (m % self.G) + m // self.G

    def bounds(self, g: int, k: int, r: int) -> Tuple[int, int]:
        """[beg, end) of relation k's segment (of spec g) in row r."""
        s = self.specs[g]
        c, t = divmod(k, s.chunk)
        si = (c * s.n_rows + r) * s.chunk + t
        beg = int(s.seg[si])
        end = int(s.seg[si + 1]) if t + 1 < s.chunk else int(s.rowptr[c * s.n_rows + r + 1])
        return beg, end

    def seg_len(self, g: int, k: int, r: int) -> int:
        beg, end = self.bounds(g, k, r)
        return end - beg

    def relation(self, i: int, g: int, k: int, r: int) -> None:
        """Wave slot i gathers relation k (of spec g) of row r."""
        beg, end = self.bounds(g, k, r)
        self.wave(i, g, r, [(k, 0, end - beg)])

    def wave(self, i: int, g: int, r: int, pieces) -> None:
        """Wave slot i gathers the pieces [(k, a, b)] of row r, in order: pairs a..b of relation
        k's segment (of spec g) — with a weight stack (layer 2 reassociated) one relation's only,
        since the wave multiplies its aggregate by that relation's W slab."""
        s = self.specs[g]
        d = self.desc
        vcs, vvs = [], []
        for k, a, b in pieces:
            beg, _ = self.bounds(g, k, r)
            vc = s.vcol[beg + a:beg + b].astype(np.int64)
            if self.proj:
                sl = int(s.slab[k]) if s.slab is not None else k
                vc = vc - sl * s.n_cols  # plain rows of H
                d["w"][i] = s.w + sl * W_SLAB_BYTES
            vcs.append(vc)
            vvs.append(s.val[beg + a:beg + b])
        if self.proj and len({k for k, _, _ in pieces}) > 1:
            raise ValueError("a reassociated wave gathers one relation")
        vc = np.concatenate(vcs) if vcs else np.zeros(0, np.int64)
        vv = np.concatenate(vvs) if vvs else np.zeros(0, np.float32)
        d["x"][i], d["x_ld"][i], d["cnt"][i] = s.x, s.x_ld, len(vc)
        self.pv[i] = np.stack([vc.astype(np.int32), vv.astype(np.float32).view(np.int32)], 1)

    def slot_pairs(self, fixed: int = 0) -> int:
        """S: `fixed` (an A/B override) or, 0, by SLOT_COVER."""
        if fixed:
            if fixed not in (16, 32, 48, 64):
                raise ValueError("DG_TAB_SLOT: 16, 32, 48 or 64")
            return fixed
        cnts = np.array([len(p) for p in self.pv.values() if len(p)], np.int64)
        if not len(cnts):
            return 16
        need = float(np.quantile(cnts, self.SLOT_COVER))
        return next(S for S in (16, 32, 48, 64) if S >= need or S == 64)

    def layout(self, S: int):
        """(pairs [n_slots·S, 2], ovf [.., 2]) for first-batch slots of S pairs; sets desc.ovf."""
        pairs = np.zeros((self.n_slots * S, 2), np.int32)
        ovf: List[np.ndarray] = []
        n_ovf = 0
        m = np.arange(S)
        compact = (m % self.G) * (S // self.G) + m // self.G  # slot entry of pair m (its lane's row-major rank)
        for i, pv in self.pv.items():
            cnt = len(pv)
            m0 = min(cnt, S)
            pairs[i * S + compact[:m0]] = pv[:m0]
            if cnt > S:
                self.desc["ovf"][i] = n_ovf
                for q0 in range(S, cnt, 64):
                    blk = np.zeros((64, 2), np.int32)
                    n = min(64, cnt - q0)
                    blk[self.lane_of[:n]] = pv[q0:q0 + n]
                    ovf.append(blk)
                    n_ovf += 64
        return pairs, (np.concatenate(ovf) if ovf else np.zeros((64, 2), np.int32))

    def finish(self, n_blocks: int, nw: int, stride: int, plan, slot: int = 0) -> HostTable:
        S = self.slot_pairs(slot)
        pairs, ovf = self.layout(S)
        return HostTable(self.desc, pairs, ovf, n_blocks, nw, stride, S, plan)


def wave_pairs(tab: HostTable, i: int, lp: int = 16) -> np.ndarray:
    """Wave slot i's pairs [cnt, 2] read back, in order, from the compact slot and the overflow
    batches (the inverse of _WaveTable.layout; lp = d_in / 4)."""
    G, S, cnt = 64 // lp, tab.slot_pairs, int(tab.desc["cnt"][i])
    m = np.arange(64)
    first = tab.pairs[i * S + (m[:S] % G) * (S // G) + m[:S] // G][:cnt]
    rest, o = [], int(tab.desc["ovf"][i])
    for q0 in range(S, cnt, 64):
        rest.append(tab.ovf[o + ((64 // G) * (m % G) + m // G)[:min(64, cnt - q0)]])
        o += 64
    return np.concatenate([first] + rest)


# ---------------------------------------------------------------------------------------
# Geometry and dealing of the fused table
# ---------------------------------------------------------------------------------------
def _tab_shape(d_in: int, d_out: int, specs) -> bool:
    """The shapes both table forms take (specs: SegData or kernels.SegSpec; w None = no stack)."""
    return d_in == 64 and (d_out == 64 or (d_out == 32 and all(s.w is not None for s in specs)))


def _tab_geometry(waves_t: Sequence[int], balance: bool) -> Tuple[int, int, List[int]]:
    """(waves per workgroup, wave-slot stride, rows per workgroup of each target) of a wave-table
    fused launch whose target t has waves_t[t] relations a row."""
    nw = max([1] + list(waves_t))
    stride = 8 if nw <= 8 else 16
    if balance:
        nw = stride  # every wave slot of a workgroup takes a share of its rows' pairs
    return nw, stride, [min(nw // max(1, w), DG_TAB_MAX_ROW_SLOTS) for w in waves_t]


def _proj_jobs(rows_present: Sequence[bool], n_rels: int, nw: int, share: bool = False):
    """Projection jobs of one workgroup: per wave slot (nw of them) its job (row slots, relation)
    or None.  The workgroup holds len(rows_present) row slots, each projected onto n_rels
    relations; a slot without a row (the last workgroup of an odd row count) projects nothing.
    Every (row, relation) goes to exactly one wave, and a wave holds one relation (one W slice).
    Without `share` a wave takes one row, so no wave takes two (row, relation) jobs; with it, one
    wave projects every present row onto its relation, so the relation's W slab is read once a
    workgroup, not once a row.  The waves that do not finish a row (slots rpb .. nw-1: idle while
    the finishing waves 0 .. rpb-1 work) are filled first.  None when the jobs of a full workgroup
    (rows per workgroup × relations; with `share`, the relations) exceed nw: the form is not built."""
    rpb = len(rows_present)
    if (n_rels if share else rpb * n_rels) > nw:
        return None
    jobs: List[Optional[Tuple[Tuple[int, ...], int]]] = [None] * nw
    order = list(range(rpb, nw)) + list(range(min(rpb, nw)))
    present = tuple(slot for slot in range(rpb) if rows_present[slot])
    if share:
        todo = [(present, k) for k in range(n_rels)] if present else []
    else:
        todo = [((slot,), k) for slot in present for k in range(n_rels)]
    for w, job in zip(order, todo):
        jobs[w] = job
    return jobs


def tab_proj_fit(waves_t: Sequence[int], sourced_t: Sequence[int], balance: bool, share: bool = False) -> bool:
    """Whether a wave-table launch whose target t has waves_t[t] relations a row has a wave slot
    for every projection job: rows per workgroup × sourced_t[t] relations projected per row (with
    `share`: sourced_t[t] jobs a workgroup)."""
    nw, _, rpbs = _tab_geometry(waves_t, balance)
    return all(_proj_jobs([True] * rpb, k, nw, share) is not None for rpb, k in zip(rpbs, sourced_t))


WEIGHTED_STRIDE = 16               # wave slots of a workgroup of a weighted table


def _weighted_slots(sizes: Sequence[int], T: int) -> int:
    """Wave slots of one row of a weighted table: a wave for every T pairs of each group (at
    least one a group), capped at the workgroup's WEIGHTED_STRIDE — a row past the cap has waves
    of more than T pairs."""
    if len(sizes) > WEIGHTED_STRIDE:
        raise ValueError(f"{len(sizes)} groups for {WEIGHTED_STRIDE} wave slots")
    return min(max(sum(max(1, -(-int(n) // T)) for n in sizes), len(sizes)), WEIGHTED_STRIDE)


def _weighted_max_rows(n_rels: int, share: bool) -> int:
    """Rows a workgroup of a weighted table may hold when each is projected onto n_rels relations:
    the most (up to DG_TAB_MAX_ROW_SLOTS) whose jobs (_proj_jobs_paired) fit its wave slots; 0 =
    not even one row's."""
    for rows in range(DG_TAB_MAX_ROW_SLOTS, 0, -1):
        if (-(-rows // 2) if share else rows) * n_rels <= WEIGHTED_STRIDE:
            return rows
    return 0


def _proj_jobs_paired(rows_present: Sequence[bool], n_rels: int, nw: int, share: bool = True):
    """_proj_jobs for a workgroup of up to DG_TAB_MAX_ROW_SLOTS rows in which no wave projects
    more than two: with `share`, row slots (0, 1) and (2, 3) each share a wave per relation (a
    slot without a row is left out, a pair without rows has no job); without, a wave per (row,
    relation).  Same filling order as _proj_jobs; None when the jobs of a full workgroup exceed nw."""
    rpb = len(rows_present)
    if not share:
        return _proj_jobs(rows_present, n_rels, nw, False)
    if -(-rpb // 2) * n_rels > nw:
        return None
    jobs: List[Optional[Tuple[Tuple[int, ...], int]]] = [None] * nw
    order = list(range(rpb, nw)) + list(range(min(rpb, nw)))
    todo = []
    for s0 in range(0, rpb, 2):
        present = tuple(s for s in range(s0, min(s0 + 2, rpb)) if rows_present[s])
        if present:
            todo += [(present, k) for k in range(n_rels)]
    for w, job in zip(order, todo):
        jobs[w] = job
    return jobs


def weighted_proj_fit(sourced_t: Sequence[int], share: bool = True) -> bool:
    """tab_proj_fit for a weighted table: every target's workgroups can hold at least one row with
    a wave slot for each of its projection jobs."""
    return all(_weighted_max_rows(k, share) >= 1 for k in sourced_t)


def _weighted_plan(tb: "_WaveTable", targets, g_first, T: int, max_rows: Sequence[int]):
    """(plan, first wave slot of each row of each workgroup) of a weighted table: consecutive rows
    of one target packed in order into a workgroup while their wave slots (_weighted_slots) sum to
    at most WEIGHTED_STRIDE and they are at most max_rows[target]."""
    plan, firsts = [], []
    for t, (_, n_rows, gspecs, _) in enumerate(targets):
        gs = [int(g_first[t]) + gl for gl in range(len(gspecs))]
        r0, cur = 0, []
        for r in range(n_rows):
            w = _weighted_slots([sum(tb.seg_len(g, k, r) for k in range(s.n_rels)) for g, s in zip(gs, gspecs)], T)
            if cur and (sum(cur) + w > WEIGHTED_STRIDE or len(cur) >= max_rows[t]):
                plan.append((t, r0, len(cur)))
                firsts.append(cur)
                r0, cur = r, []
            cur.append(w)
        if cur:
            plan.append((t, r0, len(cur)))
            firsts.append(cur)
    # per workgroup, per row: (first wave slot, wave slots)
    return plan, [[(sum(c[:i]), c[i]) for i in range(len(c))] for c in firsts]


def _split_even(n: int, parts: int) -> List[Tuple[int, int]]:
    """[a, b) slices of n items over `parts` waves, the first n % parts one longer."""
    q, rem = divmod(n, parts)
    out, a = [], 0
    for p in range(parts):
        e = a + q + (1 if p < rem else 0)
        out.append((a, e))
        a = e
    return out


def _balanced_waves(tb: "_WaveTable", gs, nr, r: int, slots: int, proj: bool):
    """Row r's waves of a balanced fused table: per group, a list of waves, each a list
    of pieces (relation k, first pair, end pair) of the relation's segment.  `slots` wave slots
    in all, at least one per group (per relation with weight stacks); the spare slots go, one at
    a time, to the job whose share per wave is the largest (ties: the first)."""
    if proj:  # jobs are relations: a reassociated wave multiplies by one relation's W slab
        jobs = [(gl, k) for gl in range(len(gs)) for k in range(nr[gl])]
        sizes = [tb.seg_len(gs[gl], k, r) for gl, k in jobs]
    else:  # jobs are groups: every pair of a group gathers one row of the stacked operand
        jobs = [(gl, None) for gl in range(len(gs))]
        sizes = [sum(tb.seg_len(gs[gl], k, r) for k in range(nr[gl])) for gl in range(len(gs))]
    if len(jobs) > slots:
        raise ValueError(f"{len(jobs)} jobs for {slots} wave slots")
    parts = [1] * len(jobs)
    for _ in range(slots - len(jobs)):
        j = max(range(len(jobs)), key=lambda x: (-(-sizes[x] // parts[x]), -x))
        if sizes[j] <= parts[j]:
            break  # no job left with more than one pair per wave
        parts[j] += 1
    waves = [[] for _ in gs]
    for (gl, k), n, p in zip(jobs, sizes, parts):
        if k is not None:
            waves[gl] += [[(k, a, e)] for a, e in _split_even(n, p)]
            continue
        # a group: its relations' segments back to back, cut into p contiguous slices
        lens = [tb.seg_len(gs[gl], kk, r) for kk in range(nr[gl])]
        starts = np.cumsum([0] + lens)
        for a, e in _split_even(n, p):
            pieces = []
            for kk in range(nr[gl]):
                lo, hi = max(a, starts[kk]), min(e, starts[kk + 1])
                if lo < hi:
                    pieces.append((kk, int(lo - starts[kk]), int(hi - starts[kk])))
            waves[gl].append(pieces)
    return waves


def _mark_dec_rows(desc: np.ndarray, plan, stride: int, target: int, n_rows: int, q_ptr: int) -> int:
    """Flag the finishing waves of `target`'s rows in a wave table's descriptors: the decoder-row
    role bit and the Q row's address (q_ptr + 128 B · row) in the auxiliary words.  plan: (target,
    first row, rows per workgroup) per workgroup, in launch order; wave w < rows per workgroup of
    a workgroup finishes row first + w, if the target has it.  Returns the number of rows flagged."""
    done = 0
    for b, (t, r0, rpb) in enumerate(plan):
        if t != target:
            continue
        for w in range(rpb):
            if r0 + w >= n_rows:
                continue
            i = b * stride + w
            desc["role"][i] |= np.uint32(encode_role(dec=True))
            desc["aux_lo"][i], desc["aux_hi"][i] = split_addr(q_ptr + (r0 + w) * PROJ_ROW_BYTES)
            done += 1
    return done


def fused_table(targets, d_in: int, d_out: int, balance: bool = False, projs: Sequence[ProjData] = (),
                share_proj: bool = True, dec: Optional[DecData] = None, peer: bool = False,
                slot: int = 0, weighted: int = 0) -> HostTable:
    """The table of a dg_gcn_fused_tab_*_f32 launch.  targets = [(out address, n_rows, [SegData],
    relu)]; a workgroup finishes rows-per-workgroup consecutive rows of one target
    (HostTable.plan: (target, first row, rows per workgroup) per workgroup).  balance: each row's
    pairs dealt over every wave slot its workgroup gives the row (_balanced_waves), else one wave
    a relation.  projs / share_proj: projection jobs of a 64 -> 64 table (_proj_jobs).  dec: the
    finishing waves of one target's rows also store the decoder's row operand.  peer: the table of
    the exchange form (the auxiliary words of a finishing wave are the same in every table without
    jobs; the exchange needs at least one workgroup).  slot: a fixed slot_pairs, 0 = by cover.
    weighted = T > 0 (a balanced table of plain sums, d_in == d_out, without an exchange): wave
    slots in proportion to pairs instead of an equal share a row — workgroups of WEIGHTED_STRIDE
    slots, a row taking _weighted_slots of them (a wave for every T pairs of a group), rows packed
    in order (_weighted_plan), projection jobs at most two rows a wave (_proj_jobs_paired).

    The auxiliary words (aux_lo, aux_hi) of a wave hold, in this order of precedence: its
    projection job's first P row address; its decoder row's address; on any other finishing
    wave the row's byte offset in its target and the target's bytes (read by the peer form)."""
    specs = [s for _, _, gs, _ in targets for s in gs]
    proj = d_out != d_in
    waves_t = [sum(s.n_rels for s in gs) for _, _, gs, _ in targets]
    g_first = np.cumsum([0] + [len(gs) for _, _, gs, _ in targets])
    row_slots = None  # weighted: per workgroup, per row, (first wave slot, wave slots)
    if weighted:
        if weighted < 1 or not balance or proj or peer:
            raise ValueError("a weighted table: balanced plain sums (d_in == d_out) without an exchange, T >= 1")
        nw = stride = WEIGHTED_STRIDE
        max_rows = [_weighted_max_rows(sum(pj.n_rels for pj in projs if pj.target == t), share_proj)
                    for t in range(len(targets))]
        if not all(max_rows):
            raise ValueError(f"one row's projection jobs for {nw} wave slots")
        plan, row_slots = _weighted_plan(_WaveTable(specs, 0, proj, lp=d_in // 4), targets, g_first, weighted,
                                         max_rows)
    else:
        nw, stride, rpbs = _tab_geometry(waves_t, balance)
        plan = []
        for t, (_, n_rows, _, _) in enumerate(targets):
            plan += [(t, r0, rpbs[t]) for r0 in range(0, n_rows, rpbs[t])]
    tb = _WaveTable(specs, len(plan) * stride, proj, lp=d_in // 4)
    d = tb.desc
    for b, (t, r0, rpb) in enumerate(plan):
        out, n_rows, gspecs, relu = targets[t]
        gc = len(gspecs)
        nr = [s.n_rels for s in gspecs]
        gs = [int(g_first[t]) + gl for gl in range(gc)]
        per_row = nw // rpb if balance else waves_t[t]  # wave slots of one row
        for slot_r in range(rpb):
            r = r0 + slot_r
            if r >= n_rows:
                continue
            first = slot_r * per_row
            if row_slots is not None:
                first, per_row = row_slots[b][slot_r]
            if balance:
                waves = _balanced_waves(tb, gs, nr, r, per_row, proj)
            else:  # one wave per relation, groups in order
                waves = [[[(k, 0, tb.seg_len(gs[gl], k, r))] for k in range(nr[gl])] for gl in range(gc)]
            w = first
            for gl, wg in enumerate(waves):
                for pieces in wg:
                    tb.wave(b * stride + w, gs[gl], r, pieces)
                    w += 1
            # the row's finishing wave: each group's wave count and the row slot's first wave
            i = b * stride + slot_r
            d["orow"][i] = out + r * d_out * 4
            d["wr"][i] = encode_wr(gc, relu, slot_r)
            d["aux_lo"][i], d["aux_hi"][i] = r * d_out * 4, n_rows * d_out * 4
            d["gwaves"][i] = encode_gwaves([len(wg) for wg in waves])
            d["first_wave"][i] = first
        # projection jobs: W2_k in `w`, the address of row slot 0's P row in the auxiliary words
        # (a projecting launch has no exchange)
        rels = [(pj, k) for pj in projs if pj.target == t for k in range(pj.n_rels)]
        if rels:
            jobs = (_proj_jobs_paired if weighted else _proj_jobs)([r0 + s < n_rows for s in range(rpb)], len(rels),
                                                                   nw, share_proj)
            if jobs is None:
                raise ValueError(f"{rpb} rows x {len(rels)} projection jobs for {nw} wave slots")
            for w, job in enumerate(jobs):
                if job is None:
                    continue
                slots, (pj, k) = job[0], rels[job[1]]
                sl = k if pj.slab is None else int(pj.slab[k])
                i = b * stride + w
                d["role"][i] |= np.uint32(encode_role(proj_slots=slots))
                d["w"][i] = pj.w + sl * W_SLAB_BYTES
                d["aux_lo"][i], d["aux_hi"][i] = split_addr(pj.out + (sl * n_rows + r0) * PROJ_ROW_BYTES)
    if not plan and peer:
        raise ValueError("dg_gcn_fused_tab_peer_f32: the exchange needs at least one row a rank")
    if dec is not None:
        _mark_dec_rows(d, plan, stride, dec.target, targets[dec.target][1], dec.out)
    return tb.finish(len(plan), nw, stride, plan, slot)


def seg_table(specs: Sequence[SegData], d_in: int, d_out: int, slot: int = 0) -> HostTable:
    """The table of a dg_spmm_seg_tab_f32 launch: dg_spmm_seg_f32's workgroups in its
    XCD-contiguous item order.  HostTable.plan: per workgroup (spec, chunk, first row, rows per
    workgroup), or None for a dead workgroup of the padding to a multiple of 8."""
    live = [g for g, s in enumerate(specs) if s.n_rows > 0 and s.n_rels > 0]
    nw = max([1] + [specs[g].chunk for g in live])
    stride = 8 if nw <= 8 else 16
    blocks = []
    for g in live:
        s = specs[g]
        rpb = nw // s.chunk
        row_blocks = -(-s.n_rows // rpb)
        items = s.n_chunks * row_blocks
        n_blocks = 8 * (-(-items // 8))
        per = n_blocks >> 3
        for lb in range(n_blocks):
            item = (lb & 7) * per + (lb >> 3)
            blocks.append(None if item >= items else (g, item // row_blocks, (item % row_blocks) * rpb, rpb))
    tb = _WaveTable(specs, len(blocks) * stride, d_out != d_in)
    for b, blk in enumerate(blocks):
        if blk is None:
            continue
        g, c, r0, rpb = blk
        s = specs[g]
        for w in range(nw):
            i = b * stride + w
            slot_r, t = divmod(w, s.chunk)
            r = r0 + slot_r
            if not (slot_r < rpb and r < s.n_rows):
                continue
            k = c * s.chunk + t
            if k < s.n_rels:
                tb.relation(i, g, k, r)
            if t == 0:  # the first wave of the (chunk, row): it sums the chunk's waves
                tb.desc["orow"][i] = s.out + (c * s.n_rows + r) * d_out * 4
                tb.desc["role"][i] = encode_role(seg_waves=s.chunk)
    return tb.finish(len(blocks), nw, stride, blocks, slot)

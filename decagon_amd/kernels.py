"""Typed Python entry points over the C ABI (include/decagon_hip.h).

Every wrapper checks on the host, before launching, that the device buffers are large
enough for the indices the kernel will form (a bad shape must fail here, never fault on the
GPU), then launches on the current torch stream.  Launches are asynchronous and
graph-capturable; no wrapper synchronises.

The `Prepared*` classes hold the ctypes argument blocks of a fixed launch so that the hot
loop (engine.py) pays one ctypes call per kernel and nothing else.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, wavetable
from .tuning import knob
from ._lib import (DgAdamSeg, DgEpiGroup, DgFusedTarget, DgGemmDesc, DgL2gGroup, DgProj, DgRelGroup,
                   DgStagedGroup, DgStagedProj, check)


def _stream_ptr(stream: Optional[torch.cuda.Stream] = None) -> int:
    s = torch.cuda.current_stream() if stream is None else stream
    return s.cuda_stream


def _dev(t: torch.Tensor, dtype: torch.dtype, what: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what}: expected a torch.Tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise ValueError(f"{what}: must be a device (HIP) tensor")
    if t.dtype != dtype:
        raise TypeError(f"{what}: dtype {t.dtype}, expected {dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{what}: must be contiguous")
    return t


# --------------------------------------------------------------------------------------
# SpMM over relation groups
# --------------------------------------------------------------------------------------
@dataclass
class RelGroupSpec:
    """One relation group in the chunk-merged layout of dg_rel_group (decagon_hip.h)."""

    rowptr: torch.Tensor          # int32 [n_chunks*n_rows + 1]
    vcol: torch.Tensor            # int32 [nnz] virtual columns (rows of x)
    val: torch.Tensor             # float32 [nnz]
    x: torch.Tensor               # float32, relation-stacked dense operand, row v at v*x_ld
    out: Optional[torch.Tensor]   # float32 [n_chunks, n_rows, d] (None in fused mode)
    n_rows: int
    n_chunks: int
    x_ld: int
    x_rows: int                   # rows of x the kernel may address (per chunk when shared)
    vcol_max: int = -1            # host-known max(vcol) (-1: no nonzeros)
    shared: bool = False          # DG_GROUP_SHARED_PATTERN: one CSR [n_rows] for every chunk, chunk c
                                  # reading x rows [c*x_rows, (c+1)*x_rows) (dg_spmm_groups_f32 only)
    drop: Optional[Tuple[torch.Tensor, int, float]] = None  # DG_GROUP_DROPOUT (shared only):
                                  # (device state {seed, step}, stream tag, keep) — chunk c scales
                                  # nonzero p by mask element c·nnz + (drop_index[p] or p)
    drop_index: Optional[torch.Tensor] = None
    dense: bool = False           # DG_GROUP_DENSE_ROWS (dg_gcn_fused_f32 only): row r of the sum
                                  # is x[r] — or, with n_chunks = S slots, Σ_c x[c·x_rows·x_ld + r]
                                  # in slot order; rowptr / vcol / val unused (may be None)

    def validate(self, d: int, need_out: bool = True) -> None:
        if self.dense:
            _dev(self.x, torch.float32, "x")
            if not 1 <= self.n_chunks <= _lib.DG_PEER_MAX or self.shared or self.drop is not None:
                raise ValueError("a dense-rows group has 1..8 slots, no shared pattern, no dropout")
            if self.x_ld < d or self.x_ld % 4:
                raise ValueError("x_ld must be >= d and a multiple of 4")
            last = (self.n_chunks - 1) * self.x_rows * self.x_ld + (self.n_rows - 1) * self.x_ld + d
            if self.x_rows < self.n_rows or (self.n_rows and self.x.numel() < last):
                raise ValueError("x smaller than the group's rows (slots)")
            return
        _dev(self.rowptr, torch.int32, "rowptr")
        _dev(self.vcol, torch.int32, "vcol")
        _dev(self.val, torch.float32, "val")
        _dev(self.x, torch.float32, "x")
        if need_out or self.out is not None:
            _dev(self.out, torch.float32, "out")
        if self.n_rows == 0:
            return
        if self.n_chunks < 1:
            raise ValueError("n_chunks must be >= 1")
        n_ptr = (self.n_rows if self.shared else self.n_chunks * self.n_rows) + 1
        if self.rowptr.numel() < n_ptr:
            raise ValueError(f"rowptr has {self.rowptr.numel()} entries, kernel reads {n_ptr}")
        if self.vcol.numel() != self.val.numel():
            raise ValueError("vcol/val length mismatch")
        if self.x_ld < d or self.x_ld % 4:
            raise ValueError("x_ld must be >= d and a multiple of 4")
        if self.vcol_max >= self.x_rows:
            raise ValueError(f"vcol reaches row {self.vcol_max} of a {self.x_rows}-row operand")
        slabs = self.n_chunks if self.shared else 1
        if self.x_rows > 0 and self.x.numel() < (slabs * self.x_rows - 1) * self.x_ld + d:
            raise ValueError(f"x has {self.x.numel()} elements, kernel may read {(slabs * self.x_rows - 1) * self.x_ld + d}")
        if self.x_rows * self.x_ld >= 2**31:
            raise ValueError("dense operand too large for 32-bit gather offsets")
        if need_out and self.out.numel() < self.n_chunks * self.n_rows * d:
            raise ValueError("out too small for [n_chunks, n_rows, d]")
        if self.drop is not None:
            state, _, keep = self.drop
            if not self.shared:
                raise ValueError("dropout masks apply to a shared pattern only")
            if not (isinstance(state, torch.Tensor) and state.is_cuda and state.dtype == torch.int64
                    and state.numel() >= 2):
                raise ValueError("dropout state: int64 device tensor {seed, step}")
            if not 0.0 < float(keep) <= 1.0:
                raise ValueError("keep must be in (0, 1]")
            if self.n_chunks * self.vcol.numel() >= 2**32:
                raise ValueError("dropout mask counter exceeds 32 bits")
            if self.drop_index is not None:
                _dev(self.drop_index, torch.int32, "drop_index")
                if self.drop_index.numel() != self.vcol.numel():
                    raise ValueError("drop_index must have one entry per nonzero")


def _fill_group(g, s: RelGroupSpec) -> None:
    if s.dense:
        g.rowptr = g.vcol = g.val = g.out = None
        g.x = s.x.data_ptr()
        g.x_ld, g.n_rows, g.n_chunks, g.x_rows = s.x_ld, s.n_rows, s.n_chunks, s.x_rows
        g.flags = _lib.DG_GROUP_DENSE_ROWS
        g.drop_state = g.drop_index = None
        return
    g.rowptr = s.rowptr.data_ptr()
    g.vcol = s.vcol.data_ptr() if s.vcol.numel() else None
    g.val = s.val.data_ptr() if s.val.numel() else None
    g.x = s.x.data_ptr()
    g.out = s.out.data_ptr() if s.out is not None else None
    g.x_ld = s.x_ld
    g.n_rows = s.n_rows
    g.n_chunks = s.n_chunks
    g.x_rows = s.x_rows
    g.flags = _lib.DG_GROUP_SHARED_PATTERN if s.shared else 0
    g.drop_state = None
    g.drop_index = None
    if s.drop is not None:
        state, tag, keep = s.drop
        g.flags |= _lib.DG_GROUP_DROPOUT
        g.drop_state = state.data_ptr()
        g.drop_tag = int(tag)
        g.drop_keep = float(keep)
        g.drop_stride = int(s.vcol.numel())
        g.drop_index = s.drop_index.data_ptr() if s.drop_index is not None else None


FUSED_RPB = 1  # spmm.hip kFusedRpb: rows per fused workgroup, at most
SPMM_LDS_MAX_ROWS = 160 * 1024 // 144  # dg_spmm_groups_lds_f32: operand rows staged in LDS


class PreparedSpmm:
    """A fixed dg_spmm_groups_f32 launch (descriptor block built once); lds=True: the
    dg_spmm_groups_lds_f32 form for small shared operands (x_rows <= SPMM_LDS_MAX_ROWS)."""

    def __init__(self, specs: Sequence[RelGroupSpec], d: int, lds: bool = False):
        if len(specs) > _lib.DG_MAX_GROUPS:
            raise ValueError(f"at most {_lib.DG_MAX_GROUPS} groups per launch")
        for s in specs:
            s.validate(d)
        self.specs = list(specs)  # keep tensors alive
        self.d = d
        arr = (DgRelGroup * max(1, len(specs)))()
        for i, s in enumerate(specs):
            g = arr[i]
            _fill_group(g, s)
        self._arr = arr
        self._n = len(specs)
        if lds and any(s.x_rows > SPMM_LDS_MAX_ROWS for s in specs):
            raise ValueError("dg_spmm_groups_lds_f32: operand too large for LDS")
        self._name = "dg_spmm_groups_lds_f32" if lds else "dg_spmm_groups_f32"
        self._fn = getattr(_lib.load(), self._name)

    def __call__(self, stream: Optional[torch.cuda.Stream] = None) -> None:
        check(self._fn(self._arr, self._n, self.d, _stream_ptr(stream)), self._name)


@dataclass
class SegSpec:
    """One group of dg_spmm_seg_f32 (decagon_hip.h): the chunk-merged CSR, its segment starts
    (sparse.chunk_segments) and, for the reassociated layer 2, the weight stack w with each
    local relation's slab."""

    rowptr: torch.Tensor          # int32 [n_chunks*n_rows + 1]
    seg: torch.Tensor             # int32 [n_chunks*n_rows*chunk]
    vcol: torch.Tensor            # int32 [nnz]
    val: torch.Tensor             # float32 [nnz]
    x: torch.Tensor               # float32: stacked X (no w) or H [n_cols, x_ld]
    out: Optional[torch.Tensor]   # float32 [n_chunks, n_rows, d_out] (None in the fused form)
    n_rows: int
    n_cols: int
    n_chunks: int
    chunk: int
    n_rels: int
    x_ld: int
    x_rows: int                   # bound on vcol
    vcol_max: int = -1
    w: Optional[torch.Tensor] = None      # float32 [K, 64, 32]
    slab: Optional[torch.Tensor] = None   # int32 [n_rels] (None: relation k is slab k)
    slab_max: int = -1

    def validate(self, d_in: int, d_out: int, need_out: bool = True) -> None:
        for t, what in ((self.rowptr, "rowptr"), (self.seg, "seg"), (self.vcol, "vcol")):
            _dev(t, torch.int32, what)
        _dev(self.val, torch.float32, "val")
        _dev(self.x, torch.float32, "x")
        if need_out:
            _dev(self.out, torch.float32, "out")
        if not 1 <= self.chunk <= 16:
            raise ValueError("chunk must be in [1, 16]")
        if not (self.n_chunks - 1) * self.chunk < self.n_rels <= self.n_chunks * self.chunk:
            raise ValueError("every chunk must hold at least one relation")
        if self.rowptr.numel() < self.n_chunks * self.n_rows + 1:
            raise ValueError("rowptr too short")
        if self.seg.numel() < self.n_chunks * self.n_rows * self.chunk:
            raise ValueError("seg too short")
        if self.vcol.numel() != self.val.numel():
            raise ValueError("vcol/val length mismatch")
        if self.vcol_max >= self.x_rows:
            raise ValueError(f"vcol reaches row {self.vcol_max} of a {self.x_rows}-row operand")
        if self.x_ld < d_in or self.x_ld % 4:
            raise ValueError("x_ld must be >= d_in and a multiple of 4")
        if self.x_rows * self.x_ld >= 2**31:
            raise ValueError("dense operand too large for 32-bit gather offsets")
        if need_out and self.out.numel() < self.n_chunks * self.n_rows * d_out:
            raise ValueError("out too small for [n_chunks, n_rows, d_out]")
        if self.w is None:
            if self.n_rows and self.x_rows and self.x.numel() < (self.x_rows - 1) * self.x_ld + d_in:
                raise ValueError("x smaller than x_rows rows")
            return
        _dev(self.w, torch.float32, "w")
        K = self.w.shape[0]
        if tuple(self.w.shape[1:]) != (64, 32) or (d_in, d_out) != (64, 32):
            raise ValueError("the reassociated form takes a [K, 64, 32] stack (d_in 64, d_out 32)")
        if self.x_rows > K * self.n_cols:
            raise ValueError("vcol bound beyond the stack's slabs")
        if self.x.numel() < (self.n_cols - 1) * self.x_ld + 64:
            raise ValueError("H smaller than n_cols rows")
        if self.slab is not None:
            _dev(self.slab, torch.int32, "slab")
            if self.slab.numel() < self.n_rels or not 0 <= self.slab_max < K:
                raise ValueError("slab map must index inside w")
        elif self.n_rels > K:
            raise ValueError("n_rels > K")


def _seg_array(specs: Sequence[SegSpec], d_in: int, d_out: int, need_out: bool):
    if len(specs) > _lib.DG_MAX_GROUPS:
        raise ValueError(f"at most {_lib.DG_MAX_GROUPS} groups per launch")
    if len({s.w is None for s in specs}) > 1:
        raise ValueError("every group of a launch has a weight stack, or none")
    arr = (_lib.DgSegGroup * max(1, len(specs)))()
    for i, s in enumerate(specs):
        s.validate(d_in, d_out, need_out)
        g = arr[i]
        g.rowptr, g.seg = s.rowptr.data_ptr(), s.seg.data_ptr()
        g.vcol = s.vcol.data_ptr() if s.vcol.numel() else None
        g.val = s.val.data_ptr() if s.val.numel() else None
        g.slab = s.slab.data_ptr() if s.slab is not None else None
        g.x = s.x.data_ptr()
        g.out = s.out.data_ptr() if s.out is not None else None
        g.w = s.w.data_ptr() if s.w is not None else None
        g.x_ld, g.n_rows, g.n_cols, g.n_chunks = s.x_ld, s.n_rows, s.n_cols, s.n_chunks
        g.chunk, g.n_rels, g.x_rows = s.chunk, s.n_rels, s.x_rows
    return arr


class PreparedSeg:
    """A fixed dg_spmm_seg_f32 launch (every group with w, or none)."""

    def __init__(self, specs: Sequence[SegSpec], d_in: int, d_out: int):
        arr = _seg_array(specs, d_in, d_out, True)
        self.specs = list(specs)
        self._arr, self._n, self.d_in, self.d_out = arr, len(specs), d_in, d_out
        self._fn = _lib.load().dg_spmm_seg_f32

    def __call__(self, stream=None) -> None:
        check(self._fn(self._arr, self._n, self.d_in, self.d_out, _stream_ptr(stream)), "dg_spmm_seg_f32")


class PreparedFusedSeg:
    """A fixed dg_gcn_fused_seg_f32 launch: targets = [(out tensor, n_rows, [SegSpec], relu)],
    each output row finished by one workgroup, one wave per relation (at most 16 a row; groups
    chunk-merged, any chunks); with weight stacks (d_in 64 → d_out 32) the reassociated layer 2."""

    def __init__(self, targets, d_in: int, d_out: int, peer=None):
        """peer = (PeerExchange, slot): every target's `out` lies in the exchange region; the
        launch also pushes the rows to every peer and ends with the exchange
        (dg_gcn_fused_seg_peer_f32)."""
        specs, tarr = [], (DgFusedTarget * len(targets))()
        for t, (out, n_rows, gspecs, relu) in enumerate(targets):
            _dev(out, torch.float32, "out")
            if out.numel() < n_rows * d_out:
                raise ValueError("fused output too small")
            if sum(s.n_rels for s in gspecs) > 16:
                raise ValueError("at most 16 relations per target row")
            tarr[t].out, tarr[t].n_rows = out.data_ptr(), n_rows
            tarr[t].g_begin, tarr[t].g_count = len(specs), len(gspecs)
            tarr[t].flags = _lib.DG_EPI_RELU if relu else 0
            for s in gspecs:
                if s.n_rows != n_rows or s.n_rels < 1:
                    raise ValueError("fused seg groups: the target's rows, at least one relation")
                specs.append(s)
        if len(targets) > _lib.DG_MAX_GROUPS:
            raise ValueError(f"at most {_lib.DG_MAX_GROUPS} targets per launch")
        self._garr = _seg_array(specs, d_in, d_out, False)
        self._keep = (specs, [t[0] for t in targets])
        self._tarr, self._ng, self._nt, self.d_in, self.d_out = tarr, len(specs), len(targets), d_in, d_out
        self._xchg = None
        if peer is not None:
            ex, slot = peer
            for out, *_ in targets:
                ex.offset(out)  # raises unless inside the region
            self._xchg = ctypes.byref(ex.xchg(slot))
            self._keep = self._keep + (ex,)
            self._fn = _lib.load().dg_gcn_fused_seg_peer_f32
        else:
            self._fn = _lib.load().dg_gcn_fused_seg_f32

    def __call__(self, stream=None) -> None:
        if self._xchg is not None:
            check(self._fn(self._garr, self._ng, self._tarr, self._nt, self.d_in, self.d_out, self._xchg,
                           _stream_ptr(stream)), "dg_gcn_fused_seg_peer_f32")
            return
        check(self._fn(self._garr, self._ng, self._tarr, self._nt, self.d_in, self.d_out, _stream_ptr(stream)),
              "dg_gcn_fused_seg_f32")


def _seg_data(s: SegSpec) -> wavetable.SegData:
    """A validated SegSpec as the host table builder takes it: host arrays, integer addresses."""
    return wavetable.SegData(s.rowptr.cpu().numpy(), s.seg.cpu().numpy(), s.vcol.cpu().numpy(), s.val.cpu().numpy(),
                             None if s.slab is None else s.slab.cpu().numpy(), s.x.data_ptr(),
                             None if s.w is None else s.w.data_ptr(), None if s.out is None else s.out.data_ptr(),
                             s.x_ld, s.n_rows, s.n_cols, s.chunk, s.n_chunks, s.n_rels)


def _upload_table(owner, tab: wavetable.HostTable, dev) -> "_lib.DgWaveTable":
    """A host-built wave table on the device (descriptors 64-byte aligned), its tensors and
    counts kept on `owner`; returns the launch's dg_wave_table."""
    owner._pairs = torch.from_numpy(tab.pairs).to(dev)
    owner._ovf = torch.from_numpy(tab.ovf).to(dev)
    owner.n_blocks, owner.nw, owner.slot_pairs = tab.n_blocks, tab.nw, tab.slot_pairs
    owner.host_plan = list(tab.plan)  # per workgroup, as the builder documents
    raw = torch.from_numpy(tab.desc.view(np.uint8).copy())
    owner._desc = torch.empty(raw.numel() + 64, dtype=torch.uint8, device=dev)
    off = (-owner._desc.data_ptr()) % 64
    owner._desc_v = owner._desc[off:off + raw.numel()]
    owner._desc_v.copy_(raw.to(dev))
    t = _lib.DgWaveTable()
    t.pairs, t.ovf, t.desc = owner._pairs.data_ptr(), owner._ovf.data_ptr(), owner._desc_v.data_ptr()
    t.n_blocks, t.nw, t.nw_stride, t.slot_pairs = tab.n_blocks, tab.nw, tab.stride, tab.slot_pairs
    return t


@dataclass
class TabProjSpec:
    """Projection jobs of a 64 -> 64 PreparedFusedTab launch (layer 1), one spec per edge type
    sourced from a target's node type: for every row r of target `target` and every local
    relation k, out[slab(k), r] = H1[r] · w[slab(k)] — layer 2's operand P_k, made in the
    workgroup that finishes the H1 row (dg_gcn_fused_tab_post_f32)."""

    target: int                   # index into the launch's targets: the rows projected
    w: torch.Tensor               # float32 [K, 64, 32]
    out: torch.Tensor             # float32 [K, n_rows, 32]
    n_rels: int
    slab: Optional[Sequence[int]] = None  # relation k -> slab (None: slab k)


@dataclass
class TabDecSpec:
    """The decoder's row operands made by a 32 -> 32 PreparedFusedTab launch (layer 2): for every
    row r of target `target`, out[r] = l ∘ ((E[r] ∘ l)·G), stored by the wave that finishes E[r]
    (dg_gcn_fused_tab_dec_f32), so that a DEDICOM score is out[r]·E[c]."""

    target: int                   # index into the launch's targets
    G: torch.Tensor               # float32 [32, 32]
    l: Optional[torch.Tensor]     # float32 [32], or None (all ones)
    out: torch.Tensor             # float32 [n_rows, 32]


class PreparedFusedTab(PreparedFusedSeg):
    """The same launch as PreparedFusedSeg (same targets, rows, waves and arithmetic: bitwise the
    same rows) through dg_gcn_fused_tab_f32: the wave table — each wave's 64-byte descriptor and
    its segment's first pairs at a fixed slot — is built once, on the host, from the chunk-merged
    CSR and segment starts of the specs (wavetable.fused_table; decagon_hip.h documents the layout).
    Shapes: d_in = d_out = 64, 64 -> 32 with weight stacks, or d_in = d_out = 32 (one GPU: no peer
    form).  projs (TabProjSpec, d_in = d_out = 64, no peer): the launch also makes layer 2's
    operands from the rows it finishes (dg_gcn_fused_tab_post_f32); seg_form() then still runs the
    plain seg launch, which writes the rows only.  share_proj: one wave projects every row of
    its workgroup onto its relation (wavetable._proj_jobs).  dec (TabDecSpec, d_in = d_out = 32): the launch
    also stores the decoder's row operands of one target's rows (dg_gcn_fused_tab_dec_f32); the
    rows themselves are bitwise the plain launch's.  peer = (PeerExchange, slot):
    the rows also go to every peer and the launch ends with the exchange
    (dg_gcn_fused_tab_peer_f32; PreparedFusedSeg's peer form, bitwise the same rows).

    balance (round 6): spread each row's pairs over every wave slot its workgroup gives the row
    instead of one wave per relation.  A relation segment of config S runs 7 to 81 pairs, and a
    workgroup waits for its slowest wave.  Layer 1 deals each group's pairs (its relations back
    to back: every pair gathers one row of the stacked operand) in contiguous slices over the
    group's waves, waves given to groups by their pairs; the reassociated layer 2 keeps one
    relation per wave (its W slab) and gives the spare slots to the longest segments.  The kernel
    and its finishing roles are unchanged — a group's normalising wave sums its waves' rows in
    order — so only the fp32 summation order within a group differs from the per-relation form.

    weighted = T > 0 (with balance; plain sums, d_in == d_out, no peer): wave slots in proportion
    to pairs — a wave for every T pairs of a row's group in 16-slot workgroups, rows packed while
    their slots fit (wavetable.fused_table) — so that a wave runs one gather round whatever its
    row's length.  The same kernel and roles again: only the summation order within a group differs."""

    def __init__(self, targets, d_in: int, d_out: int, peer=None, balance: bool = False,
                 projs: Sequence[TabProjSpec] = (), share_proj: bool = True, dec: Optional[TabDecSpec] = None,
                 weighted: int = 0):
        super().__init__(targets, d_in, d_out, peer=peer)
        specs = self._keep[0]
        narrow = d_in == d_out == 32 and all(s.w is None for s in specs) and peer is None
        self.dec = dec
        if dec is not None:
            _dev(dec.G, torch.float32, "G")
            _dev(dec.out, torch.float32, "Q")
            if dec.l is not None:
                _dev(dec.l, torch.float32, "l")
            if (not narrow or not 0 <= dec.target < len(targets) or tuple(dec.G.shape) != (32, 32)
                    or tuple(dec.out.shape) != (targets[dec.target][1], 32) or not dec.out.is_contiguous()
                    or not dec.G.is_contiguous() or (dec.l is not None and tuple(dec.l.shape) != (32,))
                    or dec.G.data_ptr() % 16 or dec.out.data_ptr() % 16
                    or (dec.l is not None and dec.l.data_ptr() % 16)):
                raise ValueError("dg_gcn_fused_tab_dec_f32: a 32 -> 32 launch, G [32, 32], l [32] or None, "
                                 "Q [target rows, 32], all 16-byte aligned")
        if not (wavetable._tab_shape(d_in, d_out, specs) or narrow):
            raise ValueError("dg_gcn_fused_tab_f32: d_in = d_out = 64, 64 -> 32 with weight stacks, or "
                             "d_in = d_out = 32 without an exchange")
        if any(len(gs) > 64 // (d_out // 4) for _, _, gs, _ in targets):
            raise ValueError("dg_gcn_fused_tab_f32: at most 64 / (d_out / 4) groups a target (one lane set each)")
        self.projs = list(projs)
        if self.projs and (d_in != 64 or d_out != 64 or peer is not None):
            raise ValueError("dg_gcn_fused_tab_post_f32: projection jobs follow a 64 -> 64 layer without an exchange")
        for pj in self.projs:
            _dev(pj.w, torch.float32, "w")
            _dev(pj.out, torch.float32, "P")
            K, rows = pj.w.shape[0], targets[pj.target][1]
            slabs = list(range(pj.n_rels)) if pj.slab is None else [int(x) for x in pj.slab[:pj.n_rels]]
            if (tuple(pj.w.shape[1:]) != (64, 32) or tuple(pj.out.shape) != (K, rows, 32) or len(slabs) != pj.n_rels
                    or any(not 0 <= x < K for x in slabs) or pj.out.data_ptr() % 16 or pj.w.data_ptr() % 16):
                raise ValueError("projection jobs: w [K, 64, 32], P [K, target rows, 32], slabs inside both")
        self.balance, self.weighted = balance, weighted
        data = {id(s): _seg_data(s) for s in specs}
        self._tab = _upload_table(self, wavetable.fused_table(
            [(out.data_ptr(), n_rows, [data[id(s)] for s in gs], relu) for out, n_rows, gs, relu in targets],
            d_in, d_out, balance=balance,
            projs=[wavetable.ProjData(pj.target, pj.w.data_ptr(), pj.out.data_ptr(), pj.n_rels, pj.slab)
                   for pj in self.projs],
            share_proj=share_proj, dec=None if dec is None else wavetable.DecData(dec.target, dec.out.data_ptr()),
            peer=peer is not None, slot=knob("DG_TAB_SLOT", 0), weighted=weighted), specs[0].x.device)
        if dec is not None:
            self._keep = self._keep + (dec,)
            self._tfn, self._tname = _lib.load().dg_gcn_fused_tab_dec_f32, "dg_gcn_fused_tab_dec_f32"
        elif self._xchg is not None:
            self._tfn, self._tname = _lib.load().dg_gcn_fused_tab_peer_f32, "dg_gcn_fused_tab_peer_f32"
        elif self.projs:
            self._keep = self._keep + (self.projs,)
            self._tfn, self._tname = _lib.load().dg_gcn_fused_tab_post_f32, "dg_gcn_fused_tab_post_f32"
        else:
            self._tfn, self._tname = _lib.load().dg_gcn_fused_tab_f32, "dg_gcn_fused_tab_f32"

    def __call__(self, stream=None) -> None:
        if self.dec is not None:
            check(self._tfn(ctypes.byref(self._tab), self.d_in, self.d_out, self.dec.G.data_ptr(),
                            self.dec.l.data_ptr() if self.dec.l is not None else None, _stream_ptr(stream)),
                  self._tname)
        elif self._xchg is not None:
            check(self._tfn(ctypes.byref(self._tab), self.d_in, self.d_out, self._xchg, _stream_ptr(stream)),
                  self._tname)
        else:
            check(self._tfn(ctypes.byref(self._tab), self.d_in, self.d_out, _stream_ptr(stream)), self._tname)

    def seg_form(self, stream=None) -> None:
        """The same rows through dg_gcn_fused_seg_f32 (tests: bitwise equal unless balanced)."""
        PreparedFusedSeg.__call__(self, stream)


class PreparedSegTab(PreparedSeg):
    """The same launch as PreparedSeg (dg_spmm_seg_f32's workgroups in its XCD-contiguous item
    order, waves and chunk partials — bit for bit) through dg_spmm_seg_tab_f32, from a wave
    table built once on the host (wavetable.seg_table).  Shapes as PreparedFusedTab."""

    def __init__(self, specs: Sequence[SegSpec], d_in: int, d_out: int):
        super().__init__(specs, d_in, d_out)
        if not wavetable._tab_shape(d_in, d_out, specs):
            raise ValueError("dg_spmm_seg_tab_f32: d_in = d_out = 64, or 64 -> 32 with weight stacks")
        self._tab = _upload_table(self, wavetable.seg_table([_seg_data(s) for s in specs], d_in, d_out,
                                                            slot=knob("DG_TAB_SLOT", 0)), specs[0].x.device)
        self._tfn = _lib.load().dg_spmm_seg_tab_f32

    def __call__(self, stream=None) -> None:
        check(self._tfn(ctypes.byref(self._tab), self.d_in, self.d_out, _stream_ptr(stream)), "dg_spmm_seg_tab_f32")

    def seg_form(self, stream=None) -> None:
        """The same partials through dg_spmm_seg_f32 (tests: bitwise equal)."""
        PreparedSeg.__call__(self, stream)


@dataclass
class ProjSpec:
    """Projection epilogue of a fused launch: out[kk] = row · w[rel_map[kk] or kk]."""

    w: torch.Tensor                     # float32 [K, d, d_out]
    out: torch.Tensor                   # float32 [n_rels, n_rows, d_out]
    n_rels: int
    target: int                         # index into the fused launch's targets
    rel_map: Optional[torch.Tensor] = None
    rel_map_max: Optional[int] = None


class PreparedFused:
    """A fixed dg_gcn_fused_f32 launch.

    targets = [(out tensor, n_rows, [group specs], relu)], projs = [ProjSpec]."""

    def __init__(self, targets, d: int, projs: Sequence[ProjSpec] = (), waves_per_group: int = 1):
        specs, tarr = [], (DgFusedTarget * len(targets))()
        max_groups = 1
        for t, (out, n_rows, gspecs, relu) in enumerate(targets):
            _dev(out, torch.float32, "out")
            if out.numel() < n_rows * d:
                raise ValueError("fused output too small")
            tarr[t].out = out.data_ptr()
            tarr[t].n_rows = n_rows
            tarr[t].g_begin = len(specs)
            tarr[t].g_count = len(gspecs)
            tarr[t].flags = _lib.DG_EPI_RELU if relu else 0
            max_groups = max(max_groups, len(gspecs))
            for s in gspecs:
                if s.n_rows != n_rows:
                    raise ValueError("group rows != target rows")
                s.validate(d, need_out=False)
                specs.append(s)
        if len(specs) > _lib.DG_MAX_GROUPS or len(targets) > _lib.DG_MAX_GROUPS:
            raise ValueError(f"at most {_lib.DG_MAX_GROUPS} groups / targets per fused launch")
        if not 1 <= waves_per_group or max_groups * waves_per_group > 16:
            raise ValueError("groups x waves_per_group must be <= 16")
        if len(projs) > _lib.DG_MAX_GROUPS:
            raise ValueError(f"at most {_lib.DG_MAX_GROUPS} projections per fused launch")
        parr = (DgProj * max(1, len(projs)))()
        for i, pj in enumerate(projs):
            _dev(pj.w, torch.float32, "proj w")
            _dev(pj.out, torch.float32, "proj out")
            K, din, dout = pj.w.shape
            n_rows = targets[pj.target][1]
            if din != d or pj.out.numel() < pj.n_rels * n_rows * dout:
                raise ValueError("projection shapes do not match the fused layer")
            if pj.rel_map is not None:
                _dev(pj.rel_map, torch.int32, "proj rel_map")
                if pj.rel_map_max is None or not 0 <= pj.rel_map_max < K:
                    raise ValueError("proj rel_map_max must index inside w")
            elif pj.n_rels > K:
                raise ValueError("projection n_rels > K")
            parr[i].w = pj.w.data_ptr()
            parr[i].rel_map = pj.rel_map.data_ptr() if pj.rel_map is not None else None
            parr[i].out = pj.out.data_ptr()
            parr[i].n_rels = pj.n_rels
            parr[i].target = pj.target
            parr[i].d_out = dout
        garr = (DgRelGroup * len(specs))()
        for i, s in enumerate(specs):
            _fill_group(garr[i], s)
        self.projs = list(projs)
        self._keep = (specs, [t[0] for t in targets], self.projs)
        self._garr, self._tarr, self._parr = garr, tarr, parr
        self._ng, self._nt, self._np, self.d = len(specs), len(targets), len(projs), d
        self.wpg = waves_per_group
        self._max_groups = max_groups
        self._fn = _lib.load().dg_gcn_fused_f32

    def block_threads(self) -> int:
        """Waves per workgroup of this launch (dg_gcn_fused_f32's rows-per-workgroup rule)."""
        rpb = max(1, min(FUSED_RPB, 16 // (self._max_groups * self.wpg)))
        return rpb * self._max_groups * self.wpg

    def __call__(self, stream=None) -> None:
        check(self._fn(self._garr, self._ng, self._tarr, self._nt, self._parr if self._np else None, self._np,
                       self.wpg, self.d, _stream_ptr(stream)), "dg_gcn_fused_f32")


def staged_block(lrowptr: np.ndarray, lcol: np.ndarray, lval: np.ndarray, rlw: np.ndarray,
                 n_cols: int) -> np.ndarray:
    """One relation's pair block of the staged layout with the library's bank-conflict-avoiding
    diagonals and hole columns (dg_staged_block, host-only).  Lanes as a CSR over 64·waves
    virtual rows; returns pairs [sum(rlw)·64, 2] int32."""
    lrowptr = np.ascontiguousarray(lrowptr, np.int32)
    lcol = np.ascontiguousarray(lcol, np.int32)
    lval = np.ascontiguousarray(lval, np.float32)
    rlw = np.ascontiguousarray(rlw, np.int32)
    pairs = np.zeros((int(rlw.sum()) * 64, 2), np.int32)
    check(_lib.load().dg_staged_block(lrowptr.ctypes.data, lcol.ctypes.data, lval.ctypes.data, len(lrowptr) - 1,
                                      rlw.ctypes.data, n_cols, pairs.ctypes.data), "dg_staged_block")
    return pairs


@dataclass
class StagedDevice:
    """A StagedLayout (sparse.py) uploaded to the device."""

    pairs: torch.Tensor
    jm: torch.Tensor
    jmoff: torch.Tensor
    n_rows: int
    n_cols: int
    n_rels: int
    jm_len: int                   # ints in jm (tables + spare)
    jm_end: int                   # jmoff[n_rels]

    @classmethod
    def upload(cls, layout, device) -> "StagedDevice":
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
        return cls(t(layout.pairs), t(layout.jm), t(layout.jmoff), layout.n_rows, layout.n_cols,
                   len(layout.jmoff) - 1, layout.jm_len, int(layout.jmoff[-1]))


STAGED_LDS_BYTES = 160 * 1024
STAGED_MAX_CHUNKS = _lib.DG_STAGED_MAX_CHUNKS
STAGED_JM_SPARE = 1024


def staged_lds_bytes(n_rows: int, n_cols: int) -> int:
    """LDS of one staged workgroup (mirrors dg_spmm_staged_f32): two slab buffers of n_cols + 16
    columns 80 B apart (the slab rows, then sixteen zero columns), 1 KiB of chunk tables,
    n_rows 64-byte accumulators (80-byte rows when LDS has room)."""
    return 2 * (n_cols + 16) * 80 + 1024 + n_rows * 64


@dataclass
class StagedSpec:
    """One group for dg_spmm_staged_f32."""

    layout: StagedDevice
    slab: Optional[torch.Tensor]  # int32 [n_rels] or None
    x: torch.Tensor
    out: torch.Tensor             # float32 [ceil(n_rels/out_chunk), n_rows, d]
    out_chunk: int
    x_ld: int
    x_rows: int
    slab_max: int = -1            # host-known max(slab) (or n_rels-1 without slab), for checks
    # (H [n_cols][64], W [K][64][d]): relation k's operand is H·W[slab(k)], made in the kernel
    # (dg_spmm_staged_proj_f32); x / x_ld / x_rows are then unused
    proj: Optional[Tuple[torch.Tensor, torch.Tensor]] = None
    # variable output chunks: host int32 [n_chunks + 1], chunk c = relations [cs[c], cs[c+1])
    # (out is then [n_chunks, n_rows, d]); None: runs of out_chunk relations
    chunk_start: Optional[np.ndarray] = None

    def n_out(self) -> int:
        if self.chunk_start is not None:
            return len(self.chunk_start) - 1
        return -(-self.layout.n_rels // self.out_chunk)

    def validate(self, d: int) -> None:
        L = self.layout
        for t, nm, dt in ((L.pairs, "pairs", torch.int32), (L.jm, "jm", torch.int32),
                          (L.jmoff, "jmoff", torch.int32), (self.out, "out", torch.float32)):
            _dev(t, dt, nm)
        if self.proj is None:
            _dev(self.x, torch.float32, "x")
        if L.pairs.data_ptr() % 16:
            raise ValueError("pairs must be 16-byte aligned")
        if not (0 < L.n_rows < 1023 and 0 < L.n_cols <= 1024):
            raise ValueError("staged groups need n_rows < 1023, n_cols <= 1024")
        if L.jm_len < L.jm_end + STAGED_JM_SPARE or L.jm.numel() < L.jm_len:
            raise ValueError("staged jm must end with 1024 spare ints")
        if staged_lds_bytes(L.n_rows, L.n_cols) > STAGED_LDS_BYTES:
            raise ValueError("staged group does not fit LDS (two slab buffers + accumulators)")
        if not 1 <= self.out_chunk <= 64:
            raise ValueError("staged out_chunk must be 1..64")
        if self.slab is not None:
            _dev(self.slab, torch.int32, "slab")
            if self.slab.numel() < L.n_rels:
                raise ValueError("slab shorter than n_rels")
        smax = self.slab_max if self.slab_max >= 0 else L.n_rels - 1
        if self.proj is not None:
            h, w = self.proj
            if not (isinstance(h, torch.Tensor) and h.is_cuda and h.dtype == torch.float32):
                raise ValueError("proj h: float32 device tensor required (rows may be padded)")
            _dev(w, torch.float32, "proj w")
            if h.dim() != 2 or h.shape[0] < L.n_cols or h.shape[1] != 64 or h.stride(1) != 1 or h.stride(0) % 4:
                raise ValueError("proj h must be [n_cols][64], rows 16-byte aligned")
            if w.dim() != 3 or tuple(w.shape[1:]) != (64, d) or not w.is_contiguous() or w.shape[0] <= smax:
                raise ValueError("proj w must be a contiguous [K][64][d] stack covering the slabs")
        else:
            if (smax + 1) * L.n_cols > self.x_rows or self.x.numel() < (self.x_rows - 1) * self.x_ld + d:
                raise ValueError("dense operand smaller than the slabs address")
            if self.x_rows * self.x_ld >= 2**31:
                raise ValueError("dense operand too large for 32-bit gather offsets")
        if self.chunk_start is not None:
            cs = np.asarray(self.chunk_start)
            if (cs.ndim != 1 or not 2 <= len(cs) <= STAGED_MAX_CHUNKS + 1 or cs[0] != 0 or cs[-1] != L.n_rels
                    or L.n_rels > 65535 or np.diff(cs).min() < 1 or np.diff(cs).max() > 64):
                raise ValueError("staged chunk_start: 0 = c_0 < ... < c_n = n_rels, 1..64 relations a chunk, "
                                 f"at most {STAGED_MAX_CHUNKS} chunks")
        n_out = self.n_out()
        if self.out.numel() < n_out * L.n_rows * d:
            raise ValueError("staged out too small")


class PreparedStaged:
    """A fixed dg_spmm_staged_f32 launch."""

    def __init__(self, specs: Sequence[StagedSpec], d: int):
        if not 1 <= len(specs) <= _lib.DG_MAX_GROUPS:
            raise ValueError(f"1..{_lib.DG_MAX_GROUPS} groups per launch")
        arr = (DgStagedGroup * len(specs))()
        proj = specs[0].proj is not None
        if any((s.proj is not None) != proj for s in specs):
            raise ValueError("a staged launch's groups are all projected or none")
        parr = (DgStagedProj * len(specs))() if proj else None
        cstarts = []
        for i, s in enumerate(specs):
            s.validate(d)
            L, g = s.layout, arr[i]
            g.pairs, g.jm, g.jmoff = L.pairs.data_ptr(), L.jm.data_ptr(), L.jmoff.data_ptr()
            g.slab = s.slab.data_ptr() if s.slab is not None else None
            g.x = s.x.data_ptr() if s.x is not None else None
            if proj:
                h, w = s.proj
                parr[i].h, parr[i].w, parr[i].h_ld, parr[i].din = h.data_ptr(), w.data_ptr(), h.stride(0), 64
            g.out = s.out.data_ptr()
            g.x_ld = s.x_ld
            g.n_rows, g.n_cols, g.n_rels = L.n_rows, L.n_cols, L.n_rels
            g.out_chunk, g.x_rows, g.jm_len = s.out_chunk, s.x_rows, L.jm_len
            if s.chunk_start is not None:
                cs = np.ascontiguousarray(s.chunk_start, np.int32)
                cstarts.append(cs)  # (read at each launch: kept alive with the launch)
                g.chunk_start, g.n_chunks = cs.ctypes.data, len(cs) - 1
        self._keep = list(specs) + cstarts
        self._arr, self._parr, self._n, self.d = arr, parr, len(specs), d
        lib = _lib.load()
        self._fn = lib.dg_spmm_staged_proj_f32 if proj else lib.dg_spmm_staged_f32

    def __call__(self, stream=None) -> None:
        if self._parr is not None:
            check(self._fn(self._arr, self._parr, self._n, self.d, _stream_ptr(stream)), "dg_spmm_staged_proj_f32")
        else:
            check(self._fn(self._arr, self._n, self.d, _stream_ptr(stream)), "dg_spmm_staged_f32")


def spmm_groups(specs: Sequence[RelGroupSpec], d: int, stream=None) -> None:
    PreparedSpmm(specs, d)(stream)


def spmm_csr(rowptr: torch.Tensor, col: torch.Tensor, val: torch.Tensor, x: torch.Tensor,
             n_rows: int, out: Optional[torch.Tensor] = None, stream=None, beta: float = 0.0) -> torch.Tensor:
    """Y = A·X + beta·Y for one CSR relation (tf.sparse_tensor_dense_matmul, layers.py:90, :114),
    through dg_spmm_csr_f32.  beta = 1 adds the relation's product into a running sum (tf.add_n
    of layers.py:92 one relation at a time); beta = 0 overwrites out without reading it."""
    if x.dim() != 2:
        raise ValueError("x must be 2-D")
    if not np.isfinite(beta):
        raise ValueError("beta must be finite")
    x = x.contiguous()
    n_cols, d = x.shape
    if out is None:
        if beta != 0.0:
            raise ValueError("beta != 0 needs out (the running sum)")
        out = torch.empty((n_rows, d), device=x.device, dtype=torch.float32)
    vmax = int(col.max()) if col.numel() else -1
    spec = RelGroupSpec(rowptr, col, val, x, out, n_rows, 1, d, n_cols, vcol_max=vmax)
    spec.validate(d)
    if out.dim() != 2 or out.shape[0] < n_rows or out.shape[1] != d:
        raise ValueError("out must be [n_rows, d]")
    check(_lib.load().dg_spmm_csr_f32(rowptr.data_ptr(), col.data_ptr(), val.data_ptr(), n_rows, n_cols,
                                      x.data_ptr(), d, out.data_ptr(), d, d, ctypes.c_float(beta),
                                      _stream_ptr(stream)), "dg_spmm_csr_f32")
    return out


def rownorm_l2(x: torch.Tensor, out: Optional[torch.Tensor] = None, relu: bool = False,
               stream=None) -> torch.Tensor:
    """tf.nn.l2_normalize(x, dim=1) (layers.py:93, :117), then relu if asked (model.py:75), through
    dg_rownorm_l2_f32.  out may be x (in place)."""
    _dev(x, torch.float32, "x")
    if x.dim() != 2:
        raise ValueError("x must be 2-D")
    n_rows, d = x.shape
    if out is None:
        out = torch.empty_like(x)
    _dev(out, torch.float32, "out")
    if out.shape != x.shape:
        raise ValueError("out must have x's shape")
    flags = _lib.DG_EPI_RELU if relu else 0
    check(_lib.load().dg_rownorm_l2_f32(x.data_ptr(), out.data_ptr(), n_rows, d, flags, _stream_ptr(stream)),
          "dg_rownorm_l2_f32")
    return out


# --------------------------------------------------------------------------------------
# Epilogue
# --------------------------------------------------------------------------------------
class PreparedEpilogue:
    def __init__(self, partials: Sequence[Tuple[torch.Tensor, int]], out: torch.Tensor, n_rows: int,
                 d: int, flags: int):
        if not partials:
            raise ValueError("at least one group")
        if len(partials) > _lib.DG_MAX_GROUPS:
            raise ValueError(f"at most {_lib.DG_MAX_GROUPS} groups")
        _dev(out, torch.float32, "out")
        if out.numel() < n_rows * d:
            raise ValueError("out too small")
        arr = (DgEpiGroup * len(partials))()
        for i, (p, nc, *rest) in enumerate(partials):
            _dev(p, torch.float32, "partial")
            if p.numel() < nc * n_rows * d:
                raise ValueError("partial too small for [n_chunks, n_rows, d]")
            arr[i].partial = p.data_ptr()
            arr[i].n_chunks = nc
        self._keep = [p for p, *_ in partials] + [out]
        self._arr = arr
        self._args = (len(partials), out.data_ptr(), n_rows, d, flags)
        self._fn = _lib.load().dg_gcn_epilogue_f32

    def __call__(self, stream=None) -> None:
        n, o, r, d, f = self._args
        check(self._fn(self._arr, n, o, r, d, f, _stream_ptr(stream)), "dg_gcn_epilogue_f32")


class PreparedEpilogueMulti:
    """dg_gcn_epilogue_multi_f32: several node types' epilogues in one launch —
    targets = [(partials [(tensor, n_chunks[, sum_out[, push]])], out, n_rows)], one flag set;
    a group's optional sum_out [n_rows, d] receives its pre-normalisation sum S_ij (with a peer
    exchange and push: also every peer's copy of it — this rank's slot of the all-reduce)."""

    def __init__(self, targets: Sequence[Tuple[Sequence[Tuple[torch.Tensor, int]], torch.Tensor, int]], d: int,
                 flags: int, peer=None, push: Optional[Sequence[bool]] = None):
        """peer = (PeerExchange, slot): the targets flagged in `push` (their `out` inside the
        exchange region) also go to every peer, and the launch ends with the exchange
        (dg_gcn_epilogue_peer_f32)."""
        if not targets or len(targets) > 8:
            raise ValueError("1..8 targets per launch")
        if sum(len(p) for p, _, _ in targets) > _lib.DG_MAX_GROUPS:
            raise ValueError(f"at most {_lib.DG_MAX_GROUPS} groups over all targets")
        self._keep, self._garrs = [], []
        tarr = (_lib.DgEpiTarget * len(targets))()
        for t, (partials, out, n_rows) in enumerate(targets):
            if not partials:
                raise ValueError("at least one group per target")
            _dev(out, torch.float32, "out")
            if out.numel() < n_rows * d:
                raise ValueError("out too small")
            garr = (DgEpiGroup * len(partials))()
            for i, (p, nc, *so) in enumerate(partials):
                _dev(p, torch.float32, "partial")
                if p.numel() < nc * n_rows * d:
                    raise ValueError("partial too small for [n_chunks, n_rows, d]")
                garr[i].partial = p.data_ptr()
                garr[i].n_chunks = nc
                if so and so[0] is not None:  # the group's pre-normalisation sum S_ij
                    _dev(so[0], torch.float32, "sum_out")
                    if so[0].numel() < n_rows * d:
                        raise ValueError("sum_out too small for [n_rows, d]")
                    garr[i].sum_out = so[0].data_ptr()
                    self._keep.append(so[0])
                    if len(so) > 1 and so[1]:
                        if peer is None:
                            raise ValueError("a pushed sum needs a peer exchange")
                        peer[0].offset(so[0])  # raises unless inside the region
                        garr[i].group_flags = _lib.DG_EPI_PUSH
                self._keep.append(p)
            self._keep.append(out)
            self._garrs.append(garr)
            tarr[t].groups = ctypes.cast(garr, ctypes.POINTER(DgEpiGroup))
            tarr[t].n_groups = len(partials)
            tarr[t].out = out.data_ptr()
            tarr[t].n_rows = n_rows
            if peer is not None and (push is None or push[t]):
                peer[0].offset(out)  # raises unless inside the region
                tarr[t].target_flags = _lib.DG_EPI_PUSH
        self._tarr = tarr
        self._args = (len(targets), d, flags)
        self._xchg = None
        if peer is not None:
            self._xchg = ctypes.byref(peer[0].xchg(peer[1]))
            self._keep.append(peer[0])
            self._fn = _lib.load().dg_gcn_epilogue_peer_f32
        else:
            self._fn = _lib.load().dg_gcn_epilogue_multi_f32

    def __call__(self, stream=None) -> None:
        n, d, f = self._args
        if self._xchg is not None:
            check(self._fn(self._tarr, n, d, f, self._xchg, _stream_ptr(stream)), "dg_gcn_epilogue_peer_f32")
            return
        check(self._fn(self._tarr, n, d, f, _stream_ptr(stream)), "dg_gcn_epilogue_multi_f32")


class PreparedEpilogueTab(PreparedEpilogueMulti):
    """The same launch as PreparedEpilogueMulti (bitwise its rows) through
    dg_gcn_epilogue_tab_f32: one 64-byte descriptor per output row built here once (its
    target's output, each group's chunk-0 partial row and chunk count), so a wave issues all its
    partial loads at once.  Targets whose groups carry sum outputs, or more than four groups,
    are not supported (ValueError: use PreparedEpilogueMulti)."""

    DESC = np.dtype([("out", "<u8"), ("part", "<u8", 4), ("off", "<i4"), ("plane", "<i4"), ("n_chunks", "<u4"),
                     ("info", "<u4"), ("bytes", "<i4"), ("pad", "<i4")])

    def __init__(self, targets, d: int, flags: int, peer=None, push: Optional[Sequence[bool]] = None):
        if d not in (32, 64):
            raise ValueError("dg_gcn_epilogue_tab_f32: d = 32 or 64")
        for partials, _, _ in targets:
            if len(partials) > 4 or any(len(p) > 2 and p[2] is not None for p in partials) \
                    or any(p[1] > 255 for p in partials):
                raise ValueError("dg_gcn_epilogue_tab_f32: at most 4 groups a row, 255 chunks, no group sums")
        super().__init__(targets, d, flags, peer, push)
        assert self.DESC.itemsize == 64
        n = sum(nr for _, _, nr in targets)
        desc = np.zeros(n, self.DESC)
        i = 0
        for t, (partials, out, nr) in enumerate(targets):
            if nr == 0:
                continue
            rows = np.arange(nr, dtype=np.int64)
            sl = slice(i, i + nr)
            desc["out"][sl] = out.data_ptr()
            desc["off"][sl] = rows * d
            desc["plane"][sl] = nr * d
            desc["bytes"][sl] = nr * d * 4
            ncs = 0
            for g, (p, nc, *_) in enumerate(partials):
                desc["part"][sl, g] = p.data_ptr() + rows * d * 4
                ncs |= nc << (8 * g)
            desc["n_chunks"][sl] = ncs
            pushed = peer is not None and (push is None or push[t])
            desc["info"][sl] = len(partials) | ((1 if pushed else 0) << 8)
            i += nr
        dev = targets[0][1].device
        raw = torch.from_numpy(desc.view(np.uint8).copy())
        self._rows = torch.empty(raw.numel() + 64, dtype=torch.uint8, device=dev)
        off = (-self._rows.data_ptr()) % 64
        self._rows_v = self._rows[off:off + raw.numel()]
        self._rows_v.copy_(raw.to(dev))
        self._n_rows = n
        self._tfn = _lib.load().dg_gcn_epilogue_tab_f32

    def __call__(self, stream=None) -> None:
        _, d, f = self._args
        check(self._tfn(self._rows_v.data_ptr() if self._n_rows else None, self._n_rows, d, f, self._xchg,
                        _stream_ptr(stream)), "dg_gcn_epilogue_tab_f32")

    def multi_form(self, stream=None) -> None:
        """The same rows through dg_gcn_epilogue_multi_f32 / _peer_f32 (tests: bitwise equal)."""
        PreparedEpilogueMulti.__call__(self, stream)


def gcn_epilogue(partials, out, n_rows, d, flags, stream=None) -> None:
    PreparedEpilogue(partials, out, n_rows, d, flags)(stream)


# --------------------------------------------------------------------------------------
# GEMM
# --------------------------------------------------------------------------------------
class PreparedGemm:
    """C_b = diag(sc)·((A_b·diag(sa))·B_b) on the fp32 MFMA, batched and strided.

    a, b, c are given as (tensor, (bs, s0, s1)) with element strides; sizes m, n, k, batch.
    """

    def __init__(self, a: torch.Tensor, a_strides, b: torch.Tensor, b_strides, c: torch.Tensor,
                 c_strides, m: int, n: int, k: int, batch: int = 1,
                 sa: Optional[torch.Tensor] = None, sc: Optional[torch.Tensor] = None,
                 b_map: Optional[torch.Tensor] = None, b_batches: Optional[int] = None,
                 b_map_max: Optional[int] = None, reduce: int = 0,
                 drop: Optional[Tuple[torch.Tensor, int, float]] = None):
        for t, nm in ((a, "a"), (b, "b"), (c, "c")):
            if not (t.is_cuda and t.dtype == torch.float32):
                raise ValueError(f"{nm}: float32 device tensor required")

        def span(strides, d0, d1, nb=batch):
            bs, s0, s1 = strides
            return (nb - 1) * bs + (d0 - 1) * s0 + (d1 - 1) * s1 + 1

        nb_b = batch
        if b_map is not None:
            _dev(b_map, torch.int32, "b_map")
            nb_b = batch if b_batches is None else b_batches
            if b_map.numel() < batch or b_map_max is None or not (0 <= b_map_max < nb_b):
                raise ValueError("b_map must cover the batch and index inside b")
        if m and n and k and batch:
            if a.numel() < span(a_strides, m, k) or b.numel() < span(b_strides, k, n, nb_b):
                raise ValueError("gemm operand too small for its strides")
        if reduce < 0:
            raise ValueError("reduce must be >= 0")
        n_out = -(-batch // reduce) if reduce else nb_b
        if m and n and batch and c.numel() < span(c_strides, m, n, n_out):
            raise ValueError("gemm output too small for its strides")
        if sa is not None and (sa.numel() < k or sa.dtype != torch.float32 or not sa.is_cuda):
            raise ValueError("sa must be a float32 device vector of length k")
        if sc is not None and (sc.numel() < n or sc.dtype != torch.float32 or not sc.is_cuda):
            raise ValueError("sc must be a float32 device vector of length n")
        desc = DgGemmDesc()
        desc.a, desc.b, desc.c = a.data_ptr(), b.data_ptr(), c.data_ptr()
        desc.sa = sa.data_ptr() if sa is not None else None
        desc.sc = sc.data_ptr() if sc is not None else None
        desc.b_map = b_map.data_ptr() if b_map is not None else None
        desc.a_bs, desc.a_sm, desc.a_sk = a_strides
        desc.b_bs, desc.b_sk, desc.b_sn = b_strides
        desc.c_bs, desc.c_sm, desc.c_sn = c_strides
        desc.m, desc.n, desc.k, desc.batch = m, n, k, batch
        desc.reduce = reduce
        if drop is not None:  # (device state {seed, step}, stream tag, keep): masked batch-reduce
            state, tag, keep_p = drop
            if not reduce:
                raise ValueError("the dropout mask applies in batch-reduce mode")
            if state.dtype != torch.int64 or not state.is_cuda:
                raise ValueError("dropout state: int64 device tensor {seed, step}")
            if nb_b * m * n >= 2**32:
                raise ValueError("dropout mask indices are 32-bit: (mapped) batches·m·n < 2^32")
            desc.drop_state, desc.drop_tag, desc.drop_keep = state.data_ptr(), int(tag), float(keep_p)
        self._desc = desc
        self._keep = (a, b, c, sa, sc, b_map, drop)
        self._fn = _lib.load().dg_gemm_f32

    def __call__(self, stream=None) -> None:
        check(self._fn(ctypes.byref(self._desc), 1, _stream_ptr(stream)), "dg_gemm_f32")


class PreparedGemmMulti:
    """Several prepared GEMMs (≤ DG_MAX_GROUPS) in one dg_gemm_f32 launch."""

    def __init__(self, gemms: Sequence[PreparedGemm]):
        if not 1 <= len(gemms) <= _lib.DG_MAX_GROUPS:
            raise ValueError(f"1..{_lib.DG_MAX_GROUPS} GEMMs per launch")
        arr = (DgGemmDesc * len(gemms))()
        for i, g in enumerate(gemms):
            ctypes.memmove(ctypes.byref(arr[i]), ctypes.byref(g._desc), ctypes.sizeof(DgGemmDesc))
        self._keep = list(gemms)
        self._arr, self._n = arr, len(gemms)
        self._fn = _lib.load().dg_gemm_f32

    def __call__(self, stream=None) -> None:
        check(self._fn(self._arr, self._n, _stream_ptr(stream)), "dg_gemm_f32")


class PreparedGemmTN:
    """dg_gemm_tn_f32: c[b] = a[b]ᵀ·b_stack[b] for a [rows][M] shared (or [batch][rows][M]) and
    b_stack [batch][rows][N] (contiguous), c [batch][M][N]; rows split into ranges of about
    `rows_per_split` (0: enough to fill the chip)."""

    def __init__(self, a: torch.Tensor, b: torch.Tensor, c: torch.Tensor, rows_per_split: int = 0):
        _dev(a, torch.float32, "a")
        _dev(b, torch.float32, "b")
        _dev(c, torch.float32, "c")
        batch, rb, N = b.shape
        if a.dim() == 3:
            if a.shape[0] != batch:
                raise ValueError("gemm_tn: batched a must have one matrix per batch")
            rows, M = a.shape[1], a.shape[2]
            a_bs = rows * M
        else:
            rows, M = a.shape
            a_bs = 0
        if rb != rows or tuple(c.shape) != (batch, M, N):
            raise ValueError("gemm_tn: shapes")
        if rows_per_split <= 0:  # enough workgroups to fill the chip, ranges of >= 64 rows
            self.n_split = max(1, min(-(-1024 // max(1, batch)), -(-rows // 64)))
        else:
            self.n_split = max(1, -(-rows // max(2, rows_per_split)))
        self.partial = (torch.empty((self.n_split, batch, M, N), device=a.device) if self.n_split > 1 else None)
        self._keep = (a, b, c)
        self._args = (a.data_ptr(), M, a_bs, b.data_ptr(), N, rows * N, c.data_ptr(), rows, M, N, batch, self.n_split,
                      self.partial.data_ptr() if self.partial is not None else None)
        self._fn = _lib.load().dg_gemm_tn_f32

    def __call__(self, stream=None) -> None:
        check(self._fn(*self._args, _stream_ptr(stream)), "dg_gemm_tn_f32")


def matmul(a: torch.Tensor, b: torch.Tensor, out: Optional[torch.Tensor] = None,
           sa: Optional[torch.Tensor] = None, sc: Optional[torch.Tensor] = None, stream=None):
    """out = diag-scaled a @ b for 2-D fp32 device tensors (any strides)."""
    m, k = a.shape
    k2, n = b.shape
    if k != k2:
        raise ValueError("inner dimensions differ")
    if out is None:
        out = torch.empty((m, n), device=a.device, dtype=torch.float32)
    PreparedGemm(a, (0, a.stride(0), a.stride(1)), b, (0, b.stride(0), b.stride(1)), out,
                 (0, out.stride(0), out.stride(1)), m, n, k, 1, sa, sc)(stream)
    return out


# --------------------------------------------------------------------------------------
# Decoder, losses, sampler
# --------------------------------------------------------------------------------------
def decoder_score(row_table: torch.Tensor, col_table: torch.Tensor, row_idx: torch.Tensor,
                  col_idx: torch.Tensor, G: torch.Tensor, l: Optional[torch.Tensor],
                  out: Optional[torch.Tensor] = None, stream=None) -> torch.Tensor:
    """out[p] = row_table[row_idx[p]]ᵀ · L · G · L · col_table[col_idx[p]]."""
    _dev(row_table, torch.float32, "row_table")
    _dev(col_table, torch.float32, "col_table")
    _dev(row_idx, torch.int32, "row_idx")
    _dev(col_idx, torch.int32, "col_idx")
    _dev(G, torch.float32, "G")
    d = G.shape[0]
    if G.shape != (d, d) or row_table.shape[1] != d or col_table.shape[1] != d:
        raise ValueError("decoder: d mismatch")
    n = row_idx.numel()
    if col_idx.numel() != n:
        raise ValueError("row_idx / col_idx length mismatch")
    if l is not None:
        _dev(l, torch.float32, "l")
        if l.numel() != d:
            raise ValueError("l must have d entries")
    if out is None:
        out = torch.empty(n, device=G.device, dtype=torch.float32)
    fn = _lib.load().dg_decoder_score_f32
    check(fn(row_table.data_ptr(), row_table.shape[1], col_table.data_ptr(), col_table.shape[1],
             row_idx.data_ptr(), col_idx.data_ptr(), n, G.data_ptr(),
             l.data_ptr() if l is not None else None, d, out.data_ptr(), _stream_ptr(stream)),
          "dg_decoder_score_f32")
    return out


def _check_tensors(pairs, dtype) -> None:
    """Type, dtype and contiguity of the (tensor, name) pairs; a None tensor is an absent operand."""
    for t, nm in pairs:
        if t is None:
            continue
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{nm}: expected a torch.Tensor, got {type(t).__name__}")
        if t.dtype != dtype:
            raise TypeError(f"{nm}: dtype {t.dtype}, expected {dtype}")
        if not t.is_contiguous():
            raise ValueError(f"{nm}: must be contiguous")


def _need_device(pairs) -> None:
    for t, nm in pairs:
        if t is not None and not t.is_cuda:
            raise ValueError(f"{nm}: must be a device (HIP) tensor")


WIDTHS_SEG = (range(32, 257, 32), "a multiple of 32, at most 256")  # dg::score_tile's widths
WIDTHS_MFMA = ((32, 64), "32 or 64")                                # the register-resident tiles'


@dataclass(frozen=True)
class RelOperands:
    """The per-relation decoder operands of the all-relation entry points (decagon_hip.h,
    "Per-relation operands"), validated: G [d, d] (shared by every relation) or [K, d, d]; l None
    (identity), [d] (shared) or [K, d]; K the leading dimension of whichever is per relation,
    None when nothing is (then any relation index serves)."""
    tabs: tuple  # (tensor, name) of row_table, col_table, G, l: what the launch reads
    d: int
    K: Optional[int]
    n_rows: int
    n_cols: int

    @classmethod
    def build(cls, name, row_table, col_table, G, l, widths, idx=(), empty="empty table") -> "RelOperands":
        """Checks, in order: type, dtype and contiguity of the operands and of the int32 index
        tensors `idx` ((tensor, name) pairs); ranks; d; the width rule `widths`; empty tables;
        the relation counts of G and l agreeing; K >= 1.  Nothing is required on the device yet
        (_need_device comes last in every wrapper)."""
        tabs = ((row_table, "row_table"), (col_table, "col_table"), (G, "G"), (l, "l"))
        _check_tensors(tabs, torch.float32)
        _check_tensors(idx, torch.int32)
        if row_table.dim() != 2 or col_table.dim() != 2 or G.dim() not in (2, 3):
            raise ValueError(f"{name}: tables must be [N, d] and G [d, d] or [K, d, d]")
        d = G.shape[-1]
        if G.shape[-2] != d or row_table.shape[1] != d or col_table.shape[1] != d:
            raise ValueError(f"{name}: d mismatch")
        if l is not None and (l.dim() not in (1, 2) or l.shape[-1] != d):
            raise ValueError(f"{name}: d mismatch (l must be [d] or [K, d])")
        if d not in widths[0]:
            raise ValueError(f"{name}: d = {d} unsupported ({widths[1]})")
        n_rows, n_cols = row_table.shape[0], col_table.shape[0]
        if n_rows < 1 or n_cols < 1:
            raise ValueError(f"{name}: {empty}")
        ks = {int(t.shape[0]) for t, per in ((G, G.dim() == 3), (l, l is not None and l.dim() == 2)) if per}
        if len(ks) > 1:
            raise ValueError(f"{name}: relation counts disagree: {sorted(ks)}")
        K = ks.pop() if ks else None
        if K is not None and K < 1:
            raise ValueError(f"{name}: no relations")
        return cls(tabs, d, K, n_rows, n_cols)

    def c_args(self):
        """(G, g_stride, l, l_stride) as the entry points take them."""
        G, l = self.tabs[2][0], self.tabs[3][0]
        return (G.data_ptr(), self.d * self.d if G.dim() == 3 else 0, l.data_ptr() if l is not None else None,
                self.d if (l is not None and l.dim() == 2) else 0)

    def n_rel(self, n_slots: int, mapped: bool) -> int:
        """The relation count of the call: K; with nothing per relation, unbounded under a map and
        the slot count without one (slot s is relation s)."""
        return self.K if self.K is not None else (2**31 - 1 if mapped else n_slots)

    def need_slots(self, name, n_slots: int, what: str) -> None:
        """Without a map, per-relation operands bound the slot count."""
        if self.K is not None and n_slots > self.K:
            raise ValueError(f"{name}: {n_slots} {what} but {self.K} relations (pass seg_rel)")


def decoder_score_seg(row_table: torch.Tensor, col_table: torch.Tensor, row_idx: torch.Tensor,
                      col_idx: torch.Tensor, seg_ptr: torch.Tensor, G: torch.Tensor, l: Optional[torch.Tensor],
                      seg_rel: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                      stream=None) -> torch.Tensor:
    """Scores of pairs packed by segment, every segment with its own relation, in one launch
    (dg_decoder_score_seg_f32): for pair p of segment s = [seg_ptr[s], seg_ptr[s+1]) and
    k = seg_rel[s] (seg_rel None: k = s),
        out[p] = (row_table[row_idx[p]] ∘ l_k)ᵀ · G_k · (l_k ∘ col_table[col_idx[p]])
    — bit for bit decoder_score(…, G_k, l_k) on the segment's pairs.  Asynchronous; seg_ptr
    (device int32 [n_seg + 1], ascending from 0 to the pair count) is never read on the host.

    G: [d, d] (shared by every relation) or [K, d, d]; l: None (identity), [d] (shared) or [K, d];
    K is the leading dimension of whichever is per relation.  seg_rel: device int32 [n_seg] with
    values in [0, K).  A pair outside the tables, or a segment whose relation is outside [0, K),
    scores NaN."""
    idx = [(row_idx, "row_idx"), (col_idx, "col_idx"), (seg_ptr, "seg_ptr"), (seg_rel, "seg_rel")]
    ops = RelOperands.build("decoder_score_seg", row_table, col_table, G, l, WIDTHS_SEG, idx)
    n = row_idx.numel()
    if col_idx.numel() != n:
        raise ValueError("decoder_score_seg: row_idx / col_idx length mismatch")
    n_seg = seg_ptr.numel() - 1
    if n_seg < 1:
        raise ValueError("decoder_score_seg: seg_ptr must have n_seg + 1 >= 2 entries")
    if seg_rel is not None and seg_rel.numel() != n_seg:
        raise ValueError("decoder_score_seg: seg_rel must have one entry per segment")
    if seg_rel is None:
        ops.need_slots("decoder_score_seg", n_seg, "segments")
    if out is not None:
        if not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or not out.is_contiguous():
            raise TypeError("out: expected a contiguous float32 torch.Tensor")
        if out.numel() != n:
            raise ValueError("decoder_score_seg: out must have one entry per pair")
    _need_device(list(ops.tabs) + idx + [(out, "out")])
    if out is None:
        out = torch.empty(n, device=G.device, dtype=torch.float32)
    d = ops.d
    fn = _lib.load().dg_decoder_score_seg_f32
    check(fn(row_table.data_ptr(), d, ops.n_rows, col_table.data_ptr(), d, ops.n_cols,
             row_idx.data_ptr() if n else None, col_idx.data_ptr() if n else None, seg_ptr.data_ptr(),
             seg_rel.data_ptr() if seg_rel is not None else None, n_seg, n, *ops.c_args(),
             ops.n_rel(n_seg, seg_rel is not None), d, out.data_ptr() if n else None, _stream_ptr(stream)),
          "dg_decoder_score_seg_f32")
    return out


def _stacked_exclusion(name, exclude, n_rows: int, n_cols: int, ks: set):
    """(rowptr, col) of `exclude` — None, a sparse.ExclusionCSR (host arrays) or a (rowptr, col) pair
    of tensors in that layout — checked against the tables on the host; its relation count joins `ks`."""
    if exclude is None:
        return None, None
    if hasattr(exclude, "rowptr") and hasattr(exclude, "n_rels"):
        if (exclude.n_rows, exclude.n_cols) != (n_rows, n_cols):
            raise ValueError(f"{name}: exclusion shape does not match the tables")
        ks.add(int(exclude.n_rels))
        return exclude.rowptr, exclude.col
    ex_rowptr, ex_col = exclude
    if (ex_rowptr.numel() - 1) % n_rows:
        raise ValueError(f"{name}: exclusion rowptr must have K·N_i + 1 entries")
    ks.add((ex_rowptr.numel() - 1) // n_rows)
    return ex_rowptr, ex_col


def _exclusion_on_device(name, ex_rowptr, ex_col, K: int, n_rows: int, dev):
    """_stacked_exclusion's pair as device int32 tensors of K relations (host arrays are uploaded);
    (None, None) where nothing is excluded."""
    if isinstance(ex_rowptr, np.ndarray):
        ex_rowptr, ex_col = torch.from_numpy(ex_rowptr).to(dev), torch.from_numpy(ex_col).to(dev)
    if ex_rowptr is not None:
        _dev(ex_rowptr, torch.int32, "exclude rowptr")
        _dev(ex_col, torch.int32, "exclude col")
        if ex_rowptr.numel() != K * n_rows + 1:
            raise ValueError(f"{name}: exclusion rowptr must have K·N_i + 1 entries")
        if ex_col.numel() == 0:
            ex_rowptr = ex_col = None  # nothing excluded
    return ex_rowptr, ex_col


def _relation_count(name, ops: RelOperands, exclude):
    """(K, ex_rowptr, ex_col): the relation count the operands and `exclude` agree on (None where
    nothing is per relation) and _stacked_exclusion's pair."""
    ks = set() if ops.K is None else {ops.K}  # … and the exclusion's relation count
    ex_rowptr, ex_col = _stacked_exclusion(name, exclude, ops.n_rows, ops.n_cols, ks)
    if len(ks) > 1:
        raise ValueError(f"{name}: relation counts disagree: {sorted(ks)}")
    K = ks.pop() if ks else None
    if K is not None and K < 1:
        raise ValueError(f"{name}: no relations")
    return K, ex_rowptr, ex_col


def _segmented_ranking(name, row_table, col_table, G, l, queries, seg_ptr, seg_rel, exclude, no_self: bool,
                       own_checks=None):
    """The preparation decoder_edge_rank and decoder_node_topk share: (ops, n, n_seg, n_rel,
    ex_rowptr, ex_col).  `queries` are the (tensor, name) pairs of the per-query index tensors, n
    their common length.  Checks the operands, the segments, the 2^31 bound, no_self and the
    relation counts, then that everything is on the device, and puts the exclusion there.
    `own_checks()` raises the caller's own ValueErrors where they always stood: after the operands'."""
    idx = list(queries) + [(seg_ptr, "seg_ptr"), (seg_rel, "seg_rel")]
    ops = RelOperands.build(name, row_table, col_table, G, l, WIDTHS_MFMA, idx)
    if own_checks is not None:
        own_checks()
    n = queries[0][0].numel()
    if any(t.numel() != n for t, _ in queries):
        raise ValueError(f"{name}: {' / '.join(nm for _, nm in queries)} length mismatch")
    n_seg = seg_ptr.numel() - 1
    if n_seg < 1:
        raise ValueError(f"{name}: seg_ptr must have n_seg + 1 >= 2 entries")
    if seg_rel is not None and seg_rel.numel() != n_seg:
        raise ValueError(f"{name}: seg_rel must have one entry per segment")
    if n + 32 * n_seg >= 2**31:
        raise ValueError(f"{name}: needs queries + 32·segments < 2^31")
    if no_self and ops.n_rows != ops.n_cols:
        raise ValueError(f"{name}: no_self needs square tables")
    K, ex_rowptr, ex_col = _relation_count(name, ops, exclude)
    if seg_rel is None and K is not None and n_seg > K:
        raise ValueError(f"{name}: {n_seg} segments but {K} relations (pass seg_rel)")
    _need_device(list(ops.tabs) + idx)
    ex_rowptr, ex_col = _exclusion_on_device(name, ex_rowptr, ex_col, K, ops.n_rows, G.device)
    n_rel = K if K is not None else ops.n_rel(n_seg, seg_rel is not None)
    return ops, n, n_seg, n_rel, ex_rowptr, ex_col


def decoder_topk(row_table: torch.Tensor, col_table: torch.Tensor, G: torch.Tensor, l: Optional[torch.Tensor],
                 topk: int, exclude=None, upper: bool = False, no_diag: bool = False, stream=None
                 ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """(scores [K, topk] float32, rows [K, topk] int32, cols [K, topk] int32, counts [K] int32):
    per relation k the topk highest permitted pairs of (row_table[r] ∘ l_k)ᵀ·G_k·(l_k ∘ col_table[c])
    (dg_decoder_topk_f32: higher score first, ties by smaller r·N_j + c, −0 as +0; slots past
    counts[k] hold −inf / −1).  No N_i×N_j matrix is formed.

    G: [d, d] (shared by every relation) or [K, d, d]; l: None (identity), [d] (shared) or [K, d].
    K is the leading dimension of whichever is per relation (1 if neither), and of `exclude`.
    exclude: None, a sparse.ExclusionCSR (uploaded here), or a (rowptr, col) pair of device int32
    tensors in that layout (columns ascending and unique within each row).
    upper: only r < c (square tables); no_diag: drop r == c."""
    ops = RelOperands.build("decoder_topk", row_table, col_table, G, l, WIDTHS_MFMA,
                            empty="needs 1 <= N_i·N_j < 2^32")
    d, n_rows, n_cols = ops.d, ops.n_rows, ops.n_cols
    topk = int(topk)
    if not 1 <= topk <= _lib.DG_TOPK_MAX_K:
        raise ValueError(f"decoder_topk: topk must be in [1, {_lib.DG_TOPK_MAX_K}]")
    if n_rows * n_cols >= 2**32:
        raise ValueError("decoder_topk: needs 1 <= N_i·N_j < 2^32")
    if upper and n_rows != n_cols:
        raise ValueError("decoder_topk: upper needs square tables")
    K, ex_rowptr, ex_col = _relation_count("decoder_topk", ops, exclude)
    K = 1 if K is None else K
    _need_device(ops.tabs)
    dev = G.device
    ex_rowptr, ex_col = _exclusion_on_device("decoder_topk", ex_rowptr, ex_col, K, n_rows, dev)
    lib = _lib.load()
    nbytes = int(lib.dg_decoder_topk_workspace(K, n_rows, n_cols, topk))
    ws = torch.empty(-(-nbytes // 8), dtype=torch.int64, device=dev)
    scores = torch.empty((K, topk), dtype=torch.float32, device=dev)
    rows = torch.empty((K, topk), dtype=torch.int32, device=dev)
    cols = torch.empty((K, topk), dtype=torch.int32, device=dev)
    counts = torch.empty(K, dtype=torch.int32, device=dev)
    flags = (_lib.DG_TOPK_UPPER if upper else 0) | (_lib.DG_TOPK_NO_DIAG if no_diag else 0)
    check(lib.dg_decoder_topk_f32(
        row_table.data_ptr(), d, n_rows, col_table.data_ptr(), d, n_cols, *ops.c_args(), K, d, topk,
        ex_rowptr.data_ptr() if ex_rowptr is not None else None,
        ex_col.data_ptr() if ex_col is not None else None, flags, scores.data_ptr(), rows.data_ptr(),
        cols.data_ptr(), counts.data_ptr(), ws.data_ptr(), ws.numel() * 8, _stream_ptr(stream)),
        "dg_decoder_topk_f32")
    return scores, rows, cols, counts


def decoder_edge_rank(row_table: torch.Tensor, col_table: torch.Tensor, row_idx: torch.Tensor,
                      col_idx: torch.Tensor, seg_ptr: torch.Tensor, G: torch.Tensor, l: Optional[torch.Tensor],
                      seg_rel: Optional[torch.Tensor] = None, exclude=None, no_self: bool = False, stream=None,
                      column_split: bool = True) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(rank int32, score float32, cand int32), one entry per query: the filtered rank of held-out
    edges in one launch (dg_decoder_edge_rank_f32).  Query q = (row_idx[q], col_idx[q]) = (r, c) of
    segment s = [seg_ptr[s], seg_ptr[s+1]) has relation k = seg_rel[s] (seg_rel None: k = s); its
    candidates are the columns c' that relation k's exclusion row of r does not hold (and, with
    no_self, c' != r: square tables), plus c itself.  rank[q] = 1 + the candidates c' != c before c
    under (row_table[r] ∘ l_k)ᵀ·G_k·(l_k ∘ col_table[c']) — higher score first, ties by smaller
    column, −0 as +0; score[q] that score of (r, c); cand[q] the number of candidates, c included.
    No N_i×N_j matrix is formed.  A query outside the tables, or of a segment whose relation lies
    outside [0, K), gets rank 0, cand 0 and NaN.  Asynchronous; seg_ptr (device int32 [n_seg + 1],
    ascending from 0 to the query count) is never read on the host.

    G, l, seg_rel: as decoder_score_seg (d is 32 or 64).  exclude: as decoder_topk — None, a
    sparse.ExclusionCSR (uploaded here) or a device (rowptr, col) pair; its relation count is K too.
    column_split=False keeps every query tile's columns in one workgroup (the measured alternative
    of DESIGN.md §20; same results)."""
    ops, n, n_seg, n_rel, ex_rowptr, ex_col = _segmented_ranking(
        "decoder_edge_rank", row_table, col_table, G, l, [(row_idx, "row_idx"), (col_idx, "col_idx")], seg_ptr,
        seg_rel, exclude, no_self)
    d, n_rows, n_cols, dev = ops.d, ops.n_rows, ops.n_cols, G.device
    rank = torch.empty(n, dtype=torch.int32, device=dev)
    score = torch.empty(n, dtype=torch.float32, device=dev)
    cand = torch.empty(n, dtype=torch.int32, device=dev)
    flags = (_lib.DG_EDGE_RANK_NO_SELF if no_self else 0) | (0 if column_split else _lib.DG_EDGE_RANK_NO_SPLIT)
    fn = _lib.load().dg_decoder_edge_rank_f32
    check(fn(*_lib.pack(
        "dg_decoder_edge_rank_f32", row_table=row_table.data_ptr(), ld_row=d, n_rows=n_rows,
        col_table=col_table.data_ptr(), ld_col=d, n_cols=n_cols, row_idx=row_idx.data_ptr() if n else None,
        col_idx=col_idx.data_ptr() if n else None, seg_ptr=seg_ptr.data_ptr(),
        seg_rel=seg_rel.data_ptr() if seg_rel is not None else None, n_seg=n_seg, n_queries=n,
        **dict(zip(("G", "g_stride", "l", "l_stride"), ops.c_args())),
        n_rel=n_rel, d=d, excl_rowptr=ex_rowptr.data_ptr() if ex_rowptr is not None else None,
        excl_col=ex_col.data_ptr() if ex_col is not None else None, flags=flags,
        out_rank=rank.data_ptr() if n else None, out_score=score.data_ptr() if n else None,
        out_cand=cand.data_ptr() if n else None, stream=_stream_ptr(stream))), "dg_decoder_edge_rank_f32")
    return rank, score, cand


def decoder_node_topk(row_table: torch.Tensor, col_table: torch.Tensor, row_idx: torch.Tensor,
                      seg_ptr: torch.Tensor, G: torch.Tensor, l: Optional[torch.Tensor], topk: int,
                      seg_rel: Optional[torch.Tensor] = None, exclude=None, no_self: bool = False,
                      column_split: bool = True, stream=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(scores float32 [n, topk], cols int32 [n, topk], counts int32 [n]): every query node's topk
    best permitted partners in one fused launch pair (dg_decoder_node_topk_f32).  Query q =
    row_idx[q] = r of segment s = [seg_ptr[s], seg_ptr[s+1]) has relation k = seg_rel[s] (seg_rel
    None: k = s); its permitted columns are those relation k's exclusion row of r does not hold
    (and, with no_self, c' != r: square tables).  They are ranked under
    (row_table[r] ∘ l_k)ᵀ·G_k·(l_k ∘ col_table[c']) — higher score first, ties by smaller column,
    −0 as +0; counts[q] = min(topk, permitted columns), and slots past it hold −inf / −1.  No
    N_i×N_j matrix is formed.  A query outside the table, or of a segment whose relation lies
    outside [0, K), gets count 0.  Asynchronous; seg_ptr (device int32 [n_seg + 1], ascending from
    0 to the query count) is never read on the host.

    G, l, seg_rel, exclude: as decoder_edge_rank (d is 32 or 64).  column_split=False keeps every
    query tile's columns in one workgroup (the measured alternative of DESIGN.md §21; same
    results)."""
    def topk_in_range():
        if not 1 <= int(topk) <= _lib.DG_NODE_TOPK_MAX_K:
            raise ValueError(f"decoder_node_topk: topk must be in [1, {_lib.DG_NODE_TOPK_MAX_K}]")

    ops, n, n_seg, n_rel, ex_rowptr, ex_col = _segmented_ranking(
        "decoder_node_topk", row_table, col_table, G, l, [(row_idx, "row_idx")], seg_ptr, seg_rel, exclude, no_self,
        own_checks=topk_in_range)
    topk = int(topk)
    d, n_rows, n_cols, dev = ops.d, ops.n_rows, ops.n_cols, G.device
    lib = _lib.load()
    nbytes = int(lib.dg_decoder_node_topk_workspace(n, n_seg, n_cols, topk))
    ws = torch.empty(-(-nbytes // 16) * 2, dtype=torch.int64, device=dev) if nbytes else None
    scores = torch.empty((n, topk), dtype=torch.float32, device=dev)
    cols = torch.empty((n, topk), dtype=torch.int32, device=dev)
    counts = torch.empty(n, dtype=torch.int32, device=dev)
    flags = (_lib.DG_NODE_TOPK_NO_SELF if no_self else 0) | (0 if column_split else _lib.DG_NODE_TOPK_NO_SPLIT)
    check(lib.dg_decoder_node_topk_f32(*_lib.pack(
        "dg_decoder_node_topk_f32", row_table=row_table.data_ptr(), ld_row=d, n_rows=n_rows,
        col_table=col_table.data_ptr(), ld_col=d, n_cols=n_cols, row_idx=row_idx.data_ptr() if n else None,
        seg_ptr=seg_ptr.data_ptr(), seg_rel=seg_rel.data_ptr() if seg_rel is not None else None, n_seg=n_seg,
        n_queries=n, **dict(zip(("G", "g_stride", "l", "l_stride"), ops.c_args())),
        n_rel=n_rel, d=d, topk=topk,
        excl_rowptr=ex_rowptr.data_ptr() if ex_rowptr is not None else None,
        excl_col=ex_col.data_ptr() if ex_col is not None else None, flags=flags,
        out_score=scores.data_ptr() if n else None, out_col=cols.data_ptr() if n else None,
        out_count=counts.data_ptr() if n else None, workspace=ws.data_ptr() if ws is not None else None,
        workspace_bytes=ws.numel() * 8 if ws is not None else 0, stream=_stream_ptr(stream))),
        "dg_decoder_node_topk_f32")
    return scores, cols, counts


def cross_slot_chunk(n_pairs: int, n_sel: int) -> int:
    """The slot chunk C dg_decoder_score_cross_f32 uses for n_pairs pairs against n_sel slots (one
    wave scores a 32-pair tile against C consecutive slots): the library's own choice, host only."""
    return int(_lib.load().dg_decoder_score_cross_chunk(int(n_pairs), int(n_sel)))


def _cross_operands(name, row_table, col_table, row_idx, col_idx, G, l, rel_idx):
    """Validation shared by decoder_score_cross and decoder_top_relations: (ops, n_pairs, n_sel)."""
    ops = RelOperands.build(name, row_table, col_table, G, l, WIDTHS_MFMA,
                            [(row_idx, "row_idx"), (col_idx, "col_idx"), (rel_idx, "rel_idx")])
    if row_idx.dim() != 1 or col_idx.dim() != 1 or col_idx.numel() != row_idx.numel():
        raise ValueError(f"{name}: row_idx / col_idx must be vectors of one length")
    if rel_idx is not None and (rel_idx.dim() != 1 or rel_idx.numel() < 1):
        raise ValueError(f"{name}: rel_idx must be a non-empty vector")
    if rel_idx is None and ops.K is None:
        raise ValueError(f"{name}: no per-relation operand: pass rel_idx to name the slots")
    return ops, row_idx.numel(), rel_idx.numel() if rel_idx is not None else ops.K


def _score_cross_call(ops, row_idx, col_idx, rel_idx, n_sel, p0, n, out, stream) -> None:
    """Pairs [p0, p0 + n) into the rows of `out` (row stride out.stride(0)); arguments validated."""
    if n == 0:
        return
    (row_table, _), (col_table, _) = ops.tabs[:2]
    check(_lib.load().dg_decoder_score_cross_f32(
        row_table.data_ptr(), ops.d, ops.n_rows, col_table.data_ptr(), ops.d, ops.n_cols,
        row_idx.data_ptr() + 4 * p0, col_idx.data_ptr() + 4 * p0, n, *ops.c_args(),
        rel_idx.data_ptr() if rel_idx is not None else None, n_sel, ops.n_rel(n_sel, rel_idx is not None), ops.d,
        out.data_ptr(), out.stride(0), _stream_ptr(stream)), "dg_decoder_score_cross_f32")


def decoder_score_cross(row_table: torch.Tensor, col_table: torch.Tensor, row_idx: torch.Tensor,
                        col_idx: torch.Tensor, G: torch.Tensor, l: Optional[torch.Tensor],
                        rel_idx: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                        stream=None) -> torch.Tensor:
    """Every relation's score of every given pair in one launch (dg_decoder_score_cross_f32): a
    float32 device tensor [P, n_sel],
        out[p, s] = (row_table[row_idx[p]] ∘ l_k)ᵀ · G_k · (l_k ∘ col_table[col_idx[p]]),  k = rel_idx[s]
    (rel_idx None: k = s, every relation in order) — bit for bit decoder_score(…, G_k, l_k) on
    the same pairs.  Asynchronous; nothing is read on the host.

    G: [d, d] (shared by every relation) or [K, d, d]; l: None (identity), [d] (shared) or [K, d];
    K is the leading dimension of whichever is per relation; d is 32 or 64.  rel_idx: device int32
    [n_sel] with values in [0, K), repeats and any order allowed (required when no operand is per
    relation).  out: float32 [P, ≥ n_sel] device tensor or row-strided view (stride(1) == 1,
    stride(0) ≥ n_sel); its columns past n_sel are not written, and out[:, :n_sel] is returned.
    A pair outside the tables scores a row of NaN, a slot whose relation is outside [0, K) a
    column of NaN."""
    ops, n, n_sel = _cross_operands("decoder_score_cross", row_table, col_table, row_idx, col_idx, G, l, rel_idx)
    if out is not None:
        if not isinstance(out, torch.Tensor) or out.dtype != torch.float32:
            raise TypeError("out: expected a float32 torch.Tensor")
        if out.dim() != 2 or out.shape[0] != n or out.shape[1] < n_sel:
            raise ValueError("decoder_score_cross: out must be [P, >= n_sel]")
        if out.stride(1) != 1 or out.stride(0) < max(n_sel, out.shape[1]):
            raise ValueError("decoder_score_cross: out must have stride(1) == 1 and stride(0) >= n_sel")
    _need_device(list(ops.tabs) + [(row_idx, "row_idx"), (col_idx, "col_idx"), (rel_idx, "rel_idx"), (out, "out")])
    if n * (out.stride(0) if out is not None else n_sel) >= 2**38:
        raise ValueError("decoder_score_cross: P·ld_out must stay below 2^38 (score in chunks of pairs)")
    if out is None:
        out = torch.empty((n, n_sel), device=G.device, dtype=torch.float32)
    _score_cross_call(ops, row_idx, col_idx, rel_idx, n_sel, 0, n, out, stream)
    return out[:, :n_sel]


def _pair_lists(name, exclude, n):
    """The (ptr, slot) exclusion lists of n rows, checked but for the device: int32 vectors,
    contiguous, ptr of n + 1 entries (sparse.PairExclusion's layout)."""
    if not isinstance(exclude, (tuple, list)) or len(exclude) != 2:
        raise TypeError(f"{name}: exclude must be a (ptr, slot) pair of int32 device tensors")
    ptr, slot = exclude
    for t, nm in ((ptr, "exclude ptr"), (slot, "exclude slot")):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{nm}: expected a torch.Tensor, got {type(t).__name__}")
        if t.dtype != torch.int32:
            raise TypeError(f"{nm}: dtype {t.dtype}, expected {torch.int32}")
        if t.dim() != 1 or not t.is_contiguous():
            raise ValueError(f"{nm}: must be a contiguous vector")
    if ptr.numel() != n + 1:
        raise ValueError(f"{name}: exclude ptr must have one entry per row and one more ({n + 1})")
    if slot.numel() >= 2**31:
        raise ValueError(f"{name}: exclude slot exceeds int32 offsets")
    return ptr, slot


def row_topk(x: torch.Tensor, topk: int, stream=None, exclude=None
             ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(values [n, topk] float32, idx [n, topk] int32, counts [n] int32): the topk highest entries
    of every row of the float32 device matrix x, descending (dg_row_topk_f32: higher value first,
    ties by smaller column, −0 as +0; counts = min(topk, columns), slots past it hold −inf / −1).
    x may be a row-strided view (stride(1) == 1).  Asynchronous.

    exclude: None, or a (ptr, slot) pair of int32 device tensors, ptr [n + 1] and slot [nnz] —
    row r is selected among the columns that slot[ptr[r] : ptr[r + 1]] (ascending, unique) does
    not name (dg_row_topk_excl_f32), and counts[r] = min(topk, permitted columns)."""
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"x: expected a torch.Tensor, got {type(x).__name__}")
    if x.dtype != torch.float32:
        raise TypeError(f"x: dtype {x.dtype}, expected {torch.float32}")
    if x.dim() != 2 or x.shape[1] < 1:
        raise ValueError("row_topk: x must be [n, columns >= 1]")
    if x.stride(1) != 1 or (x.shape[0] > 1 and x.stride(0) < x.shape[1]):
        raise ValueError("row_topk: x must have stride(1) == 1 and stride(0) >= its columns")
    topk = int(topk)
    if not 1 <= topk <= _lib.DG_TOPK_MAX_K:
        raise ValueError(f"row_topk: topk must be in [1, {_lib.DG_TOPK_MAX_K}]")
    n = x.shape[0]
    if exclude is not None:
        exclude = _pair_lists("row_topk", exclude, n)
    _need_device([(x, "x")] + ([(exclude[0], "exclude ptr"), (exclude[1], "exclude slot")] if exclude else []))
    if exclude and (exclude[0].device != x.device or exclude[1].device != x.device):
        raise ValueError("row_topk: exclude must be on x's device")
    vals = torch.empty((n, topk), dtype=torch.float32, device=x.device)
    idx = torch.empty((n, topk), dtype=torch.int32, device=x.device)
    counts = torch.empty(n, dtype=torch.int32, device=x.device)
    _row_topk_call(x, topk, vals, idx, counts, stream, exclude)
    return vals, idx, counts


def _row_topk_call(x, topk, vals, idx, counts, stream, exclude=None, p0=0) -> None:
    """The rows of x selected into vals / idx / counts; with `exclude` = (ptr, slot), row r under
    list p0 + r: ptr is passed from entry p0 on with the whole of slot, whose offsets are absolute."""
    n = x.shape[0]
    if n == 0:
        return
    ld = max(x.stride(0), x.shape[1])
    if exclude is None or exclude[1].numel() == 0:  # (an empty tensor has no address: nothing is excluded)
        check(_lib.load().dg_row_topk_f32(x.data_ptr(), ld, n, x.shape[1], topk, vals.data_ptr(), idx.data_ptr(),
                                          counts.data_ptr(), None, 0, _stream_ptr(stream)), "dg_row_topk_f32")
        return
    ptr, slot = exclude
    check(_lib.load().dg_row_topk_excl_f32(x.data_ptr(), ld, n, x.shape[1], topk, ptr.data_ptr() + 4 * p0,
                                           slot.data_ptr(), slot.numel(), vals.data_ptr(), idx.data_ptr(),
                                           counts.data_ptr(), _stream_ptr(stream)), "dg_row_topk_excl_f32")


def top_relations_chunks(n_pairs: int, n_sel: int, max_workspace_bytes: int):
    """The pair ranges [(start, stop), …] decoder_top_relations scores one after the other: every
    range but the last holds the same number of pairs, a multiple of 32 and at least 32, and the
    largest such number whose [pairs, n_sel] float32 score workspace fits max_workspace_bytes (32
    pairs when not even those fit).  Pure host arithmetic."""
    n_pairs, n_sel = int(n_pairs), int(n_sel)
    if n_pairs < 0 or n_sel < 1:
        raise ValueError("top_relations_chunks: needs n_pairs >= 0 and n_sel >= 1")
    rows = max(32, int(max_workspace_bytes) // (4 * n_sel) // 32 * 32)
    rows = min(rows, max(32, -(-n_pairs // 32) * 32))
    return [(p, min(p + rows, n_pairs)) for p in range(0, n_pairs, rows)]


def decoder_top_relations(row_table: torch.Tensor, col_table: torch.Tensor, row_idx: torch.Tensor,
                          col_idx: torch.Tensor, G: torch.Tensor, l: Optional[torch.Tensor], topk: int,
                          rel_idx: Optional[torch.Tensor] = None, max_workspace_bytes: int = 64 << 20,
                          stream=None, exclude=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(scores [P, topk] float32, slots [P, topk] int32, counts [P] int32): for every pair the topk
    highest-scoring slots of decoder_score_cross's row (operands and rel_idx as there; a slot is a
    position of rel_idx, or the relation itself when rel_idx is None), in row_topk's order.

    The pairs are scored top_relations_chunks(…) at a time into one [chunk, n_sel] workspace of at
    most max_workspace_bytes (at least 32 rows) and each chunk is selected into its rows of the
    outputs, so no P×n_sel matrix exists at any time.  A pair's scores do not depend on its
    neighbours and the selection order is total: the result is the same, bytes and all, whatever
    the bound.

    exclude: None, or row_topk's (ptr, slot) pair with one list per PAIR (sparse.PairExclusion's
    layout): pair p is ranked among the slots its list does not name, counts[p] = min(topk,
    n_sel − its entries).  A chunk reads ptr from its first pair on and the whole of slot — the
    offsets are absolute — so the bound still does not change a byte."""
    ops, n, n_sel = _cross_operands("decoder_top_relations", row_table, col_table, row_idx, col_idx, G, l, rel_idx)
    topk = int(topk)
    if not 1 <= topk <= _lib.DG_TOPK_MAX_K:
        raise ValueError(f"decoder_top_relations: topk must be in [1, {_lib.DG_TOPK_MAX_K}]")
    if exclude is not None:
        exclude = _pair_lists("decoder_top_relations", exclude, n)
    _need_device(list(ops.tabs) + [(row_idx, "row_idx"), (col_idx, "col_idx"), (rel_idx, "rel_idx")]
                 + ([(exclude[0], "exclude ptr"), (exclude[1], "exclude slot")] if exclude else []))
    dev = G.device
    if exclude and (exclude[0].device != dev or exclude[1].device != dev):
        raise ValueError("decoder_top_relations: exclude must be on the operands' device")
    vals = torch.empty((n, topk), dtype=torch.float32, device=dev)
    idx = torch.empty((n, topk), dtype=torch.int32, device=dev)
    counts = torch.empty(n, dtype=torch.int32, device=dev)
    chunks = top_relations_chunks(n, n_sel, max_workspace_bytes)
    if chunks:
        ws = torch.empty((chunks[0][1] - chunks[0][0], n_sel), dtype=torch.float32, device=dev)
    for p0, p1 in chunks:
        m = p1 - p0
        _score_cross_call(ops, row_idx, col_idx, rel_idx, n_sel, p0, m, ws, stream)
        _row_topk_call(ws[:m], topk, vals[p0:p1], idx[p0:p1], counts[p0:p1], stream, exclude, p0)
    return vals, idx, counts


def decoder_score_bf16(row_table: torch.Tensor, col_table: torch.Tensor, rows: torch.Tensor,
                       cols: torch.Tensor, G: torch.Tensor, l_table: Optional[torch.Tensor] = None,
                       rel: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                       stream=None, paired: bool = False) -> torch.Tensor:
    """bf16 DEDICOM scores of pairs (rows[p], cols[p]) of relations rel[p] (dg_decoder_score_bf16):
    uᵀ·D_k·G·D_k·v with bf16 tables / G / diagonals and fp32 accumulation (config 5).
    paired: the caller promises pair p and pair p + n/2 share the column and the relation (a
    positive and its negative); dg_decoder_score_bf16_paired contracts the shared side once,
    T = G·bf16(D_k∘v), and dots it with both rows (half the MFMA work; the bf16 operand rounding
    sits on D_k∘v instead of u∘D_k), reading cols and rel of the first half only."""
    n = rows.numel()
    if paired and (n % 2 or cols.numel() != n or (rel is not None and rel.numel() != n)):
        raise ValueError("paired scoring needs an even number of pairs, cols / rel of the same length")
    d = G.shape[0]
    for t, nm in ((row_table, "row_table"), (col_table, "col_table"), (G, "G")):
        _dev(t, torch.bfloat16, nm)
    if l_table is not None:
        _dev(l_table, torch.bfloat16, "l_table")
        if l_table.shape[-1] != d or l_table.stride(-1) != 1 or (l_table.dim() == 2 and l_table.stride(0) != d):
            raise ValueError("l_table must be a contiguous [n_rel, d] bf16 tensor")
    for t, nm in ((rows, "rows"), (cols, "cols")):
        _dev(t, torch.int32, nm)
    if rel is not None:
        _dev(rel, torch.int32, "rel")
    if G.shape != (d, d) or not G.is_contiguous():
        raise ValueError("G must be a contiguous d×d bf16 matrix")
    if row_table.shape[1] != d or col_table.shape[1] != d or row_table.stride(1) != 1 or col_table.stride(1) != 1:
        raise ValueError("tables must have d contiguous columns")
    if out is None:
        out = torch.empty(n, device=rows.device, dtype=torch.float32)
    if paired:
        name = "dg_decoder_score_bf16_paired"
        tabs = (row_table.data_ptr(), row_table.stride(0), row_table.shape[0], col_table.data_ptr(),
                col_table.stride(0), col_table.shape[0])
    else:
        name = "dg_decoder_score_bf16"
        tabs = (row_table.data_ptr(), row_table.stride(0), col_table.data_ptr(), col_table.stride(0))
    check(getattr(_lib.load(), name)(
        *tabs, rows.data_ptr(), cols.data_ptr(), rel.data_ptr() if rel is not None else None,
        n // 2 if paired else n, G.data_ptr(), l_table.data_ptr() if l_table is not None else None, d,
        out.data_ptr(), _stream_ptr(stream)), name)
    return out


def hinge_loss(pos: torch.Tensor, neg: torch.Tensor, margin: float,
               out: Optional[torch.Tensor] = None, stream=None,
               workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Σ relu(neg − pos + margin) (optimizer.py:116-120): one workgroup, or — with a
    workspace of DG_HINGE_WS_BYTES (first word zero; hinge_workspace()) — up to 256."""
    _dev(pos, torch.float32, "pos")
    _dev(neg, torch.float32, "neg")
    if pos.numel() != neg.numel():
        raise ValueError("pos/neg length mismatch")
    if out is None:
        out = torch.empty(1, device=pos.device, dtype=torch.float32)
    if workspace is not None:
        if workspace.numel() * workspace.element_size() < _lib.DG_HINGE_WS_BYTES or not workspace.is_cuda:
            raise ValueError("hinge workspace too small")
        check(_lib.load().dg_hinge_loss_ws_f32(pos.data_ptr(), neg.data_ptr(), pos.numel(), float(margin),
                                                out.data_ptr(), workspace.data_ptr(), _stream_ptr(stream)),
              "dg_hinge_loss_ws_f32")
        return out
    check(_lib.load().dg_hinge_loss_f32(pos.data_ptr(), neg.data_ptr(), pos.numel(), float(margin),
                                         out.data_ptr(), _stream_ptr(stream)), "dg_hinge_loss_f32")
    return out


def hinge_workspace(device) -> torch.Tensor:
    return torch.zeros(_lib.DG_HINGE_WS_BYTES // 4, dtype=torch.int32, device=device)


def xent_loss(pos: torch.Tensor, neg: torch.Tensor, neg_weight: float,
              out: Optional[torch.Tensor] = None, stream=None,
              workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Σ softplus(−pos) + neg_weight·Σ softplus(neg) (optimizer.py:122-127): one workgroup, or — with
    a workspace as hinge_loss takes it (hinge_workspace() serves both) — up to 256, in fp32 terms."""
    _dev(pos, torch.float32, "pos")
    _dev(neg, torch.float32, "neg")
    if pos.numel() != neg.numel():
        raise ValueError("pos/neg length mismatch")
    if out is None:
        out = torch.empty(1, device=pos.device, dtype=torch.float32)
    if workspace is not None:
        if workspace.numel() * workspace.element_size() < _lib.DG_HINGE_WS_BYTES or not workspace.is_cuda:
            raise ValueError("xent workspace too small")
        check(_lib.load().dg_xent_loss_ws_f32(pos.data_ptr(), neg.data_ptr(), pos.numel(), float(neg_weight),
                                               out.data_ptr(), workspace.data_ptr(), _stream_ptr(stream)),
              "dg_xent_loss_ws_f32")
        return out
    check(_lib.load().dg_xent_loss_f32(pos.data_ptr(), neg.data_ptr(), pos.numel(), float(neg_weight),
                                        out.data_ptr(), _stream_ptr(stream)), "dg_xent_loss_f32")
    return out


LOSSES = ("hinge", "xent")  # the costs of optimizer.py:116-127 the backward kernels know


def loss_param(loss: str, margin: float, neg_weight: float) -> float:
    """The one parameter of the cost's kernels: the hinge's margin, the cross-entropy's neg_weight."""
    if loss not in LOSSES:
        raise ValueError(f"loss must be one of {LOSSES}, got {loss!r}")
    return float(margin) if loss == "hinge" else float(neg_weight)


def unigram_sample(table: torch.Tensor, n: int, seed: int, offset: int,
                   out: Optional[torch.Tensor] = None, stream=None) -> torch.Tensor:
    """n draws from an alias table (sampling.alias_table, uploaded as int32 [range, 2])."""
    _dev(table, torch.int32, "alias table")
    if table.dim() != 2 or table.shape[1] != 2:
        raise ValueError("alias table must be [range, 2]")
    if out is None:
        out = torch.empty(n, device=table.device, dtype=torch.int32)
    _dev(out, torch.int32, "out")
    if out.numel() < n:
        raise ValueError("out too small")
    check(_lib.load().dg_unigram_sample(table.data_ptr(), table.shape[0], n, seed & (2**64 - 1),
                                         offset & (2**64 - 1), out.data_ptr(), _stream_ptr(stream)),
          "dg_unigram_sample")
    return out


def unigram_sample_slots(table: torch.Tensor, slot0: int, batch: int, n: int, seed: int,
                         out: Optional[torch.Tensor] = None, stream=None, first_slot: int = 0) -> torch.Tensor:
    """n draws, draw i from the alias table of relation slot slot0 + i // batch (table: int32
    [n_slots, range, 2], one per GLOBAL slot; or a shared [range, 2]) — counter slot0·batch + i,
    so the draws do not depend on how slots are dealt to ranks (dg_unigram_sample_slots).
    first_slot: the global slot of table[0] when the table holds only slots [first_slot,
    first_slot + n_slots) (the entry point is given the address slot 0's table would have; it
    reads the slots it draws from only)."""
    _dev(table, torch.int32, "alias table")
    base = table.data_ptr()
    if table.dim() == 3 and table.shape[2] == 2 and table.is_contiguous():
        rng, stride = table.shape[1], table.shape[1]
        if first_slot < 0 or slot0 < first_slot or slot0 - first_slot + -(-n // batch) > table.shape[0]:
            raise ValueError("slot range outside the alias tables")
        base = (base - first_slot * stride * 8) % 2**64
    elif table.dim() == 2 and table.shape[1] == 2:
        rng, stride = table.shape[0], 0
    else:
        raise ValueError("alias tables must be [n_slots, range, 2] (contiguous) or [range, 2]")
    if out is None:
        out = torch.empty(n, device=table.device, dtype=torch.int32)
    _dev(out, torch.int32, "out")
    if out.numel() < n:
        raise ValueError("out too small")
    check(_lib.load().dg_unigram_sample_slots(base, rng, stride, slot0, batch, n, seed & (2**64 - 1),
                                               out.data_ptr(), _stream_ptr(stream)), "dg_unigram_sample_slots")
    return out


def epoch_batch(edges: torch.Tensor, edge_ptr: torch.Tensor, seg_rel: torch.Tensor,
                wrap_mask: Optional[torch.Tensor], batch: int, t: int, epoch: int, seed: int, first_slot: int,
                bad_row: int, rows: Optional[torch.Tensor] = None, cols: Optional[torch.Tensor] = None,
                stream=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Step t's batch of `batch` pairs for every listed relation of one edge type, gathered from
    its device-resident edges in the epoch's shuffled order (dg_epoch_batch_i32): (rows, cols),
    int32 [n_seg·batch] in the segmented kernels' layout, segment s of relation seg_rel[s].

    edges: int32 [n_edges, 2] (row, col), relation-major; edge_ptr: int64 [K + 1]; seg_rel: int32
    [n_seg]; wrap_mask: None or int32 [⌈K/32⌉], bit k set when relation k wraps round (batch
    t mod ⌊n_k/batch⌋) instead of leaving the epoch at t >= ⌊n_k/batch⌋.  Relation k's order is
    epochs.perm under epochs.epoch_key(seed, epoch, first_slot + k).  A segment without a batch
    gets rows `bad_row` (the row table's length) and columns 0.  Asynchronous."""
    for tns, nm, dt in ((edges, "edges", torch.int32), (edge_ptr, "edge_ptr", torch.int64),
                        (seg_rel, "seg_rel", torch.int32), (wrap_mask, "wrap_mask", torch.int32),
                        (rows, "rows", torch.int32), (cols, "cols", torch.int32)):
        if tns is None and nm in ("wrap_mask", "rows", "cols"):
            continue
        if not isinstance(tns, torch.Tensor):
            raise TypeError(f"{nm}: expected a torch.Tensor, got {type(tns).__name__}")
        if tns.dtype != dt:
            raise TypeError(f"{nm}: dtype {tns.dtype}, expected {dt}")
        if not tns.is_contiguous():
            raise ValueError(f"{nm}: must be contiguous")
    if edges.dim() != 2 or edges.shape[1] != 2:
        raise ValueError("epoch_batch: edges must be [n_edges, 2]")
    K = edge_ptr.numel() - 1
    if edge_ptr.dim() != 1 or K < 1:
        raise ValueError("epoch_batch: edge_ptr must have K + 1 >= 2 entries")
    if seg_rel.dim() != 1:
        raise ValueError("epoch_batch: seg_rel must be [n_seg]")
    if wrap_mask is not None and wrap_mask.numel() < -(-K // 32):
        raise ValueError("epoch_batch: wrap_mask must hold one bit per relation")
    for v, nm, hi in ((batch, "batch", 2**31), (t, "t", 2**31), (epoch, "epoch", 2**32),
                      (first_slot, "first_slot", 2**31 - K), (bad_row, "bad_row", 2**31)):
        if int(v) != v or not (1 if nm == "batch" else 0) <= int(v) < hi:
            raise ValueError(f"epoch_batch: {nm} = {v!r} out of range")
    n_seg = seg_rel.numel()
    n = n_seg * int(batch)
    if n > 2**31 - 257:
        raise ValueError("epoch_batch: too many pairs")
    for o, nm in ((rows, "rows"), (cols, "cols")):
        if o is not None and o.numel() != n:
            raise ValueError(f"epoch_batch: {nm} must have n_seg·batch = {n} entries")
    for tns, nm in ((edges, "edges"), (edge_ptr, "edge_ptr"), (seg_rel, "seg_rel"), (wrap_mask, "wrap_mask"),
                    (rows, "rows"), (cols, "cols")):
        if tns is not None and not tns.is_cuda:
            raise ValueError(f"{nm}: must be a device (HIP) tensor")
    if rows is None or cols is None:
        buf = torch.empty((2, n), device=edges.device, dtype=torch.int32)
        rows = buf[0] if rows is None else rows
        cols = buf[1] if cols is None else cols
    ptr = lambda x: x.data_ptr() if x is not None and x.numel() else None  # noqa: E731
    check(_lib.load().dg_epoch_batch_i32(ptr(edges), edges.shape[0], edge_ptr.data_ptr(), K, ptr(seg_rel), n_seg,
                                         ptr(wrap_mask), int(batch), int(t), int(epoch), int(seed) & (2**64 - 1),
                                         int(first_slot), int(bad_row), ptr(rows), ptr(cols), _stream_ptr(stream)),
          "dg_epoch_batch_i32")
    return rows, cols


def slot_score_hinge_bf16(E_row: torch.Tensor, E_col: torch.Tensor, pos_rows: torch.Tensor, pos_cols: torch.Tensor,
                          table: torch.Tensor, slot0: int, n_slots: int, batch: int, seed: int, G: torch.Tensor,
                          D: torch.Tensor, margin: float, out: torch.Tensor, neg_rows: torch.Tensor,
                          loss: torch.Tensor, workspace: torch.Tensor, stream=None) -> None:
    """Config 5's step in one launch (dg_slot_score_hinge_bf16): local slots [0, n_slots) are
    relations slot0 .. slot0 + n_slots − 1; pos_rows / pos_cols hold their n = n_slots·batch
    positives (slot-major).  neg_rows ← each slot's alias draws (unigram_sample_slots' draws),
    out[:n] / out[n:] ← positive / negative scores (decoder_score_bf16(paired=True)), loss ←
    the hinge sum."""
    n = n_slots * batch
    for t, nm in ((E_row, "E_row"), (E_col, "E_col"), (G, "G"), (D, "D")):
        _dev(t, torch.bfloat16, nm)
    for t, nm in ((pos_rows, "pos_rows"), (pos_cols, "pos_cols"), (neg_rows, "neg_rows"), (table, "alias table")):
        _dev(t, torch.int32, nm)
    _dev(out, torch.float32, "out")
    _dev(loss, torch.float32, "loss")
    d = G.shape[0]
    if d != 256 or G.shape != (256, 256) or D.dim() != 2 or D.shape[1] != d or E_row.shape[1] != d \
            or E_col.shape[1] != d:
        raise ValueError("slot scorer: d = 256 tables, G and D rows")
    if table.dim() == 3 and table.shape[2] == 2:
        rng, stride = table.shape[1], table.shape[1]
        if slot0 + n_slots > table.shape[0]:
            raise ValueError("slot range outside the alias tables")
    elif table.dim() == 2 and table.shape[1] == 2:
        rng, stride = table.shape[0], 0
    else:
        raise ValueError("alias tables must be [n_slots, range, 2] or [range, 2]")
    if rng > E_row.shape[0] or slot0 + n_slots > D.shape[0]:
        raise ValueError("sampler range exceeds the row table, or slots exceed D")
    if pos_rows.numel() < n or pos_cols.numel() < n or neg_rows.numel() < n or out.numel() < 2 * n:
        raise ValueError("pairs / outputs shorter than n_slots·batch")
    if workspace.numel() * workspace.element_size() < _lib.DG_HINGE_WS_BYTES or not workspace.is_cuda:
        raise ValueError("hinge workspace too small")
    check(_lib.load().dg_slot_score_hinge_bf16(
        E_row.data_ptr(), E_row.stride(0), E_row.shape[0], E_col.data_ptr(), E_col.stride(0), E_col.shape[0],
        pos_rows.data_ptr(), pos_cols.data_ptr(),
        table.data_ptr(), rng, stride, slot0, n_slots, batch, seed & (2**64 - 1), G.data_ptr(), D.data_ptr(), d,
        float(margin), out.data_ptr(), neg_rows.data_ptr(), loss.data_ptr(), workspace.data_ptr(),
        _stream_ptr(stream)), "dg_slot_score_hinge_bf16")


def upload_alias(degrees, device) -> torch.Tensor:
    """The alias table of one degree vector, int32 [range, 2]; a list of degree vectors (one per
    relation) gives [n, range, 2] (every vector the same length)."""
    from .sampling import alias_table

    if isinstance(degrees, (list, tuple)) or (isinstance(degrees, np.ndarray) and degrees.ndim == 2):
        tabs = np.stack([alias_table(d) for d in degrees])
        return torch.from_numpy(tabs.view(np.int32)).to(device)
    return torch.from_numpy(alias_table(degrees).view(np.int32)).to(device)


# Row producers: plans whose embedding tensors a decoder may ask for row operands
# (ForwardPlan.attach_decoder_rows), found from the tensor a PreparedDecoderHinge is given.
_ROW_PRODUCERS: dict = {}  # data_ptr -> (weakref to the plan, node type)


def register_row_producer(tensor: torch.Tensor, plan, node_type) -> None:
    """`tensor` is plan.embeddings[node_type]: a decoder built on it may attach to the plan."""
    import weakref

    for k in [k for k, (ref, _) in _ROW_PRODUCERS.items() if ref() is None]:
        del _ROW_PRODUCERS[k]
    _ROW_PRODUCERS[tensor.data_ptr()] = (weakref.ref(plan), node_type)


def row_producer(tensor: torch.Tensor):
    """(plan, node type) whose embedding table `tensor` is, or None."""
    hit = _ROW_PRODUCERS.get(tensor.data_ptr())
    if hit is None:
        return None
    plan, node_type = hit[0](), hit[1]
    if plan is None or plan.embeddings.get(node_type) is None:
        return None
    e = plan.embeddings[node_type]
    if e.data_ptr() != tensor.data_ptr() or e.shape != tensor.shape or e.stride() != tensor.stride():
        return None
    return plan, node_type


def _pack_prepared(name: str, **values) -> list:
    """_lib.pack for a prepared call: every argument but the trailing `stream`, which each launch adds."""
    assert _lib.arg_index(name, "stream") == len(values)
    return _lib.pack(name, stream=None, **values)[:-1]


class PreparedDecoderHinge:
    """dg_decoder_hinge_f32 on fixed buffers: sampled (or given) negatives, positive and
    negative scores of n pairs and the hinge loss, in one launch.

    preproject (None: the DG_DEC_PREPROJECT knob, default on): when row_table is the embedding
    table of a ForwardPlan that accepts the attachment (ForwardPlan.attach_decoder_rows: a
    one-GPU forward-only plan in the 32 -> 32 wave-table form) and the batch scores at least as
    many pair sides as the table has rows (2n >= rows), the plan's layer-2 launch also stores
    Q[r] = l ∘ ((E[r] ∘ l)·G) and this decoder scores by dot products
    (dg_decoder_hinge_rows_f32).  Q is valid only once the plan has run since the attachment: a
    call before that launches dg_decoder_hinge_f32 (`entry` names the entry point of the last
    call).  Contract: an attached decoder scores with G and l as they were when the plan last
    ran — they must not change between the plan's run and the decoder's call (in training, Adam
    updates them after the decoder).  release() detaches."""

    def __init__(self, row_table: torch.Tensor, col_table: torch.Tensor, rows: torch.Tensor,
                 cols: torch.Tensor, G: torch.Tensor, l: Optional[torch.Tensor], margin: float,
                 alias: Optional[torch.Tensor] = None, neg_rows: Optional[torch.Tensor] = None,
                 seed: int = 0, offset: int = 0, preproject: Optional[bool] = None):
        for t, nm, dt in ((row_table, "row_table", torch.float32), (col_table, "col_table", torch.float32),
                          (rows, "rows", torch.int32), (cols, "cols", torch.int32), (G, "G", torch.float32)):
            _dev(t, dt, nm)
        d = G.shape[0]
        n = rows.numel()
        if n < 1:
            raise ValueError("empty batch")
        if G.shape != (d, d) or row_table.shape[1] != d or col_table.shape[1] != d or cols.numel() != n:
            raise ValueError("decoder_hinge: shape mismatch")
        if l is not None:
            _dev(l, torch.float32, "l")
        if neg_rows is None:
            if alias is None:
                raise ValueError("need either negatives or a sampler alias table")
            _dev(alias, torch.int32, "alias")
            if alias.shape[0] > row_table.shape[0]:
                raise ValueError("sampler range exceeds the row table")
        else:
            _dev(neg_rows, torch.int32, "neg_rows")
        dev = G.device
        self.pos = torch.empty(n, device=dev)
        self.neg = torch.empty(n, device=dev)
        self.neg_rows = torch.empty(n, device=dev, dtype=torch.int32)
        self.loss = torch.empty(1, device=dev)
        self._ws = torch.zeros(4 + -(-n // 8), device=dev)  # ticket word + partials (either entry point)
        self._keep = (row_table, col_table, rows, cols, G, l, alias, neg_rows)
        self.seed, self.offset = seed, offset
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        shared = dict(col_table=col_table.data_ptr(), ld_col=col_table.shape[1], rows=rows.data_ptr(),
                      cols=cols.data_ptr(), neg_rows=ptr(neg_rows), alias_table=ptr(alias),
                      range=alias.shape[0] if alias is not None else 0, seed=seed, offset=offset, n=n, d=d,
                      margin=float(margin), pos=self.pos.data_ptr(), neg=self.neg.data_ptr(),
                      neg_rows_out=self.neg_rows.data_ptr(), loss=self.loss.data_ptr(),
                      workspace=self._ws.data_ptr())  # what both entry points take
        self._args = _pack_prepared("dg_decoder_hinge_f32", row_table=row_table.data_ptr(),
                                    ld_row=row_table.shape[1], G=G.data_ptr(), l=ptr(l), **shared)
        self._slots = self._call_slots("dg_decoder_hinge_f32")
        self._fn = _lib.load().dg_decoder_hinge_f32
        self.entry = "dg_decoder_hinge_f32"  # the entry point of the last call
        # row operands from the plan that makes row_table
        self._plan = self.Q = None
        if preproject is None:
            preproject = knob("DG_DEC_PREPROJECT", True)
        prod = row_producer(row_table) if preproject else None
        if (prod is not None and d == 32 and 2 * n >= row_table.shape[0] and col_table.data_ptr() % 16 == 0
                and col_table.is_contiguous()):
            plan, node_type = prod
            Q = plan.attach_decoder_rows(node_type, G, l)
            if Q is not None:
                self._plan, self.Q = plan, Q
                self._rows_fn = _lib.load().dg_decoder_hinge_rows_f32
                self._rows_args = _pack_prepared("dg_decoder_hinge_rows_f32", Q=Q.data_ptr(), ld_q=Q.shape[1],
                                                 **shared)
                self._rows_slots = self._call_slots("dg_decoder_hinge_rows_f32")

    @staticmethod
    def _call_slots(name: str) -> Tuple[int, int]:
        """Where the arguments hold what a call sets anew: the seed and the offset."""
        return _lib.arg_index(name, "seed"), _lib.arg_index(name, "offset")

    def _launch(self, fn, args, slots, stream) -> None:
        a = list(args)
        a[slots[0]], a[slots[1]] = self.seed & (2**64 - 1), self.offset & (2**64 - 1)
        check(fn(*a, _stream_ptr(stream)), self.entry)

    @property
    def attached(self) -> bool:
        return self._plan is not None

    def release(self) -> None:
        """Detach from the plan (its layer 2 goes back to the plain launch); later calls score
        with dg_decoder_hinge_f32."""
        if self._plan is not None:
            self._plan.release_decoder_rows(self.Q)
            self._plan = self.Q = None

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass

    def __call__(self, stream=None) -> None:
        # Q holds the rows of the plan's last run only if it ran since the attachment (host-side
        # check; under graph capture it sees the plan.run() captured before this call)
        if self._plan is not None and self._plan.decoder_rows_valid(self.Q):
            self.entry = "dg_decoder_hinge_rows_f32"
            self._launch(self._rows_fn, self._rows_args, self._rows_slots, stream)
            return
        self.entry = "dg_decoder_hinge_f32"
        self._launch(self._fn, self._args, self._slots, stream)


# --------------------------------------------------------------------------------------
# Training step (train.hip): decoder gradient, gather-gradient scatter, l2-norm backward, Adam
# --------------------------------------------------------------------------------------
class PreparedDecoderGrad:
    """dg_decoder_grad_f32 for one batch: row / column gradient rows of the n positive and n
    negative pairs, and the decoder parameter gradients dG = L·dM·L, dl, diag(dG) (each
    written only if its output tensor is given).  loss="xent": dg_decoder_grad_xent_f32, the
    same outputs for the cross-entropy cost with `neg_weight` (margin is then unused)."""

    def __init__(self, row_table, col_table, rows, cols, neg_rows, pos, neg, G, l, margin: float,
                 dG: Optional[torch.Tensor] = None, dl: Optional[torch.Tensor] = None,
                 dG_diag: Optional[torch.Tensor] = None, loss: str = "hinge", neg_weight: float = 1.0):
        param = loss_param(loss, margin, neg_weight)
        for t, nm, dt in ((row_table, "row_table", torch.float32), (col_table, "col_table", torch.float32),
                          (rows, "rows", torch.int32), (cols, "cols", torch.int32),
                          (neg_rows, "neg_rows", torch.int32), (pos, "pos", torch.float32),
                          (neg, "neg", torch.float32), (G, "G", torch.float32)):
            _dev(t, dt, nm)
        d = G.shape[0]
        n = rows.numel()
        if G.shape != (d, d) or row_table.shape[1] != d or col_table.shape[1] != d:
            raise ValueError("decoder_grad: shape mismatch")
        if cols.numel() != n or neg_rows.numel() != n or pos.numel() != n or neg.numel() != n:
            raise ValueError("decoder_grad: batch sizes differ")
        if l is not None:
            _dev(l, torch.float32, "l")
        if dl is not None and l is None:
            raise ValueError("dl needs a diagonal L")
        for t, nm, sz in ((dG, "dG", d * d), (dl, "dl", d), (dG_diag, "dG_diag", d)):
            if t is not None:
                _dev(t, torch.float32, nm)
                if t.numel() != sz:
                    raise ValueError(f"{nm} must have {sz} elements")
        dev = G.device
        self.grad_rows = torch.empty((2 * n, d), device=dev)
        self.grad_cols = torch.empty((n, d), device=dev)
        lib = _lib.load()
        nbytes = int(lib.dg_decoder_grad_workspace(n, d))
        self._ws = torch.empty(max(1, nbytes // 4), device=dev)
        self.row_idx = torch.empty(2 * n, device=dev, dtype=torch.int32)  # positives, then negatives
        self._rows, self._negs = rows, neg_rows
        self._keep = (row_table, col_table, rows, cols, neg_rows, pos, neg, G, l, dG, dl, dG_diag)
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        self._name, cost = (("dg_decoder_grad_f32", {"margin": param}) if loss == "hinge" else
                            ("dg_decoder_grad_xent_f32", {"neg_weight": param}))
        self._args = _pack_prepared(
            self._name, row_table=row_table.data_ptr(), ld_row=row_table.shape[1], col_table=col_table.data_ptr(),
            ld_col=col_table.shape[1], rows=rows.data_ptr(), cols=cols.data_ptr(), neg_rows=neg_rows.data_ptr(), n=n,
            pos=pos.data_ptr(), neg=neg.data_ptr(), G=G.data_ptr(), l=ptr(l), d=d, **cost,
            grad_rows=self.grad_rows.data_ptr(), grad_cols=self.grad_cols.data_ptr(), dG=ptr(dG), dl=ptr(dl),
            dG_diag=ptr(dG_diag), workspace=self._ws.data_ptr(), workspace_bytes=nbytes)
        self._fn = getattr(lib, self._name)

    def __call__(self, stream=None) -> None:
        check(self._fn(*self._args, _stream_ptr(stream)), self._name)
        n = self._rows.numel()  # the scatter's row index list (negatives may be resampled per step)
        self.row_idx[:n].copy_(self._rows)
        self.row_idx[n:].copy_(self._negs)


def scatter_rows(idx: torch.Tensor, src: torch.Tensor, out: torch.Tensor, stream=None) -> None:
    """out[idx[q]] += Σ src[q'] over the occurrences q' of idx[q] (fixed order); indices
    outside out's rows update nothing (checked on the device: no host synchronisation, so
    the call is capturable)."""
    _dev(idx, torch.int32, "idx")
    _dev(src, torch.float32, "src")
    _dev(out, torch.float32, "out")
    n = idx.numel()
    if src.dim() != 2 or src.shape[0] != n or out.dim() != 2 or out.shape[1] != src.shape[1]:
        raise ValueError("scatter_rows: shapes")
    check(_lib.load().dg_scatter_rows_f32(idx.data_ptr(), n, src.data_ptr(), src.shape[1], out.data_ptr(),
                                          out.stride(0), out.shape[0], _stream_ptr(stream)), "dg_scatter_rows_f32")


class PreparedDecoderGradSeg:
    """dg_decoder_grad_seg_f32 for the packed batches of one edge type: per pair p of segment s
    (relation k = seg_rel[s]; None: k = s), `mv[p]` = a_p·M_k·v_p (the gradient of the negative
    row; minus it that of the positive row) and `grad_cols[p]`, and the decoder variables'
    gradients (each written only if its tensor is given): dG [d, d] (G shared: summed over the
    segments) or [K, d, d], dG_diag [K, d], dl [K, d].  The relations of the segments must be
    distinct; outputs of relations without a segment are left untouched.

    G: [d, d] or [K, d, d]; l: None, [d] or [K, d]; seg_ptr device int32 [n_seg + 1], never read
    on the host.

    loss="xent": dg_decoder_grad_seg_xent_f32 for the cross-entropy cost with `neg_weight` (margin is
    then unused).  `mv[p]` = M_k·v_p is then unweighted and `.coef` [2n] holds the weights of the
    two rows it serves: coef[p] = −σ(−pos_p) for the positive row, coef[n + p] = +neg_weight·σ(neg_p)
    for the negative one (segment_rows_sum's `sign`).  With the hinge there is no `.coef`."""

    def __init__(self, row_table, col_table, rows, cols, neg_rows, seg_ptr, seg_rel, pos, neg, G, l,
                 margin: float, dG: Optional[torch.Tensor] = None, dl: Optional[torch.Tensor] = None,
                 dG_diag: Optional[torch.Tensor] = None, loss: str = "hinge", neg_weight: float = 1.0):
        param = loss_param(loss, margin, neg_weight)
        idx = [(rows, "rows"), (cols, "cols"), (neg_rows, "neg_rows"), (seg_ptr, "seg_ptr"), (seg_rel, "seg_rel")]
        outs = [(pos, "pos"), (neg, "neg"), (dG, "dG"), (dl, "dl"), (dG_diag, "dG_diag")]
        ops = RelOperands.build("decoder_grad_seg", row_table, col_table, G, l, WIDTHS_MFMA, idx)
        _check_tensors(outs, torch.float32)
        d, K = ops.d, ops.K
        n = rows.numel()
        if any(t.numel() != n for t in (cols, neg_rows, pos, neg)):
            raise ValueError("decoder_grad_seg: batch sizes differ")
        n_seg = seg_ptr.numel() - 1
        if n_seg < 1:
            raise ValueError("decoder_grad_seg: seg_ptr must have n_seg + 1 >= 2 entries")
        if seg_rel is not None and seg_rel.numel() != n_seg:
            raise ValueError("decoder_grad_seg: seg_rel must have one entry per segment")
        g_per, l_per = G.dim() == 3, l is not None and l.dim() == 2
        if seg_rel is None:
            ops.need_slots("decoder_grad_seg", n_seg, "segments")
        if dl is not None and not l_per:
            raise ValueError("dl needs a per-relation diagonal l [K, d]")
        if dG_diag is not None and not g_per:
            raise ValueError("dG_diag needs a per-relation G [K, d, d]")
        n_out = K if K is not None else n_seg
        for t, nm, sz in ((dG, "dG", (n_out if g_per else 1) * d * d), (dl, "dl", n_out * d),
                          (dG_diag, "dG_diag", n_out * d)):
            if t is not None and t.numel() != sz:
                raise ValueError(f"{nm} must have {sz} elements")
        _need_device(list(ops.tabs) + idx + outs)
        dev = G.device
        self.mv = torch.empty((n, d), device=dev)
        self.grad_cols = torch.empty((n, d), device=dev)
        lib = _lib.load()
        nbytes = int(lib.dg_decoder_grad_seg_workspace(n_seg, d))
        vars_ = dG is not None or dl is not None or dG_diag is not None
        self._ws = torch.empty(max(1, nbytes // 4), device=dev) if vars_ else None
        self._keep = (row_table, col_table, rows, cols, neg_rows, seg_ptr, seg_rel, pos, neg, G, l, dG, dl, dG_diag)
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        self._name, cost = "dg_decoder_grad_seg_f32", {"margin": param}
        if loss == "xent":  # (zeros: pairs outside every segment are not written, and weigh nothing)
            self.coef = torch.zeros(2 * n, device=dev)
            self._name = "dg_decoder_grad_seg_xent_f32"
            cost = {"neg_weight": param, "coef": ptr(self.coef) if n else None}
        G_, g_stride, l_, l_stride = ops.c_args()
        self._args = _pack_prepared(
            self._name, row_table=row_table.data_ptr(), ld_row=d, n_rows=ops.n_rows, col_table=col_table.data_ptr(),
            ld_col=d, n_cols=ops.n_cols, rows=ptr(rows) if n else None, cols=ptr(cols) if n else None,
            neg_rows=ptr(neg_rows) if n else None, seg_ptr=seg_ptr.data_ptr(), seg_rel=ptr(seg_rel), n_seg=n_seg,
            n_pairs=n, pos=ptr(pos) if n else None, neg=ptr(neg) if n else None, **cost, G=G_, g_stride=g_stride,
            l=l_, l_stride=l_stride, n_rel=ops.n_rel(n_seg, seg_rel is not None), d=d,
            mv=ptr(self.mv) if n else None, grad_cols=ptr(self.grad_cols) if n else None, dG=ptr(dG), dl=ptr(dl),
            dG_diag=ptr(dG_diag), workspace=ptr(self._ws), workspace_bytes=nbytes if vars_ else 0)
        self._fn = getattr(lib, self._name)

    def __call__(self, stream=None) -> None:
        check(self._fn(*self._args, _stream_ptr(stream)), self._name)


def segment_rows_chunk() -> Tuple[int, int]:
    """(items per wave chunk, waves per output row) of segment_rows_sum's launch."""
    lib = _lib.load()
    return int(lib.dg_segment_rows_sum_chunk()), int(lib.dg_segment_rows_sum_waves())


def occurrence_list(idx: torch.Tensor, n_out_rows: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """The node-major occurrence list of an index array (device plumbing: one stable sort):
    (node_ptr int32 [n_out_rows + 1], order int32 [n]) with order[node_ptr[r] : node_ptr[r+1]] the
    positions q of idx[q] == r, ascending.  Indices outside [0, n_out_rows) are in no list."""
    # (keys in the narrowest type that holds [-1, n_out_rows]: the radix sort's passes follow its width)
    kt = torch.int16 if n_out_rows < 2**15 - 1 else torch.int32
    key, order = torch.sort(idx.clamp(-1, n_out_rows).to(kt), stable=True)
    bounds = torch.arange(n_out_rows + 1, device=idx.device, dtype=kt)
    node_ptr = torch.searchsorted(key, bounds).to(torch.int32)
    return node_ptr, order.to(torch.int32)


def segment_rows_sum(node_ptr: torch.Tensor, item: torch.Tensor, src: torch.Tensor, out: torch.Tensor,
                     sign: Optional[torch.Tensor] = None, stream=None) -> None:
    """out[r] += Σ_q sign[q]·src[item[q]] for q in [node_ptr[r], node_ptr[r+1]) in q order
    (dg_segment_rows_sum_f32; fixed order: bitwise reproducible).  Items outside src's rows add
    nothing."""
    _dev(node_ptr, torch.int32, "node_ptr")
    _dev(item, torch.int32, "item")
    _dev(src, torch.float32, "src")
    # (out may be a column block of a wider buffer: rows ld_out = out.stride(0) apart)
    if not isinstance(out, torch.Tensor) or not out.is_cuda or out.dtype != torch.float32:
        raise TypeError("out: expected a float32 device tensor")
    if sign is not None:
        _dev(sign, torch.float32, "sign")
        if sign.numel() != item.numel():
            raise ValueError("segment_rows_sum: one sign per item")
    if src.dim() != 2 or out.dim() != 2 or out.shape[1] != src.shape[1]:
        raise ValueError("segment_rows_sum: shapes")
    if out.shape[0] > 1 and (out.stride(1) != 1 or out.stride(0) < out.shape[1]):
        raise ValueError("segment_rows_sum: out's rows must be dense and at least d apart")
    if not 1 <= src.shape[1] <= 256:
        raise ValueError("segment_rows_sum: d must be in [1, 256]")
    if node_ptr.numel() != out.shape[0] + 1:
        raise ValueError("segment_rows_sum: node_ptr must have one entry per output row, plus one")
    check(_lib.load().dg_segment_rows_sum_f32(node_ptr.data_ptr(), item.data_ptr(),
                                              sign.data_ptr() if sign is not None else None, item.numel(),
                                              src.data_ptr(), src.shape[0], src.shape[1], out.data_ptr(),
                                              max(out.stride(0), out.shape[1]), out.shape[0],
                                              _stream_ptr(stream)),
          "dg_segment_rows_sum_f32")


class PreparedL2Grad:
    """dg_l2norm_grad_f32: ds_g = backward of l2_normalize(s_g) at dy (∘ [mask > 0]) for the
    groups (s_g, ds_g) of one node type."""

    def __init__(self, groups: Sequence[Tuple[torch.Tensor, torch.Tensor]], dy: torch.Tensor,
                 mask: Optional[torch.Tensor], n_rows: int, d: int):
        if not 1 <= len(groups) <= _lib.DG_MAX_GROUPS:
            raise ValueError("1..DG_MAX_GROUPS groups")
        for t, nm in [(dy, "dy")] + ([(mask, "mask")] if mask is not None else []):
            _dev(t, torch.float32, nm)
            if t.numel() < n_rows * d:
                raise ValueError(f"{nm} too small")
        arr = (DgL2gGroup * len(groups))()
        for i, (s_, ds) in enumerate(groups):
            _dev(s_, torch.float32, "s")
            _dev(ds, torch.float32, "ds")
            if s_.numel() < n_rows * d or ds.numel() < n_rows * d:
                raise ValueError("l2 grad group too small")
            arr[i].s, arr[i].ds = s_.data_ptr(), ds.data_ptr()
        self._arr, self._n = arr, len(groups)
        self._keep = (list(groups), dy, mask)
        self._args = (dy.data_ptr(), mask.data_ptr() if mask is not None else None, n_rows, d)
        self._fn = _lib.load().dg_l2norm_grad_f32

    def __call__(self, stream=None) -> None:
        check(self._fn(self._arr, self._n, *self._args, _stream_ptr(stream)), "dg_l2norm_grad_f32")


class PreparedAdam:
    """dg_adam_f32 over fixed (param, grad or None, m, v) segments (≤ DG_MAX_ADAM_SEGS per
    launch; more segments → several launches)."""

    def __init__(self, segs: Sequence[Tuple[torch.Tensor, Optional[torch.Tensor], torch.Tensor, torch.Tensor]]):
        self._arrs = []
        for s0 in range(0, len(segs), _lib.DG_MAX_ADAM_SEGS):
            chunk = segs[s0:s0 + _lib.DG_MAX_ADAM_SEGS]
            arr = (DgAdamSeg * len(chunk))()
            for i, (p, g, m, v) in enumerate(chunk):
                for t, nm in ((p, "param"), (m, "m"), (v, "v")) + (((g, "grad"),) if g is not None else ()):
                    _dev(t, torch.float32, nm)
                    if t.numel() != p.numel():
                        raise ValueError(f"adam {nm}: {t.numel()} elements, param has {p.numel()}")
                arr[i].param, arr[i].m, arr[i].v = p.data_ptr(), m.data_ptr(), v.data_ptr()
                arr[i].grad = g.data_ptr() if g is not None else None
                arr[i].n = p.numel()
            self._arrs.append((arr, len(chunk)))
        self._keep = list(segs)
        self._fn = _lib.load().dg_adam_f32

    def __call__(self, alpha: float, beta1: float, beta2: float, eps: float,
                 state: Optional[torch.Tensor] = None, stream=None) -> None:
        """alpha from the argument, or (state given: device float[3] {β1^t, β2^t, alpha}) from
        the device — the graph-capturable form."""
        sp = None
        if state is not None:
            _dev(state, torch.float32, "adam state")
            sp = state.data_ptr()
        for arr, n in self._arrs:
            check(self._fn(arr, n, alpha, beta1, beta2, eps, sp, _stream_ptr(stream)), "dg_adam_f32")


def adam_advance(state: torch.Tensor, lr: float, beta1: float, beta2: float, stream=None) -> None:
    """β1^t, β2^t ← ·β1, ·β2 and the next alpha, on the device (TF's _finish)."""
    _dev(state, torch.float32, "adam state")
    check(_lib.load().dg_adam_advance(state.data_ptr(), lr, beta1, beta2, _stream_ptr(stream)), "dg_adam_advance")


# --------------------------------------------------------------------------------------
# Dropout (dropout.hip)
# --------------------------------------------------------------------------------------
def _drop_state(state: torch.Tensor) -> None:
    if not (isinstance(state, torch.Tensor) and state.is_cuda and state.dtype == torch.int64
            and state.numel() >= 2):
        raise ValueError("dropout state must be an int64 device tensor {seed, step}")


def dropout_rows(inp: torch.Tensor, out: torch.Tensor, state: torch.Tensor, tag: int, keep: float,
                 stream=None) -> None:
    """out[r] = inp[r] · s(r) over the rows of a 2-D view (in place allowed)."""
    _dev(inp, torch.float32, "in")
    _dev(out, torch.float32, "out")
    _drop_state(state)
    d = inp.shape[-1]
    if d < 1:
        raise ValueError("dropout_rows: rows of at least one column")
    n = inp.numel() // d
    if out.numel() != inp.numel():
        raise ValueError("dropout_rows: shapes")
    check(_lib.load().dg_dropout_rows_f32(inp.data_ptr(), out.data_ptr(), n, d, state.data_ptr(), tag, keep,
                                          _stream_ptr(stream)), "dg_dropout_rows_f32")


def dropout_elems(src: torch.Tensor, out: torch.Tensor, state: torch.Tensor, tag: int, keep: float,
                  stream=None) -> None:
    """out[k] = src ∘ M_k / keep for k < out.shape[0] (src [n][d], out [K][n][d])."""
    _dev(src, torch.float32, "src")
    _dev(out, torch.float32, "out")
    _drop_state(state)
    K, n, d = out.shape
    if tuple(src.shape) != (n, d):
        raise ValueError("dropout_elems: shapes")
    check(_lib.load().dg_dropout_elems_f32(src.data_ptr(), out.data_ptr(), K, n, d, state.data_ptr(), tag, keep,
                                           _stream_ptr(stream)), "dg_dropout_elems_f32")


def _map_max(rel_map: torch.Tensor, rel_map_max: Optional[int]) -> int:
    """max(rel_map): host-known (plans pass it, so a captured step never syncs) or read once."""
    if not rel_map.numel():
        return -1
    return int(rel_map.max()) if rel_map_max is None else int(rel_map_max)


def dropout_rows_map(inp: torch.Tensor, out: torch.Tensor, rel_map: torch.Tensor, rows_per_slab: int,
                     state: torch.Tensor, tag: int, keep: float, in_global: bool, out_global: bool,
                     stream=None, rel_map_max: Optional[int] = None) -> None:
    """Row masks of a relation shard: local slab b (rows_per_slab rows) is global relation
    rel_map[b] and takes its mask bits; in / out addressed at global slabs (in_global /
    out_global) or local ones (dg_dropout_rows_map_f32).  The mask bit of a row is its global
    row index, 32-bit: (max(rel_map) + 1)·rows_per_slab must stay below 2^32, as the
    unmapped dg_dropout_rows_f32 requires of its rows."""
    _dev(inp, torch.float32, "in")
    _dev(out, torch.float32, "out")
    _dev(rel_map, torch.int32, "rel_map")
    _drop_state(state)
    d = inp.shape[-1]
    if d < 1:
        raise ValueError("dropout_rows_map: rows of at least one column")
    n_map = rel_map.numel()
    mx = _map_max(rel_map, rel_map_max)
    if (mx + 1) * rows_per_slab >= 0xFFFFFFFF:
        raise ValueError("dropout_rows_map: global row indices exceed the 32-bit mask counter")
    for t, glob in ((inp, in_global), (out, out_global)):
        slabs = t.numel() // (rows_per_slab * d) if rows_per_slab else 0
        need = (mx + 1) if (glob and n_map) else n_map
        if t.shape[-1] != d or slabs < need:
            raise ValueError("dropout_rows_map: operand too small for its slabs")
    check(_lib.load().dg_dropout_rows_map_f32(inp.data_ptr(), out.data_ptr(), rel_map.data_ptr(), n_map,
                                              rows_per_slab, d, (1 if in_global else 0) | (2 if out_global else 0),
                                              state.data_ptr(), tag, keep, _stream_ptr(stream)),
          "dg_dropout_rows_map_f32")


def dropout_elems_map(src: torch.Tensor, out: torch.Tensor, rel_map: torch.Tensor, state: torch.Tensor, tag: int,
                      keep: float, stream=None, rel_map_max: Optional[int] = None) -> None:
    """out[b] = src ∘ M_{rel_map[b]} / keep (src [n][d], out [K_local][n][d]): the per-relation
    tf.nn.dropout masks of a relation shard (dg_dropout_elems_map_f32).  Mask elements are
    rel_map[b]·n·d + r·d + f, 32-bit: (max(rel_map) + 1)·n·d must stay below 2^32, as the
    unmapped dg_dropout_elems_f32 requires of its K·n·d."""
    _dev(src, torch.float32, "src")
    _dev(out, torch.float32, "out")
    _dev(rel_map, torch.int32, "rel_map")
    _drop_state(state)
    K, n, d = out.shape
    if tuple(src.shape) != (n, d) or rel_map.numel() != K:
        raise ValueError("dropout_elems_map: shapes")
    if (_map_max(rel_map, rel_map_max) + 1) * n * d >= 0xFFFFFFFF:
        raise ValueError("dropout_elems_map: mask element indices exceed the 32-bit mask counter")
    check(_lib.load().dg_dropout_elems_map_f32(src.data_ptr(), out.data_ptr(), rel_map.data_ptr(), K, n, d,
                                               state.data_ptr(), tag, keep, _stream_ptr(stream)),
          "dg_dropout_elems_map_f32")


def dropout_advance(state: torch.Tensor, stream=None) -> None:
    _drop_state(state)
    check(_lib.load().dg_dropout_advance(state.data_ptr(), _stream_ptr(stream)), "dg_dropout_advance")

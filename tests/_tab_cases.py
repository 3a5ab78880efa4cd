"""Case generator of the wave-table kernel tests (test_gpu_tab_instances.py on the GPU,
test_cpu_tab_cases.py on the host builder): small launches whose targets, groups and per-row
segment lengths are chosen so that every template instance of gcn_tab_kernel / seg_tab_kernel and
every branch of a wave's gather and of the finishing wave's group logic is taken.  numpy only.

A launch is a list of targets, a target a list of groups (SegSpec's layout: sparse.merge_chunks /
chunk_segments, relations in permuted slabs of an operand with two spare slabs).  The spare slabs
of every operand and weight stack hold NaN: a pair routed to one poisons its row.

Segment lengths come from LENGTHS, dealt in shuffled rounds so that every length occurs in every
launch: the lane-group rounds (4 and 8 pairs handed out at once), the unrolled steps (16 and 32
pairs), S - 1, S, S + 1 of every slot size S, a first overflow batch full, one under and one
over (S + 63 .. S + 65), and three overflow batches (193 pairs at S = 16).  Every target also has
a row whose segments are all empty; the first group of a target, if it has two or more relations,
a relation that is empty throughout (the launch of eight single-relation groups: one group
empty); row 5 of every target the longest segment in every other relation, so that a balanced
table, which deals a row's pairs over all its wave slots, still holds waves of several overflow
batches; and every row count leaves the last workgroup with an absent row slot wherever a
workgroup holds more than one row.

A fused launch takes at most DG_MAX_GROUPS = 8 groups, so the 32-wide geometries, whose
maximum-group target alone has 8, are two launches.
"""
from dataclasses import dataclass, replace
from typing import List, Optional, Sequence, Tuple

import numpy as np

from decagon_amd.sparse import HostCSR, MergedCSR, chunk_segments, merge_chunks

LENGTHS = (0, 1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 79, 80, 81, 127, 128, 129, 193)
N_COLS = 211                       # >= 200: a row's columns stay distinct
SHAPES = ((64, 64), (64, 32), (32, 32))
SLOTS = (0, 16, 32, 48, 64)        # DG_TAB_SLOT: 0 = unset (the cover rule)
U24 = 2.0 ** -24
TINY = 2.0 ** -30                  # val scale of the tiny copy: Σx² under the 1e-12 clamp (with stacks: around it)
TINIER = 2.0 ** -50                # ... and of a second copy: every row under the clamp, weight stacks included
MAX_GROUPS = 8                     # DG_MAX_GROUPS: groups of one fused launch


@dataclass
class Group:
    rels: List[HostCSR]
    slabs: np.ndarray              # int32 [n_rels]: relation k's slab
    n_slabs: int                   # n_rels + 2: two spare slabs
    m: MergedCSR
    seg: np.ndarray
    n_rows: int
    chunk: int
    x: np.ndarray                  # float32: stacked X [n_slabs * N_COLS, d_in], or H [N_COLS, 64] with a stack
    w: Optional[np.ndarray]        # float32 [n_slabs, 64, 32], or None

    @property
    def n_rels(self) -> int:
        return len(self.rels)


@dataclass
class Target:
    n_rows: int
    groups: List[Group]
    relu: bool


class _Lengths:
    """LENGTHS in shuffled rounds: every length once a round."""

    def __init__(self, rng):
        self.rng, self.left = rng, []

    def __call__(self) -> int:
        if not self.left:
            self.left = list(self.rng.permutation(LENGTHS))
        return min(int(self.left.pop()), N_COLS)


def _values(rng, kind: str, what: str, shape):
    if kind == "int":
        pick = {"val": [-3, -2, -1, 1, 2, 3], "x": [-2, -1, 1, 2], "w": [-4, -3, -2, -1, 0, 1, 2, 3, 4]}[what]
        return rng.choice(np.float32(pick), size=shape)
    scale = {"val": 0.1, "x": 1.0, "w": 0.2}[what]
    return (scale * rng.standard_normal(shape)).astype(np.float32)


def make_group(rng, draw, n_rows: int, n_rels: int, chunk: int, d_in: int, stack: bool, kind: str,
               empty_rows: Sequence[int] = (), empty_rel: Optional[int] = None,
               full_rows: Sequence[int] = ()) -> Group:
    rels = []
    for k in range(n_rels):
        lens = [0 if (k == empty_rel or r in empty_rows) else LENGTHS[-1] if r in full_rows else draw()
                for r in range(n_rows)]
        cols = [rng.choice(N_COLS, size=n, replace=False) for n in lens]
        rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        rels.append(HostCSR(rowptr, np.concatenate(cols).astype(np.int32) if sum(lens) else np.zeros(0, np.int32),
                            _values(rng, kind, "val", int(sum(lens))), (n_rows, N_COLS)))
    n_slabs = n_rels + 2
    slabs = rng.permutation(n_slabs)[:n_rels].astype(np.int32)
    m = merge_chunks(rels, slabs, chunk, n_slabs)
    spare = np.setdiff1d(np.arange(n_slabs), slabs)
    if stack:
        x = _values(rng, kind, "x", (N_COLS, 64))
        w = _values(rng, kind, "w", (n_slabs, 64, 32))
        w[spare] = np.nan
    else:
        x = _values(rng, kind, "x", (n_slabs, N_COLS, d_in))
        x[spare] = np.nan
        x, w = x.reshape(n_slabs * N_COLS, d_in), None
    return Group(rels, slabs, n_slabs, m, chunk_segments(rels, m), n_rows, m.chunk, x, w)


def scaled(g: Group, s: float) -> Group:
    """The group with every adjacency value times s (a power of two: sums stay exact)."""
    s = np.float32(s)
    return replace(g, rels=[replace(c, val=c.val * s) for c in g.rels], m=replace(g.m, val=g.m.val * s))


def geometry(stride, d_out: int) -> List[List[Tuple[int, Tuple[int, ...], bool]]]:
    """The launches of a geometry: per launch its targets (rows, relations of each group, relu).
    stride 8 / 16: the four targets of the wave-slot stride (one launch, or two where the groups
    exceed MAX_GROUPS); "one": a single target of one 9-relation group — balanced, the group
    takes all 16 wave slots of its row."""
    gmax = 64 // (d_out // 4)  # lane sets of the finishing wave: groups a target may have
    if stride == "one":
        return [[(9, (9,), True)]]
    if stride == 8:
        tg = [(7, (3, 4), True), (10, (2,), False), (13, (1,), True), (9, (1,) * gmax, False)]
    else:
        tg = [(7, (5, 6), True), (10, (3,), False), (13, (1,), True), (9, (2,) * gmax, False)]
    if sum(len(g) for _, g, _ in tg) > MAX_GROUPS:
        return [tg[:3], tg[3:]]
    return [tg]


def make_launch(spec, d_in: int, d_out: int, kind: str, seed: int) -> List[Target]:
    rng = np.random.default_rng(seed)
    draw = _Lengths(rng)
    out = []
    for t, (n_rows, groups, relu) in enumerate(spec):
        empty_rows = (2 + t % 3,)
        # a relation empty throughout: relation 1 of the first group, or, in a launch that has
        # single-relation groups only, the whole of group 3
        single = len(spec) == 1 and len(groups) > 1 and max(groups) == 1
        gs = [make_group(rng, draw, n_rows, k, k, d_in, d_in != d_out, kind, empty_rows,
                         0 if single and gi == 3 else 1 if k >= 2 and gi == 0 else None, (5,))
              for gi, k in enumerate(groups)]
        out.append(Target(n_rows, gs, relu))
    return out


def make_seg_groups(chunk: int, d_in: int, d_out: int, kind: str, seed: int) -> List[Group]:
    """Two groups of a dg_spmm_seg_tab_f32 launch: 2·chunk relations, and chunk + max(1, chunk/2)
    (a short last chunk once chunk > 1)."""
    rng = np.random.default_rng(seed)
    draw = _Lengths(rng)
    return [make_group(rng, draw, 13, 2 * chunk, chunk, d_in, d_in != d_out, kind, (3,), 1 if chunk > 1 else None),
            make_group(rng, draw, 7, chunk + max(1, chunk // 2), chunk, d_in, d_in != d_out, kind, (0,), 0)]


# ------------------------------------------------------------------------------ float64 references
def dense(c: HostCSR) -> np.ndarray:
    a = np.zeros(c.shape, np.float64)
    rows = np.repeat(np.arange(c.shape[0]), np.diff(c.rowptr))
    assert len(set(zip(rows.tolist(), c.col.tolist()))) == len(rows), "a row's columns are distinct"
    a[rows, c.col] = c.val
    return a


def group_sums(g: Group) -> Tuple[np.ndarray, np.ndarray]:
    """(S, M) [n_chunks, n_rows, d_out] in float64: chunk c's Σ_k Â_k·X[slab_k], or with a stack
    Σ_k (Â_k·H)·W[slab_k], and the same sum over absolute values (a bound on every partial sum,
    in any order)."""
    d_out = 32 if g.w is not None else g.x.shape[1]
    S = np.zeros((g.m.n_chunks, g.n_rows, d_out))
    M = np.zeros_like(S)
    for k, c in enumerate(g.rels):
        a, sl = dense(c), int(g.slabs[k])
        if g.w is None:
            xk = g.x[sl * N_COLS:(sl + 1) * N_COLS].astype(np.float64)
            S[k // g.chunk] += a @ xk
            M[k // g.chunk] += np.abs(a) @ np.abs(xk)
        else:
            h, wk = g.x.astype(np.float64), g.w[sl].astype(np.float64)
            S[k // g.chunk] += (a @ h) @ wk
            M[k // g.chunk] += (np.abs(a) @ np.abs(h)) @ np.abs(wk)
    return S, M


def assert_exact(g: Group, scale: float = 1.0) -> None:
    """The precondition of the exact data sets: every term is an integer multiple of `scale` and
    the absolute terms of a chunk sum stay below 2^24 of it, so fp32 adds them exactly in any order."""
    S, M = group_sums(g)
    assert np.isfinite(S).all() and np.all(S / scale == np.round(S / scale)) and M.max() / scale < 2 ** 24


def l2n(S: np.ndarray) -> np.ndarray:
    """tf.nn.l2_normalize of the rows: x · rsqrt(max(Σx², 1e-12))."""
    return S / np.sqrt(np.maximum((S * S).sum(-1, keepdims=True), 1e-12))


def fused_reference(t: Target) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(ref, A, empty) of a fused target: act(Σ_g l2norm(S_g)) in float64, A = Σ_g |n_g| per
    element (the error bound's scale), and the rows without a pair."""
    ns = [l2n(group_sums(g)[0][0]) for g in t.groups]
    tot = sum(ns)
    empty = np.all([np.diff(c.rowptr) == 0 for g in t.groups for c in g.rels], axis=0)
    return (np.maximum(tot, 0.0) if t.relu else tot), sum(np.abs(n) for n in ns), empty


def least_shift_of_a_dropped_pair(t: Target) -> float:
    """How far the float64 reference of a target moves when one pair is left out, in units of the
    finished row's bound (8 + gc)·2^-24·Σ_g|n_g|: the largest shift over the pair's row, and of
    that the least over all pairs of the target."""
    ref, A, _ = fused_reference(t)
    B = (8 + len(t.groups)) * U24 * A
    S = [group_sums(g)[0][0] for g in t.groups]
    tot = sum(l2n(s) for s in S)
    least = np.inf
    for g, s in zip(t.groups, S):
        for k, c in enumerate(g.rels):
            if not len(c.val):
                continue
            rows, sl = np.repeat(np.arange(g.n_rows), np.diff(c.rowptr)), int(g.slabs[k])
            if g.w is None:
                xr = g.x[sl * N_COLS + c.col].astype(np.float64)
            else:
                xr = g.x[c.col].astype(np.float64) @ g.w[sl].astype(np.float64)
            new = tot[rows] - l2n(s)[rows] + l2n(s[rows] - c.val[:, None].astype(np.float64) * xr)
            shift = np.abs((np.maximum(new, 0.0) if t.relu else new) - ref[rows])
            ratio = np.divide(shift, B[rows], out=np.zeros_like(shift), where=B[rows] > 0)
            least = min(least, float(ratio.max(1).min()))
    return least


# ------------------------------------------------------------------------------ host tables
def seg_data(g: Group, x: int, w: Optional[int], out: Optional[int], d_in: int):
    """The group as the host builder takes it, its buffers at the given (fake or device) addresses."""
    from decagon_amd import wavetable as wt

    return wt.SegData(g.m.rowptr, g.seg, g.m.vcol, g.m.val, g.slabs, x, w if g.w is not None else None, out,
                      d_in, g.n_rows, N_COLS, g.chunk, g.m.n_chunks, g.n_rels)


def expected_geometry(spec, balance: bool) -> Tuple[int, int, List[int]]:
    """(nw, stride, rows per workgroup of each target), restated from the launch rules: a wave per
    relation of the widest row, 8 or 16 wave slots, a workgroup's slots filled with up to 4 rows."""
    widest = max(sum(g) for _, g, _ in spec)
    stride = 8 if widest <= 8 else 16
    nw = stride if balance else widest
    return nw, stride, [min(nw // sum(g), 4) for _, g, _ in spec]

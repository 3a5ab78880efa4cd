"""The small graph of the weighted wave-table tests (test_cpu_tab_weighted.py on the host builder,
test_gpu_tab_weighted.py on the GPU): two targets, groups of 1 and 2 relations on the first and of
6 on the second, built with _tab_cases' generator (relations in permuted slabs of an operand whose
two spare slabs hold NaN).  numpy only.

A group's pairs in a row — what a weighted table sizes the row's wave slots by — run through
TOTALS: 0 and 1, one under, at and one over 16, 32 and 64 (a wave's T, a gather round, a slot),
48, 257 (more than 16 waves of 16) and 400; a relation holds at most 200 pairs a row (its
columns are distinct, of _tab_cases.N_COLS), so the single-relation group stops there.  The groups
of a target take TOTALS at different offsets, so light and heavy groups meet in a row.
"""
from typing import List

import numpy as np

import _tab_cases as tc

TOTALS = (0, 1, 15, 16, 17, 31, 32, 33, 48, 64, 65, 257, 400)
TS = (16, 24, 32, 48)              # pairs a wave; the engine ships 24 at 64 floats, 32 at 32
GROUPS = ((1, 2), (6,))            # relations of each group of the two targets
ROWS = (14, 13)
OFFSETS = ((0, 5), (9,))           # where in TOTALS each group starts


def group_total(t: int, gl: int, r: int) -> int:
    """Pairs of group gl of target t in row r."""
    n_rels = GROUPS[t][gl]
    return min(TOTALS[(OFFSETS[t][gl] + r) % len(TOTALS)], n_rels * 200)


def _split(total: int, n_rels: int) -> List[int]:
    """A row's pairs over the group's relations: uneven, with empty relations where the total is
    small, each at most 211."""
    if n_rels == 1:
        return [total]
    weights = np.arange(1, n_rels + 1, dtype=np.float64)
    lens = np.floor(total * weights / weights.sum()).astype(int)
    lens[-1] += total - lens.sum()
    if lens.max() > 200:  # (400 pairs over two relations)
        lens = np.full(n_rels, total // n_rels)
        lens[: total - lens.sum()] += 1
    assert lens.sum() == total and lens.max() <= tc.N_COLS
    return [int(x) for x in lens]


def make_targets(d_in: int, kind: str, seed: int = 5) -> List[tc.Target]:
    """The two targets with plain sums over a d_in-wide stacked operand (relu on the first)."""
    rng = np.random.default_rng(seed)
    out = []
    for t, (groups, n_rows) in enumerate(zip(GROUPS, ROWS)):
        gs = []
        for gl, n_rels in enumerate(groups):
            # make_group draws relation by relation, row by row
            per_row = [_split(group_total(t, gl, r), n_rels) for r in range(n_rows)]
            queue = [per_row[r][k] for k in range(n_rels) for r in range(n_rows)]
            gs.append(tc.make_group(rng, lambda q=queue: q.pop(0), n_rows, n_rels, n_rels, d_in, False, kind))
            assert not queue
        out.append(tc.Target(n_rows, gs, t == 0))
    return out


def row_pairs(g: tc.Group, r: int) -> np.ndarray:
    """[pairs, 2] int32 of row r of a one-chunk group, in segment order: (vcol, value bits)."""
    assert g.m.n_chunks == 1
    a, b = int(g.m.rowptr[r]), int(g.m.rowptr[r + 1])
    return np.stack([g.m.vcol[a:b].astype(np.int32), g.m.val[a:b].astype(np.float32).view(np.int32)], 1)


def expected_slots(t: int, r: int, T: int) -> int:
    """w_r = clamp(Σ_groups max(1, ⌈pairs / T⌉), groups, 16), restated."""
    raw = sum(max(1, -(-group_total(t, gl, r) // T)) for gl in range(len(GROUPS[t])))
    return min(max(raw, len(GROUPS[t])), 16)


def capped(t: int, r: int, T: int) -> bool:
    return sum(max(1, -(-group_total(t, gl, r) // T)) for gl in range(len(GROUPS[t]))) > 16

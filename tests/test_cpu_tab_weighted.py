"""The weighted wave table (wavetable.fused_table(weighted=T)) on the host: wave slots in
proportion to pairs.  On _tab_weighted_cases' graph, at both row widths and every T of its TS:

1. every pair of every row is in exactly one wave, inside its row's slot range, in segment order
   (read back with wave_pairs), and the waves outside every range are empty;
2. gwaves, first_wave and wr of a row's finishing wave decode to the dealing;
3. no wave holds more than T pairs unless its row is at the 16-slot cap;
4. the rows of a workgroup are consecutive, at most 4 (fewer where the projection jobs need the
   slots), take at most 16 slots, and the next row would not have fitted;
5. the decoder flag and the projection jobs, with their addresses, land on the right waves, and no
   job wave holds more than 2 rows;
6. with the option off the table is today's, array for array.
"""
import functools

import numpy as np
import pytest

import _tab_cases as tc
import _tab_weighted_cases as wc
from decagon_amd import wavetable as wt

WIDTHS = (64, 32)
X0, OUT0, W0, P0, Q0 = 0x10000000, 0x20000000, 0x30000000, 0x7f40000000, 0x7f80000000


@functools.lru_cache(maxsize=None)
def _targets(d):
    return wc.make_targets(d, "int")


def _table_targets(d):
    """fused_table's targets at fake addresses; [(out, n_rows, [SegData], relu)]."""
    out, g = [], 0
    for t, tg in enumerate(_targets(d)):
        specs = []
        for grp in tg.groups:
            specs.append(tc.seg_data(grp, X0 + 0x1000000 * g, None, None, d))
            g += 1
        out.append((OUT0 + 0x1000000 * t, tg.n_rows, specs, tg.relu))
    return out


def _rows_of(tab):
    """Per workgroup b and row slot s: (b, t, r, s, finishing descriptor index)."""
    for b, (t, r0, rows) in enumerate(tab.plan):
        for s in range(rows):
            yield b, t, r0 + s, s, b * tab.stride + s


@pytest.mark.parametrize("T", wc.TS)
@pytest.mark.parametrize("d", WIDTHS)
def test_every_pair_once_in_its_rows_slots(d, T):
    tab = wt.fused_table(_table_targets(d), d, d, balance=True, weighted=T)
    targets = _targets(d)
    assert (tab.nw, tab.stride) == (16, 16) and tab.n_blocks == len(tab.plan)
    assert len(tab.desc) == tab.n_blocks * 16
    used = np.zeros(len(tab.desc), bool)
    gbase = np.cumsum([0] + [len(tg.groups) for tg in targets])
    for b, t, r, s, i in _rows_of(tab):
        dsc = tab.desc[i]
        wr = wt.decode_wr(dsc["wr"])
        gc = len(targets[t].groups)
        # 2: the finishing wave's words
        assert (wr.groups, wr.relu, wr.slot) == (gc, targets[t].relu, s)
        assert int(dsc["orow"]) == OUT0 + 0x1000000 * t + r * d * 4
        counts = wt.decode_gwaves(dsc["gwaves"], gc)
        first = int(dsc["first_wave"])
        w_r = wc.expected_slots(t, r, T)
        assert sum(counts) == w_r, (t, r, counts, w_r)
        r0 = tab.plan[b][1]
        assert first == sum(wc.expected_slots(t, rr, T) for rr in range(r0, r)), (t, r)
        assert first + w_r <= 16
        # 1, 3: each group's waves hold its pairs, in order
        w = first
        for gl, (grp, k) in enumerate(zip(targets[t].groups, counts)):
            want = wc.row_pairs(grp, r)
            assert len(want) == wc.group_total(t, gl, r)
            got = []
            for j in range(b * 16 + w, b * 16 + w + k):
                assert not used[j], "a wave slot dealt twice"
                used[j] = True
                cnt = int(tab.desc["cnt"][j])
                if cnt:
                    assert int(tab.desc["x"][j]) == X0 + 0x1000000 * (int(gbase[t]) + gl)
                    assert int(tab.desc["x_ld"][j]) == d
                    got.append(wt.wave_pairs(tab, j, lp=d // 4))
                assert cnt <= T or wc.capped(t, r, T), (t, r, gl, cnt, T)
                assert cnt <= -(-len(want) // k), "a group's pairs are dealt evenly over its waves"
            got = np.concatenate(got) if got else np.zeros((0, 2), np.int32)
            assert np.array_equal(got, want), (t, r, gl)
            w += k
    assert np.all(tab.desc["cnt"][~used] == 0), "a wave outside every row's slots holds pairs"
    assert int(tab.desc["cnt"].sum()) == sum(grp.m.nnz for tg in targets for grp in tg.groups)
    # the rows at the cap exist at the small T, and some wave there is longer than T
    if T == 16:
        assert any(wc.capped(t, r, T) for t in range(2) for r in range(wc.ROWS[t]))
        assert int(tab.desc["cnt"].max()) > T


@pytest.mark.parametrize("T", wc.TS)
@pytest.mark.parametrize("d", WIDTHS)
def test_rows_packed_in_order_while_their_slots_fit(d, T):
    tab = wt.fused_table(_table_targets(d), d, d, balance=True, weighted=T)
    nxt = [0, 0]
    last = {}
    for b, (t, r0, rows) in enumerate(tab.plan):
        assert r0 == nxt[t] and 1 <= rows <= wt.DG_TAB_MAX_ROW_SLOTS
        assert b == 0 or tab.plan[b - 1][0] <= t, "the targets' workgroups in order"
        slots = sum(wc.expected_slots(t, r, T) for r in range(r0, r0 + rows))
        assert slots <= 16
        nxt[t] = r0 + rows
        if nxt[t] < wc.ROWS[t]:  # greedy: the next row did not fit
            assert rows == wt.DG_TAB_MAX_ROW_SLOTS or slots + wc.expected_slots(t, nxt[t], T) > 16
        last[t] = rows
    assert nxt == list(wc.ROWS)
    assert all(last[t] < wt.DG_TAB_MAX_ROW_SLOTS for t in (0, 1)), "a short last workgroup"


@pytest.mark.parametrize("share", [True, False])
@pytest.mark.parametrize("T", wc.TS[:2])
def test_projection_jobs(T, share):
    """64 -> 64 with the projecting tail: target 0's rows onto 3 + 2 relations of two specs (one
    with a slab map), target 1's onto 7."""
    d = 64
    projs = [wt.ProjData(0, W0, P0, 3, [4, 0, 2]), wt.ProjData(0, W0 + 0x100000, P0 + 0x1000000, 2),
             wt.ProjData(1, W0 + 0x200000, P0 + 0x2000000, 7)]
    n_rels = {0: 5, 1: 7}
    tab = wt.fused_table(_table_targets(d), d, d, balance=True, weighted=T, projs=projs, share_proj=share)
    plain = wt.fused_table(_table_targets(d), d, d, balance=True, weighted=T)
    max_rows = {t: max(rows for tt, _, rows in tab.plan if tt == t) for t in (0, 1)}
    if share:
        assert max_rows[0] > 2 or max_rows[1] > 2, "a workgroup with a second pair of rows"
    else:
        assert max_rows == {0: 3, 1: 2}  # rows × relations <= 16 wave slots
    for b, (t, r0, rows) in enumerate(tab.plan):
        seen = set()
        jobs = 0
        for w in range(16):
            i = b * 16 + w
            role = wt.decode_role(tab.desc["role"][i])
            assert not role.dec and role.seg_waves == 0
            if not role.proj_slots:
                continue
            jobs += 1
            assert 1 <= len(role.proj_slots) <= 2 and all(s < rows for s in role.proj_slots)
            assert share or len(role.proj_slots) == 1
            assert len({s // 2 for s in role.proj_slots}) == 1, "a job's rows are one pair of slots"
            # which (spec, relation): from the W slab's address
            wptr = int(tab.desc["w"][i])
            pj = max((p for p in projs if p.target == t and p.w <= wptr), key=lambda p: p.w)
            sl = (wptr - pj.w) // wt.W_SLAB_BYTES
            slabs = list(range(pj.n_rels)) if pj.slab is None else list(pj.slab)
            assert (wptr - pj.w) % wt.W_SLAB_BYTES == 0 and sl in slabs
            # the P row of row slot 0: slot s's row is 128 bytes · s further
            aux = wt.join_addr(tab.desc["aux_lo"][i], tab.desc["aux_hi"][i])
            assert aux == pj.out + (sl * wc.ROWS[t] + r0) * wt.PROJ_ROW_BYTES
            for s in role.proj_slots:
                assert (s, id(pj), sl) not in seen
                seen.add((s, id(pj), sl))
        assert len(seen) == rows * n_rels[t], "every (row, relation) of the workgroup projected once"
        assert jobs == (-(-rows // 2) if share else rows) * n_rels[t]
        # the jobs fill the waves that finish no row first
        with_job = [w for w in range(16) if wt.decode_role(tab.desc["role"][b * 16 + w]).proj_slots]
        assert set(range(rows, min(16, rows + jobs))) <= set(with_job)
    # the gathers and the finishing words are the table's without jobs, where the plan is the same
    if tab.plan == plain.plan:
        for f in ("x", "cnt", "x_ld", "ovf", "orow", "wr", "gwaves", "first_wave"):
            assert np.array_equal(tab.desc[f], plain.desc[f]), f
        assert np.array_equal(tab.pairs, plain.pairs) and np.array_equal(tab.ovf, plain.ovf)


@pytest.mark.parametrize("T", wc.TS[2:])
@pytest.mark.parametrize("target", [0, 1])
def test_decoder_rows(T, target):
    d = 32
    tab = wt.fused_table(_table_targets(d), d, d, balance=True, weighted=T, dec=wt.DecData(target, Q0))
    plain = wt.fused_table(_table_targets(d), d, d, balance=True, weighted=T)
    flagged = np.zeros(len(tab.desc), bool)
    for b, t, r, s, i in _rows_of(tab):
        if t != target:
            continue
        flagged[i] = True
        assert wt.decode_role(tab.desc["role"][i]).dec
        assert wt.join_addr(tab.desc["aux_lo"][i], tab.desc["aux_hi"][i]) == Q0 + r * wt.PROJ_ROW_BYTES
    assert flagged.sum() == wc.ROWS[target]
    assert not any(wt.decode_role(x).dec for x in tab.desc["role"][~flagged])
    for f in tab.desc.dtype.names:
        if f in ("role", "aux_lo", "aux_hi"):
            assert np.array_equal(tab.desc[f][~flagged], plain.desc[f][~flagged]), f
        else:
            assert np.array_equal(tab.desc[f], plain.desc[f]), f


@pytest.mark.parametrize("balance", [False, True])
@pytest.mark.parametrize("d", WIDTHS)
def test_option_off_is_todays_table(d, balance):
    off = wt.fused_table(_table_targets(d), d, d, balance=balance, weighted=0)
    today = wt.fused_table(_table_targets(d), d, d, balance=balance)
    nw, stride, rpbs = tc.expected_geometry([(n, g, False) for n, g in zip(wc.ROWS, wc.GROUPS)], balance)
    want_plan = [(t, r0, rpbs[t]) for t in (0, 1) for r0 in range(0, wc.ROWS[t], rpbs[t])]
    for tab in (off, today):
        assert (tab.nw, tab.stride, tab.plan) == (nw, stride, want_plan)
    assert off.slot_pairs == today.slot_pairs and off.n_blocks == today.n_blocks
    assert off.desc.tobytes() == today.desc.tobytes()
    assert np.array_equal(off.pairs, today.pairs) and np.array_equal(off.ovf, today.ovf)
    # and in today's balanced table a row's first wave is its equal share of the workgroup
    if balance:
        for b, (t, r0, rpb) in enumerate(off.plan):
            for s in range(min(rpb, wc.ROWS[t] - r0)):
                assert int(off.desc["first_wave"][b * stride + s]) == s * (nw // rpb)


def test_weighted_needs_balanced_plain_sums():
    d = 64
    with pytest.raises(ValueError):
        wt.fused_table(_table_targets(d), d, d, balance=False, weighted=24)
    with pytest.raises(ValueError):
        wt.fused_table(_table_targets(d), d, d, balance=True, weighted=24, peer=True)
    with pytest.raises(ValueError):  # 17 relations: not one row's jobs in 16 wave slots
        wt.fused_table(_table_targets(d), d, d, balance=True, weighted=24, projs=[wt.ProjData(0, W0, P0, 17)])
    assert wt.weighted_proj_fit([5, 7], True) and wt.weighted_proj_fit([16, 0], False)
    assert not wt.weighted_proj_fit([17], True)

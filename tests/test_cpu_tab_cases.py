"""CPU: the host wave tables of every case test_gpu_tab_instances.py launches (tests/_tab_cases.py),
built with fake addresses for every shape, balance setting and slot size and read back wave by
wave: a builder fault shows here before a kernel runs on its table.

* every row's pairs appear exactly once, relation by relation in CSR order, in the waves its
  finishing wave names (`first_wave`, `gwaves`, `wr`), and no other wave gathers anything;
* the geometry the GPU tests rely on holds: the wave-slot stride, waves per workgroup (11 < 16 and
  16), rows per workgroup 1 to 4 with an absent row slot in the last workgroup, 1 / 2 / 4 / 8 groups
  a row, a group of 16 waves (a `gwaves` field of 15);
* waves hold S + 65 pairs and more at every slot size S (balanced, where a row's pairs are dealt
  over all its wave slots: wherever an even dealing leaves such a wave, and 16 + 65 always), and
  every length of LENGTHS occurs.
"""
import numpy as np
import pytest

import _tab_cases as tc

FAKE = 0x100 << 32  # buffer b sits at FAKE + (b << 32)

FUSED = [(shape, stride, balance) for shape in tc.SHAPES for stride in (8, 16, "one") for balance in (False, True)
         if balance or stride != "one"]


def _pairs(g, k, r, stack):
    c = g.rels[k]
    a, b = int(c.rowptr[r]), int(c.rowptr[r + 1])
    vc = c.col[a:b].astype(np.int64) + (0 if stack else int(g.slabs[k]) * tc.N_COLS)
    return np.stack([vc.astype(np.int32), c.val[a:b].view(np.int32)], 1).reshape(-1, 2)


def _fused_table(targets, d_in, d_out, balance, slot):
    from decagon_amd import wavetable as wt

    groups = [g for t in targets for g in t.groups]
    idx = {id(g): i for i, g in enumerate(groups)}
    n = len(groups)
    data = {id(g): tc.seg_data(g, FAKE + (idx[id(g)] << 32), FAKE + ((n + idx[id(g)]) << 32), None, d_in)
            for g in groups}
    tab = wt.fused_table([(FAKE + ((2 * n + t) << 32), tg.n_rows, [data[id(g)] for g in tg.groups], tg.relu)
                          for t, tg in enumerate(targets)], d_in, d_out, balance=balance, slot=slot)
    return tab, idx, n


def _best_longest_wave(targets, rpbs, nw, stack):
    """The longest wave of a balanced table if every row is dealt as evenly as can be: per row the
    least m for which its jobs (groups; with weight stacks, relations), each cut into waves of at
    most m pairs and at least one wave, fit the row's wave slots; the largest such m over the rows."""
    best = 0
    for tg, rpb in zip(targets, rpbs):
        for r in range(tg.n_rows):
            lens = [[int(c.rowptr[r + 1] - c.rowptr[r]) for c in g.rels] for g in tg.groups]
            jobs = [n for g in lens for n in g] if stack else [sum(g) for g in lens]
            m = next(m for m in range(1, max(jobs) + 2) if sum(max(1, -(-n // m)) for n in jobs) <= nw // rpb)
            best = max(best, m if max(jobs) else 0)
    return best


@pytest.mark.parametrize("shape,stride,balance", FUSED)
def test_fused_case_tables_read_back(shape, stride, balance):
    from decagon_amd import wavetable as wt

    d_in, d_out = shape
    stack, lp = d_in != d_out, d_in // 4
    gmax = 64 // (d_out // 4)
    seen_rpb, seen_gc, seen_k, seen_nw = set(), set(), set(), set()
    for li, spec in enumerate(tc.geometry(stride, d_out)):
        targets = tc.make_launch(spec, d_in, d_out, "int", 100 + li)
        nw, want_stride, rpbs = tc.expected_geometry(spec, balance)
        for slot in tc.SLOTS:
            tab, idx, n = _fused_table(targets, d_in, d_out, balance, slot)
            d, S = tab.desc, tab.slot_pairs
            assert (tab.nw, tab.stride) == (nw, want_stride) and (slot == 0 or S == slot) and S in (16, 32, 48, 64)
            assert len(d) == tab.n_blocks * tab.stride == len(tab.plan) * tab.stride
            seen_nw.add(tab.nw)
            rows_done = [set() for _ in targets]
            lengths = set()
            for b, (t, r0, rpb) in enumerate(tab.plan):
                tg = targets[t]
                assert rpb == rpbs[t] and (rpb == 1 or tg.n_rows % rpb), "an absent row slot in the last workgroup"
                seen_rpb.add(rpb)
                i0, used = b * tab.stride, set()
                for sr in range(rpb):
                    r, i = r0 + sr, i0 + sr
                    if r >= tg.n_rows:
                        assert d["orow"][i] == 0
                        continue
                    assert r not in rows_done[t]
                    rows_done[t].add(r)
                    gc = len(tg.groups)
                    assert d["orow"][i] == FAKE + ((2 * n + t) << 32) + r * d_out * 4
                    assert wt.decode_wr(d["wr"][i]) == wt.Wr(gc, tg.relu, sr)
                    counts, w = wt.decode_gwaves(d["gwaves"][i], gc), int(d["first_wave"][i])
                    seen_gc.add(gc)
                    seen_k |= set(counts)
                    for g, cnt in zip(tg.groups, counts):
                        waves = list(range(w, w + cnt))
                        assert not used & set(waves) and waves[-1] < tab.nw
                        used |= set(waves)
                        got = [wt.wave_pairs(tab, i0 + x, lp) for x in waves]
                        want = [_pairs(g, k, r, stack) for k in range(g.n_rels)]
                        assert np.array_equal(np.concatenate(got), np.concatenate(want)), (t, r)
                        if not balance:  # one wave a relation
                            assert cnt == g.n_rels and all(np.array_equal(a, e) for a, e in zip(got, want))
                            lengths |= {len(e) for e in want}
                        for x, p in zip(waves, got):
                            if not len(p):
                                continue
                            assert d["x"][i0 + x] == FAKE + (idx[id(g)] << 32) and d["x_ld"][i0 + x] == d_in
                            if stack:  # the wave's W slab names the one relation its pairs come from
                                w0 = FAKE + ((n + idx[id(g)]) << 32)
                                sl, rem = divmod(int(d["w"][i0 + x]) - w0, wt.W_SLAB_BYTES)
                                k = list(g.slabs).index(sl)
                                assert rem == 0 and (_pairs(g, k, r, True)[:, None] == p[None]).all(2).any(0).all()
                        w += cnt
                for x in range(tab.stride):
                    if x not in used:
                        assert d["cnt"][i0 + x] == 0
            assert all(done == set(range(tg.n_rows)) for done, tg in zip(rows_done, targets))
            # whole relations reach S + 65 at every S; dealt over a row's wave slots, S + 65 wherever
            # the best dealing of some row leaves a wave that long
            assert int(d["cnt"].max()) >= (min(S + 65, _best_longest_wave(targets, rpbs, nw, stack)) if balance
                                           else S + 65)
            assert not balance or int(d["cnt"].max()) >= 16 + 65
            if not balance:
                assert lengths == set(tc.LENGTHS)
    # the geometry the GPU tests are written for
    if stride == "one":
        # (the row without pairs: one wave, or with weight stacks one a relation)
        assert seen_k == {9 if stack else 1, 16} and seen_gc == {1} and seen_nw == {16}
    else:
        assert seen_gc == {1, 2, gmax}
        assert {1, 4} <= seen_rpb <= {1, 2, 3, 4} and (balance or 3 in seen_rpb)
        if stride == 16 and not balance:
            assert 11 in seen_nw and (16 in seen_nw) == (d_out == 32)
        if stride == 8:
            assert max(seen_nw) <= 8


@pytest.mark.parametrize("chunk", [1, 3, 8, 9, 16])
@pytest.mark.parametrize("shape", [(64, 64), (64, 32)])
def test_seg_case_tables_read_back(chunk, shape):
    from decagon_amd import wavetable as wt

    d_in, d_out = shape
    stack = d_in != d_out
    groups = tc.make_seg_groups(chunk, d_in, d_out, "int", 200 + chunk)
    assert groups[0].m.n_chunks == 2 and (chunk == 1 or groups[1].n_rels % chunk), "a short last chunk"
    data = [tc.seg_data(g, FAKE + (i << 32), FAKE + ((2 + i) << 32), FAKE + ((4 + i) << 32), d_in)
            for i, g in enumerate(groups)]
    for slot in tc.SLOTS:
        tab = wt.seg_table(data, d_in, d_out, slot=slot)
        d, S = tab.desc, tab.slot_pairs
        assert (tab.nw, tab.stride) == (chunk, 8 if chunk <= 8 else 16) and (slot == 0 or S == slot)
        done = set()
        for b, blk in enumerate(tab.plan):
            i0 = b * tab.stride
            if blk is None:
                assert not d["cnt"][i0:i0 + tab.stride].any() and not d["orow"][i0:i0 + tab.stride].any()
                continue
            gi, c, r0, rpb = blk
            g = groups[gi]
            for w in range(tab.stride):
                sr, t = divmod(w, chunk)
                r, k = r0 + sr, c * chunk + t
                live = w < tab.nw and sr < rpb and r < g.n_rows
                want = _pairs(g, k, r, stack) if live and k < g.n_rels else np.zeros((0, 2), np.int32)
                assert np.array_equal(wt.wave_pairs(tab, i0 + w), want)
                if live and t == 0:
                    assert (gi, c, r) not in done
                    done.add((gi, c, r))
                    assert d["orow"][i0 + w] == FAKE + ((4 + gi) << 32) + (c * g.n_rows + r) * d_out * 4
                    assert wt.decode_role(d["role"][i0 + w]) == wt.Role((), False, chunk)
                else:
                    assert d["orow"][i0 + w] == 0
                if stack and len(want):
                    assert d["w"][i0 + w] == FAKE + ((2 + gi) << 32) + int(g.slabs[k]) * wt.W_SLAB_BYTES
        assert done == {(gi, c, r) for gi, g in enumerate(groups) for c in range(g.m.n_chunks) for r in range(g.n_rows)}
        assert int(d["cnt"].max()) >= S + 65 and {int(x) for x in d["cnt"]} >= set(tc.LENGTHS)


@pytest.mark.parametrize("shape", tc.SHAPES)
def test_integer_cases_are_exact_in_fp32(shape):
    """The precondition the GPU tests' exact comparisons rest on, the shape of the references, and
    their sensitivity to a single pair."""
    d_in, d_out = shape
    clamped = {tc.TINY: [], tc.TINIER: []}
    for stride in (8, 16, "one"):
        for li, spec in enumerate(tc.geometry(stride, d_out)):
            for t in tc.make_launch(spec, d_in, d_out, "int", 100 + li):
                for g in t.groups:
                    tc.assert_exact(g)
                    for s in clamped:
                        tc.assert_exact(tc.scaled(g, s), s)
                        ss = (tc.group_sums(tc.scaled(g, s))[0][0] ** 2).sum(1)
                        assert np.all(ss[ss > 0] >= 2.0 ** -100)  # far above fp32's subnormals
                        clamped[s] += list(ss[ss > 0] < 1e-12)
                ref, A, empty = tc.fused_reference(t)
                assert ref.shape == A.shape == (t.n_rows, d_out) and empty.any() and not empty.all()
                assert np.all(ref[empty] == 0) and np.isfinite(ref).all()
                # no pair is too light to see: leaving any one out moves its row by over 1000 bounds
                assert tc.least_shift_of_a_dropped_pair(t) > 1000
    assert any(clamped[tc.TINY]) and all(clamped[tc.TINIER])  # the tiny copies run the clamp

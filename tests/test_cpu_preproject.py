"""Host side of layer 1's projection jobs (PreparedFusedTab(projs=...), DG_L2_PREPROJECT): the
pure job assignment wavetable._proj_jobs / tab_proj_fit, and dg_gcn_fused_tab_post_f32's argument
checks, which run on the host before any HIP call.
"""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")


def test_every_row_relation_gets_exactly_one_wave():
    from decagon_amd.wavetable import _proj_jobs

    rng = np.random.default_rng(5)
    fitted = refused = 0
    for _ in range(2000):
        rpb = int(rng.integers(1, 5))
        n_rels = int(rng.integers(0, 9))
        nw = int(rng.integers(1, 17))
        present = [bool(x) for x in rng.integers(0, 2, rpb)]
        want = {(s, k) for s in range(rpb) if present[s] for k in range(n_rels)}
        # one (row, relation) a wave
        jobs = _proj_jobs(present, n_rels, nw)
        if rpb * n_rels > nw:  # refused on the full workgroup, whatever rows are present
            assert jobs is None
            refused += 1
        else:
            fitted += 1
            assert len(jobs) == nw  # one entry per wave slot: no wave can hold two jobs
            got = [j for j in jobs if j is not None]
            assert all(len(slots) == 1 for slots, _ in got)  # ... and a job is one row
            pairs = [(slots[0], k) for slots, k in got]
            assert len(pairs) == len(want) and set(pairs) == want  # each (row, relation) exactly once
            assert all(present[s] for s, _ in pairs)  # an empty row slot projects nothing
            # the waves that finish no row are filled before the finishing waves 0 .. rpb-1
            if len(want) <= nw - rpb:
                assert all(jobs[w] is None for w in range(min(rpb, nw)))
        # one relation a wave, over every present row of the workgroup (the shipped form)
        jobs = _proj_jobs(present, n_rels, nw, share=True)
        if n_rels > nw:
            assert jobs is None
            continue
        assert len(jobs) == nw
        got = [j for j in jobs if j is not None]
        rels = [k for _, k in got]
        assert len(set(rels)) == len(rels)  # no relation (W slab) in two waves
        pairs = [(s, k) for slots, k in got for s in slots]
        assert len(pairs) == len(want) and set(pairs) == want  # each (row, relation) exactly once
        assert all(present[s] for s, _ in pairs)
    assert fitted > 200 and refused > 200


def test_config_S_jobs_fill_the_idle_waves():
    """Config S: drug rows (one row a workgroup) take 7 jobs in waves 1-7, gene rows (two rows a
    workgroup) 2 x 3 in waves 2-7; the last gene workgroup of an odd row count projects one row."""
    from decagon_amd.wavetable import _proj_jobs, _tab_geometry, tab_proj_fit

    for balance in (False, True):
        nw, stride, rpbs = _tab_geometry([3, 7], balance)
        assert (nw, stride, rpbs) == (8 if balance else 7, 8, [2, 1])
        assert tab_proj_fit([3, 7], [3, 7], balance)
        assert tab_proj_fit([3, 7], [3, 7], balance, share=True)
    assert _proj_jobs([True], 7, 8) == [None] + [((0,), k) for k in range(7)]
    assert _proj_jobs([True, True], 3, 8) == [None, None] + [((s,), k) for s in (0, 1) for k in range(3)]
    assert _proj_jobs([True, False], 3, 8) == [None, None, ((0,), 0), ((0,), 1), ((0,), 2), None, None, None]
    assert _proj_jobs([True], 7, 7) == [((0,), 6)] + [((0,), k) for k in range(6)]  # unbalanced: wave 0 takes one
    # shared: a gene workgroup's three relations each project both rows with one W slice
    assert _proj_jobs([True, True], 3, 8, share=True) == [None, None] + [((0, 1), k) for k in range(3)] + [None] * 3
    assert _proj_jobs([True, False], 3, 8, share=True) == [None, None] + [((0,), k) for k in range(3)] + [None] * 3
    assert _proj_jobs([False, False], 3, 8, share=True) == [None] * 8
    assert _proj_jobs([True], 7, 8, share=True) == _proj_jobs([True], 7, 8)


def test_form_refused_when_jobs_do_not_fit():
    from decagon_amd.wavetable import _proj_jobs, tab_proj_fit

    assert _proj_jobs([True, True], 5, 8) is None
    assert _proj_jobs([True, False], 5, 8) is None  # the full workgroup decides, not this one's rows
    assert not tab_proj_fit([3, 7], [5, 7], True)   # two gene rows x 5 relations > 8 waves
    assert not tab_proj_fit([3, 7], [3, 9], True)
    assert tab_proj_fit([3, 7], [4, 8], True)
    assert not tab_proj_fit([3, 7], [3, 8], False)  # seven waves a workgroup without balancing
    assert _proj_jobs([True, True], 9, 8, share=True) is None  # shared: one wave a relation
    assert tab_proj_fit([3, 7], [5, 7], True, share=True) and not tab_proj_fit([3, 7], [5, 9], True, share=True)


def test_post_entry_point_rejects_bad_arguments_like_the_plain_one():
    from decagon_amd import _lib

    lib = _lib.load()
    keep = np.zeros(64, np.uint8)  # (never dereferenced: the checks come first)
    base = keep.ctypes.data

    def table(desc_off=0, nw=8, stride=8, slot=16, blocks=1, pairs=True):
        t = _lib.DgWaveTable()
        t.pairs = (base + 15) // 16 * 16 if pairs else None
        t.ovf = None
        t.desc = 4096 + desc_off
        t.n_blocks, t.nw, t.nw_stride, t.slot_pairs = blocks, nw, stride, slot
        return t

    plain, post = lib.dg_gcn_fused_tab_f32, lib.dg_gcn_fused_tab_post_f32
    assert post(None, 64, 64, None) == plain(None, 64, 64, None) == _lib.DG_EINVAL  # null table
    good = table()
    for d_in, d_out in ((48, 48), (64, 16), (32, 64), (0, 0)):  # no such shape in either
        assert post(ctypes.byref(good), d_in, d_out, None) == plain(ctypes.byref(good), d_in, d_out, None) \
            == _lib.DG_EINVAL
    for d_in, d_out in ((64, 32), (32, 32)):  # the projecting tail follows a 64 -> 64 layer only
        assert post(ctypes.byref(good), d_in, d_out, None) == _lib.DG_EINVAL
    for bad in (table(nw=0), table(nw=17, stride=16), table(stride=16), table(slot=24), table(blocks=-1)):
        assert post(ctypes.byref(bad), 64, 64, None) == plain(ctypes.byref(bad), 64, 64, None) == _lib.DG_EINVAL
    for bad in (table(desc_off=16), table(desc_off=32), table(pairs=False)):  # misaligned / missing arrays
        assert post(ctypes.byref(bad), 64, 64, None) == plain(ctypes.byref(bad), 64, 64, None) == _lib.DG_EALIGN
    empty = table(blocks=0)  # nothing to launch
    assert post(ctypes.byref(empty), 64, 64, None) == plain(ctypes.byref(empty), 64, 64, None) == _lib.DG_OK

"""Host side of the decoder's row operands (DG_DEC_PREPROJECT): the argument checks of
dg_gcn_fused_tab_dec_f32 and dg_decoder_hinge_rows_f32, which run before any HIP call, and the
wave-table flagging wavetable._mark_dec_rows.
"""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")


def _table(_lib, base, desc_off=0, nw=8, stride=8, slot=16, blocks=1):
    t = _lib.DgWaveTable()
    t.pairs = (base + 15) // 16 * 16
    t.ovf = None
    t.desc = 4096 + desc_off
    t.n_blocks, t.nw, t.nw_stride, t.slot_pairs = blocks, nw, stride, slot
    return t


def test_tab_dec_entry_point_rejects_bad_arguments():
    from decagon_amd import _lib

    lib = _lib.load()
    keep = np.zeros(64, np.uint8)  # (never dereferenced: the checks come first)
    dec = lib.dg_gcn_fused_tab_dec_f32
    G, l = 1 << 20, (1 << 20) + 4096
    good = _table(_lib, keep.ctypes.data)
    assert dec(None, 32, 32, G, l, None) == _lib.DG_EINVAL  # null table
    assert dec(ctypes.byref(good), 32, 32, None, l, None) == _lib.DG_EINVAL  # null G
    for d_in, d_out in ((64, 64), (64, 32), (32, 64), (16, 16), (0, 0)):  # the 32 -> 32 layer only
        assert dec(ctypes.byref(good), d_in, d_out, G, l, None) == _lib.DG_EINVAL
    assert dec(ctypes.byref(good), 32, 32, G + 4, l, None) == _lib.DG_EALIGN  # misaligned G
    assert dec(ctypes.byref(good), 32, 32, G, l + 8, None) == _lib.DG_EALIGN  # misaligned l
    for bad in (_table(_lib, keep.ctypes.data, nw=0), _table(_lib, keep.ctypes.data, slot=24),
                _table(_lib, keep.ctypes.data, blocks=-1)):
        assert dec(ctypes.byref(bad), 32, 32, G, l, None) == _lib.DG_EINVAL
    assert dec(ctypes.byref(_table(_lib, keep.ctypes.data, desc_off=16)), 32, 32, G, None, None) == _lib.DG_EALIGN
    empty = _table(_lib, keep.ctypes.data, blocks=0)  # nothing to launch; l may be NULL
    assert dec(ctypes.byref(empty), 32, 32, G, None, None) == _lib.DG_OK


def test_rows_hinge_entry_point_rejects_bad_arguments():
    from decagon_amd import _lib

    fn = _lib.load().dg_decoder_hinge_rows_f32
    p = 1 << 20  # (an aligned address, never dereferenced)

    def call(**kw):
        a = dict(Q=p, ld_q=32, col=p, ld_col=32, rows=p, cols=p, negs=p, alias=None, range=0, seed=0, offset=0,
                 n=4, d=32, margin=0.1, pos=p, neg=p, nro=None, loss=p, ws=p)
        a.update(kw)
        return fn(*a.values(), None)

    for kw in (dict(Q=None), dict(col=None), dict(rows=None), dict(cols=None), dict(pos=None), dict(neg=None),
               dict(loss=None), dict(ws=None)):  # null pointers
        assert call(**kw) == _lib.DG_EINVAL, kw
    assert call(negs=None) == _lib.DG_EINVAL  # neither negatives nor a sampler
    assert call(negs=None, alias=p, range=0) == _lib.DG_EINVAL
    for d in (0, 16, 64, 33):
        assert call(d=d) == _lib.DG_EINVAL
    for n in (0, -1):
        assert call(n=n) == _lib.DG_EINVAL
    assert call(ld_q=16) == _lib.DG_EINVAL and call(ld_col=31) == _lib.DG_EINVAL
    for kw in (dict(Q=p + 4), dict(col=p + 8), dict(ws=p + 4), dict(ld_q=34), dict(ld_col=33)):
        assert call(**kw) == _lib.DG_EALIGN, kw


def test_dec_flag_sits_on_exactly_the_finishing_waves():
    """_mark_dec_rows: the decoder-row role bit and the Q row's address on wave w < rows-per-workgroup of the
    attached target's workgroups, when the target has row first + w — config S's geometry at odd
    row counts (two gene rows a workgroup, one drug row), attached at either node type."""
    from decagon_amd.wavetable import (DESC, DG_TAB_ROLE_DEC_BIT, _mark_dec_rows, _tab_geometry, decode_role,
                                       encode_role, join_addr)

    assert DG_TAB_ROLE_DEC_BIT == 29
    other = encode_role(proj_slots=(1,))
    n_rows = [151, 97]
    nw, stride, rpbs = _tab_geometry([3, 7], True)
    plan = [(t, r0, rpbs[t]) for t in (0, 1) for r0 in range(0, n_rows[t], rpbs[t])]
    q_ptr = (5 << 32) + 0xfff00000  # the low half has its top bit set, the high half is not zero
    for target in (0, 1):
        desc = np.zeros(len(plan) * stride, DESC)
        desc["role"] = other  # (bits of other roles stay)
        desc["gwaves"] = 7
        assert _mark_dec_rows(desc, plan, stride, target, n_rows[target], q_ptr) == n_rows[target]
        seen = []
        for b, (t, r0, rpb) in enumerate(plan):
            for w in range(stride):
                d = desc[b * stride + w]
                flagged = bool((int(d["role"]) >> DG_TAB_ROLE_DEC_BIT) & 1)
                assert decode_role(d["role"]).dec == flagged
                assert flagged == (t == target and w < rpb and r0 + w < n_rows[t]), (b, w)
                assert int(d["role"]) & ~encode_role(dec=True) == other and d["gwaves"] == 7
                if flagged:
                    addr = join_addr(d["aux_lo"], d["aux_hi"])
                    assert addr == (int(np.uint32(d["aux_hi"])) << 32) | int(np.uint32(d["aux_lo"]))
                    assert addr == q_ptr + 128 * (r0 + w) and addr % 16 == 0
                    seen.append(r0 + w)
                else:
                    assert d["aux_lo"] == 0 and d["aux_hi"] == 0
        assert seen == list(range(n_rows[target]))  # every row once

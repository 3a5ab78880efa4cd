"""CPU: the host side of the bf16 decoders (decoder_bf16.hip) — every argument rejection of
dg_decoder_score_bf16, dg_decoder_score_bf16_paired and dg_slot_score_hinge_bf16 that returns
before a launch, so it runs without a device, with the code each one returns (DG_EINVAL for a
bad value, DG_EALIGN for a leading dimension or an address the 16-byte loads cannot take).  The
pointers are fakes: no call below reaches a kernel."""
import pytest

P = 4096  # a non-null, 16-byte aligned fake device pointer (never dereferenced)


@pytest.fixture(scope="module")
def L():
    from decagon_amd import _lib

    return _lib, _lib.load()


def _score(lib, **over):
    """dg_decoder_score_bf16 with arguments that would be valid, except for `over`."""
    a = dict(row_table=P, ld_row=256, col_table=P, ld_col=256, row_idx=P, col_idx=P, rel_idx=P, n_pairs=77, G=P,
             l_table=P, d=256, out=P, stream=None)
    assert set(over) <= set(a), over
    a.update(over)
    return lib.dg_decoder_score_bf16(*a.values())


def _paired(lib, **over):
    a = dict(row_table=P, ld_row=256, n_row_table=40, col_table=P, ld_col=256, n_col_table=30, row_idx=P, col_idx=P,
             rel_idx=P, n_half=45, G=P, l_table=P, d=256, out=P, stream=None)
    assert set(over) <= set(a), over
    a.update(over)
    return lib.dg_decoder_score_bf16_paired(*a.values())


def _fused(lib, **over):
    a = dict(row_table=P, ld_row=256, n_row_table=40, col_table=P, ld_col=256, n_col_table=30, pos_rows=P,
             pos_cols=P, alias_table=P, range=20, alias_stride=20, slot0=0, n_slots=3, batch=32, seed=11, G=P,
             l_table=P, d=256, margin=0.125, out=P, neg_rows=P, loss=P, workspace=P, stream=None)
    assert set(over) <= set(a), over
    a.update(over)
    return lib.dg_slot_score_hinge_bf16(*a.values())


LD512 = dict(ld_row=512, ld_col=512)
MISALIGNED = (2, 4, 8)  # byte offsets from a 16-byte boundary (bf16 elements are 2 bytes)


def test_decoder_score_bf16_rejections(L):
    _lib, lib = L
    EINVAL, EALIGN, OK = _lib.DG_EINVAL, _lib.DG_EALIGN, _lib.DG_OK
    for nm in ("row_table", "col_table", "row_idx", "col_idx", "G", "out"):
        assert _score(lib, **{nm: None}) == EINVAL, nm
        assert _score(lib, n_pairs=0, **{nm: None}) == EINVAL, nm  # an empty batch still names its operands
    for n in (-1, -77, -2**31):
        assert _score(lib, n_pairs=n) == EINVAL, n
    for d in (0, -64, 8, 32, 96, 192, 255, 257, 512):
        assert _score(lib, d=d, ld_row=1024, ld_col=1024) == EINVAL, d
    for d in (64, 128, 256):
        for nm in ("ld_row", "ld_col"):
            assert _score(lib, d=d, **{**LD512, nm: d - 8}) == EALIGN, (d, nm)   # ld < d
            assert _score(lib, d=d, **{**LD512, nm: 0}) == EALIGN, (d, nm)
            for ld in (d + 1, d + 4, d + 12):                                                    # ld % 8 != 0
                assert _score(lib, d=d, **{**LD512, nm: ld}) == EALIGN, (d, nm, ld)
    for off in MISALIGNED:
        for nm in ("row_table", "col_table", "l_table"):
            assert _score(lib, **{nm: P + off}) == EALIGN, (nm, off)
    # a bad value is named before a bad alignment
    assert _score(lib, d=96, ld_row=100, row_table=P + 2) == EINVAL
    assert _score(lib, n_pairs=-1, ld_row=100) == EINVAL
    # no pairs: no launch.  rel_idx and l_table are optional; G is read element by element here,
    # so it needs no 16-byte alignment
    assert _score(lib, n_pairs=0) == OK
    assert _score(lib, n_pairs=0, rel_idx=None, l_table=None) == OK
    for off in MISALIGNED:
        assert _score(lib, n_pairs=0, G=P + off) == OK, off
    # ... but the shape and the tables are checked first
    assert _score(lib, n_pairs=0, d=96) == EINVAL
    assert _score(lib, n_pairs=0, ld_col=250) == EALIGN
    assert _score(lib, n_pairs=0, col_table=P + 8) == EALIGN


def test_decoder_score_bf16_paired_rejections(L):
    _lib, lib = L
    EINVAL, EALIGN, OK = _lib.DG_EINVAL, _lib.DG_EALIGN, _lib.DG_OK
    for nm in ("row_table", "col_table", "row_idx", "col_idx", "G", "out"):
        assert _paired(lib, **{nm: None}) == EINVAL, nm
        assert _paired(lib, n_half=0, **{nm: None}) == EINVAL, nm
    for n in (-1, -45, -2**31):
        assert _paired(lib, n_half=n) == EINVAL, n
    for nm in ("n_row_table", "n_col_table"):
        for n in (0, -1, -2**40):
            assert _paired(lib, **{nm: n}) == EINVAL, (nm, n)
    for d in (0, -64, 8, 32, 96, 192, 255, 257, 512):
        assert _paired(lib, d=d, ld_row=1024, ld_col=1024) == EINVAL, d
    for d in (64, 128, 256):
        for nm in ("ld_row", "ld_col"):
            assert _paired(lib, d=d, **{**LD512, nm: d - 8}) == EALIGN, (d, nm)
            assert _paired(lib, d=d, **{**LD512, nm: 0}) == EALIGN, (d, nm)
            for ld in (d + 1, d + 4, d + 12):
                assert _paired(lib, d=d, **{**LD512, nm: ld}) == EALIGN, (d, nm, ld)
    for off in MISALIGNED:
        for nm in ("row_table", "col_table", "l_table", "G"):  # G's rows are staged into LDS 16 bytes at a time
            for d in (64, 128, 256):
                assert _paired(lib, d=d, **{nm: P + off}) == EALIGN, (nm, off, d)
        # ... on the 64-bit addressed path too (a table past 2^31 bytes)
        assert _paired(lib, n_row_table=4_200_000, G=P + off) == EALIGN, off
        assert _paired(lib, n_col_table=4_200_000, row_table=P + off) == EALIGN, off
    assert _paired(lib, d=96, ld_row=100, row_table=P + 2) == EINVAL
    assert _paired(lib, n_row_table=0, ld_row=100) == EINVAL
    # no pairs: no launch (G's alignment is looked at only when there is one)
    assert _paired(lib, n_half=0) == OK
    assert _paired(lib, n_half=0, rel_idx=None, l_table=None) == OK
    assert _paired(lib, n_half=0, G=P + 8) == OK
    assert _paired(lib, n_half=0, n_row_table=0) == EINVAL
    assert _paired(lib, n_half=0, d=96) == EINVAL
    assert _paired(lib, n_half=0, ld_row=250) == EALIGN
    assert _paired(lib, n_half=0, l_table=P + 8) == EALIGN


def test_slot_score_hinge_bf16_rejections(L):
    _lib, lib = L
    EINVAL, EALIGN = _lib.DG_EINVAL, _lib.DG_EALIGN
    # every pointer is required — the diagonals too (the fused step has no identity form)
    for nm in ("row_table", "col_table", "pos_rows", "pos_cols", "alias_table", "G", "l_table", "out", "neg_rows",
               "loss", "workspace"):
        assert _fused(lib, **{nm: None}) == EINVAL, nm
        assert _fused(lib, n_slots=0, **{nm: None}) == EINVAL, nm
    for n in (-1, -3, -2**31):
        assert _fused(lib, n_slots=n) == EINVAL, n
    for b in (0, -1, -32):
        assert _fused(lib, batch=b) == EINVAL, b
    for r in (0, -1, -20):
        assert _fused(lib, range=r, alias_stride=0) == EINVAL, r
    for s in (-1, -2**31):
        assert _fused(lib, slot0=s) == EINVAL, s
    assert _fused(lib, alias_stride=-1) == EINVAL
    assert _fused(lib, alias_stride=-20) == EINVAL
    # the sampler's range within the row table; a column table with a row
    assert _fused(lib, n_row_table=19) == EINVAL
    assert _fused(lib, n_row_table=0) == EINVAL
    assert _fused(lib, range=41) == EINVAL
    assert _fused(lib, range=2**31 - 1, alias_stride=0) == EINVAL
    assert _fused(lib, n_col_table=0) == EINVAL
    assert _fused(lib, n_col_table=-1) == EINVAL
    # d = 256 only
    for d in (0, -256, 32, 64, 128, 192, 255, 257, 512):
        assert _fused(lib, d=d, ld_row=1024, ld_col=1024) == EINVAL, d
    for nm in ("ld_row", "ld_col"):
        for ld in (248, 0, -256):
            assert _fused(lib, **{nm: ld}) == EALIGN, (nm, ld)
        for ld in (257, 260, 268):
            assert _fused(lib, **{nm: ld}) == EALIGN, (nm, ld)
    for off in MISALIGNED:
        for nm in ("row_table", "col_table", "l_table", "G", "workspace"):
            assert _fused(lib, **{nm: P + off}) == EALIGN, (nm, off)
            assert _fused(lib, batch=37, **{nm: P + off}) == EALIGN, (nm, off)                 # either kernel
            assert _fused(lib, n_row_table=4_200_000, **{nm: P + off}) == EALIGN, (nm, off)
    # pair indices are 32-bit: n_slots·batch <= 2^31 − 1 (seen after the alignments)
    assert _fused(lib, n_slots=2**16, batch=2**15) == EINVAL                # 2^31
    assert _fused(lib, n_slots=2**31 - 1, batch=2) == EINVAL
    assert _fused(lib, n_slots=2**31 - 1, batch=2**31 - 1) == EINVAL
    assert _fused(lib, n_slots=2**16, batch=2**15, workspace=P + 8) == EALIGN
    # a bad value is named before a bad alignment
    assert _fused(lib, d=128, ld_row=100, G=P + 2) == EINVAL
    assert _fused(lib, batch=0, ld_row=100) == EINVAL
    assert _fused(lib, l_table=None, ld_col=100) == EINVAL

"""CPU: the host side of the pair-profile query (dg_decoder_score_cross_f32, dg_row_topk_f32;
additive to ABI 39) — exports and bindings, every argument rejection (they run before any HIP
call, so they work without a device), the slot chunk and the pair chunks the launches use, and the
Python wrappers' validation."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

P = 4096  # a non-null, 16-byte aligned fake device pointer (never dereferenced: every call below is rejected)


def _cross(lib, **over):
    """dg_decoder_score_cross_f32 with arguments that would be valid, except for `over`."""
    a = dict(row_table=P, ld_row=32, n_rows=100, col_table=P, ld_col=32, n_cols=80, row_idx=P, col_idx=P,
             n_pairs=500, G=P, g_stride=0, l=P, l_stride=32, rel_idx=None, n_sel=7, n_rel=7, d=32, out=P,
             ld_out=7, stream=None)
    assert set(over) <= set(a), over
    a.update(over)
    return lib.dg_decoder_score_cross_f32(*a.values())


def _rows(lib, **over):
    """dg_row_topk_f32 with arguments that would be valid, except for `over`."""
    a = dict(x=P, ld=70, n_rows=95, n_cols=70, topk=10, out_val=P, out_idx=P, out_count=P, ws=None, ws_bytes=0,
             stream=None)
    assert set(over) <= set(a), over
    a.update(over)
    return lib.dg_row_topk_f32(*a.values())


def test_symbols_exported_and_bound():
    from decagon_amd import _lib

    lib = _lib.load()
    for s in ("dg_decoder_score_cross_f32", "dg_row_topk_workspace", "dg_row_topk_f32",
              "dg_decoder_score_cross_chunk"):
        assert hasattr(lib, s), s
        assert s in _lib.SIGNATURES, s
    assert len(_lib.SIGNATURES["dg_decoder_score_cross_f32"][1]) == 20
    assert len(_lib.SIGNATURES["dg_row_topk_f32"][1]) == 11
    assert lib.dg_abi_version() == _lib.ABI_VERSION == 39


def test_scorer_rejections_without_a_device():
    from decagon_amd import _lib

    lib = _lib.load()
    EINVAL, EALIGN = _lib.DG_EINVAL, _lib.DG_EALIGN
    for nm in ("row_table", "col_table", "row_idx", "col_idx", "G", "out"):
        assert _cross(lib, **{nm: None}) == EINVAL, nm
    # alignment: the tables 16 bytes, the leading dimensions a multiple of 4
    assert _cross(lib, row_table=P + 4) == EALIGN
    assert _cross(lib, col_table=P + 8) == EALIGN
    assert _cross(lib, ld_row=34) == EALIGN
    assert _cross(lib, ld_col=33) == EALIGN
    assert _cross(lib, G=P + 4, l=P + 4, n_pairs=0) == _lib.DG_OK  # (G and l need none)
    for n_sel in (0, -1):
        assert _cross(lib, n_sel=n_sel) == EINVAL, n_sel
    for n_rel in (0, -3):
        assert _cross(lib, n_rel=n_rel) == EINVAL, n_rel
        assert _cross(lib, n_rel=n_rel, rel_idx=P) == EINVAL, n_rel
    assert _cross(lib, n_pairs=-1) == EINVAL
    assert _cross(lib, n_rows=0) == EINVAL
    assert _cross(lib, n_cols=0) == EINVAL
    for d in (0, -32, 16, 48, 96, 128):
        assert _cross(lib, d=d, ld_row=512, ld_col=512, l_stride=d) == EINVAL, d
    assert _cross(lib, ld_row=28) == EINVAL
    assert _cross(lib, ld_col=16) == EINVAL
    assert _cross(lib, ld_out=6) == EINVAL
    assert _cross(lib, g_stride=32) == EINVAL
    assert _cross(lib, l_stride=16) == EINVAL
    # without a map, per-relation operands bound the slots; a shared operand set does not
    assert _cross(lib, n_sel=8, ld_out=8, n_rel=7) == EINVAL
    assert _cross(lib, n_sel=8, ld_out=8, n_rel=7, g_stride=1024, l=None) == EINVAL
    assert _cross(lib, n_sel=8, ld_out=8, n_rel=7, l_stride=0, n_pairs=0) == _lib.DG_OK
    assert _cross(lib, n_sel=8, ld_out=8, n_rel=7, rel_idx=P, n_pairs=0) == _lib.DG_OK
    # the stated bound on n_pairs·ld_out: 2^38
    assert _cross(lib, n_pairs=2**20, n_sel=7, ld_out=2**18) == EINVAL
    assert _cross(lib, n_pairs=2**31 - 1, n_sel=7, ld_out=256) == EINVAL
    assert _cross(lib, n_pairs=2**31 - 64, n_sel=1, ld_out=1, n_rel=1) == EINVAL  # 32-bit pair offsets
    # nothing to score is not an error (and launches nothing: no device here)
    assert _cross(lib, n_pairs=0, row_idx=None, col_idx=None, out=None) == _lib.DG_OK


def test_row_topk_rejections_without_a_device():
    from decagon_amd import _lib

    lib = _lib.load()
    EINVAL = _lib.DG_EINVAL
    for nm in ("x", "out_val", "out_idx", "out_count"):
        assert _rows(lib, **{nm: None}) == EINVAL, nm
    for topk in (0, -1, _lib.DG_TOPK_MAX_K + 1):
        assert _rows(lib, topk=topk) == EINVAL, topk
    assert _rows(lib, n_cols=0) == EINVAL
    assert _rows(lib, n_rows=-1) == EINVAL
    assert _rows(lib, ld=69) == EINVAL
    assert _rows(lib, n_rows=0, x=None, out_val=None, out_idx=None, out_count=None) == _lib.DG_OK
    # no workspace is needed: the size is 0 for every argument, in range or not
    ws = lib.dg_row_topk_workspace
    assert ws(95, 70, 10) == 0
    assert ws(-1, 70, 10) == 0 and ws(95, 0, 10) == 0 and ws(95, 70, 0) == 0 and ws(95, 70, 2000) == 0


def test_slot_chunk_fills_the_chip_and_stays_a_row_piece():
    from decagon_amd import kernels

    assert kernels.cross_slot_chunk(-1, 5) == 0 and kernels.cross_slot_chunk(5, 0) == 0
    for n_pairs, n_sel in ((1, 1), (32, 1928), (95, 70), (4096, 1928), (207690, 1928), (10**6, 3), (33, 10**5)):
        c = kernels.cross_slot_chunk(n_pairs, n_sel)
        assert c in (4, 8, 16, 32), (n_pairs, n_sel, c)
        waves = -(-n_pairs // 32) * -(-n_sel // c)
        if c > 4:
            assert waves >= 2048, (n_pairs, n_sel, c)  # it was not halved further: the grid is full
        if c < 32:
            assert -(-n_pairs // 32) * -(-n_sel // (2 * c)) < 2048  # … and was halved only while it was not
    assert kernels.cross_slot_chunk(4096, 1928) == 32
    assert kernels.cross_slot_chunk(207690, 1928) == 32
    assert kernels.cross_slot_chunk(32, 1928) == 4


@pytest.mark.parametrize("n_pairs", [0, 1, 31, 32, 33, 95, 4096, 207690])
@pytest.mark.parametrize("n_sel", [1, 70, 1928])
@pytest.mark.parametrize("bound", [0, 1, 70 * 4 * 32, 70 * 4 * 33, 1 << 20, 64 << 20])
def test_pair_chunks_cover_every_pair_once(n_pairs, n_sel, bound):
    from decagon_amd import kernels

    ch = kernels.top_relations_chunks(n_pairs, n_sel, bound)
    pos = 0
    for a, b in ch:  # consecutive, non-empty, exactly once
        assert a == pos and b > a
        pos = b
    assert pos == n_pairs
    if not ch:
        return
    rows = ch[0][1] - ch[0][0] if len(ch) > 1 else None
    for a, b in ch[:-1]:
        assert b - a == rows
    if rows is not None:
        assert rows % 32 == 0 and rows >= 32
        assert ch[-1][1] - ch[-1][0] <= rows
    # the workspace a chunk needs: its pairs rounded up to the 32-row granule
    need = max(-(-(b - a) // 32) * 32 for a, b in ch) * n_sel * 4
    if bound >= 32 * n_sel * 4:
        assert need <= bound, (need, bound)
    else:
        assert need == 32 * n_sel * 4  # the bound does not allow even one granule: exactly one
    with pytest.raises(ValueError):
        kernels.top_relations_chunks(-1, n_sel, bound)
    with pytest.raises(ValueError):
        kernels.top_relations_chunks(n_pairs, 0, bound)


def _ops(d=32, K=5, n=10):
    f = torch.zeros
    return dict(row_table=f(20, d), col_table=f(30, d), row_idx=f(n, dtype=torch.int32),
                col_idx=f(n, dtype=torch.int32), G=f(d, d), l=f(K, d))


def _bad_operands(call):
    """Wrong type, dtype, contiguity, d and shapes of G, l, rel_idx: raised before the device check,
    so CPU tensors serve."""
    a = _ops()
    for nm in a:
        with pytest.raises(TypeError):
            call(**{**a, nm: np.zeros(3)})
    for nm in ("row_table", "col_table", "G", "l"):
        with pytest.raises(TypeError):
            call(**{**a, nm: a[nm].double()})
    for nm in ("row_idx", "col_idx"):
        with pytest.raises(TypeError):
            call(**{**a, nm: a[nm].long()})
    with pytest.raises(TypeError):
        call(**a, rel_idx=torch.zeros(3, dtype=torch.int64))
    with pytest.raises(TypeError):
        call(**a, rel_idx=[0, 1])
    with pytest.raises(ValueError, match="contiguous"):
        call(**{**a, "row_table": torch.zeros(20, 64)[:, :32]})
    with pytest.raises(ValueError, match="contiguous"):
        call(**{**a, "row_idx": torch.zeros(20, dtype=torch.int32)[::2]})
    for d in (16, 48, 96, 128):
        with pytest.raises(ValueError, match="unsupported"):
            call(**_ops(d=d))
    with pytest.raises(ValueError, match="d mismatch"):
        call(**{**a, "col_table": torch.zeros(30, 64)})
    with pytest.raises(ValueError, match="d mismatch"):
        call(**{**a, "G": torch.zeros(32, 64)})
    with pytest.raises(ValueError, match="d mismatch"):
        call(**{**a, "l": torch.zeros(5, 64)})
    with pytest.raises(ValueError):
        call(**{**a, "G": torch.zeros(2, 5, 32, 32)})
    with pytest.raises(ValueError):
        call(**{**a, "l": torch.zeros(1, 5, 32)})
    with pytest.raises(ValueError, match="disagree"):
        call(**{**a, "G": torch.zeros(4, 32, 32)})
    with pytest.raises(ValueError, match="no relations"):
        call(**{**a, "l": torch.zeros(0, 32)})
    with pytest.raises(ValueError, match="empty table"):
        call(**{**a, "row_table": torch.zeros(0, 32)})
    with pytest.raises(ValueError, match="length"):
        call(**{**a, "col_idx": torch.zeros(9, dtype=torch.int32)})
    with pytest.raises(ValueError, match="rel_idx"):
        call(**a, rel_idx=torch.zeros((2, 2), dtype=torch.int32))
    with pytest.raises(ValueError, match="rel_idx"):
        call(**a, rel_idx=torch.zeros(0, dtype=torch.int32))
    with pytest.raises(ValueError, match="rel_idx"):  # nothing per relation: the slots must be named
        call(**{**a, "l": torch.zeros(32)})
    with pytest.raises(ValueError, match="device"):  # all else valid: the device check is the last
        call(**a)


def test_decoder_score_cross_validation():
    from decagon_amd import kernels

    _bad_operands(kernels.decoder_score_cross)
    a = _ops()
    with pytest.raises(TypeError):
        kernels.decoder_score_cross(**a, out=torch.zeros(10, 5, dtype=torch.float64))
    with pytest.raises(TypeError):
        kernels.decoder_score_cross(**a, out=np.zeros((10, 5), np.float32))
    for bad in (torch.zeros(10, 4), torch.zeros(9, 5), torch.zeros(50), torch.zeros(5, 10).t(),
                torch.zeros(10, 10)[:, ::2]):
        with pytest.raises(ValueError, match="out"):
            kernels.decoder_score_cross(**a, out=bad)
    with pytest.raises(ValueError, match="out"):  # three slots named: two columns do not hold them
        kernels.decoder_score_cross(**a, rel_idx=torch.zeros(3, dtype=torch.int32), out=torch.zeros(10, 2))
    with pytest.raises(ValueError, match="device"):  # a row-strided view is accepted: on to the device check
        kernels.decoder_score_cross(**a, out=torch.zeros(10, 10)[:, :5])


def test_decoder_top_relations_validation():
    from decagon_amd import kernels

    _bad_operands(lambda **kw: kernels.decoder_top_relations(topk=3, **kw))
    for topk in (0, -1, 1025):
        with pytest.raises(ValueError, match="topk"):
            kernels.decoder_top_relations(**_ops(), topk=topk)


def test_row_topk_validation():
    from decagon_amd import kernels

    with pytest.raises(TypeError):
        kernels.row_topk(np.zeros((3, 4), np.float32), 2)
    with pytest.raises(TypeError):
        kernels.row_topk(torch.zeros(3, 4, dtype=torch.float64), 2)
    for bad in (torch.zeros(12), torch.zeros(3, 0), torch.zeros(4, 3).t(), torch.zeros(3, 8)[:, ::2]):
        with pytest.raises(ValueError, match="row_topk"):
            kernels.row_topk(bad, 2)
    for topk in (0, -1, 1025):
        with pytest.raises(ValueError, match="topk"):
            kernels.row_topk(torch.zeros(3, 4), topk)
    with pytest.raises(ValueError, match="device"):  # a row-strided view is accepted
        kernels.row_topk(torch.zeros(3, 8)[:, :4], 2)

"""CPU: the host side of the filtered edge rank (dg_decoder_edge_rank_f32, declared in
include/decagon_hip_ext.h; additive to ABI 39) — the extension header's parse, export and binding,
every argument rejection (they run before any HIP call, so they work without a device),
sparse.ExclusionCSR.transposed, evaluate.ranking_metrics and the Python wrappers' validation."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
sp = pytest.importorskip("scipy.sparse")

P = 4096  # a non-null, 16-byte aligned fake device pointer (never dereferenced: every call below is rejected)
NAME = "dg_decoder_edge_rank_f32"


def _call(lib, **over):
    """dg_decoder_edge_rank_f32 with arguments that would be valid, except for `over`."""
    from decagon_amd import _lib

    a = dict(row_table=P, ld_row=32, n_rows=100, col_table=P, ld_col=32, n_cols=80, row_idx=P, col_idx=P,
             seg_ptr=P, seg_rel=None, n_seg=3, n_queries=500, G=P, g_stride=0, l=P, l_stride=32, n_rel=3, d=32,
             excl_rowptr=P, excl_col=P, flags=0, out_rank=P, out_score=P, out_cand=P, stream=None)
    assert set(over) <= set(a), over
    a.update(over)
    return getattr(lib, NAME)(*_lib.pack(NAME, **a))


def test_extension_header_parses_into_its_own_table():
    from decagon_amd import _lib, abi

    assert list(abi.EXT.prototypes) == [NAME] and not abi.EXT.structs
    assert abi.EXT.constants == {"DG_EDGE_RANK_NO_SELF": 1, "DG_EDGE_RANK_NO_SPLIT": 2}
    assert NAME not in abi.PROTOTYPES and "DG_EDGE_RANK_NO_SELF" not in abi.CONSTANTS
    assert len(abi.PROTOTYPES) == 78 and len(abi.ABI.structs) == 15
    p = abi.EXT.prototypes[NAME]
    assert p.restype is ctypes.c_int32 and len(p.argtypes) == len(p.names) == 25
    assert p.names[:3] == ("row_table", "ld_row", "n_rows") and p.names[-4:] == ("out_rank", "out_score", "out_cand",
                                                                                  "stream")
    by_name = dict(zip(p.names, p.argtypes))
    assert by_name["ld_row"] is by_name["g_stride"] is ctypes.c_int64
    assert by_name["n_queries"] is by_name["flags"] is ctypes.c_int32
    assert all(by_name[n] is ctypes.c_void_p for n in ("row_table", "seg_ptr", "excl_col", "out_score", "stream"))
    assert _lib.DG_EDGE_RANK_NO_SELF == 1 and _lib.arg_index(NAME, "flags") == 20
    # the first header's names are in scope of the second parse, and only there
    text = "#ifndef DECAGON_HIP_EXT_H\n#define DECAGON_HIP_EXT_H\n#define DG_X (DG_MAX_GROUPS + 1)\n" \
           "int dg_f(const dg_rel_group* g /* HOST */);\n#endif\n"
    got = abi.parse(text, "x.h", base=abi.ABI)
    assert got.constants == {"DG_X": 9} and not got.structs
    assert got.prototypes["dg_f"].argtypes == [ctypes.POINTER(abi.ABI.structs["dg_rel_group"])]
    with pytest.raises(abi.AbiError, match="DG_MAX_GROUPS"):
        abi.parse(text, "x.h")
    with pytest.raises(abi.AbiError, match="x.h:1: unsupported directive"):
        abi.parse("#define SOMETHING_ELSE_H\n", "x.h")


def test_symbol_exported_bound_and_typed():
    from decagon_amd import _lib, abi

    lib = _lib.load()
    assert hasattr(lib, NAME) and NAME in _lib.SIGNATURES
    p = abi.EXT.prototypes[NAME]
    fn = getattr(lib, NAME)
    assert fn.restype is p.restype and list(fn.argtypes) == p.argtypes
    assert _lib.SIGNATURES[NAME] == (p.restype, p.argtypes)
    assert all(s in _lib.SIGNATURES for s in abi.PROTOTYPES)
    assert lib.dg_abi_version() == _lib.ABI_VERSION == 39


def test_rejections_without_a_device():
    from decagon_amd import _lib

    lib = _lib.load()
    EINVAL, EALIGN = _lib.DG_EINVAL, _lib.DG_EALIGN
    for nm in ("row_table", "col_table", "row_idx", "col_idx", "seg_ptr", "G", "out_rank"):
        assert _call(lib, **{nm: None}) == EINVAL, nm
    assert _call(lib, excl_rowptr=None) == EINVAL and _call(lib, excl_col=None) == EINVAL  # one alone
    for n_seg in (0, -1):
        assert _call(lib, n_seg=n_seg) == EINVAL, n_seg
    assert _call(lib, n_queries=-1) == EINVAL
    for d in (0, -32, 16, 48, 96, 128):
        assert _call(lib, d=d, ld_row=512, ld_col=512, l_stride=d) == EINVAL, d
    assert _call(lib, ld_row=28) == EINVAL and _call(lib, ld_col=31) == EINVAL
    assert _call(lib, n_rows=0) == EINVAL and _call(lib, n_cols=0) == EINVAL
    # strides: 0 or d·d for G, 0 or d for l
    for over in (dict(g_stride=32), dict(g_stride=-1024), dict(l_stride=16), dict(l_stride=1024)):
        assert _call(lib, **over) == EINVAL, over
    # a relation map needs a relation count; without a map per-relation operands and the exclusion bound n_seg
    assert _call(lib, seg_rel=P, n_rel=0) == EINVAL and _call(lib, seg_rel=P, n_rel=-3) == EINVAL
    assert _call(lib, n_seg=4, n_rel=3) == EINVAL
    assert _call(lib, n_seg=4, n_rel=3, g_stride=1024, l=None) == EINVAL
    assert _call(lib, n_seg=4, n_rel=3, l_stride=0) == EINVAL  # (the exclusion is per relation)
    # flags
    assert _call(lib, flags=4) == EINVAL and _call(lib, flags=-1) == EINVAL
    assert _call(lib, flags=_lib.DG_EDGE_RANK_NO_SELF) == EINVAL  # 100 x 80 tables
    # 32-bit query offsets
    assert _call(lib, n_queries=2**31 - 1, n_seg=1) == EINVAL
    assert _call(lib, n_queries=2**31 - 96, n_seg=3) == EINVAL
    assert _call(lib, n_queries=0, n_seg=2**26, l_stride=0, seg_rel=P) == EINVAL
    # alignment: 16-byte tables, ld % 4 == 0
    assert _call(lib, row_table=P + 4) == EALIGN and _call(lib, col_table=P + 8) == EALIGN
    assert _call(lib, ld_row=34) == EALIGN and _call(lib, ld_col=33) == EALIGN
    # nothing to rank is not an error (and launches nothing: no device here)
    nothing = dict(n_queries=0, row_idx=None, col_idx=None, out_rank=None, out_score=None, out_cand=None)
    assert _call(lib, **nothing) == _lib.DG_OK
    assert _call(lib, excl_rowptr=None, excl_col=None, n_seg=4, l_stride=0, **nothing) == _lib.DG_OK
    assert _call(lib, n_rows=80, flags=_lib.DG_EDGE_RANK_NO_SELF | _lib.DG_EDGE_RANK_NO_SPLIT, **nothing) == _lib.DG_OK


def test_exclusion_transposed_matches_scipy():
    from decagon_amd.sparse import exclusion_csr

    rng = np.random.default_rng(5)
    n_r, n_c = 37, 23
    dense = [rng.random((n_r, n_c)) < 0.15, np.ones((n_r, n_c), bool), np.zeros((n_r, n_c), bool),
             rng.random((n_r, n_c)) < 0.5]
    dense[0][[0, 5, 36]] = False   # empty rows
    dense[0][:, [0, 22]] = False   # empty columns: empty rows of the transpose
    ex = exclusion_csr([sp.csr_matrix(m.astype(np.float32)) for m in dense], (n_r, n_c))
    t = ex.transposed()
    assert (t.n_rows, t.n_cols, t.n_rels, t.nnz) == (n_c, n_r, 4, ex.nnz)
    assert t.rowptr.dtype == t.col.dtype == np.int32 and t.rowptr.shape == (4 * n_c + 1,)
    for k, m in enumerate(dense):
        want = sp.csr_matrix(m.T.astype(np.float32))
        want.sort_indices()
        lo = t.rowptr[k * n_c]
        assert np.array_equal(t.rowptr[k * n_c:(k + 1) * n_c + 1] - lo, want.indptr), k
        assert np.array_equal(t.col[lo:t.rowptr[(k + 1) * n_c]], want.indices), k
    back = t.transposed()
    assert np.array_equal(back.rowptr, ex.rowptr) and np.array_equal(back.col, ex.col)
    assert (back.n_rows, back.n_cols, back.n_rels) == (n_r, n_c, 4)
    none = exclusion_csr([None, None], (4, 6)).transposed()
    assert none.nnz == 0 and none.rowptr.tolist() == [0] * 13 and (none.n_rows, none.n_cols) == (6, 4)


def test_ranking_metrics_on_hand_written_ranks():
    from decagon_amd.evaluate import ranking_metrics

    rank = np.array([1, 2, 4, 1, 10, 11, 3], np.int32)
    got = ranking_metrics(rank, [0, 3, 3, 7])
    assert got.dtype == np.float64 and got.shape == (3, 5)
    assert np.array_equal(got[0], [(1 + 1 / 2 + 1 / 4) / 3, 7 / 3, 1 / 3, 2 / 3, 1.0])
    assert np.all(np.isnan(got[1]))  # an empty segment
    assert np.array_equal(got[2], [(1 + 1 / 10 + 1 / 11 + 1 / 3) / 4, 25 / 4, 1 / 4, 2 / 4, 3 / 4])
    one = ranking_metrics(rank, [0, 7], hits=(2, 11))
    assert one.shape == (1, 4) and np.array_equal(one[0, 1:], [32 / 7, 3 / 7, 1.0])
    assert ranking_metrics(np.zeros(0, np.int32), [0, 0]).shape == (1, 5)
    with pytest.raises(ValueError, match="seg_ptr"):
        ranking_metrics(rank, [0, 9])
    with pytest.raises(ValueError, match="seg_ptr"):
        ranking_metrics(rank, [0, 4, 2])
    with pytest.raises(ValueError, match="start at 1"):
        ranking_metrics(np.array([1, 0, 3]), [0, 3])


def test_wrappers_validate_before_touching_the_library(monkeypatch):
    from decagon_amd import _lib, evaluate, kernels
    from decagon_amd.sparse import exclusion_csr

    def no_library(*a, **k):
        raise AssertionError("the library was loaded before the arguments were checked")

    monkeypatch.setattr(_lib, "load", no_library)
    E = torch.zeros(10, 32)
    G = torch.zeros(32, 32)
    l = torch.zeros(3, 32)
    idx = torch.zeros(8, dtype=torch.int32)
    ptr = torch.tensor([0, 3, 3, 8], dtype=torch.int32)
    f = kernels.decoder_edge_rank
    with pytest.raises(TypeError, match="dtype"):
        f(E.double(), E, idx, idx, ptr, G, l)
    with pytest.raises(TypeError, match="dtype"):
        f(E, E, idx.long(), idx, ptr, G, l)
    with pytest.raises(TypeError, match="dtype"):
        f(E, E, idx, idx, ptr, G, l, seg_rel=torch.zeros(3))
    with pytest.raises(TypeError, match="torch.Tensor"):
        f(E, E, idx, idx, ptr.numpy(), G, l)
    with pytest.raises(ValueError, match="contiguous"):
        f(torch.zeros(10, 64)[:, ::2], E, idx, idx, ptr, G, l)
    with pytest.raises(ValueError, match="d mismatch"):
        f(torch.zeros(10, 64), E, idx, idx, ptr, G, l)
    with pytest.raises(ValueError, match="unsupported"):  # the register-resident tiles: 32 or 64
        f(torch.zeros(10, 96), torch.zeros(10, 96), idx, idx, ptr, torch.zeros(96, 96), None)
    with pytest.raises(ValueError, match="length mismatch"):
        f(E, E, idx, idx[:5], ptr, G, l)
    with pytest.raises(ValueError, match="seg_ptr"):
        f(E, E, idx, idx, ptr[:1], G, l)
    with pytest.raises(ValueError, match="seg_rel"):
        f(E, E, idx, idx, ptr, G, l, seg_rel=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError, match="disagree"):
        f(E, E, idx, idx, ptr, torch.zeros(2, 32, 32), l)
    with pytest.raises(ValueError, match="pass seg_rel"):
        f(E, E, idx, idx, ptr, G, l[:2])
    with pytest.raises(ValueError, match="square"):
        f(E, torch.zeros(9, 32), idx, idx, ptr, G, l, no_self=True)
    with pytest.raises(ValueError, match="exclusion shape"):
        f(E, E, idx, idx, ptr, G, l, exclude=exclusion_csr([None] * 3, (10, 9)))
    with pytest.raises(ValueError, match="disagree"):
        f(E, E, idx, idx, ptr, G, l, exclude=exclusion_csr([None] * 4, (10, 10)))
    with pytest.raises(ValueError, match="pass seg_rel"):  # the exclusion's relations bound the segments too
        f(E, E, idx, idx, ptr, G, None, exclude=exclusion_csr([None] * 2, (10, 10)))
    with pytest.raises(ValueError, match="rowptr"):
        f(E, E, idx, idx, ptr, G, l, exclude=(torch.zeros(32, dtype=torch.int32), idx))
    # everything else right, but host tensors: the device check
    with pytest.raises(ValueError, match="device"):
        f(E, E, idx, idx, ptr, G, l, exclude=exclusion_csr([None] * 3, (10, 10)))

    with pytest.raises(ValueError, match="side"):
        evaluate.edge_ranks(None, None, {}, {}, {}, (0, 0), side="column")
    with pytest.raises(ValueError, match="side"):
        evaluate.ranking_scores_all(None, None, {}, {}, {}, (0, 0), side="all")

"""CPU: the host side of the top-k candidate ranking (dg_decoder_topk_f32, ABI 39) — exports and
bindings, every argument rejection (they run before any HIP call, so they work without a device),
the workspace bound, sparse.exclusion_csr and kernels.decoder_topk's own validation."""
import numpy as np
import pytest
import scipy.sparse as sp

torch = pytest.importorskip("torch")

P = 4096  # a non-null, 16-byte aligned fake device pointer (never dereferenced: every call below is rejected)


def _call(lib, **over):
    """dg_decoder_topk_f32 with arguments that would be valid, except for `over`."""
    a = dict(row_table=P, ld_row=32, n_rows=100, col_table=P, ld_col=32, n_cols=80, G=P, g_stride=0, l=P,
             l_stride=32, n_rel=3, d=32, topk=16, ex_rowptr=None, ex_col=None, flags=0, out_score=P, out_row=P,
             out_col=P, out_count=P, ws=P, ws_bytes=1 << 62, stream=None)
    assert set(over) <= set(a), over
    a.update(over)
    return lib.dg_decoder_topk_f32(*a.values())


def test_symbols_exported_and_bound():
    from decagon_amd import _lib

    lib = _lib.load()
    for s in ("dg_decoder_topk_workspace", "dg_decoder_topk_f32"):
        assert hasattr(lib, s), s
        assert s in _lib.SIGNATURES, s
    assert len(_lib.SIGNATURES["dg_decoder_topk_f32"][1]) == 23
    assert lib.dg_abi_version() == _lib.ABI_VERSION == 39
    assert _lib.DG_TOPK_MAX_K >= 1024


def test_rejections_without_a_device():
    from decagon_amd import _lib

    lib = _lib.load()
    EINVAL, EALIGN = _lib.DG_EINVAL, _lib.DG_EALIGN
    # null tables / operands / outputs
    for nm in ("row_table", "col_table", "G", "out_score", "out_row", "out_col", "out_count", "ws"):
        assert _call(lib, **{nm: None}) == EINVAL, nm
    # topk outside [1, DG_TOPK_MAX_K]
    for k in (0, -1, _lib.DG_TOPK_MAX_K + 1):
        assert _call(lib, topk=k) == EINVAL, k
    # unsupported d
    for d in (0, 16, 48, 128):
        assert _call(lib, d=d, ld_row=128, ld_col=128) == EINVAL, d
    # sizes: empty, leading dimension below d, a linear index that does not fit 32 bits
    assert _call(lib, n_rel=0) == EINVAL
    assert _call(lib, n_rows=0) == EINVAL
    assert _call(lib, n_cols=0) == EINVAL
    assert _call(lib, ld_row=28) == EINVAL
    assert _call(lib, n_rows=65536, n_cols=65536) == EINVAL
    assert _call(lib, n_rows=1 << 20, n_cols=1 << 12) == EINVAL
    # strides
    assert _call(lib, g_stride=32) == EINVAL
    assert _call(lib, l_stride=16) == EINVAL
    # workspace too small
    need = lib.dg_decoder_topk_workspace(3, 100, 80, 16)
    assert need > 0
    assert _call(lib, ws_bytes=need - 1) == EINVAL
    assert _call(lib, ws_bytes=0) == EINVAL
    # flags: unknown bit; UPPER on tables of different row counts; one exclusion array alone
    assert _call(lib, flags=4) == EINVAL
    assert _call(lib, flags=_lib.DG_TOPK_UPPER) == EINVAL
    assert _call(lib, flags=_lib.DG_TOPK_UPPER | _lib.DG_TOPK_NO_DIAG, n_rows=100, n_cols=101) == EINVAL
    assert _call(lib, ex_rowptr=P) == EINVAL
    assert _call(lib, ex_col=P) == EINVAL
    # rows not 16-byte aligned
    assert _call(lib, row_table=P + 4) == EALIGN
    assert _call(lib, col_table=P + 8) == EALIGN
    assert _call(lib, ld_row=34) == EALIGN
    assert _call(lib, ld_col=33) == EALIGN
    assert _call(lib, ws=P + 8) == EALIGN


def test_workspace_does_not_hide_a_full_matrix():
    from decagon_amd import _lib

    lib = _lib.load()
    ws = lib.dg_decoder_topk_workspace(8, 4096, 4096, 64)
    assert 0 < ws < 8 * 4096 * 4096 * 4 // 16
    # it does not depend on the column count at all, and out-of-range arguments give 0
    assert lib.dg_decoder_topk_workspace(8, 4096, 8, 64) == ws
    assert lib.dg_decoder_topk_workspace(8, 4096, 4096, 0) == 0
    assert lib.dg_decoder_topk_workspace(0, 4096, 4096, 64) == 0


def test_exclusion_csr_sorts_dedups_and_keeps_empty_rows():
    from decagon_amd.sparse import exclusion_csr

    pairs0 = np.array([[2, 4], [0, 3], [2, 1], [2, 4], [0, 0], [2, 1], [4, 2]])   # duplicates, unsorted
    m1 = sp.coo_matrix((np.ones(3), ([1, 1, 3], [4, 0, 2])), shape=(5, 6))
    coo2 = (np.array([[4, 5], [4, 0]]), np.array([7.0, 0.0]), (5, 6))              # values do not matter
    ex = exclusion_csr([pairs0, m1, coo2, None], (5, 6))
    assert ex.n_rels == 4 and (ex.n_rows, ex.n_cols) == (5, 6)
    assert ex.rowptr.dtype == np.int32 and ex.col.dtype == np.int32
    assert ex.rowptr.shape == (4 * 5 + 1,)
    want = [
        {0: [0, 3], 2: [1, 4], 4: [2]},
        {1: [0, 4], 3: [2]},
        {4: [0, 5]},
        {},
    ]
    for k, rows in enumerate(want):
        for r in range(5):
            a, b = ex.rowptr[k * 5 + r], ex.rowptr[k * 5 + r + 1]
            assert ex.col[a:b].tolist() == rows.get(r, []), (k, r)
    assert ex.rowptr[-1] == ex.nnz == 10
    assert np.all(np.diff(ex.rowptr) >= 0)


def test_exclusion_csr_rejects_bad_input():
    from decagon_amd.sparse import exclusion_csr

    with pytest.raises(ValueError, match="out of range"):
        exclusion_csr([np.array([[0, 6]])], (5, 6))
    with pytest.raises(ValueError, match="out of range"):
        exclusion_csr([np.array([[-1, 0]])], (5, 6))
    with pytest.raises(ValueError, match="out of range"):
        exclusion_csr([None, np.array([[5, 0]])], (5, 6))
    with pytest.raises(ValueError, match="shape"):
        exclusion_csr([sp.identity(5, format="csr"), sp.identity(6, format="csr")], (5, 5))
    with pytest.raises(ValueError, match="shape"):
        exclusion_csr([(np.array([[0, 0]]), np.array([1.0]), (4, 6))], (5, 6))
    with pytest.raises(ValueError):
        exclusion_csr([], (5, 6))


def test_decoder_topk_validates_before_touching_the_library(monkeypatch):
    from decagon_amd import _lib, kernels

    def no_library(*a, **k):
        raise AssertionError("the library was loaded before the arguments were checked")

    monkeypatch.setattr(_lib, "load", no_library)
    E = torch.zeros(10, 32)
    G = torch.zeros(32, 32)
    l = torch.zeros(3, 32)
    with pytest.raises(TypeError, match="dtype"):
        kernels.decoder_topk(E.double(), E, G, l, 4)
    with pytest.raises(TypeError, match="dtype"):
        kernels.decoder_topk(E, E, G, l.half(), 4)
    with pytest.raises(TypeError, match="torch.Tensor"):
        kernels.decoder_topk(E.numpy(), E, G, l, 4)
    with pytest.raises(ValueError, match="contiguous"):
        kernels.decoder_topk(torch.zeros(10, 64)[:, ::2], E, G, l, 4)
    with pytest.raises(ValueError, match="d mismatch"):
        kernels.decoder_topk(torch.zeros(10, 64), E, G, l, 4)
    with pytest.raises(ValueError, match="d mismatch"):
        kernels.decoder_topk(E, E, torch.zeros(32, 64), l, 4)
    with pytest.raises(ValueError, match="d mismatch"):
        kernels.decoder_topk(E, E, G, torch.zeros(3, 16), 4)
    with pytest.raises(ValueError, match="unsupported"):
        kernels.decoder_topk(torch.zeros(10, 16), torch.zeros(10, 16), torch.zeros(16, 16), None, 4)
    with pytest.raises(ValueError, match="topk"):
        kernels.decoder_topk(E, E, G, l, 0)
    with pytest.raises(ValueError, match="topk"):
        kernels.decoder_topk(E, E, G, l, _lib.DG_TOPK_MAX_K + 1)
    with pytest.raises(ValueError, match="square"):
        kernels.decoder_topk(E, torch.zeros(11, 32), G, l, 4, upper=True)
    with pytest.raises(ValueError, match="disagree"):
        kernels.decoder_topk(E, E, torch.zeros(2, 32, 32), l, 4)
    # everything else right, but host tensors: the device check
    with pytest.raises(ValueError, match="device"):
        kernels.decoder_topk(E, E, G, l, 4)

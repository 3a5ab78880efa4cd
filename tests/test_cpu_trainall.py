"""CPU: the host side of the all-relation training step (dg_decoder_grad_seg_f32,
dg_segment_rows_sum_f32; additive to ABI 39) — exports and bindings, every argument rejection
(they run before any HIP call, so they work without a device), trainall.pack_batches against a
hand-written expectation, and the node-major occurrence list against brute force."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

P = 4096  # a non-null, 16-byte aligned fake device pointer (never dereferenced: every call below is rejected)


def _grad(lib, **over):
    """dg_decoder_grad_seg_f32 with arguments that would be valid, except for `over`."""
    a = dict(row_table=P, ld_row=32, n_rows=100, col_table=P, ld_col=32, n_cols=80, rows=P, cols=P, neg_rows=P,
             seg_ptr=P, seg_rel=None, n_seg=7, n_pairs=500, pos=P, neg=P, margin=0.1, G=P, g_stride=0, l=P,
             l_stride=32, n_rel=7, d=32, mv=P, grad_cols=P, dG=P, dl=P, dG_diag=None, ws=P, ws_bytes=4 * 7 * 32 * 32,
             stream=None)
    assert set(over) <= set(a), over
    a.update(over)
    return lib.dg_decoder_grad_seg_f32(*a.values())


def _sum(lib, **over):
    """dg_segment_rows_sum_f32 with arguments that would be valid, except for `over`."""
    a = dict(node_ptr=P, item=P, sign=P, n_items=500, src=P, n_src_rows=250, d=32, out=P, ld_out=32, n_out_rows=37,
             stream=None)
    assert set(over) <= set(a), over
    a.update(over)
    return lib.dg_segment_rows_sum_f32(*a.values())


def test_symbols_exported_and_bound():
    from decagon_amd import _lib, kernels, trainall

    lib = _lib.load()
    for s in ("dg_decoder_grad_seg_workspace", "dg_decoder_grad_seg_f32", "dg_segment_rows_sum_f32",
              "dg_segment_rows_sum_chunk", "dg_segment_rows_sum_waves"):
        assert hasattr(lib, s), s
        assert s in _lib.SIGNATURES, s
    assert len(_lib.SIGNATURES["dg_decoder_grad_seg_f32"][1]) == 30
    assert len(_lib.SIGNATURES["dg_segment_rows_sum_f32"][1]) == 11
    assert lib.dg_abi_version() == _lib.ABI_VERSION == 39
    chunk, waves = lib.dg_segment_rows_sum_chunk(), lib.dg_segment_rows_sum_waves()
    assert chunk >= 1 and waves >= 1
    for name in ("PreparedDecoderGradSeg", "segment_rows_sum", "occurrence_list", "segment_rows_chunk"):
        assert hasattr(kernels, name), name
    for name in ("pack_batches", "train_step_all"):
        assert hasattr(trainall, name), name


def test_gradient_rejections_without_a_device():
    from decagon_amd import _lib

    lib = _lib.load()
    EINVAL, EALIGN = _lib.DG_EINVAL, _lib.DG_EALIGN
    for d in (0, -32, 16, 48, 96, 128, 256):
        assert _grad(lib, d=d, ld_row=512, ld_col=512, l_stride=d) == EINVAL, d
    for nm in ("row_table", "col_table", "seg_ptr", "G", "rows", "cols", "neg_rows", "pos", "neg", "mv", "grad_cols"):
        assert _grad(lib, **{nm: None}) == EINVAL, nm
    # alignment: tables, G, l and the workspace 16 bytes; the leading dimensions a multiple of 4
    for nm in ("row_table", "col_table", "G", "l", "ws"):
        assert _grad(lib, **{nm: P + 4}) == EALIGN, nm
    assert _grad(lib, ld_row=34) == EALIGN
    assert _grad(lib, ld_col=33) == EALIGN
    # workspace: missing or short only matters when a variable's gradient is asked for
    assert _grad(lib, ws=None) == EINVAL
    assert _grad(lib, ws_bytes=4 * 7 * 32 * 32 - 1) == EINVAL
    assert _grad(lib, ws=None, ws_bytes=0, dG=None, dl=None, n_pairs=0) == _lib.DG_OK
    # negative counts, empty tables, short rows
    assert _grad(lib, n_pairs=-1) == EINVAL
    for n_seg in (0, -1):
        assert _grad(lib, n_seg=n_seg) == EINVAL
    assert _grad(lib, n_rows=0) == EINVAL
    assert _grad(lib, n_cols=0) == EINVAL
    assert _grad(lib, ld_row=28) == EINVAL
    assert _grad(lib, ld_col=16) == EINVAL
    assert _grad(lib, g_stride=32) == EINVAL
    assert _grad(lib, l_stride=16) == EINVAL
    # dl is the gradient of a per-relation l
    assert _grad(lib, l=None) == EINVAL
    assert _grad(lib, l_stride=0) == EINVAL
    assert _grad(lib, l=None, dl=None, n_pairs=0) == _lib.DG_OK
    # a per-relation output of a shared G
    assert _grad(lib, dG_diag=P) == EINVAL
    assert _grad(lib, dG_diag=P, g_stride=1024, dl=None, n_pairs=0) == _lib.DG_OK
    # relations: a map needs n_rel >= 1; without one, per-relation operands bound the segments
    assert _grad(lib, seg_rel=P, n_rel=0) == EINVAL
    assert _grad(lib, n_seg=8, ws_bytes=4 * 8 * 1024) == EINVAL
    assert _grad(lib, n_seg=8, ws_bytes=4 * 8 * 1024, seg_rel=P, n_pairs=0) == _lib.DG_OK
    assert _grad(lib, n_pairs=2**31 - 100) == EINVAL  # 32-bit pair offsets
    # nothing to do is not an error (and launches nothing: no device here)
    assert _grad(lib, n_pairs=0, rows=None, cols=None, neg_rows=None, pos=None, neg=None, mv=None,
                 grad_cols=None) == _lib.DG_OK
    ws = lib.dg_decoder_grad_seg_workspace
    assert ws(7, 32) == 4 * 7 * 32 * 32 and ws(3, 64) == 4 * 3 * 64 * 64
    assert ws(0, 32) == 0 and ws(-1, 32) == 0 and ws(7, 16) == 0 and ws(7, 128) == 0 and ws(7, 0) == 0


def test_row_sum_rejections_without_a_device():
    from decagon_amd import _lib

    lib = _lib.load()
    EINVAL = _lib.DG_EINVAL
    for nm in ("node_ptr", "item", "src", "out"):
        assert _sum(lib, **{nm: None}) == EINVAL, nm
    for d in (0, -1, 257):
        assert _sum(lib, d=d, ld_out=512) == EINVAL, d
    assert _sum(lib, ld_out=31) == EINVAL
    assert _sum(lib, n_items=-1) == EINVAL
    assert _sum(lib, n_out_rows=-1) == EINVAL
    assert _sum(lib, n_src_rows=-1) == EINVAL
    assert _sum(lib, n_src_rows=0) == EINVAL
    assert _sum(lib, n_items=0, item=None, src=None) == _lib.DG_OK
    assert _sum(lib, n_out_rows=0) == _lib.DG_OK


def test_pack_batches_against_a_hand_written_expectation():
    from decagon_amd.trainall import pack_batches

    edge_types = {(0, 0): 2, (0, 1): 1, (1, 1): 4}
    shapes = {(0, 0): (5, 5), (0, 1): (5, 9), (1, 1): (9, 9)}
    batches = {(1, 1): {3: np.array([[8, 0], [1, 2]]), 0: np.zeros((0, 2), np.int64), 2: np.array([[4, 4]])},
               (0, 1): {0: [[4, 8], [0, 0], [3, 7]]}}
    got = pack_batches(batches, edge_types, shapes)
    assert list(got) == [(1, 1), (0, 1)]
    want = {(1, 1): dict(rows=[8, 1, 4], cols=[0, 2, 4], seg_ptr=[0, 2, 2, 3], seg_rel=[3, 0, 2]),
            (0, 1): dict(rows=[4, 0, 3], cols=[8, 0, 7], seg_ptr=[0, 3], seg_rel=[0])}
    for et, w in want.items():
        for name, v in w.items():
            assert got[et][name].dtype == np.int32, (et, name)
            assert got[et][name].tolist() == v, (et, name)
    # an edge type with no relation listed: one empty array set, no segment
    e = pack_batches({(0, 0): {}}, edge_types, shapes)[0, 0]
    assert e["rows"].size == 0 and e["seg_ptr"].tolist() == [0] and e["seg_rel"].size == 0
    ok = np.array([[1, 1]])
    for bad in ({(2, 2): {0: ok}},                                 # unknown edge type
                {(0, 0): {2: ok}}, {(0, 0): {-1: ok}},              # unknown relation
                {(0, 0): [(1, ok), (0, ok), (1, ok)]},              # a relation listed twice
                {(0, 0): {0: np.array([[5, 0]])}}, {(0, 1): {0: np.array([[0, 9]])}},   # outside the shape
                {(0, 0): {0: np.array([[0, -1]])}},
                {(0, 0): {0: np.array([1, 2, 3])}}, {(0, 0): {0: np.array([[0.5, 1.0]])}}):
        with pytest.raises(ValueError):
            pack_batches(bad, edge_types, shapes)


def test_occurrence_list_against_brute_force():
    from decagon_amd.trainall import occurrence_list, row_occurrences

    rng = np.random.default_rng(7)
    n_out, n = 37, 400
    rows = rng.integers(0, n_out, n)
    negs = rng.integers(0, n_out, n)
    rows[rows == 5] = 6   # node 5 never occurs among the positives ...
    negs[negs == 5] = 4   # ... nor among the negatives
    rows[11], negs[13] = -1, n_out  # outside the table: in no list
    node_ptr, order = occurrence_list(rows, n_out)
    assert node_ptr.shape == (n_out + 1,) and np.all(np.diff(node_ptr) >= 0)
    for r in range(n_out):
        assert order[node_ptr[r]:node_ptr[r + 1]].tolist() == [q for q in range(n) if rows[q] == r], r
    assert node_ptr[-1] - node_ptr[0] == n - 1
    node_ptr, item, sign = row_occurrences(rows, negs, n_out)
    assert node_ptr[6] == node_ptr[5]
    src = rng.integers(-3, 4, (n, 8)).astype(np.float64)
    want = np.zeros((n_out, 8))
    for q in range(n):
        if 0 <= rows[q] < n_out:
            want[rows[q]] -= src[q]
        if 0 <= negs[q] < n_out:
            want[negs[q]] += src[q]
    got = np.zeros((n_out, 8))
    for r in range(n_out):
        for q in range(node_ptr[r], node_ptr[r + 1]):
            got[r] += sign[q] * src[item[q]]
        # a node's positives come before its negatives, each in batch order
        seg = list(zip(sign[node_ptr[r]:node_ptr[r + 1]], item[node_ptr[r]:node_ptr[r + 1]]))
        assert seg == sorted(seg), r
    assert np.array_equal(got, want)


def test_grad_seg_wrapper_validates_shapes_before_the_device(monkeypatch):
    """PreparedDecoderGradSeg checks its operands like its four all-relation siblings
    (kernels.RelOperands): shapes first, with their messages, on host tensors and without the
    library; the device requirement comes last."""
    from decagon_amd import _lib, kernels

    def no_library(*a, **k):
        raise AssertionError("the library was loaded before the arguments were checked")

    monkeypatch.setattr(_lib, "load", no_library)
    E = torch.zeros(10, 32)
    G = torch.zeros(32, 32)
    l = torch.zeros(3, 32)
    idx = torch.zeros(8, dtype=torch.int32)
    sc = torch.zeros(8)
    ptr = torch.tensor([0, 3, 3, 8], dtype=torch.int32)

    def f(row=E, col=E, rows=idx, cols=idx, negs=idx, seg_ptr=ptr, seg_rel=None, pos=sc, neg=sc, G=G, l=l, **kw):
        return kernels.PreparedDecoderGradSeg(row, col, rows, cols, negs, seg_ptr, seg_rel, pos, neg, G, l, 0.1, **kw)

    with pytest.raises(TypeError, match="dtype"):
        f(rows=idx.long())
    with pytest.raises(TypeError, match="dtype"):
        f(pos=sc.double())
    with pytest.raises(TypeError, match="torch.Tensor"):
        f(row=E.numpy())
    with pytest.raises(ValueError, match="contiguous"):
        f(row=torch.zeros(10, 64)[:, ::2])
    with pytest.raises(ValueError, match="d mismatch"):
        f(row=torch.zeros(10, 64))
    with pytest.raises(ValueError, match="d mismatch"):
        f(l=torch.zeros(3, 16))
    with pytest.raises(ValueError, match="unsupported"):
        f(row=torch.zeros(10, 16), col=torch.zeros(10, 16), G=torch.zeros(16, 16), l=None)
    with pytest.raises(ValueError, match="unsupported"):  # (the segmented scorer's widths are not the backward's)
        f(row=torch.zeros(10, 96), col=torch.zeros(10, 96), G=torch.zeros(96, 96), l=None)
    with pytest.raises(ValueError, match="disagree"):
        f(G=torch.zeros(4, 32, 32))
    with pytest.raises(ValueError, match="pass seg_rel"):
        f(l=torch.zeros(2, 32))
    with pytest.raises(ValueError, match="seg_rel"):
        f(seg_rel=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError, match="batch sizes differ"):
        f(cols=idx[:5])
    with pytest.raises(ValueError, match="dl needs"):
        f(l=torch.zeros(32), dl=torch.zeros(3, 32))
    with pytest.raises(ValueError, match="device"):  # every shape is right: only now the device
        f()
    with pytest.raises(ValueError, match="device"):
        f(seg_rel=torch.zeros(3, dtype=torch.int32), dl=torch.zeros(3, 32))

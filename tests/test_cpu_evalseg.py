"""CPU: the host side of the fused per-edge-type evaluation (dg_decoder_score_seg_f32,
dg_rank_metrics_seg_f32; additive to ABI 39) — exports and bindings, every argument rejection
(they run before any HIP call, so they work without a device), the workspace size, the
virtual-tile map both launches use (dg_seg_tile_lookup runs the device's own lookup on the host),
evaluate.pack_edge_samples and the Python wrappers' validation."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

P = 4096  # a non-null, 16-byte aligned fake device pointer (never dereferenced: every call below is rejected)


def _score(lib, **over):
    """dg_decoder_score_seg_f32 with arguments that would be valid, except for `over`."""
    a = dict(row_table=P, ld_row=32, n_rows=100, col_table=P, ld_col=32, n_cols=80, row_idx=P, col_idx=P,
             seg_ptr=P, seg_rel=None, n_seg=3, n_pairs=500, G=P, g_stride=0, l=P, l_stride=32, n_rel=3, d=32,
             out=P, stream=None)
    assert set(over) <= set(a), over
    a.update(over)
    return lib.dg_decoder_score_seg_f32(*a.values())


def _rank(lib, **over):
    """dg_rank_metrics_seg_f32 with arguments that would be valid, except for `over`."""
    a = dict(pos=P, pos_ptr=P, n_pos=300, neg=P, neg_ptr=P, n_neg=400, n_seg=5, k=50, mode=1, out=P, ws=P,
             ws_bytes=1 << 40, stream=None)
    assert set(over) <= set(a), over
    a.update(over)
    return lib.dg_rank_metrics_seg_f32(*a.values())


def test_symbols_exported_and_bound():
    from decagon_amd import _lib

    lib = _lib.load()
    for s in ("dg_decoder_score_seg_f32", "dg_rank_metrics_seg_workspace", "dg_rank_metrics_seg_f32",
              "dg_seg_tile_lookup"):
        assert hasattr(lib, s), s
        assert s in _lib.SIGNATURES, s
    assert len(_lib.SIGNATURES["dg_decoder_score_seg_f32"][1]) == 20
    assert len(_lib.SIGNATURES["dg_rank_metrics_seg_f32"][1]) == 13
    assert lib.dg_abi_version() == _lib.ABI_VERSION == 39


def test_scorer_rejections_without_a_device():
    from decagon_amd import _lib

    lib = _lib.load()
    EINVAL = _lib.DG_EINVAL
    for nm in ("row_table", "col_table", "row_idx", "col_idx", "seg_ptr", "G", "out"):
        assert _score(lib, **{nm: None}) == EINVAL, nm
    for n_seg in (0, -1):
        assert _score(lib, n_seg=n_seg) == EINVAL, n_seg
    assert _score(lib, n_pairs=-1) == EINVAL
    for d in (0, -32, 16, 48, 288):
        assert _score(lib, d=d, ld_row=512, ld_col=512, l_stride=d) == EINVAL, d
    assert _score(lib, ld_row=28) == EINVAL
    assert _score(lib, ld_col=31) == EINVAL
    assert _score(lib, n_rows=0) == EINVAL
    assert _score(lib, n_cols=0) == EINVAL
    # strides: 0 or d·d for G, 0 or d for l
    assert _score(lib, g_stride=32) == EINVAL
    assert _score(lib, g_stride=-1024) == EINVAL
    assert _score(lib, l_stride=16) == EINVAL
    assert _score(lib, l_stride=1024) == EINVAL
    # a relation map needs a relation count; without a map per-relation operands bound n_seg
    assert _score(lib, seg_rel=P, n_rel=0) == EINVAL
    assert _score(lib, seg_rel=P, n_rel=-3) == EINVAL
    assert _score(lib, n_seg=4, n_rel=3) == EINVAL
    assert _score(lib, n_seg=4, n_rel=3, g_stride=1024, l=None) == EINVAL
    # 32-bit pair offsets
    assert _score(lib, n_pairs=2**31 - 1, n_seg=1) == EINVAL
    assert _score(lib, n_pairs=0, n_seg=2**26, l_stride=0) == EINVAL
    # nothing to score is not an error (and launches nothing: no device here)
    assert _score(lib, n_pairs=0, row_idx=None, col_idx=None, out=None) == _lib.DG_OK


def test_metrics_rejections_without_a_device():
    from decagon_amd import _lib

    lib = _lib.load()
    EINVAL, EALIGN = _lib.DG_EINVAL, _lib.DG_EALIGN
    for nm in ("pos", "pos_ptr", "neg", "neg_ptr", "out", "ws"):
        assert _rank(lib, **{nm: None}) == EINVAL, nm
    for n_seg in (0, -2):
        assert _rank(lib, n_seg=n_seg) == EINVAL, n_seg
    assert _rank(lib, n_pos=-1) == EINVAL
    assert _rank(lib, n_neg=-1) == EINVAL
    for k in (0, -5):
        assert _rank(lib, k=k) == EINVAL, k
    for mode in (-1, 3, 7):
        assert _rank(lib, mode=mode) == EINVAL, mode
    need = lib.dg_rank_metrics_seg_workspace(300, 400, 5)
    assert need > 0
    assert _rank(lib, ws_bytes=need - 1) == EINVAL
    assert _rank(lib, ws_bytes=0) == EINVAL
    assert _rank(lib, ws=P + 8, ws_bytes=need) == EALIGN
    assert _rank(lib, n_pos=2**30, n_neg=2**30) == EINVAL  # 32-bit offsets


def test_workspace_is_linear_in_the_totals():
    from decagon_amd import _lib

    ws = _lib.load().dg_rank_metrics_seg_workspace
    base = ws(0, 0, 7)
    assert 0 <= base <= 64
    for p, n in ((1, 0), (0, 1), (1000, 3000), (10**6, 2 * 10**6)):
        assert ws(p, n, 7) - base == p * (ws(1, 0, 7) - base) + n * (ws(0, 1, 7) - base), (p, n)
    assert ws(1, 0, 7) - base == 40 and ws(0, 1, 7) - base == 8  # a key and a record; a key
    # what one relation needs through the per-relation entry point, not more
    assert ws(700, 6000, 1) == _lib.load().dg_rank_metrics_ex_workspace(700, 6000)
    assert ws(-1, 0, 1) == 0 and ws(0, -1, 1) == 0 and ws(0, 0, -1) == 0


def _coverage(lib, lens, tile):
    """Every (segment, tile) of the segments with lengths `lens` exactly once over the grid."""
    lens = np.asarray(lens, np.int64)
    ptr = np.zeros(lens.size + 1, np.int32)
    ptr[1:] = np.cumsum(lens)
    n_seg = lens.size
    grid = int(ptr[-1]) // tile + n_seg
    seg, loc = ctypes.c_int32(), ctypes.c_int32()
    seen = {}
    empty = 0
    pp = ptr.ctypes.data_as(ctypes.c_void_p)
    for vt in range(grid):
        rc = lib.dg_seg_tile_lookup(pp, n_seg, tile, vt, ctypes.byref(seg), ctypes.byref(loc))
        assert rc in (0, 1), (vt, rc)
        assert 0 <= seg.value < n_seg and loc.value >= 0
        if rc == 0:
            assert loc.value * tile >= lens[seg.value]
            empty += 1
            continue
        key = (seg.value, loc.value)
        assert key not in seen, (key, vt, seen[key])
        seen[key] = vt
    want = {(s, t) for s in range(n_seg) for t in range(-(-int(lens[s]) // tile))}
    assert set(seen) == want
    assert empty <= n_seg
    # outside the grid
    for vt in (-1, grid):
        assert lib.dg_seg_tile_lookup(pp, n_seg, tile, vt, ctypes.byref(seg), ctypes.byref(loc)) < 0


@pytest.mark.parametrize("tile", [32, 256])
def test_virtual_tiles_cover_every_segment_tile_once(tile):
    from decagon_amd import _lib

    lib = _lib.load()
    _coverage(lib, [0, 1, 31, 32, 33, 64, 0, 255, 256, 257], tile)
    _coverage(lib, [0], tile)
    _coverage(lib, [0, 0, 0], tile)
    _coverage(lib, [tile * 5], tile)
    rng = np.random.default_rng(tile)
    for _ in range(200):
        n = int(rng.integers(1, 40))
        hi = int(rng.choice([2, tile, 3 * tile, 10 * tile]))
        lens = rng.integers(0, hi + 1, n)
        lens[rng.random(n) < 0.2] = 0
        _coverage(lib, lens, tile)


def test_tile_lookup_rejects_bad_arguments():
    from decagon_amd import _lib

    lib = _lib.load()
    ptr = np.array([0, 5], np.int32)
    pp = ptr.ctypes.data_as(ctypes.c_void_p)
    s, t = ctypes.c_int32(), ctypes.c_int32()
    assert lib.dg_seg_tile_lookup(None, 1, 32, 0, ctypes.byref(s), ctypes.byref(t)) == _lib.DG_EINVAL
    assert lib.dg_seg_tile_lookup(pp, 0, 32, 0, ctypes.byref(s), ctypes.byref(t)) == _lib.DG_EINVAL
    assert lib.dg_seg_tile_lookup(pp, 1, 0, 0, ctypes.byref(s), ctypes.byref(t)) == _lib.DG_EINVAL
    assert lib.dg_seg_tile_lookup(pp, 1, 32, 0, None, ctypes.byref(t)) == _lib.DG_EINVAL
    assert lib.dg_seg_tile_lookup(pp, 1, 32, 0, ctypes.byref(s), ctypes.byref(t)) == 1 and (s.value, t.value) == (0, 0)


# ---------------------------------------------------------------- pack_edge_samples
def _edges():
    pos = {(1, 1): {0: np.array([[1, 2], [3, 4]]), 2: np.array([[5, 6]]), 3: np.array([[9, 7], [0, 0], [2, 2]])},
           (0, 1): {0: np.array([[4, 4]])}}
    neg = {(1, 1): [np.array([[0, 1]]), None, np.zeros((0, 2)), np.array([[7, 7], [8, 8]])],   # a list: 4 relations
           (0, 1): [np.array([[1, 1]])]}
    return pos, neg


def test_pack_edge_samples_orders_positives_then_negatives_by_relation():
    from decagon_amd.evaluate import pack_edge_samples

    pos, neg = _edges()
    r, c, pp, npt, rels = pack_edge_samples(pos, neg, (1, 1), 5, (10, 9))
    for a in (r, c, pp, npt, rels):
        assert a.dtype == np.int32 and a.flags.c_contiguous
    assert rels.tolist() == [0, 1, 2, 3, 4]
    assert pp.tolist() == [0, 2, 2, 3, 6, 6]          # relation 1 missing, relation 4 past both containers
    assert npt.tolist() == [0, 1, 1, 1, 3, 3]         # relation 1 None, relation 2 empty
    assert r.tolist() == [1, 3, 5, 9, 0, 2] + [0, 7, 8]
    assert c.tolist() == [2, 4, 6, 7, 0, 2] + [1, 7, 8]
    # an edge type with no entry at all: every segment empty
    r, c, pp, npt, rels = pack_edge_samples({}, {}, (1, 1), 2, (10, 9))
    assert r.size == 0 and c.size == 0 and pp.tolist() == [0, 0, 0] and npt.tolist() == [0, 0, 0]


def test_pack_edge_samples_relation_subset_out_of_order():
    from decagon_amd.evaluate import pack_edge_samples

    pos, neg = _edges()
    r, c, pp, npt, rels = pack_edge_samples(pos, neg, (1, 1), 5, (10, 9), relations=[3, 0, 1])
    assert rels.tolist() == [3, 0, 1]
    assert pp.tolist() == [0, 3, 5, 5] and npt.tolist() == [0, 2, 3, 3]
    assert r.tolist() == [9, 0, 2, 1, 3] + [7, 8, 0]
    assert c.tolist() == [7, 0, 2, 2, 4] + [7, 8, 1]
    # a relation listed twice is two segments
    _, _, pp, npt, rels = pack_edge_samples(pos, neg, (1, 1), 5, (10, 9), relations=[2, 2])
    assert rels.tolist() == [2, 2] and pp.tolist() == [0, 1, 2] and npt.tolist() == [0, 0, 0]


def test_pack_edge_samples_range_errors():
    from decagon_amd.evaluate import pack_edge_samples

    pos, neg = _edges()
    with pytest.raises(ValueError, match="outside the embedding tables"):
        pack_edge_samples(pos, neg, (1, 1), 4, (9, 9))        # row 9
    with pytest.raises(ValueError, match="outside the embedding tables"):
        pack_edge_samples(pos, neg, (1, 1), 4, (10, 7))       # column 7 (positive) and 8 (negative)
    with pytest.raises(ValueError, match="outside the embedding tables"):
        pack_edge_samples(pos, {(1, 1): {0: np.array([[0, -1]])}}, (1, 1), 4, (10, 9))
    with pytest.raises(ValueError, match="relation"):
        pack_edge_samples(pos, neg, (1, 1), 4, (10, 9), relations=[0, 4])
    with pytest.raises(ValueError, match="relation"):
        pack_edge_samples(pos, neg, (1, 1), 4, (10, 9), relations=[-1])
    with pytest.raises(ValueError, match="no relations"):
        pack_edge_samples(pos, neg, (1, 1), 4, (10, 9), relations=[])
    # the out-of-range sample of a relation that is not listed does not matter
    pack_edge_samples(pos, neg, (1, 1), 4, (9, 9), relations=[0, 2])


# ---------------------------------------------------------------- the Python wrappers
def test_wrappers_validate_before_touching_the_library(monkeypatch):
    from decagon_amd import _lib, evaluate, kernels

    def no_library(*a, **k):
        raise AssertionError("the library was loaded before the arguments were checked")

    monkeypatch.setattr(_lib, "load", no_library)
    E = torch.zeros(10, 32)
    G = torch.zeros(32, 32)
    l = torch.zeros(3, 32)
    idx = torch.zeros(8, dtype=torch.int32)
    ptr = torch.tensor([0, 3, 3, 8], dtype=torch.int32)
    f = kernels.decoder_score_seg
    with pytest.raises(TypeError, match="dtype"):
        f(E.double(), E, idx, idx, ptr, G, l)
    with pytest.raises(TypeError, match="dtype"):
        f(E, E, idx, idx, ptr, G, l.half())
    with pytest.raises(TypeError, match="dtype"):
        f(E, E, idx.long(), idx, ptr, G, l)
    with pytest.raises(TypeError, match="dtype"):
        f(E, E, idx, idx, ptr.long(), G, l)
    with pytest.raises(TypeError, match="dtype"):
        f(E, E, idx, idx, ptr, G, l, seg_rel=torch.zeros(3))
    with pytest.raises(TypeError, match="torch.Tensor"):
        f(E.numpy(), E, idx, idx, ptr, G, l)
    with pytest.raises(TypeError, match="torch.Tensor"):
        f(E, E, idx, idx, ptr.numpy(), G, l)
    with pytest.raises(ValueError, match="contiguous"):
        f(torch.zeros(10, 64)[:, ::2], E, idx, idx, ptr, G, l)
    with pytest.raises(ValueError, match="contiguous"):
        f(E, E, torch.zeros(16, dtype=torch.int32)[::2], idx, ptr, G, l)
    with pytest.raises(ValueError, match="d mismatch"):
        f(torch.zeros(10, 64), E, idx, idx, ptr, G, l)
    with pytest.raises(ValueError, match="d mismatch"):
        f(E, E, idx, idx, ptr, torch.zeros(32, 64), l)
    with pytest.raises(ValueError, match="d mismatch"):
        f(E, E, idx, idx, ptr, G, torch.zeros(3, 16))
    with pytest.raises(ValueError, match="unsupported"):
        f(torch.zeros(10, 16), torch.zeros(10, 16), idx, idx, ptr, torch.zeros(16, 16), None)
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
    with pytest.raises(ValueError, match="out"):
        f(E, E, idx, idx, ptr, G, l, out=torch.zeros(7))
    # everything else right, but host tensors: the device check
    with pytest.raises(ValueError, match="device"):
        f(E, E, idx, idx, ptr, G, l)

    g = evaluate.rank_metrics_seg_device
    x = torch.zeros(8)
    with pytest.raises(ValueError, match="sigmoid"):
        g(x, ptr, x, ptr, sigmoid="logistic")
    with pytest.raises(ValueError, match="k must"):
        g(x, ptr, x, ptr, k=0)
    with pytest.raises(ValueError, match="device"):
        g(x, ptr, x, ptr)
    with pytest.raises(TypeError, match="torch.Tensor"):
        g(x.numpy(), ptr, x, ptr)

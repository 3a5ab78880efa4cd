"""CPU: epochs of all-relation training (decagon_amd/epochs.py, csrc/permute.h, dg_epoch_batch_i32;
additive to ABI 39) — the stateless permutation (bijection, the C++ header against the numpy twin
through dg_epoch_perm_host, uniformity), EdgeBatches' host logic and rejections, the coverage of an
epoch by host_batch, split_edges, and the kernel entry's rejections (they run before any HIP call)."""
import numpy as np
import pytest
import scipy.sparse as sp

from decagon_amd import epochs as E

KEYS = (0, 12345, 0xDEADBEEF)
# every n in 1..300 (n = 1, 2, 3; powers of 4: 4, 16, 64, 256; powers of 4 plus 1: 5, 17, 65, 257;
# powers of 2 that are no power of 4: 2, 8, 32, 128) and four larger sizes
SIZES = list(range(1, 301)) + [1000, 4097, 65537, 2**20 + 1]


def test_perm_is_a_bijection():
    for n in SIZES:
        for key in KEYS:
            p = E.perm(n, key, np.arange(n))
            assert p.dtype == np.int64 and np.array_equal(np.sort(p), np.arange(n)), (n, key)
    assert {4, 16, 64, 256, 5, 17, 65, 257, 2, 8, 32, 128, 1, 3} <= set(SIZES)
    with pytest.raises(ValueError):
        E.perm(0, 1, [0])
    with pytest.raises(ValueError):
        E.perm(2**31, 1, [0])
    with pytest.raises(ValueError):
        E.perm(5, 1, [5])
    with pytest.raises(ValueError):
        E.perm(5, 1, [-1])


def test_header_equals_numpy_integer_for_integer():
    from decagon_amd import _lib

    lib = _lib.load()
    for n in SIZES:
        x = np.arange(n, dtype=np.int32)
        for key in KEYS:
            out = np.full(n, -7, np.int32)
            assert lib.dg_epoch_perm_host(n, key, x.ctypes.data, out.ctypes.data, n) == _lib.DG_OK
            assert np.array_equal(out, E.perm(n, key, x)), (n, key)
    # a scattered subset in arbitrary order, near 2^31
    n = 2**31 - 1
    x = np.asarray([0, 1, n - 1, n // 2, 123456789, 2**30, 2**30 + 1], np.int32)
    out = np.empty(len(x), np.int32)
    assert lib.dg_epoch_perm_host(n, 99, x.ctypes.data, out.ctypes.data, len(x)) == _lib.DG_OK
    assert np.array_equal(out, E.perm(n, 99, x))
    # the key derivation
    for seed, epoch, slot in ((0, 0, 0), (1, 2, 3), (2**40 + 5, 7, 1931), (2**64 - 1, 2**32 - 1, 2**31 - 1)):
        assert lib.dg_epoch_key_host(seed, epoch, slot) == E.epoch_key(seed, epoch, slot)
    # rejections
    EINVAL = _lib.DG_EINVAL
    assert lib.dg_epoch_perm_host(0, 1, x.ctypes.data, out.ctypes.data, 1) == EINVAL
    assert lib.dg_epoch_perm_host(5, 1, x.ctypes.data, out.ctypes.data, -1) == EINVAL
    assert lib.dg_epoch_perm_host(5, 1, None, out.ctypes.data, 1) == EINVAL
    assert lib.dg_epoch_perm_host(5, 1, x.ctypes.data, None, 1) == EINVAL
    assert lib.dg_epoch_perm_host(5, 1, x.ctypes.data, out.ctypes.data, 3) == EINVAL  # x[2] >= n
    assert lib.dg_epoch_perm_host(5, 1, None, None, 0) == _lib.DG_OK


@pytest.mark.parametrize("n", [7, 64, 65])
def test_perm_is_uniform_over_keys(n):
    """Over the keys of 2,000 relation slots (seed 0, epoch 0) every (position, image) count lies
    within 5 standard deviations of 2000/n, σ = √(2000·(1/n)(1 − 1/n))."""
    trials = 2000
    cnt = np.zeros((n, n))
    for slot in range(trials):
        cnt[np.arange(n), E.perm(n, E.epoch_key(0, 0, slot), np.arange(n))] += 1
    sd = np.sqrt(trials * (1 / n) * (1 - 1 / n))
    dev = np.abs(cnt - trials / n).max() / sd
    print(f"n = {n}: largest deviation {dev:.2f} sigma")
    assert dev <= 5.0


def test_epochs_and_relations_give_different_orders():
    n = 1000
    orders = {(e, s): tuple(E.perm(n, E.epoch_key(3, e, s), np.arange(n))) for e in range(4) for s in range(4)}
    assert len(set(orders.values())) == 16
    assert E.epoch_key(3, 0, 0) != E.epoch_key(4, 0, 0)
    assert E.epoch_key(3, 0, 0) != E.epoch_key(3 + 2**32, 0, 0)  # the seed's high word counts


# ------------------------------------------------------------------ EdgeBatches (host)
B = 8
ET = {(0, 0): 2, (0, 1): 3, (1, 1): 5}
SHAPES = {(0, 0): (40, 40), (0, 1): (40, 30), (1, 1): (30, 30)}
#               exactly B, B − 1 | 0 edges, 3 batches + 5, (not listed) | 2B, 5B + 3, B − 1, 0, 3B + 7
COUNTS = {(0, 0): [B, B - 1], (0, 1): [0, 3 * B + 5, None], (1, 1): [2 * B, 5 * B + 3, B - 1, 0, 3 * B + 7]}


def _edges(seed=0):
    rng = np.random.default_rng(seed)
    out = {}
    for et, cs in COUNTS.items():
        n_r, n_c = SHAPES[et]
        out[et] = {}
        for k, c in enumerate(cs):
            if c is not None:  # distinct pairs: an edge is recognisable
                flat = rng.choice(n_r * n_c, c, replace=False)
                out[et][k] = np.stack([flat // n_c, flat % n_c], 1).astype(np.int64)
    return out


def _eb(wrap=(), edges=None, **kw):
    a = dict(train_edges=_edges() if edges is None else edges, edge_types=ET, shapes=SHAPES, batch_size=B, seed=11,
             device=None, wrap=wrap)
    a.update(kw)
    return E.EdgeBatches(**a)


def test_steps_active_lists_skipped_and_wrap():
    eb = _eb()
    assert eb.steps(0) == eb.steps(5) == 5
    assert eb.skipped == [((0, 0), 1), ((0, 1), 0), ((0, 1), 2), ((1, 1), 2), ((1, 1), 3)]
    want = {  # t -> active relations
        (0, 0): {0: [0], 1: [], 4: []},
        (0, 1): {0: [1], 2: [1], 3: [], 4: []},
        (1, 1): {0: [0, 1, 4], 1: [0, 1, 4], 2: [1, 4], 3: [1], 4: [1], 5: []},
    }
    for et, per in want.items():
        for t, rel in per.items():
            got = eb.active(et, t)
            assert got.dtype == np.int32 and got.tolist() == rel, (et, t)
    # the levels that key the device cache: one per distinct threshold
    te = eb.types[1, 1]
    assert [te.level(t) for t in range(7)] == [1, 1, 2, 3, 3, 4, 4]
    for t in range(6):  # host_batch lists exactly the active relations, B pairs each
        hb = eb.host_batch(0, t)
        for et in ET:
            rel = eb.active(et, t).tolist()
            assert (et in hb) == bool(rel)
            if rel:
                assert list(hb[et]) == rel
                assert all(v.shape == (B, 2) and v.dtype == np.int64 for v in hb[et].values())
    assert eb.host_batch(0, 5) == {}
    # wrapping edge types do not count toward the length, and stay active
    ew = _eb(wrap=[(1, 1)])
    assert ew.steps(0) == 3
    assert ew.active((1, 1), 0).tolist() == ew.active((1, 1), 77).tolist() == [0, 1, 4]
    assert ew.types[1, 1].level(0) == ew.types[1, 1].level(77) == 0
    assert ew.skipped == eb.skipped  # a wrapping relation below B is skipped, not spun on
    with pytest.raises(ValueError):
        _eb(wrap=list(ET)).steps(0)
    with pytest.raises(RuntimeError):
        eb.batch(0, 0)  # built without a device


def test_rejections():
    good = _edges()
    bad = lambda et, k, v: {**good, et: {**good[et], k: v}}  # noqa: E731
    with pytest.raises(ValueError, match="unknown edge type"):
        _eb(edges={**good, (1, 0): {0: np.zeros((1, 2), np.int64)}})
    with pytest.raises(ValueError, match="unknown relation"):
        _eb(edges=bad((0, 0), 2, np.zeros((1, 2), np.int64)))
    with pytest.raises(ValueError, match="unknown relation"):
        _eb(edges=bad((0, 0), -1, np.zeros((1, 2), np.int64)))
    with pytest.raises(ValueError, match="listed twice"):
        _eb(edges={**good, (0, 0): [(0, good[0, 0][0]), (0, good[0, 0][0])]})
    with pytest.raises(ValueError, match=r"\[n, 2\]"):
        _eb(edges=bad((0, 0), 0, np.zeros((4, 3), np.int64)))
    with pytest.raises(ValueError, match=r"\[n, 2\]"):
        _eb(edges=bad((0, 0), 0, np.zeros((4, 2), np.float32)))
    for v in ([[40, 0]], [[0, 30]], [[-1, 0]], [[0, -1]]):
        with pytest.raises(ValueError, match=r"edge type \(0, 1\), relation 1: index outside"):
            _eb(edges=bad((0, 1), 1, np.concatenate([good[0, 1][1], np.asarray(v)])))
    for bs in (0, -1, 2.5):
        with pytest.raises(ValueError, match="batch_size"):
            _eb(batch_size=bs)
    with pytest.raises(ValueError, match="wrap"):
        _eb(wrap=[(1, 0)])
    with pytest.raises(ValueError, match="too many pairs"):
        _eb(batch_size=2**29)
    eb = _eb()
    for e, t in ((-1, 0), (2**32, 0), (0, -1), (0, 2**31), (0.5, 0)):
        with pytest.raises(ValueError):
            eb.host_batch(e, t)
    # sequences of pairs are accepted where mappings are
    seq = E.EdgeBatches(list((et, list(per.items())) for et, per in good.items()), ET, SHAPES, B, 11, None)
    assert seq.steps(0) == 5 and seq.skipped == eb.skipped


@pytest.mark.parametrize("epoch", [0, 3])
def test_an_epoch_covers_every_edge_at_most_once(epoch):
    edges = _edges()
    eb = _eb(edges=edges)
    seen = {(et, k): [] for et, per in edges.items() for k in per}
    for t in range(eb.steps(epoch)):
        for et, per in eb.host_batch(epoch, t).items():
            for k, b in per.items():
                seen[et, k].append(b)
    for (et, k), got in seen.items():
        n = len(edges[et][k])
        got = np.concatenate(got) if got else np.zeros((0, 2), np.int64)
        key = lambda a: set(map(tuple, a.tolist()))  # noqa: E731
        assert len(got) == (n // B) * B and len(key(got)) == len(got)  # no edge twice
        assert key(got) <= key(edges[et][k])
        assert n - len(got) == n % B                                   # exactly n mod B are missing
    # another epoch: another order of the same relation
    other = _eb(edges=edges).host_batch(epoch + 1, 0)
    assert not np.array_equal(other[1, 1][1], eb.host_batch(epoch, 0)[1, 1][1])
    # another seed too
    assert not np.array_equal(_eb(edges=edges, seed=12).host_batch(epoch, 0)[1, 1][1],
                              eb.host_batch(epoch, 0)[1, 1][1])


def test_a_wrapping_relation_repeats_with_its_period():
    edges = _edges()
    plain, ew = _eb(edges=edges), _eb(edges=edges, wrap=[(1, 1)])
    nb = {0: 2, 1: 5, 4: 3}
    for t in range(12):
        hb = ew.host_batch(2, t)[1, 1]
        assert sorted(hb) == [0, 1, 4]
        for k, period in nb.items():
            assert np.array_equal(hb[k], plain.host_batch(2, t % period)[1, 1][k])  # the same permutation
            assert np.array_equal(hb[k], ew.host_batch(2, t + period)[1, 1][k])


# ------------------------------------------------------------------ the split
def _adj(seed=5):
    rng = np.random.default_rng(seed)
    mats = {}
    for et, (shape, ks) in {(0, 0): ((60, 60), [900, 300]), (0, 1): ((60, 45), [700]), (1, 0): ((45, 60), [700])}.items():
        mats[et] = []
        for n in ks:
            flat = rng.choice(shape[0] * shape[1], n, replace=False)
            mats[et].append(sp.csr_matrix((np.ones(n), (flat // shape[1], flat % shape[1])), shape=shape))
    mats[1, 0] = [mats[0, 1][0].T.tocsr()]
    return mats


def _set(a):
    return set(map(tuple, np.asarray(a).tolist()))


def test_split_edges():
    from decagon_amd.sparse import preprocess_graph, sparse_to_tuple

    adj = _adj()
    train, val, false, adj_train = E.split_edges(adj, val_fraction=0.1, min_val=50, seed=4, mirror={(1, 0): (0, 1)})
    assert list(train) == list(val) == list(false) == list(adj_train) == list(adj)
    for et, mats in adj.items():
        for k, m in enumerate(mats):
            coords = sparse_to_tuple(m)[0]
            n = len(coords)
            num_val = min(max(50, int(n * 0.1)), n // 2)
            assert len(val[et][k]) == num_val and len(train[et][k]) == n - num_val
            assert _set(train[et][k]) | _set(val[et][k]) == _set(coords)
            assert not _set(train[et][k]) & _set(val[et][k])
            f = false[et][k]
            assert f.shape == (num_val, 2) and len(_set(f)) == num_val           # distinct
            assert f.min() >= 0 and (f < np.asarray(m.shape)).all()               # inside the shape
            assert not _set(f) & _set(coords)                                     # none is an edge
            t = train[et][k]
            want = preprocess_graph(sp.csr_matrix((np.ones(len(t)), (t[:, 0], t[:, 1])), shape=m.shape))
            got = adj_train[et][k]
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]
    assert [len(v) for v in val[0, 0].values()] == [90, 50]  # ⌊n·fraction⌋ above min_val, and min_val
    # the mirror is the flipped split
    for d in (train, val, false):
        assert np.array_equal(d[1, 0][0], d[0, 1][0][:, ::-1])
    # deterministic in the seed
    again = E.split_edges(adj, val_fraction=0.1, min_val=50, seed=4, mirror={(1, 0): (0, 1)})
    other = E.split_edges(adj, val_fraction=0.1, min_val=50, seed=5, mirror={(1, 0): (0, 1)})
    for a, b, c in zip((train, val, false), again, other):
        for et in adj:
            for k in a[et]:
                assert np.array_equal(a[et][k], b[et][k])
        assert not np.array_equal(a[0, 0][0], c[0, 0][0])
    # n // 2 caps the validation set; an empty relation splits into nothing
    small = {(0, 0): [sp.csr_matrix((np.ones(5), (np.arange(5), np.arange(5))), shape=(9, 9)), sp.csr_matrix((9, 9))]}
    tr, va, fa, _ = E.split_edges(small)
    assert len(va[0, 0][0]) == 2 and len(tr[0, 0][0]) == 3 and len(fa[0, 0][0]) == 2
    assert len(va[0, 0][1]) == len(tr[0, 0][1]) == len(fa[0, 0][1]) == 0
    # the outputs plug into EdgeBatches
    eb = E.EdgeBatches(train, {et: len(m) for et, m in adj.items()}, {et: m[0].shape for et, m in adj.items()},
                       64, 0, None, wrap=[(0, 1), (1, 0)])
    assert eb.steps(0) == 810 // 64


def test_split_of_a_nearly_dense_relation_is_refused():
    dense = np.ones((12, 12))
    dense[0, :10] = 0  # 10 non-edges, 134 edges: num_val = 50 > 10
    with pytest.raises(ValueError, match="not edges"):
        E.split_edges({(0, 0): [sp.csr_matrix(dense)]})
    # … and with few edges to find among many non-edges it succeeds, however the stream falls
    tr, va, fa, _ = E.split_edges({(0, 0): [sp.csr_matrix(dense)]}, min_val=10)
    assert _set(fa[0, 0][0]) == {(0, c) for c in range(10)}
    with pytest.raises(ValueError, match="mirror"):
        E.split_edges(_adj(), mirror={(1, 0): (1, 1)})


# ------------------------------------------------------------------ ABI
P = 4096  # a non-null, 16-byte aligned fake device pointer (never dereferenced: every call below is rejected)


def _batch(lib, **over):
    """dg_epoch_batch_i32 with arguments that would be valid, except for `over`."""
    a = dict(edges=P, n_edges=1000, edge_ptr=P, n_rel=7, seg_rel=P, n_seg=5, wrap_mask=None, batch=64, t=0, epoch=0,
             seed=1, first_slot=0, bad_row=37, rows=P, cols=P, stream=None)
    assert set(over) <= set(a), over
    a.update(over)
    return lib.dg_epoch_batch_i32(*a.values())


def test_symbols_exported_and_bound():
    from decagon_amd import _lib, kernels

    lib = _lib.load()
    for s in ("dg_epoch_batch_i32", "dg_epoch_perm_host", "dg_epoch_key_host"):
        assert hasattr(lib, s), s
        assert s in _lib.SIGNATURES, s
    assert len(_lib.SIGNATURES["dg_epoch_batch_i32"][1]) == 16
    assert lib.dg_abi_version() == _lib.ABI_VERSION == 39
    assert callable(kernels.epoch_batch)


def test_batch_entry_rejections_without_a_device():
    from decagon_amd import _lib

    lib = _lib.load()
    EINVAL, EALIGN = _lib.DG_EINVAL, _lib.DG_EALIGN
    for nm in ("edges", "edge_ptr", "seg_rel", "rows", "cols"):
        assert _batch(lib, **{nm: None}) == EINVAL, nm
    for batch in (0, -64):
        assert _batch(lib, batch=batch) == EINVAL
    assert _batch(lib, n_seg=-1) == EINVAL
    assert _batch(lib, n_rel=0) == EINVAL
    assert _batch(lib, n_edges=-1) == EINVAL
    assert _batch(lib, t=-1) == EINVAL
    assert _batch(lib, first_slot=-1) == EINVAL
    assert _batch(lib, n_seg=2**25, batch=64) == EINVAL  # 32-bit pair offsets
    assert _batch(lib, edges=P + 4) == EALIGN
    assert _batch(lib, edge_ptr=P + 4) == EALIGN
    for nm in ("seg_rel", "rows", "cols", "wrap_mask"):
        assert _batch(lib, **{nm: P + 2}) == EALIGN, nm
    # nothing to form is not an error (and launches nothing: no device here)
    assert _batch(lib, n_seg=0) == _lib.DG_OK
    assert _batch(lib, n_seg=0, seg_rel=None, rows=None, cols=None) == _lib.DG_OK
    assert _batch(lib, n_seg=0, n_edges=0, edges=None) == _lib.DG_OK


def test_epoch_batch_wrapper_validation():
    torch = pytest.importorskip("torch")
    from decagon_amd import kernels

    i32, i64 = torch.int32, torch.int64
    a = dict(edges=torch.zeros((10, 2), dtype=i32), edge_ptr=torch.zeros(4, dtype=i64),
             seg_rel=torch.zeros(2, dtype=i32), wrap_mask=None, batch=4, t=0, epoch=0, seed=0, first_slot=0, bad_row=9)
    for nm in ("edges", "edge_ptr", "seg_rel"):
        with pytest.raises(TypeError):
            kernels.epoch_batch(**{**a, nm: np.zeros(3)})
    with pytest.raises(TypeError):
        kernels.epoch_batch(**{**a, "edges": a["edges"].long()})
    with pytest.raises(TypeError):
        kernels.epoch_batch(**{**a, "edge_ptr": a["edge_ptr"].int()})
    with pytest.raises(ValueError, match="contiguous"):
        kernels.epoch_batch(**{**a, "edges": torch.zeros((10, 4), dtype=i32)[:, :2]})
    with pytest.raises(ValueError, match="edges"):
        kernels.epoch_batch(**{**a, "edges": torch.zeros((10, 3), dtype=i32)})
    with pytest.raises(ValueError, match="edge_ptr"):
        kernels.epoch_batch(**{**a, "edge_ptr": torch.zeros(1, dtype=i64)})
    with pytest.raises(ValueError, match="wrap_mask"):
        kernels.epoch_batch(**{**a, "edge_ptr": torch.zeros(34, dtype=i64), "wrap_mask": torch.zeros(1, dtype=i32)})
    for nm, v in (("batch", 0), ("t", -1), ("epoch", 2**32), ("first_slot", -1), ("bad_row", -1), ("batch", 1.5)):
        with pytest.raises(ValueError, match=nm):
            kernels.epoch_batch(**{**a, nm: v})
    with pytest.raises(ValueError, match="rows"):
        kernels.epoch_batch(**a, rows=torch.zeros(7, dtype=i32))
    with pytest.raises(ValueError, match="device"):  # all else valid: the device check is the last
        kernels.epoch_batch(**a)

"""GPU: epochs of all-relation training — dg_epoch_batch_i32 against the numpy restatement (exact
integers), EdgeBatches.batch against EdgeBatches.host_batch over an epoch, train_step_all /
train_epoch_all fed from the device against the same steps fed from the host on the golden S model
(bit for bit: the same kernels on the same indices), and split_edges' validation sets through
accuracy_scores_all."""
import numpy as np
import pytest

from decagon_amd import epochs as E
from test_gpu_model import _setup

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


# ------------------------------------------------------------------ the kernel
NR, NC = 37, 29
COUNTS = [0, 1, 63, 64, 65, 200, 1000]
K = len(COUNTS)
FIRST_SLOT, SEED = 5, 2**40 + 77
SENTINEL = -99
SEG_REL = [6, 2, 4, K, 0, 5, 3]  # non-monotone, a subset (no relation 1), one relation outside [0, K)


@pytest.fixture(scope="module")
def kernel_case():
    rng = np.random.default_rng(9)
    per = {k: np.stack([rng.integers(0, NR, n), rng.integers(0, NC, n)], 1).astype(np.int64)
           for k, n in enumerate(COUNTS)}
    ptr = np.concatenate([[0], np.cumsum(COUNTS)]).astype(np.int64)
    edges = np.concatenate([per[k] for k in range(K)]).astype(np.int32)
    return per, ptr, edges


def _expected(per, B, t, epoch, wrap):
    """rows, cols [n_seg·B] by the numpy perm; batch-less segments: (NR, 0)."""
    rows = np.full(len(SEG_REL) * B, NR, np.int64)
    cols = np.zeros(len(SEG_REL) * B, np.int64)
    live = 0
    for s, k in enumerate(SEG_REL):
        if not 0 <= k < K:
            continue
        n = COUNTS[k]
        nb = n // B
        if nb == 0 or (not wrap and t >= nb):
            continue
        tb = t % nb if wrap else t
        q = E.perm(n, E.epoch_key(SEED, epoch, FIRST_SLOT + k), np.arange(tb * B, (tb + 1) * B))
        rows[s * B:(s + 1) * B], cols[s * B:(s + 1) * B] = per[k][q, 0], per[k][q, 1]
        live += 1
    return rows, cols, live


@pytest.mark.parametrize("wrap", [False, True])
@pytest.mark.parametrize("B", [64, 32])
def test_kernel_equals_the_numpy_restatement(kernel_case, B, wrap):
    from decagon_amd import kernels

    dev = _dev()
    per, ptr, edges = kernel_case
    T = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x)).to(dev, dt)  # noqa: E731
    d_edges, d_ptr, d_rel = T(edges, torch.int32), T(ptr, torch.int64), T(SEG_REL, torch.int32)
    mask = T(np.asarray([(1 << K) - 1]), torch.int32) if wrap else None
    n = len(SEG_REL) * B
    side = torch.cuda.Stream()
    lives = set()
    for epoch in (0, 3):
        for t in (0, 1, 3, 15, 40):  # B = 64: 64 and 65 edges end at t = 1, 200 at 3, 1000 at 15; B = 32: by 40
            want_r, want_c, live = _expected(per, B, t, epoch, wrap)
            lives.add(live)
            for stream in (None, side):
                rows = torch.full((n + 64,), SENTINEL, device=dev, dtype=torch.int32)
                cols = torch.full((n + 64,), SENTINEL, device=dev, dtype=torch.int32)
                if stream is not None:
                    stream.wait_stream(torch.cuda.current_stream())
                kernels.epoch_batch(d_edges, d_ptr, d_rel, mask, B, t, epoch, SEED, FIRST_SLOT, bad_row=NR,
                                    rows=rows[:n], cols=cols[:n], stream=stream)
                (stream or torch.cuda.current_stream()).synchronize()
                r, c = rows.cpu().numpy(), cols.cpu().numpy()
                assert np.all(r[n:] == SENTINEL) and np.all(c[n:] == SENTINEL)  # nothing beyond n_seg·B
                assert np.array_equal(r[:n], want_r), (epoch, t)
                assert np.array_equal(c[:n], want_c), (epoch, t)
    # relations 0 and K never have a batch (and 63 edges give none at B = 64); without wrapping the
    # others leave one by one until the last step has batch-less segments only
    full = 5 if B == 32 else 4
    assert lives == ({full} if wrap else ({5, 4, 2, 1, 0} if B == 32 else {4, 2, 1, 0}))
    # buffers the wrapper allocates; an empty segment list
    rows, cols = kernels.epoch_batch(d_edges, d_ptr, d_rel, mask, B, 0, 0, SEED, FIRST_SLOT, bad_row=NR)
    torch.cuda.synchronize()
    want_r, want_c, _ = _expected(per, B, 0, 0, wrap)
    assert np.array_equal(rows.cpu().numpy(), want_r) and np.array_equal(cols.cpu().numpy(), want_c)
    rows, cols = kernels.epoch_batch(d_edges, d_ptr, d_rel[:0], mask, B, 0, 0, SEED, FIRST_SLOT, bad_row=NR)
    assert rows.numel() == cols.numel() == 0


@pytest.mark.parametrize("wrap", [False, True])
def test_device_batches_equal_host_batches_over_an_epoch(kernel_case, wrap):
    dev = _dev()
    per, _, _ = kernel_case
    ets, shapes = {(0, 0): 2, (0, 1): K}, {(0, 0): (NR, NR), (0, 1): (NR, NC)}
    rng = np.random.default_rng(3)
    train = {(0, 0): {1: rng.integers(0, NR, (300, 2))}, (0, 1): per}
    eb = E.EdgeBatches(train, ets, shapes, 64, SEED, dev, wrap=[(0, 1)] if wrap else ())
    assert eb.steps(0) == (4 if wrap else 15)
    for epoch in (0, 1):
        for t in range(eb.steps(epoch) + 1):
            db = eb.batch(epoch, t)
            want = eb.host_batch(epoch, t)
            got = db.to_host()
            assert list(got) == list(want)
            for et in want:
                tb = db[et]
                assert list(got[et]) == list(want[et]) == tb.seg_rel.cpu().tolist()
                assert tb.n == 64 * tb.n_seg == tb.rows.numel() == tb.cols.numel()
                assert tb.seg_ptr.cpu().tolist() == list(range(0, tb.n + 1, 64))
                assert tb.seg2.cpu().tolist() == list(range(0, 2 * tb.n + 1, 64))
                assert tb.rel2.cpu().tolist() == 2 * list(want[et])
                for k in want[et]:
                    assert np.array_equal(got[et][k], want[et][k]), (epoch, t, et, k)
    # the segment arrays are cached per threshold: the steps of one level share them
    te = eb.types[0, 1]
    assert len(te.meta) <= len(te.levels) + 1
    if not wrap:
        assert eb.batch(0, 4).types[0, 1].seg2 is eb.batch(0, 5).types[0, 1].seg2


# ------------------------------------------------------------------ steps and epochs on the golden S model
BS = 2560  # S's relations hold 2,552 to 16,460 training edges: 0 (skipped), 2, 4 and 6 batches an epoch


def _edge_batches(z, model, opt, dev, seed=21):
    train = {(i, j): {k: z[f"train_{i}_{j}_{k}"] for k in range(Kij)} for (i, j), Kij in model.edge_types.items()}
    shapes = {et: tuple(int(x) for x in opt.edge_type2dim[et][0]) for et in model.edge_types}
    return E.EdgeBatches(train, model.edge_types, shapes, BS, seed, dev)


def _fed_negatives(z, hb, seed):
    rng = np.random.default_rng(seed)
    n = [int(x) for x in z["n_nodes"]]
    return {et: {k: rng.integers(0, n[et[0]], len(b)) for k, b in per.items()} for et, per in hb.items()}


def _same(a, b):
    assert a[0] == b[0]  # the cost, bit for bit
    assert len(a[1]) == len(b[1])
    for (g0, _), (g1, _) in zip(a[1], b[1]):
        assert np.array_equal(g0, g1)


def test_device_fed_step_equals_host_fed_step_bit_for_bit(golden_S):
    from decagon_amd.trainall import train_step_all

    dg, ph, model, opt, feed = _setup(golden_S)
    sess = dg.Session()
    eb = _edge_batches(golden_S, model, opt, sess.device)
    steps = eb.steps(0)
    assert steps >= 2
    for epoch, t in ((0, 0), (1, steps - 1)):  # all relations active; the longest relations only
        hb = eb.host_batch(epoch, t)
        negs = _fed_negatives(golden_S, hb, 5 + t)
        host = train_step_all(sess, opt, ph, feed, hb, neg_samples=negs, apply=False)
        devf = train_step_all(sess, opt, ph, feed, eb.batch(epoch, t), neg_samples=negs, apply=False)
        _same(host, devf)
        assert any(np.any(g != 0) for g, _ in devf[1])
        # device-drawn negatives from the same draw counter
        sampler = sess.caches[("sampler", id(opt))] if ("sampler", id(opt)) in sess.caches else None
        start = sampler.counter if sampler is not None else 0
        host = train_step_all(sess, opt, ph, feed, hb, apply=False)
        sampler = sess.caches[("sampler", id(opt))]
        end = sampler.counter
        assert end > start
        sampler.counter = start
        devd = train_step_all(sess, opt, ph, feed, eb.batch(epoch, t), apply=False)
        assert sampler.counter == end
        _same(host, devd)
    # the rejections stay
    f = dict(feed)
    f[opt.latent_varies[0]] = np.eye(32, dtype=np.float32)
    with pytest.raises(dg.InvalidArgumentError):
        train_step_all(sess, opt, ph, f, eb.batch(0, 0))
    sess.shard = object()
    with pytest.raises(NotImplementedError):
        train_step_all(sess, opt, ph, feed, eb.batch(0, 0))


def test_an_epoch_from_the_device_equals_the_host_fed_steps(golden_S):
    from decagon_amd.train import BETA1
    from decagon_amd.trainall import train_epoch_all, train_step_all

    runs = []
    for device_fed in (True, False):
        dg, ph, model, opt, feed = _setup(golden_S)
        sess = dg.Session()
        opt.seed = 99
        eb = _edge_batches(golden_S, model, opt, sess.device)
        if device_fed:
            costs = train_epoch_all(sess, opt, ph, feed, eb, 2)
        else:
            costs = np.asarray([train_step_all(sess, opt, ph, feed, eb.host_batch(2, t))
                                for t in range(eb.steps(2))], np.float64)
        adam = [v for k, v in sess.caches.items() if isinstance(k, tuple) and k[0] == "adam"]
        assert len(adam) == 1
        runs.append((costs, [p.eval() for p in model.vars.values()], adam[0].state.cpu().numpy(),
                     sess.caches[("sampler", id(opt))].counter, eb.steps(2)))
    (c0, v0, a0, n0, steps), (c1, v1, a1, n1, _) = runs
    assert steps == 16460 // BS == 6 and len(_edge_batches(golden_S, model, opt, None).skipped) == 2
    assert c0.dtype == np.float64 and c0.shape == (steps,) and np.all(np.isfinite(c0)) and np.all(c0 > 0)
    assert np.array_equal(c0, c1)
    for x, y in zip(v0, v1):
        assert np.array_equal(x, y)
    # Adam's t: the state holds β1^t of the NEXT update (train.AdamState), t = steps + 1
    assert np.array_equal(a0, a1)
    assert round(float(np.log(a0[0]) / np.log(BETA1))) == steps + 1
    assert n0 == n1 > 0


# ------------------------------------------------------------------ the split into the evaluation
def test_split_validation_sets_feed_accuracy_scores_all(golden_S):
    import scipy.sparse as sp

    from decagon_amd.evaluate import accuracy_scores_all

    dg, ph, model, opt, feed = _setup(golden_S)
    sess = dg.Session()
    adj = {}
    for (i, j), Kij in model.edge_types.items():
        shape = tuple(int(x) for x in opt.edge_type2dim[i, j][0])
        adj[i, j] = []
        for k in range(Kij):
            e = np.unique(np.asarray(golden_S[f"train_{i}_{j}_{k}"], np.int64), axis=0)
            adj[i, j].append(sp.csr_matrix((np.ones(len(e)), (e[:, 0], e[:, 1])), shape=shape))
    train, val, false, adj_train = E.split_edges(adj, val_fraction=0.05, min_val=20, seed=1)
    for et, Kij in model.edge_types.items():
        assert all(len(val[et][k]) >= 1 for k in range(Kij))
        scores = accuracy_scores_all(sess, opt, ph, feed, val, false, et)
        assert scores.shape == (Kij, 3) and np.all(np.isfinite(scores))
        assert np.all((scores >= 0) & (scores <= 1))

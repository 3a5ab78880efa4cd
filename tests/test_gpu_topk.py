"""GPU: fused top-k candidate ranking (kernels.decoder_topk / dg_decoder_topk_f32,
evaluate.top_candidates) against a float64 numpy restatement: the full score matrix of each
relation, the permitted mask, then np.lexsort on (−score, linear index).

Exact cases use small-integer operands: every intermediate is an integer below 2^24, so fp32 is
exact under any summation order, many scores tie (some at ±0), and rows / cols / scores / counts
must equal the oracle's.  Real-valued cases are checked tolerance-aware with the project's
elementwise bar, tol(s) = 1e-4·|s| + 1e-6 (tests/test_gpu_model.py)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def tol(s):
    return 1e-4 * np.abs(s) + 1e-6


# ---------------------------------------------------------------- oracle
def oracle_scores(Ei, Ej, G, l):
    """[K, N_i, N_j] float64: (E_i ∘ l_k)·G_k·(l_k ∘ E_j)ᵀ; G [d,d] or [K,d,d]; l None, [d] or [K,d]."""
    Ei, Ej, G = np.asarray(Ei, np.float64), np.asarray(Ej, np.float64), np.asarray(G, np.float64)
    K = max(G.shape[0] if G.ndim == 3 else 1, l.shape[0] if (l is not None and np.ndim(l) == 2) else 1)
    out = []
    for k in range(K):
        Gk = G[k] if G.ndim == 3 else G
        lk = np.ones(Ei.shape[1]) if l is None else np.asarray(l[k] if np.ndim(l) == 2 else l, np.float64)
        out.append(((Ei * lk) @ Gk * lk) @ Ej.T)
    return np.stack(out)


def permitted_mask(shape, excl_pairs, upper, no_diag):
    ok = np.ones(shape, bool)
    if excl_pairs is not None and len(excl_pairs):
        e = np.asarray(excl_pairs).reshape(-1, 2)
        ok[e[:, 0], e[:, 1]] = False
    r, c = np.indices(shape)
    if upper:
        ok &= r < c
    if no_diag:
        ok &= r != c
    return ok


def oracle_topk(S, ok, topk):
    """(scores, rows, cols, count) of one relation, padded with −inf / −1."""
    lin = np.flatnonzero(ok.ravel())
    s = S.ravel()[lin]
    order = np.lexsort((lin, -s))[:topk]
    n = order.size
    sc = np.full(topk, -np.inf)
    rr = np.full(topk, -1, np.int64)
    cc = np.full(topk, -1, np.int64)
    sc[:n], rr[:n], cc[:n] = s[order], lin[order] // S.shape[1], lin[order] % S.shape[1]
    return sc, rr, cc, n


def check_exact(got, S, oks, topk):
    scores, rows, cols, counts = (t.cpu().numpy() for t in got)
    assert scores.shape == rows.shape == cols.shape == (S.shape[0], topk) and counts.shape == (S.shape[0],)
    for k in range(S.shape[0]):
        sc, rr, cc, n = oracle_topk(S[k], oks[k], topk)
        assert counts[k] == n, (k, counts[k], n)
        assert np.array_equal(rows[k], rr), k
        assert np.array_equal(cols[k], cc), k
        assert np.array_equal(scores[k].astype(np.float64), sc), k   # (−0 == +0; padding −inf)
        assert not np.any(np.signbit(scores[k][:n]) & (scores[k][:n] == 0)), "−0 returned"


def check_tolerant(got, S, oks, topk):
    """Every returned score within tol of the oracle's at the returned pair; the list
    non-increasing with the index tie-break; no permitted pair outside the list scores above the
    last returned pair by more than 2·tol.  Every relation, every slot."""
    scores, rows, cols, counts = (np.asarray(t.cpu().numpy() if hasattr(t, "cpu") else t) for t in got)
    N_j = S.shape[2]
    for k in range(S.shape[0]):
        ok = oks[k]
        n = int(counts[k])
        assert n == min(topk, int(ok.sum())), (k, n)
        r, c, s = rows[k, :n].astype(np.int64), cols[k, :n].astype(np.int64), scores[k, :n]
        assert np.all(rows[k, n:] == -1) and np.all(cols[k, n:] == -1) and np.all(np.isneginf(scores[k, n:]))
        if n == 0:
            continue
        assert r.min() >= 0 and r.max() < S.shape[1] and c.min() >= 0 and c.max() < N_j
        assert np.all(ok[r, c]), "a pair outside the permitted set was returned"
        lin = r * N_j + c
        assert np.unique(lin).size == n, "duplicate pair"
        want = S[k][r, c]
        assert np.all(np.abs(s - want) <= tol(want)), (k, np.max(np.abs(s - want) - tol(want)))
        assert np.all(np.diff(s) <= 0), "scores increase"
        tie = np.diff(s) == 0
        assert np.all(np.diff(lin)[tie] > 0), "equal scores out of index order"
        rest = ok.copy()
        rest[r, c] = False
        if rest.any():
            last = want[-1]
            assert S[k][rest].max() <= last + 2 * tol(last), (k, S[k][rest].max(), last)


def _dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


# ---------------------------------------------------------------- exact, rectangular
@pytest.fixture(scope="module")
def exact_case():
    rng = np.random.default_rng(11)
    K, Ni, Nj, d = 3, 70, 45, 32
    Ei = rng.integers(-2, 3, (Ni, d))
    Ej = rng.integers(-2, 3, (Nj, d))
    G = rng.integers(-1, 2, (K, d, d))
    l = rng.choice([-1, 1, 2], (K, d))
    # relation 0: a random exclusion whose rows 0..9, 33 and 64..69 are empty, pairs repeated and
    # unsorted; relation 1: everything but 5 pairs (in three row blocks and both column tiles);
    # relation 2: everything
    e0 = np.stack([rng.integers(0, Ni, 900), rng.integers(0, Nj, 900)], 1)
    e0 = e0[(e0[:, 0] >= 10) & (e0[:, 0] != 33) & (e0[:, 0] < 64)]
    e0 = np.concatenate([e0, e0[:50]])
    keep = {(0, 0), (31, 40), (64, 31), (69, 44), (40, 32)}
    allp = [(r, c) for r in range(Ni) for c in range(Nj)]
    e1 = np.array([p for p in allp if p not in keep])
    e2 = np.array(allp)
    excl = [e0, e1, e2]
    S = oracle_scores(Ei, Ej, G, l)
    assert np.abs(S).max() < 2**24 and np.all(S == np.round(S))
    assert np.unique(S[0]).size < S[0].size // 4 and np.any(S[0] == 0)  # many ties, some at zero
    oks = [permitted_mask((Ni, Nj), e, False, False) for e in excl]
    assert oks[1].sum() == 5 and oks[2].sum() == 0
    return Ei, Ej, G, l, excl, S, oks


@pytest.mark.parametrize("topk", [1, 7, 64, 1024])
def test_exact_rectangular(exact_case, topk):
    _need_gpu()
    from decagon_amd import kernels
    from decagon_amd.sparse import exclusion_csr

    Ei, Ej, G, l, excl, S, oks = exact_case
    ex = exclusion_csr(excl, (Ei.shape[0], Ej.shape[0]))
    got = kernels.decoder_topk(_dev(Ei), _dev(Ej), _dev(G), _dev(l), topk, exclude=ex)
    check_exact(got, S, oks, topk)
    counts = got[3].cpu().numpy()
    assert counts[1] == min(topk, 5) and counts[2] == 0
    assert np.all(np.isneginf(got[0][2].cpu().numpy())) and np.all(got[1][2].cpu().numpy() == -1)


def test_exact_two_stripes():
    """More rows than one workgroup's stripe, a row tail and a column tail, no exclusion, a shared
    G and l: the merge of lists from two workgroups, exact."""
    _need_gpu()
    from decagon_amd import kernels

    rng = np.random.default_rng(14)
    Ei, Ej = rng.integers(-2, 3, (150, 32)), rng.integers(-2, 3, (40, 32))
    G, l = rng.integers(-1, 2, (32, 32)), rng.choice([-1, 1, 2], 32)
    S = oracle_scores(Ei, Ej, G, l)
    got = kernels.decoder_topk(_dev(Ei), _dev(Ej), _dev(G), _dev(l), 64)
    check_exact(got, S, [np.ones(S.shape[1:], bool)], 64)


# ---------------------------------------------------------------- exact, square, upper
@pytest.fixture(scope="module")
def square_case():
    rng = np.random.default_rng(12)
    K, N, d = 2, 97, 64
    E = rng.integers(-1, 2, (N, d))
    G = rng.integers(-1, 2, (d, d))          # one shared G
    l = rng.choice([-1, 1], d)               # one shared l
    excl = []
    for k in range(K):
        e = np.stack([rng.integers(0, N, 700), rng.integers(0, N, 700)], 1)
        excl.append(np.concatenate([e, e[:, ::-1]]))   # symmetric
    S = np.repeat(oracle_scores(E, E, G, l), K, axis=0)
    assert np.abs(S).max() < 2**24 and np.all(S == np.round(S))
    oks = [permitted_mask((N, N), e, True, True) for e in excl]
    return E, G, l, excl, S, oks


@pytest.mark.parametrize("topk", [64, 1000])
def test_exact_square_upper(square_case, topk):
    _need_gpu()
    from decagon_amd import kernels
    from decagon_amd.sparse import exclusion_csr

    E, G, l, excl, S, oks = square_case
    Ed = _dev(E)
    got = kernels.decoder_topk(Ed, Ed, _dev(G), _dev(l), topk, exclude=exclusion_csr(excl, (E.shape[0],) * 2),
                               upper=True, no_diag=True)
    check_exact(got, S, oks, topk)
    rows, cols, counts = got[1].cpu().numpy(), got[2].cpu().numpy(), got[3].cpu().numpy()
    for k in range(len(excl)):
        n = counts[k]
        assert n == topk
        r, c = rows[k, :n], cols[k, :n]
        assert np.all(r < c), "a pair with r >= c"
        banned = set(map(tuple, excl[k].tolist()))
        assert not any((int(a), int(b)) in banned for a, b in zip(r, c)), "an excluded pair"
        assert len(set(zip(r.tolist(), c.tolist()))) == n, "a duplicate"


# ---------------------------------------------------------------- real-valued
@pytest.fixture(scope="module")
def real_case():
    rng = np.random.default_rng(13)
    K, Ni, Nj, d = 5, 130, 70, 32

    def glorot(*shape):
        a = np.sqrt(6.0 / (shape[-2] + shape[-1])) if len(shape) > 1 else np.sqrt(6.0 / (shape[0] + 1))
        return rng.uniform(-a, a, shape).astype(np.float32)

    Ei, Ej = glorot(Ni, d), glorot(Nj, d)
    G1, lK = glorot(d, d), np.stack([glorot(d) for _ in range(K)])
    GK = glorot(K, d, d)
    excl = [np.stack([rng.integers(0, Ni, 600), rng.integers(0, Nj, 600)], 1) for _ in range(K)]
    return Ei, Ej, G1, lK, GK, excl


@pytest.mark.parametrize("topk", [50, 300])
def test_real_shared_G_per_relation_l(real_case, topk):
    _need_gpu()
    from decagon_amd import kernels
    from decagon_amd.sparse import exclusion_csr

    Ei, Ej, G1, lK, GK, excl = real_case
    S = oracle_scores(Ei, Ej, G1, lK)
    oks = [permitted_mask(S.shape[1:], e, False, False) for e in excl]
    got = kernels.decoder_topk(_dev(Ei), _dev(Ej), _dev(G1), _dev(lK), topk, exclude=exclusion_csr(excl, S.shape[1:]))
    check_tolerant(got, S, oks, topk)


@pytest.mark.parametrize("topk", [50, 300])
def test_real_per_relation_G_null_l(real_case, topk):
    _need_gpu()
    from decagon_amd import kernels

    Ei, Ej, G1, lK, GK, excl = real_case
    S = oracle_scores(Ei, Ej, GK, None)
    oks = [np.ones(S.shape[1:], bool)] * S.shape[0]
    got = kernels.decoder_topk(_dev(Ei), _dev(Ej), _dev(GK), None, topk)
    check_tolerant(got, S, oks, topk)


def test_deterministic(real_case):
    """Two calls on the same inputs: byte-identical outputs."""
    _need_gpu()
    from decagon_amd import kernels
    from decagon_amd.sparse import exclusion_csr

    Ei, Ej, G1, lK, GK, excl = real_case
    ex = exclusion_csr(excl, (Ei.shape[0], Ej.shape[0]))
    args = (_dev(Ei), _dev(Ej), _dev(G1), _dev(lK), 64)
    a = kernels.decoder_topk(*args, exclude=ex)
    b = kernels.decoder_topk(*args, exclude=ex)
    for x, y in zip(a, b):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()


# ---------------------------------------------------------------- end to end
def _predictions_and_candidates(z, et, k, **kw):
    """(S [K, N_i, N_j] from sess.run(opt.predictions) per relation, the exclusion pairs, and
    evaluate.top_candidates' result) on the golden-S model, excluding the training adjacency."""
    from test_gpu_model import _setup

    from decagon_amd import evaluate

    dg, ph, model, opt, feed = _setup(z)
    sess = dg.Session()
    ets = list(model.edge_types)
    first = sum(model.edge_types[t] for t in ets[:ets.index(et)])
    K = model.edge_types[et]
    excl = [z[f"adj_{et[0]}_{et[1]}_{r}_coords"] for r in range(K)]
    S = []
    for r in range(K):
        fd = dict(feed)
        fd[ph["batch_edge_type_idx"]] = first + r
        fd[ph["batch_row_edge_type"]] = et[0]
        fd[ph["batch_col_edge_type"]] = et[1]
        S.append(np.asarray(sess.run(opt.predictions, fd), np.float64))
    got = evaluate.top_candidates(sess, opt, ph, feed, et, k, exclude=excl, **kw)
    return np.stack(S), excl, got, lambda **kw2: evaluate.top_candidates(sess, opt, ph, feed, et, k, exclude=excl, **kw2)


def test_top_candidates_matches_sorted_predictions(golden_S):
    """evaluate.top_candidates on the golden-S model, edge type (1, 1) (DEDICOM: shared R, one
    diagonal per relation), k = 50, excluding the training adjacency, against
    sess.run(opt.predictions) of each relation sorted on the host."""
    S, excl, got, again = _predictions_and_candidates(golden_S, (1, 1), 50)
    K = S.shape[0]
    oks = [permitted_mask(S.shape[1:], e, False, False) for e in excl]
    assert got[0].shape == (K, 50) and got[0].dtype == np.float32
    check_tolerant(got, S, oks, 50)
    # the sigmoid only transforms the returned scores
    sg = again(sigmoid="main")
    assert np.array_equal(sg[1], got[1]) and np.array_equal(sg[2], got[2]) and np.array_equal(sg[3], got[3])
    valid = np.arange(50)[None, :] < got[3][:, None]
    e = np.exp(-got[0][valid].astype(np.float32))
    assert np.array_equal(sg[0][valid], np.nan_to_num(1.0 / (1.0 + e.astype(np.float64))))
    assert np.all(np.isneginf(sg[0][~valid]))


def test_top_candidates_bilinear_edge_type(golden_S):
    """The same for edge type (0, 0) (Bilinear: one dense G per relation, read at stride d·d from
    the decoder's flat buffer, no diagonal), upper triangle without the diagonal."""
    S, excl, got, _ = _predictions_and_candidates(golden_S, (0, 0), 50, upper=True, no_diag=True)
    oks = [permitted_mask(S.shape[1:], e, True, True) for e in excl]
    check_tolerant(got, S, oks, 50)

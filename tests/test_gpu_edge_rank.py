"""GPU: the filtered rank of held-out edges (kernels.decoder_edge_rank / dg_decoder_edge_rank_f32,
evaluate.edge_ranks / ranking_scores_all) against a float64 numpy restatement: the full score
matrix of each relation (test_gpu_topk.oracle_scores), the permitted mask, then a count under
(−score, column) over the candidates of each query.

Exact cases use small-integer operands: every intermediate is an integer below 2^24, so fp32 is
exact under any summation order, many scores tie (some at ±0), and rank / cand / score must equal
the oracle's.  Real-valued cases are checked inside the band the project's elementwise bar,
tol(s) = 1e-4·|s| + 1e-6, leaves open: lo <= rank <= hi with lo counting the candidates surely
before the true column and hi those possibly before it; the band's own width is asserted from the
oracle alone."""
import numpy as np
import pytest
from test_gpu_topk import oracle_scores, permitted_mask, real_case, tol  # noqa: F401  (real_case: a fixture)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _dev(a, dtype=np.float32):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def _ptr(lens):
    p = np.zeros(len(lens) + 1, np.int32)
    p[1:] = np.cumsum(lens)
    return p


def _host(res):
    rank, score, cand = (t.cpu().numpy() for t in res)
    return rank, score, cand


# ---------------------------------------------------------------- oracle
def oracle_rank(S, ok, r, c, no_self=False):
    """(rank, cand, score) of the queries (r[q], c[q]) of ONE relation: S [N_i, N_j] float64, ok its
    permitted mask.  Candidates: the permitted columns of row r (without column r under no_self)
    plus c; rank = 1 + the other candidates before c under (−score, column)."""
    r, c = np.asarray(r, np.int64), np.asarray(c, np.int64)
    q = np.arange(r.size)
    others = ok[r].copy()
    if no_self:
        others[q, r] = False
    others[q, c] = False
    rows, sc = S[r], S[r, c]
    col = np.arange(S.shape[1])[None, :]
    before = (rows > sc[:, None]) | ((rows == sc[:, None]) & (col < c[:, None]))
    return 1 + (others & before).sum(1), 1 + others.sum(1), sc


def oracle_band(S, ok, r, c, no_self=False):
    """(lo, hi, cand, score): the ranks a kernel whose scores lie within tol of S may return."""
    r, c = np.asarray(r, np.int64), np.asarray(c, np.int64)
    q = np.arange(r.size)
    others = ok[r].copy()
    if no_self:
        others[q, r] = False
    others[q, c] = False
    rows, sc = S[r], S[r, c]
    t = tol(rows) + tol(sc)[:, None]
    lo = 1 + (others & (rows > sc[:, None] + t)).sum(1)
    hi = 1 + (others & (rows >= sc[:, None] - t)).sum(1)
    return lo, hi, 1 + others.sum(1), sc


# ---------------------------------------------------------------- exact cases
SEG_LENS = [33, 0, 96, 1, 7, 96, 33]
SEG_REL = [2, 0, 0, 1, 5, 1, 0]   # out of order, relations 0 and 1 repeated, 5 out of range (K = 3)
FORMS = ["shared_G_rel_l", "rel_G_null_l", "shared_G_shared_l"]


def _exact(Ni, Nj, d, seed, density, no_self=False):
    """Operands, exclusions and packed queries of one exact shape, with the oracle's answer per
    operand form — computed once per shape."""
    rng = np.random.default_rng(seed)
    K = 3
    Ei, Ej = rng.integers(-2, 3, (Ni, d)), rng.integers(-2, 3, (Nj, d))
    GK, lK = rng.integers(-1, 2, (K, d, d)), rng.choice([-1, 1, 2], (K, d))
    forms = {"shared_G_rel_l": (GK[0], lK), "rel_G_null_l": (GK, None), "shared_G_shared_l": (GK[1], lK[2])}
    # relation 0: random, rows 0..3 and 33 empty, pairs repeated and unsorted, and in rows 10..40 the
    # first, a middle and the last column of every 32-column tile; relation 1: everything but 5
    # pairs; relation 2: everything
    n0 = int(density * Ni * Nj * 1.7)
    e0 = np.stack([rng.integers(0, Ni, n0), rng.integers(0, Nj, n0)], 1)
    e0 = e0[(e0[:, 0] >= 4) & (e0[:, 0] != 33)]
    edge = np.unique(np.minimum(np.add.outer(32 * np.arange((Nj + 31) // 32), [0, 15, 31]).ravel(), Nj - 1))
    tiles = np.stack(np.meshgrid(np.arange(10, 41), edge, indexing="ij"), -1).reshape(-1, 2)
    e0 = np.concatenate([e0, e0[:50], tiles[(tiles[:, 0] != 33)]])
    keep = {(0, 0), (31, 40), (64, 31), (69, Nj - 1), (40, 32)}
    allp = np.stack(np.meshgrid(np.arange(Ni), np.arange(Nj), indexing="ij"), -1).reshape(-1, 2)
    e1 = allp[[tuple(p) not in keep for p in allp.tolist()]]
    excl = [e0, e1, allp]
    oks = np.stack([permitted_mask((Ni, Nj), e, False, False) for e in excl])
    assert oks[1].sum() == 5 and oks[2].sum() == 0 and not oks[0][10:33].all(1).any() and oks[0][[0, 33]].all()

    # queries: random pairs; in relation 0's segments every other one is itself excluded (as every
    # query of relations 1 and 2 nearly is); under no_self some have c == r
    n = sum(SEG_LENS)
    r, c = rng.integers(0, Ni, n), rng.integers(0, Nj, n)
    ptr = _ptr(SEG_LENS)
    for s, k in enumerate(SEG_REL):
        if k == 0:
            pick = e0[rng.integers(0, len(e0), SEG_LENS[s])]
            sl = slice(ptr[s], ptr[s + 1], 2)
            r[sl], c[sl] = pick[::2, 0][:len(r[sl])], pick[::2, 1][:len(c[sl])]
    if no_self:
        c[5::7] = r[5::7]
    bad = [ptr[2] + 40, ptr[5] + 3, ptr[5] + 95]  # one index past each table, one negative
    r[bad[0]], c[bad[1]], r[bad[2]] = Ni, Nj, -1

    want = {}
    for name, (G, l) in forms.items():
        S = oracle_scores(Ei, Ej, G, l)
        if S.shape[0] == 1:
            S = np.repeat(S, K, axis=0)
        assert np.abs(S).max() < 2**24 and np.all(S == np.round(S))  # fp32 is exact
        assert np.unique(S[0]).size < S[0].size // 3 and np.any(S[0] == 0)  # many ties, some at zero
        rank, cand, score = np.zeros(n, np.int64), np.zeros(n, np.int64), np.full(n, np.nan)
        for s, k in enumerate(SEG_REL):
            if k >= K or SEG_LENS[s] == 0:
                continue
            sl = np.arange(ptr[s], ptr[s + 1])
            sl = sl[~np.isin(sl, bad)]
            rank[sl], cand[sl], score[sl] = oracle_rank(S[k], oks[k], r[sl], c[sl], no_self)
        want[name] = (rank, cand, score)
    return dict(Ei=Ei, Ej=Ej, forms=forms, excl=excl, oks=oks, r=r, c=c, ptr=ptr, want=want, no_self=no_self, K=K)


SHAPES = {"70x45_d32": (70, 45, 32, 31, 0.8), "70x45_d64": (70, 45, 64, 32, 0.8),
          "70x1057_d32": (70, 1057, 32, 33, 0.3), "70x70_d32_no_self": (70, 70, 32, 34, 0.5, True),
          # 69 column tiles: unsplit, a wave's run of 17 or 18 tiles is longer than the 16 whose masks it builds at once
          "70x2200_d32": (70, 2200, 32, 35, 0.3)}


@pytest.fixture(scope="module", params=list(SHAPES))
def exact_rank_case(request):
    return _exact(*SHAPES[request.param])


def _run_exact(case, form, **kw):
    from decagon_amd import kernels
    from decagon_amd.sparse import exclusion_csr

    G, l = case["forms"][form]
    ex = exclusion_csr(case["excl"], (case["Ei"].shape[0], case["Ej"].shape[0]))
    return kernels.decoder_edge_rank(_dev(case["Ei"]), _dev(case["Ej"]), _dev(case["r"], np.int32),
                                     _dev(case["c"], np.int32), _dev(case["ptr"], np.int32), _dev(G),
                                     None if l is None else _dev(l), seg_rel=_dev(SEG_REL, np.int32), exclude=ex,
                                     no_self=case["no_self"], **kw)


@pytest.mark.parametrize("form", FORMS)
def test_exact(exact_rank_case, form):
    """rank, cand and score equal the oracle's: partial row and column tiles, d = 32 and 64, a walk
    of 34 column tiles dealt over splits and waves, every exclusion form, segments of 0, 1, 33 and
    96 queries through an out-of-order map, queries that are themselves excluded."""
    case = exact_rank_case
    want_rank, want_cand, want_score = case["want"][form]
    ptr = case["ptr"]
    for split in (True, False):
        rank, score, cand = _host(_run_exact(case, form, column_split=split))
        assert rank.dtype == cand.dtype == np.int32 and score.dtype == np.float32
        assert np.array_equal(rank, want_rank), (split, np.flatnonzero(rank != want_rank)[:8])
        assert np.array_equal(cand, want_cand), (split, np.flatnonzero(cand != want_cand)[:8])
        assert np.array_equal(score.astype(np.float64), want_score, equal_nan=True), split
        assert not np.any(np.signbit(score) & (score == 0)), "−0 returned"
    live = want_rank > 0
    assert np.all((1 <= rank[live]) & (rank[live] <= cand[live]))
    # the out-of-range relation and the three out-of-range indices: rank 0, cand 0, NaN
    dead = np.flatnonzero(~live)
    assert dead.size == SEG_LENS[4] + 3 and set(range(ptr[4], ptr[5])) <= set(dead.tolist())
    assert np.all(rank[dead] == 0) and np.all(cand[dead] == 0) and np.all(np.isnan(score[dead]))
    # relation 2 excludes everything: the true column alone
    everything = np.concatenate([np.arange(ptr[s], ptr[s + 1]) for s, k in enumerate(SEG_REL) if k == 2])
    assert np.all(rank[everything] == 1) and np.all(cand[everything] == 1)
    if case["no_self"]:
        q = np.flatnonzero(live & (case["r"] == case["c"]))
        assert q.size >= 10  # c == r stays a candidate: it is the query's own column


def test_outputs_may_be_absent_and_no_exclusion():
    """Without an exclusion, a map or per-relation operands every column is a candidate, and the
    call works with out_score / out_cand NULL."""
    from decagon_amd import _lib

    case = _exact(*SHAPES["70x45_d32"])
    G, l = case["forms"]["shared_G_shared_l"]
    S = oracle_scores(case["Ei"], case["Ej"], G, l)[0]
    n = int(case["ptr"][2])  # the first two segments: in-range queries only
    r, c = case["r"][:n], case["c"][:n]
    want_rank, want_cand, _ = oracle_rank(S, np.ones(S.shape, bool), r, c)
    Ei, Ej, Gd, ld = _dev(case["Ei"]), _dev(case["Ej"]), _dev(G), _dev(l)
    ri, ci, ptr = _dev(r, np.int32), _dev(c, np.int32), _dev(case["ptr"][:3], np.int32)
    rank = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    rc = _lib.load().dg_decoder_edge_rank_f32(*_lib.pack(
        "dg_decoder_edge_rank_f32", row_table=Ei.data_ptr(), ld_row=32, n_rows=70, col_table=Ej.data_ptr(), ld_col=32,
        n_cols=45, row_idx=ri.data_ptr(), col_idx=ci.data_ptr(), seg_ptr=ptr.data_ptr(), seg_rel=None, n_seg=2,
        n_queries=n, G=Gd.data_ptr(), g_stride=0, l=ld.data_ptr(), l_stride=0, n_rel=1, d=32, excl_rowptr=None,
        excl_col=None, flags=0, out_rank=rank.data_ptr(), out_score=None, out_cand=None,
        stream=torch.cuda.current_stream().cuda_stream))
    assert rc == _lib.DG_OK
    torch.cuda.synchronize()
    assert np.array_equal(rank.cpu().numpy(), want_rank) and np.all(want_cand == 45)


# ---------------------------------------------------------------- agreement with decoder_topk
def test_agrees_with_decoder_topk():
    """With topk = the number of permitted pairs, decoder_topk's list of a relation holds every
    row's candidates in order: decoder_edge_rank of a returned pair is 1 + the earlier entries of
    its row, with the same score bits."""
    from decagon_amd import kernels
    from decagon_amd.sparse import exclusion_csr

    case = _exact(*SHAPES["70x45_d32"])
    G, l = case["forms"]["shared_G_rel_l"]
    n_ok = case["oks"].sum((1, 2))
    topk = int(n_ok.max())
    assert 500 < topk <= 1024 and n_ok.tolist()[1:] == [5, 0]
    ex = exclusion_csr(case["excl"], (70, 45))
    Ei, Ej, Gd, ld = _dev(case["Ei"]), _dev(case["Ej"]), _dev(G), _dev(l)
    scores, rows, cols, counts = (t.cpu().numpy() for t in kernels.decoder_topk(Ei, Ej, Gd, ld, topk, exclude=ex))
    assert counts.tolist() == n_ok.tolist()
    r = np.concatenate([rows[k, :counts[k]] for k in range(3)])
    c = np.concatenate([cols[k, :counts[k]] for k in range(3)])
    want_rank = np.concatenate([[1 + int(np.sum(rows[k, :t] == rows[k, t])) for t in range(counts[k])] for k in range(3)])
    want_bits = np.concatenate([scores[k, :counts[k]] for k in range(3)]).view(np.uint32)
    rank, score, cand = _host(kernels.decoder_edge_rank(Ei, Ej, _dev(r, np.int32), _dev(c, np.int32),
                                                        _dev(_ptr(counts), np.int32), Gd, ld, exclude=ex))
    assert np.array_equal(rank, want_rank)
    assert np.array_equal(score.view(np.uint32), want_bits)
    per_row = np.concatenate([case["oks"][k][rows[k, :counts[k]]].sum(1) for k in range(3)])
    assert np.array_equal(cand, per_row)


# ---------------------------------------------------------------- real-valued
REAL_FORMS = {"shared_G_rel_l": 0.95, "rel_G_null_l": 0.95}  # the share of queries whose band must be one rank wide


@pytest.fixture(scope="module")
def real_rank_case(real_case):
    """400 random queries per relation on test_gpu_topk's real case, with its random exclusions, and
    the oracle's band per operand form."""
    Ei, Ej, G1, lK, GK, excl = real_case
    rng = np.random.default_rng(21)
    K, n = 5, 400
    r, c = rng.integers(0, Ei.shape[0], K * n), rng.integers(0, Ej.shape[0], K * n)
    oks = [permitted_mask((Ei.shape[0], Ej.shape[0]), e, False, False) for e in excl]
    bands = {}
    for name, (G, l) in {"shared_G_rel_l": (G1, lK), "rel_G_null_l": (GK, None)}.items():
        S = oracle_scores(Ei, Ej, G, l)
        parts = [oracle_band(S[k], oks[k], r[k * n:(k + 1) * n], c[k * n:(k + 1) * n]) for k in range(K)]
        bands[name] = tuple(np.concatenate([p[t] for p in parts]) for t in range(4))
    return dict(Ei=Ei, Ej=Ej, forms={"shared_G_rel_l": (G1, lK), "rel_G_null_l": (GK, None)}, excl=excl, r=r, c=c,
                ptr=_ptr([n] * K), bands=bands)


def _run_real(case, form, r=None, c=None, ptr=None, rel=None):
    from decagon_amd import kernels
    from decagon_amd.sparse import exclusion_csr

    G, l = case["forms"][form]
    ex = exclusion_csr(case["excl"], (case["Ei"].shape[0], case["Ej"].shape[0]))
    r, c, ptr = (case[nm] if v is None else v for nm, v in (("r", r), ("c", c), ("ptr", ptr)))
    return kernels.decoder_edge_rank(_dev(case["Ei"]), _dev(case["Ej"]), _dev(r, np.int32), _dev(c, np.int32),
                                     _dev(ptr, np.int32), _dev(G), None if l is None else _dev(l),
                                     seg_rel=None if rel is None else _dev(rel, np.int32), exclude=ex)


def check_band(got, band, sure, max_width=1):
    """score within tol, cand exact, lo <= rank <= hi; and, from the oracle alone, the band one rank
    wide for at least `sure` of the queries and nowhere wider than max_width."""
    rank, score, cand = got
    lo, hi, want_cand, want_score = band
    print(f"band: lo == hi for {np.mean(lo == hi):.4f} of {lo.size} queries, widest {int((hi - lo).max())}; "
          f"score error / tol at most {np.max(np.abs(score - want_score) / tol(want_score)):.3f}")
    assert np.mean(lo == hi) >= sure and (max_width is None or (hi - lo).max() <= max_width)
    assert np.all(np.abs(score - want_score) <= tol(want_score))
    assert np.array_equal(cand, want_cand)
    assert np.all((lo <= rank) & (rank <= hi)), np.flatnonzero((rank < lo) | (rank > hi))[:8]


@pytest.mark.parametrize("form", list(REAL_FORMS))
def test_real_valued(real_rank_case, form):
    case = real_rank_case
    check_band(_host(_run_real(case, form)), case["bands"][form], REAL_FORMS[form], max_width=None)


def test_position_independent(real_rank_case):
    """A query's three outputs do not depend on its place: the queries permuted within their
    segments, every segment cut into two of the same relation, and two identical calls."""
    case = real_rank_case
    rng = np.random.default_rng(22)
    K, n = 5, 400
    base = [x.tobytes() for x in _host(_run_real(case, "shared_G_rel_l"))]
    again = [x.tobytes() for x in _host(_run_real(case, "shared_G_rel_l"))]
    assert base == again
    perm = np.concatenate([k * n + rng.permutation(n) for k in range(K)])
    cut = _ptr([137, n - 137] * K)
    rel = np.repeat(np.arange(K), 2)
    got = _host(_run_real(case, "shared_G_rel_l", case["r"][perm], case["c"][perm], cut, rel))
    ref = _host(_run_real(case, "shared_G_rel_l"))
    for g, b in zip(got, ref):
        assert g.tobytes() == b[perm].tobytes()


def test_captures_into_a_graph(real_rank_case):
    """The call reads nothing on the host: captured into one graph, its replays give the eager
    call's bytes."""
    from decagon_amd import kernels
    from decagon_amd.sparse import exclusion_csr

    case = real_rank_case
    G, l = case["forms"]["shared_G_rel_l"]
    ex = exclusion_csr(case["excl"], (case["Ei"].shape[0], case["Ej"].shape[0]))
    exd = (_dev(ex.rowptr, np.int32), _dev(ex.col, np.int32))
    args = (_dev(case["Ei"]), _dev(case["Ej"]), _dev(case["r"], np.int32), _dev(case["c"], np.int32),
            _dev(case["ptr"], np.int32), _dev(G), _dev(l))

    def run():
        return kernels.decoder_edge_rank(*args, exclude=exd)

    eager = [t.clone() for t in run()]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = run()
    for _ in range(2):
        for t in out:
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        for a, b in zip(out, eager):
            assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


# ---------------------------------------------------------------- through the model
def _positives(z, et, K, empty, n=300, seed=6):
    rng = np.random.default_rng(seed)
    pos = {}
    for k in range(K):
        if k != empty:
            co = z[f"adj_{et[0]}_{et[1]}_{k}_coords"]
            pos[k] = co[rng.choice(len(co), min(n, len(co)), replace=False)]
    return {et: pos}


@pytest.mark.parametrize("et,empty,no_self", [((1, 1), 4, True), ((0, 0), 0, False)], ids=["dedicom", "bilinear"])
def test_edge_ranks_through_the_model(golden_S, et, empty, no_self):
    from test_gpu_model import _setup

    from decagon_amd import evaluate, kernels
    from decagon_amd.graph import Node
    from decagon_amd.sparse import exclusion_csr

    z = golden_S
    dg, ph, model, opt, feed = _setup(z)
    sess = dg.Session()
    K = model.edge_types[et]
    ets = list(model.edge_types)
    first = sum(model.edge_types[t] for t in ets[:ets.index(et)])
    edges = _positives(z, et, K, empty)
    excl = [z[f"adj_{et[0]}_{et[1]}_{k}_coords"] for k in range(K)]
    res = evaluate.edge_ranks(sess, opt, ph, feed, edges, et, exclude=excl, side="both", no_self=no_self)
    assert res["relations"].tolist() == list(range(K))
    lens = [len(edges[et].get(k, ())) for k in range(K)]
    assert res["seg_ptr"].tolist() == _ptr(lens).tolist() and lens[empty] == 0
    r = np.concatenate([edges[et][k][:, 0] for k in range(K) if k != empty])
    c = np.concatenate([edges[et][k][:, 1] for k in range(K) if k != empty])

    # byte for byte the kernel wrapper on the optimizer's tables and the stacked latents
    def direct(ctx):
        _, row_t, col_t, G, l = evaluate._edge_type_operands("test", ctx, opt, model, et)
        ex = exclusion_csr(excl, (row_t.shape[0], col_t.shape[0]))
        ptr, rel = _dev(res["seg_ptr"], np.int32), _dev(np.arange(K), np.int32)
        a = kernels.decoder_edge_rank(row_t, col_t, _dev(r, np.int32), _dev(c, np.int32), ptr, G, l, seg_rel=rel,
                                      exclude=ex, no_self=no_self)
        b = kernels.decoder_edge_rank(col_t, row_t, _dev(c, np.int32), _dev(r, np.int32), ptr,
                                      G.transpose(-1, -2).contiguous(), l, seg_rel=rel, exclude=ex.transposed(),
                                      no_self=no_self)
        return torch.cat([t.view(torch.int32) for t in a + b])

    flat = np.asarray(sess.run(Node("test/edge_rank_direct", direct), feed_dict=feed), np.int32).reshape(6, -1)
    for t, (sd, nm) in enumerate((sd, nm) for sd in ("col", "row") for nm in ("rank", "score", "cand")):
        assert res[sd][nm].tobytes() == flat[t].tobytes(), (sd, nm)

    # against sess.run(opt.predictions) of every relation, in float64
    ptr = res["seg_ptr"]
    for k in range(K):
        if k == empty:
            continue
        fd = dict(feed)
        fd[ph["batch_edge_type_idx"]] = first + k
        fd[ph["batch_row_edge_type"]] = et[0]
        fd[ph["batch_col_edge_type"]] = et[1]
        S = np.asarray(sess.run(opt.predictions, fd), np.float64)
        ok = permitted_mask(S.shape, excl[k], False, False)
        e = edges[et][k]
        for sd, Sx, okx, rq, cq in (("col", S, ok, e[:, 0], e[:, 1]), ("row", S.T, ok.T, e[:, 1], e[:, 0])):
            got = tuple(res[sd][nm][ptr[k]:ptr[k + 1]] for nm in ("rank", "score", "cand"))
            check_band(got, oracle_band(Sx, okx, rq, cq, no_self), 0.70, max_width=4)

    # the metrics: ranking_metrics of those ranks, a subset out of order, pooled, the empty relation
    both = [np.concatenate([res[sd]["rank"][ptr[k]:ptr[k + 1]] for sd in ("col", "row")]) for k in range(K)]
    want = evaluate.ranking_metrics(np.concatenate(both), _ptr([b.size for b in both]))
    kw = dict(exclude=excl, side="both", no_self=no_self)
    rows, pooled = evaluate.ranking_scores_all(sess, opt, ph, feed, edges, et, pooled=True, **kw)
    assert rows.shape == (K, 5) and np.array_equal(rows, want, equal_nan=True) and np.all(np.isnan(rows[empty]))
    live = [k for k in range(K) if k != empty]
    assert np.all((0 < rows[live, 0]) & (rows[live, 0] <= 1) & (rows[live, 1] >= 1))
    assert np.array_equal(pooled, evaluate.ranking_metrics(np.concatenate(both), [0, sum(b.size for b in both)])[0])
    sub = [K - 1, empty, 1] if empty != 1 else [K - 1, empty, 0]
    assert np.array_equal(evaluate.ranking_scores_all(sess, opt, ph, feed, edges, et, relations=sub, **kw), want[sub],
                          equal_nan=True)
    col_only = evaluate.ranking_scores_all(sess, opt, ph, feed, edges, et, exclude=excl, no_self=no_self, hits=(5,))
    assert np.array_equal(col_only, evaluate.ranking_metrics(res["col"]["rank"], ptr, hits=(5,)), equal_nan=True)

    # refusals
    fdl = dict(feed)
    fdl[opt.latent_varies[first + 1]] = np.eye(int(z[f"emb_{et[0]}"].shape[1]), dtype=np.float32)
    with pytest.raises(dg.InvalidArgumentError, match="latent matrix is fed"):
        evaluate.edge_ranks(sess, opt, ph, fdl, edges, et)
    with pytest.raises(ValueError, match="unknown edge type"):
        evaluate.edge_ranks(sess, opt, ph, feed, edges, (5, 5))
    bad = {et: {1: np.array([[0, S.shape[1]]])}}
    with pytest.raises(ValueError, match="outside the embedding tables"):
        evaluate.edge_ranks(sess, opt, ph, feed, bad, et)
    sess.shard = object()
    with pytest.raises(NotImplementedError):
        evaluate.edge_ranks(sess, opt, ph, feed, edges, et)
    sess.shard = None

"""GPU: a node's best partners per relation (kernels.decoder_node_topk / dg_decoder_node_topk_f32,
evaluate.top_partners) against a float64 numpy restatement: the full score matrix of each relation
(test_gpu_topk.oracle_scores), the permitted mask, then per query row np.lexsort on
(−score, column).

Exact cases use test_gpu_edge_rank's small-integer operands: every intermediate is an integer
below 2^24, so fp32 is exact under any summation order, many scores tie (some at ±0), and scores,
columns and counts must equal the oracle's.  Real-valued cases are checked per row with
test_gpu_topk.check_tolerant's contract under the project's elementwise bar,
tol(s) = 1e-4·|s| + 1e-6: every query and every slot."""
import numpy as np
import pytest
from test_gpu_edge_rank import FORMS, SEG_LENS, SEG_REL, SHAPES, _dev, _exact, _ptr
from test_gpu_topk import oracle_scores, permitted_mask, real_case, tol  # noqa: F401  (real_case: a fixture)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TOPKS = [1, 7, 32, 33, 64, 128]  # list capacities 64, 128 and 256; k > n_cols and k > permitted both occur
MAX_K = 128


def _host(res):
    scores, cols, counts = (t.cpu().numpy() for t in res)
    return scores, cols, counts


# ---------------------------------------------------------------- oracle
def oracle_rows(S_rows, ok_rows, kmax=MAX_K):
    """(scores [n, kmax] float64, cols [n, kmax], permitted [n]) of query rows: S_rows [n, N_j]
    float64, ok_rows its permitted mask; each row's permitted columns under (−score, column),
    padded with −inf / −1."""
    n = S_rows.shape[0]
    sc, cc = np.full((n, kmax), -np.inf), np.full((n, kmax), -1, np.int64)
    for q in range(n):
        cols = np.flatnonzero(ok_rows[q])
        order = cols[np.lexsort((cols, -S_rows[q, cols]))][:kmax]
        sc[q, :order.size], cc[q, :order.size] = S_rows[q, order], order
    return sc, cc, ok_rows.sum(1)


def check_rows_tolerant(got, S_rows, ok_rows, k):
    """test_gpu_topk.check_tolerant's contract per query row: every returned score within tol of
    the oracle's at the returned column; the list non-increasing, ties by ascending column; no
    duplicate, nothing excluded; no permitted column outside the list scores above the last
    returned one by more than 2·tol.  Every query, every slot."""
    scores, cols, counts = got
    n, N_j = S_rows.shape
    assert scores.shape == cols.shape == (n, k) and counts.shape == (n,)
    assert np.array_equal(counts, np.minimum(k, ok_rows.sum(1)))
    worst = 0.0
    for q in range(n):
        m = int(counts[q])
        c, s = cols[q, :m].astype(np.int64), scores[q, :m]
        assert np.all(cols[q, m:] == -1) and np.all(np.isneginf(scores[q, m:])), q
        if m == 0:
            continue
        assert c.min() >= 0 and c.max() < N_j and np.all(ok_rows[q, c]), (q, "a column outside the permitted set")
        assert np.unique(c).size == m, (q, "duplicate column")
        want = S_rows[q, c]
        worst = max(worst, float(np.max(np.abs(s - want) / tol(want))))
        assert np.all(np.abs(s - want) <= tol(want)), (q, np.max(np.abs(s - want) - tol(want)))
        assert np.all(np.diff(s) <= 0), (q, "scores increase")
        assert np.all(np.diff(c)[np.diff(s) == 0] > 0), (q, "equal scores out of column order")
        rest = ok_rows[q].copy()
        rest[c] = False
        if rest.any():
            last = want[-1]
            assert S_rows[q][rest].max() <= last + 2 * tol(last), (q, S_rows[q][rest].max(), last)
    print(f"k = {k}: {n} rows, score error / tol at most {worst:.3f}")


# ---------------------------------------------------------------- exact cases
@pytest.fixture(scope="module", params=list(SHAPES))
def exact_partner_case(request):
    """test_gpu_edge_rank's exact shape with its row nodes as the queries — one at n_rows and one at
    −1 already — and one more made the duplicate of another query of its segment; the oracle's
    lists per operand form, computed once per shape."""
    case = _exact(*SHAPES[request.param])
    Ni, K, ptr = case["Ei"].shape[0], case["K"], case["ptr"]
    r = case["r"].copy()
    twin = (int(ptr[2]) + 7, int(ptr[2]) + 61)  # in a segment of relation 0
    r[twin[1]] = r[twin[0]]
    assert np.sum(r == Ni) == 1 and np.sum(r == -1) == 1 and 0 <= r[twin[0]] < Ni and SEG_REL[2] == 0
    live = np.zeros(r.size, bool)
    rel = np.zeros(r.size, np.int64)
    for s, k in enumerate(SEG_REL):
        rel[ptr[s]:ptr[s + 1]] = k
        live[ptr[s]:ptr[s + 1]] = k < K
    live &= (r >= 0) & (r < Ni)
    want = {}
    for name, (G, l) in case["forms"].items():
        S = oracle_scores(case["Ei"], case["Ej"], G, l)
        if S.shape[0] == 1:
            S = np.repeat(S, K, axis=0)
        rows = np.zeros((r.size, S.shape[2]))
        ok = np.zeros((r.size, S.shape[2]), bool)
        rows[live], ok[live] = S[rel[live], r[live]], case["oks"][rel[live], r[live]]
        if case["no_self"]:
            ok[np.flatnonzero(live), r[live]] = False
        want[name] = oracle_rows(rows, ok)
    return dict(case, r=r, twin=twin, live=live, rel=rel, want=want)


def _run_exact(case, form, topk, **kw):
    from decagon_amd import kernels
    from decagon_amd.sparse import exclusion_csr

    G, l = case["forms"][form]
    if "ex" not in case:  # (built once per shape)
        case["ex"] = exclusion_csr(case["excl"], (case["Ei"].shape[0], case["Ej"].shape[0]))
    ex = case["ex"]
    return kernels.decoder_node_topk(_dev(case["Ei"]), _dev(case["Ej"]), _dev(case["r"], np.int32),
                                     _dev(case["ptr"], np.int32), _dev(G), None if l is None else _dev(l), topk,
                                     seg_rel=_dev(SEG_REL, np.int32), exclude=ex, no_self=case["no_self"], **kw)


@pytest.mark.parametrize("form", FORMS)
def test_exact(exact_partner_case, form):
    """scores, columns and counts equal the oracle's: partial row and column tiles, d = 32 and 64,
    walks of 34 and 69 column tiles dealt over waves and splits, every exclusion form, segments of
    0, 1, 33 and 96 queries through an out-of-order map, every list capacity."""
    case = exact_partner_case
    want_s, want_c, permitted = case["want"][form]
    ptr, live = case["ptr"], case["live"]
    n_cols = case["Ej"].shape[0]
    assert permitted.max() <= n_cols and (n_cols < 128 or permitted.max() > 128) and permitted[live].min() == 0
    for topk in TOPKS:
        for split in (True, False):
            scores, cols, counts = _host(_run_exact(case, form, topk, column_split=split))
            tag = (topk, split)
            assert scores.dtype == np.float32 and cols.dtype == counts.dtype == np.int32
            assert scores.shape == cols.shape == (live.size, topk) and counts.shape == (live.size,)
            assert np.array_equal(counts, np.minimum(topk, permitted)), (tag, np.flatnonzero(counts != np.minimum(topk, permitted))[:8])
            assert np.array_equal(cols, want_c[:, :topk]), (tag, np.flatnonzero((cols != want_c[:, :topk]).any(1))[:8])
            assert np.array_equal(scores.astype(np.float64), want_s[:, :topk]), tag  # (padding −inf)
            assert not np.any(np.signbit(scores) & (scores == 0)), "−0 returned"
            pad = np.arange(topk)[None, :] >= counts[:, None]
            assert np.all(cols[pad] == -1) and np.all(np.isneginf(scores[pad])) and np.all(cols[~pad] >= 0)
            # the out-of-range relation and the two out-of-range nodes: count 0
            dead = np.flatnonzero(~live)
            assert dead.size == SEG_LENS[4] + 2 and set(range(ptr[4], ptr[5])) <= set(dead.tolist())
            assert np.all(counts[dead] == 0)
            # relation 2 excludes everything
            everything = np.flatnonzero(case["rel"] == 2)
            assert everything.size == SEG_LENS[0] and np.all(counts[everything] == 0)
            # the duplicate query: its twin's bytes
            a, b = case["twin"]
            assert counts[a] == counts[b] == min(topk, permitted[a]) > 0
            assert scores[a].tobytes() == scores[b].tobytes() and cols[a].tobytes() == cols[b].tobytes()
    if case["no_self"]:
        q = np.flatnonzero(live)
        assert not np.any(want_c[q] == case["r"][q][:, None])


def test_agrees_with_decoder_topk():
    """With topk = the number of permitted pairs, decoder_topk's list of a relation holds every
    row's permitted columns in order: each row's entries, in order, are this kernel's list for that
    row, with the same score bits."""
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
    nodes = np.tile(np.arange(70), 3)
    got_s, got_c, got_n = _host(kernels.decoder_node_topk(Ei, Ej, _dev(nodes, np.int32), _dev(_ptr([70] * 3), np.int32),
                                                          Gd, ld, 45, exclude=ex))
    for k in range(3):
        for r in range(70):
            sel = np.flatnonzero(rows[k, :counts[k]] == r)
            q = 70 * k + r
            assert got_n[q] == sel.size == case["oks"][k][r].sum(), (k, r)
            assert np.array_equal(got_c[q, :sel.size], cols[k, sel]), (k, r)
            assert got_s[q, :sel.size].tobytes() == scores[k, sel].tobytes(), (k, r)


# ---------------------------------------------------------------- real-valued
REAL_K = 5


@pytest.fixture(scope="module")
def real_partner_case(real_case):
    """Every node of test_gpu_topk's real case as a query of every relation, with its random
    exclusions, and the oracle's score rows per operand form."""
    Ei, Ej, G1, lK, GK, excl = real_case
    Ni, Nj = Ei.shape[0], Ej.shape[0]
    oks = np.stack([permitted_mask((Ni, Nj), e, False, False) for e in excl])
    forms = {"shared_G_rel_l": (G1, lK), "rel_G_null_l": (GK, None)}
    rows = {name: oracle_scores(Ei, Ej, G, l).reshape(REAL_K * Ni, Nj) for name, (G, l) in forms.items()}
    return dict(Ei=Ei, Ej=Ej, forms=forms, excl=excl, r=np.tile(np.arange(Ni), REAL_K), ptr=_ptr([Ni] * REAL_K),
                rows=rows, ok=oks.reshape(REAL_K * Ni, Nj))


def _run_real(case, form, topk, r=None, ptr=None, rel=None, exclude=None):
    from decagon_amd import kernels
    from decagon_amd.sparse import exclusion_csr

    G, l = case["forms"][form]
    ex = exclusion_csr(case["excl"], (case["Ei"].shape[0], case["Ej"].shape[0])) if exclude is None else exclude
    r, ptr = (case[nm] if v is None else v for nm, v in (("r", r), ("ptr", ptr)))
    return kernels.decoder_node_topk(_dev(case["Ei"]), _dev(case["Ej"]), _dev(r, np.int32), _dev(ptr, np.int32),
                                     _dev(G), None if l is None else _dev(l), topk,
                                     seg_rel=None if rel is None else _dev(rel, np.int32), exclude=ex)


@pytest.mark.parametrize("topk", [10, 50])
@pytest.mark.parametrize("form", ["shared_G_rel_l", "rel_G_null_l"])
def test_real_valued(real_partner_case, form, topk):
    case = real_partner_case
    check_rows_tolerant(_host(_run_real(case, form, topk)), case["rows"][form], case["ok"], topk)


def test_agrees_with_decoder_edge_rank(real_partner_case):
    """Every returned (node, partner at position t), fed to decoder_edge_rank with the same
    exclusion: rank t + 1, the same score bits, cand = the row's permitted count."""
    from decagon_amd import kernels
    from decagon_amd.sparse import exclusion_csr

    case = real_partner_case
    topk = 50
    G, l = case["forms"]["shared_G_rel_l"]
    ex = exclusion_csr(case["excl"], (case["Ei"].shape[0], case["Ej"].shape[0]))
    scores, cols, counts = _host(_run_real(case, "shared_G_rel_l", topk))
    permitted = case["ok"].sum(1)
    assert np.array_equal(counts, np.minimum(topk, permitted)) and counts.min() > 0
    valid = np.arange(topk)[None, :] < counts[:, None]
    q, t = np.nonzero(valid)  # row-major: by query, then by position — the relations stay contiguous
    lens = [int(counts[case["ptr"][k]:case["ptr"][k + 1]].sum()) for k in range(REAL_K)]
    rank, score, cand = (x.cpu().numpy() for x in kernels.decoder_edge_rank(
        _dev(case["Ei"]), _dev(case["Ej"]), _dev(case["r"][q], np.int32), _dev(cols[q, t], np.int32),
        _dev(_ptr(lens), np.int32), _dev(G), _dev(l), exclude=ex))
    assert np.array_equal(rank, t + 1)
    assert score.tobytes() == scores[q, t].tobytes()
    assert np.array_equal(cand, permitted[q])


def test_position_independent(real_partner_case):
    """A query's outputs do not depend on its place: the queries permuted within their segments,
    every segment cut into two of the same relation, and two identical calls."""
    case = real_partner_case
    rng = np.random.default_rng(23)
    n = case["Ei"].shape[0]
    base = [x.tobytes() for x in _host(_run_real(case, "shared_G_rel_l", 10))]
    again = [x.tobytes() for x in _host(_run_real(case, "shared_G_rel_l", 10))]
    assert base == again
    perm = np.concatenate([k * n + rng.permutation(n) for k in range(REAL_K)])
    cut = _ptr([37, n - 37] * REAL_K)
    rel = np.repeat(np.arange(REAL_K), 2)
    ref = _host(_run_real(case, "shared_G_rel_l", 10))
    got = _host(_run_real(case, "shared_G_rel_l", 10, case["r"][perm], case["ptr"]))
    for g, b in zip(got, ref):
        assert g.tobytes() == b[perm].tobytes()
    got = _host(_run_real(case, "shared_G_rel_l", 10, case["r"][perm], cut, rel))
    for g, b in zip(got, ref):
        assert g.tobytes() == b[perm].tobytes()


def test_captures_into_a_graph(real_partner_case):
    """The call reads nothing on the host: captured into one graph, its replays give the eager
    call's bytes."""
    from decagon_amd import kernels
    from decagon_amd.sparse import exclusion_csr

    case = real_partner_case
    G, l = case["forms"]["shared_G_rel_l"]
    ex = exclusion_csr(case["excl"], (case["Ei"].shape[0], case["Ej"].shape[0]))
    exd = (_dev(ex.rowptr, np.int32), _dev(ex.col, np.int32))
    args = (_dev(case["Ei"]), _dev(case["Ej"]), _dev(case["r"], np.int32), _dev(case["ptr"], np.int32), _dev(G),
            _dev(l), 10)

    def run():
        return kernels.decoder_node_topk(*args, exclude=exd)

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
@pytest.mark.parametrize("et,empty,no_self", [((1, 1), 4, True), ((0, 0), 0, False)], ids=["dedicom", "bilinear"])
def test_top_partners_through_the_model(golden_S, et, empty, no_self):
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
    N = int(z[f"emb_{et[0]}"].shape[0])
    k = 10
    rng = np.random.default_rng(8)
    nodes = rng.choice(N, min(N, 40), replace=False)
    excl = [z[f"adj_{et[0]}_{et[1]}_{r}_coords"] for r in range(K)]
    kw = dict(exclude=excl, no_self=no_self)
    res = evaluate.top_partners(sess, opt, ph, feed, nodes, et, k, side="both", **kw)
    n = nodes.size
    assert res["relations"].tolist() == list(range(K)) and res["seg_ptr"].tolist() == _ptr([n] * K).tolist()
    assert res["nodes"].dtype == np.int32 and res["nodes"].tolist() == np.tile(nodes, K).tolist()
    for sd in ("col", "row"):
        assert res[sd]["partner"].shape == res[sd]["score"].shape == (K * n, k) and res[sd]["count"].shape == (K * n,)
        assert res[sd]["partner"].dtype == res[sd]["count"].dtype == np.int32 and res[sd]["score"].dtype == np.float32

    # byte for byte the kernel wrapper on the optimizer's tables and the stacked latents
    def direct(ctx):
        _, row_t, col_t, G, l = evaluate._edge_type_operands("test", ctx, opt, model, et)
        ex = exclusion_csr(excl, (row_t.shape[0], col_t.shape[0]))
        idx, ptr, rel = _dev(res["nodes"], np.int32), _dev(res["seg_ptr"], np.int32), _dev(np.arange(K), np.int32)
        a = kernels.decoder_node_topk(row_t, col_t, idx, ptr, G, l, k, seg_rel=rel, exclude=ex, no_self=no_self)
        b = kernels.decoder_node_topk(col_t, row_t, idx, ptr, G.transpose(-1, -2).contiguous(), l, k, seg_rel=rel,
                                      exclude=ex.transposed(), no_self=no_self)
        return torch.cat([t.view(torch.int32).reshape(-1) for t in a + b])

    flat = np.asarray(sess.run(Node("test/node_topk_direct", direct), feed_dict=feed), np.int32)
    o = 0
    for sd in ("col", "row"):
        for nm, size in (("score", K * n * k), ("partner", K * n * k), ("count", K * n)):
            assert res[sd][nm].tobytes() == flat[o:o + size].tobytes(), (sd, nm)
            o += size

    # against sess.run(opt.predictions) of every relation, in float64
    S = []
    for r in range(K):
        fd = dict(feed)
        fd[ph["batch_edge_type_idx"]] = first + r
        fd[ph["batch_row_edge_type"]] = et[0]
        fd[ph["batch_col_edge_type"]] = et[1]
        S.append(np.asarray(sess.run(opt.predictions, fd), np.float64))
    S = np.stack(S)
    oks = np.stack([permitted_mask(S.shape[1:], e, False, no_self) for e in excl])
    for sd, Sx, okx in (("col", S, oks), ("row", S.transpose(0, 2, 1), oks.transpose(0, 2, 1))):
        got = (res[sd]["score"], res[sd]["partner"], res[sd]["count"])
        check_rows_tolerant(got, Sx[:, nodes].reshape(K * n, -1), okx[:, nodes].reshape(K * n, -1), k)

    # a subset of relations out of order; a dict of nodes with one empty relation
    sub = [K - 1, empty, 1] if empty != 1 else [K - 1, empty, 0]
    part = evaluate.top_partners(sess, opt, ph, feed, nodes, et, k, relations=sub, **kw)
    assert part["relations"].tolist() == sub and "row" not in part
    for nm in ("partner", "score", "count"):
        want = np.concatenate([res["col"][nm][r * n:(r + 1) * n] for r in sub])
        assert part["col"][nm].tobytes() == want.tobytes(), nm
    per = {r: nodes[r::K][::-1] for r in range(K) if r != empty}
    byrel = evaluate.top_partners(sess, opt, ph, feed, per, et, k, side="row", **kw)
    lens = [per[r].size if r in per else 0 for r in range(K)]
    assert byrel["seg_ptr"].tolist() == _ptr(lens).tolist() and lens[empty] == 0 and "col" not in byrel
    where = {int(v): t for t, v in enumerate(nodes)}
    pick = np.concatenate([[r * n + where[int(v)] for v in per[r]] for r in per]).astype(np.int64)
    for nm in ("partner", "score", "count"):
        assert byrel["row"][nm].tobytes() == res["row"][nm][pick].tobytes(), nm

    # the sigmoid only transforms the returned scores
    sg = evaluate.top_partners(sess, opt, ph, feed, nodes, et, k, sigmoid="main", **kw)
    col = res["col"]
    assert np.array_equal(sg["col"]["partner"], col["partner"]) and np.array_equal(sg["col"]["count"], col["count"])
    valid = np.arange(k)[None, :] < col["count"][:, None]
    e = np.exp(-col["score"][valid].astype(np.float32))
    assert sg["col"]["score"].dtype == np.float64
    assert np.array_equal(sg["col"]["score"][valid], np.nan_to_num(1.0 / (1.0 + e.astype(np.float64))))
    assert np.all(np.isneginf(sg["col"]["score"][~valid]))

    # refusals
    fdl = dict(feed)
    fdl[opt.latent_varies[first + 1]] = np.eye(int(z[f"emb_{et[0]}"].shape[1]), dtype=np.float32)
    with pytest.raises(dg.InvalidArgumentError, match="latent matrix is fed"):
        evaluate.top_partners(sess, opt, ph, fdl, nodes, et, k)
    with pytest.raises(ValueError, match="unknown edge type"):
        evaluate.top_partners(sess, opt, ph, feed, nodes, (5, 5), k)
    with pytest.raises(ValueError, match="outside the embedding table"):
        evaluate.top_partners(sess, opt, ph, feed, [0, N], et, k)
    for bad in (0, MAX_K + 1):
        with pytest.raises(ValueError, match="k must be in"):
            evaluate.top_partners(sess, opt, ph, feed, nodes, et, bad)
    sess.shard = object()
    with pytest.raises(NotImplementedError):
        evaluate.top_partners(sess, opt, ph, feed, nodes, et, k)
    sess.shard = None

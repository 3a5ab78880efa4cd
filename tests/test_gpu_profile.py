"""GPU: the pair-profile query — kernels.decoder_score_cross (dg_decoder_score_cross_f32),
kernels.row_topk (dg_row_topk_f32), kernels.decoder_top_relations and evaluate.pair_profiles /
evaluate.top_relations.

The scorer's contract is equality with the per-relation scorer, bit for bit: every column of the
[P, n_sel] result against kernels.decoder_score on the same pairs with that slot's G_k, l_k.  So
that agreement with the older kernel is not the only check, every element is also held to the
float64 formula with the project's elementwise fp32 bar tol(s) = 1e-4·|s| + 1e-6
(tests/test_gpu_evalseg.py, tests/test_gpu_topk.py).  The selection is exact on given inputs: it is
compared with numpy's lexsort by (−value, column) of the same fp32 matrix, bits and all."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

NI, NJ, KMAX = 400, 300, 70


def tol(s):
    return 1e-4 * np.abs(s) + 1e-6


def _dev(a, dtype=np.float32):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


@pytest.fixture(scope="module", params=[32, 64])
def case(request):
    """Tables 400×d and 300×d and 70 relations' operands, drawn as tests/test_gpu_evalseg.py's
    score_case draws them, and 95 pairs — uploaded once."""
    d = request.param
    rng = np.random.default_rng(300 + d)

    def glorot(*shape):
        a = np.sqrt(6.0 / (shape[-2] + shape[-1])) if len(shape) > 1 else 1.0
        return rng.uniform(-a, a, shape).astype(np.float32)

    host = dict(Ei=glorot(NI, d), Ej=glorot(NJ, d), G1=glorot(d, d), GK=glorot(KMAX, d, d),
                l1=rng.uniform(-1.5, 1.5, d).astype(np.float32),
                lK=rng.uniform(-1.5, 1.5, (KMAX, d)).astype(np.float32),
                ri=rng.integers(0, NI, 95).astype(np.int32), ci=rng.integers(0, NJ, 95).astype(np.int32))
    host["ri"][40], host["ci"][40] = host["ri"][33], host["ci"][33]  # one tile holds the same pair twice
    dev = {k: _dev(v, v.dtype) for k, v in host.items()}
    return d, host, dev


FORMS = {
    "dedicom": ("G1", "lK"),     # shared G, one l per relation
    "bilinear": ("GK", None),    # one G per relation, identity l
    "shared": ("G1", "l1"),      # one G and one l for every relation
}


def _operands(h, v, form, K):
    """(device G, device l, host G, host l) of a form, its per-relation operands cut to K relations."""
    gname, lname = FORMS[form]
    G, Gh = v[gname], h[gname]
    if G.dim() == 3:
        G, Gh = G[:K].contiguous(), Gh[:K]
    l = lh = None
    if lname:
        l, lh = v[lname], h[lname]
        if l.dim() == 2:
            l, lh = l[:K].contiguous(), lh[:K]
    return G, l, Gh, lh


def _check_scores(h, v, d, P, G, l, Gh, lh, rel, got):
    """Every column of got [P, len(rel)] against the per-relation scorer (bits) and float64 (tol)."""
    from decagon_amd import kernels

    ri, ci = v["ri"][:P].contiguous(), v["ci"][:P].contiguous()
    assert got.shape == (P, len(rel)) and got.dtype == torch.float32
    got_h = got.cpu().numpy()
    U0, V0 = h["Ei"][h["ri"][:P]].astype(np.float64), h["Ej"][h["ci"][:P]].astype(np.float64)
    for s, k in enumerate(rel):
        k = int(k)
        Gk = G[k] if G.dim() == 3 else G
        lk = None if l is None else (l[k] if l.dim() == 2 else l)
        want = kernels.decoder_score(v["Ei"], v["Ej"], ri, ci, Gk, lk)
        col = got[:, s].contiguous()
        assert torch.equal(col, want), (s, k)
        assert np.array_equal(_bits(col), _bits(want)), (s, k)
        Gk64 = (Gh[k] if Gh.ndim == 3 else Gh).astype(np.float64)
        l64 = np.ones(d) if lh is None else (lh[k] if lh.ndim == 2 else lh).astype(np.float64)
        ref = np.einsum("pi,ij,pj->p", U0 * l64, Gk64, V0 * l64)
        err = np.abs(got_h[:, s] - ref) - tol(ref)
        assert np.all(err <= 0), (s, k, float(err.max()))


def _slot_counts(P):
    """K = 1, 11 and three values that straddle the slot chunk C the launch uses at this size:
    C − 1, C, C + 1 (the last chunk partial, whole, and a second chunk of one slot).  C is read
    from the library, and must not move over these K for the straddle to mean anything."""
    from decagon_amd import kernels

    C = kernels.cross_slot_chunk(P, 11)
    ks = [1, 11, C - 1, C, C + 1]
    assert all(kernels.cross_slot_chunk(P, k) == C for k in ks[2:]), (P, C)
    return sorted(set(k for k in ks if k >= 1))


# ---------------------------------------------------------------- scorer
@pytest.mark.parametrize("P", [1, 31, 32, 33, 95])
@pytest.mark.parametrize("form", list(FORMS))
def test_scorer_equals_per_relation_scorer(case, form, P):
    from decagon_amd import kernels

    d, h, v = case
    ri, ci = v["ri"][:P].contiguous(), v["ci"][:P].contiguous()
    for K in _slot_counts(P):
        G, l, Gh, lh = _operands(h, v, form, K)
        rel = np.arange(K)
        # (nothing per relation: the slots have to be named)
        rel_idx = _dev(rel, np.int32) if form == "shared" else None
        got = kernels.decoder_score_cross(v["Ei"], v["Ej"], ri, ci, G, l, rel_idx=rel_idx)
        _check_scores(h, v, d, P, G, l, Gh, lh, rel, got)


def test_scorer_dedicom_95_pairs_70_relations(case):
    """Three pair tiles with a tail against 70 relations: eighteen slot chunks, the last partial."""
    from decagon_amd import kernels

    d, h, v = case
    G, l, Gh, lh = _operands(h, v, "dedicom", KMAX)
    got = kernels.decoder_score_cross(v["Ei"], v["Ej"], v["ri"], v["ci"], G, l)
    _check_scores(h, v, d, 95, G, l, Gh, lh, np.arange(KMAX), got)
    assert h["ri"][40] == h["ri"][33] and h["ci"][40] == h["ci"][33]  # the same pair twice in tile 1
    assert np.array_equal(_bits(got[40]), _bits(got[33]))


@pytest.mark.parametrize("C", [8, 16, 32])
def test_scorer_wider_slot_chunks(case, C):
    """The slot chunks a fuller grid gets (C = 8, 16, 32; the cases above all run at C = 4): 95
    pairs against enough slots for the library to choose C, the last chunk partial.  Slot s names
    relation s mod 70, so column s must hold the bits of column s mod 70 of the 70-relation
    result, which test_scorer_dedicom_95_pairs_70_relations holds to the per-relation scorer."""
    from decagon_amd import kernels

    d, h, v = case
    G, l, _, _ = _operands(h, v, "dedicom", KMAX)
    n_sel = -(-2048 // 3) * C + 1  # three pair tiles: the smallest grid of 2,048 waves, and one slot more
    assert kernels.cross_slot_chunk(95, n_sel) == C and n_sel % C == 1
    rel = np.arange(n_sel) % KMAX
    base = kernels.decoder_score_cross(v["Ei"], v["Ej"], v["ri"], v["ci"], G, l)
    got = kernels.decoder_score_cross(v["Ei"], v["Ej"], v["ri"], v["ci"], G, l, rel_idx=_dev(rel, np.int32))
    assert got.shape == (95, n_sel)
    assert torch.equal(got.view(torch.int32), base.view(torch.int32)[:, torch.from_numpy(rel).cuda()])


@pytest.mark.parametrize("form", list(FORMS))
def test_scorer_with_a_relation_map(case, form):
    """rel_idx not the identity: relation 2 three times, relation 0 never, eleven slots."""
    from decagon_amd import kernels

    d, h, v = case
    G, l, Gh, lh = _operands(h, v, form, 11)
    rel = np.array([3, 2, 10, 2, 7, 9, 1, 2, 4, 6, 5])
    got = kernels.decoder_score_cross(v["Ei"], v["Ej"], v["ri"], v["ci"], G, l, rel_idx=_dev(rel, np.int32))
    _check_scores(h, v, d, 95, G, l, Gh, lh, rel, got)
    assert np.array_equal(_bits(got[:, 1]), _bits(got[:, 3])) and np.array_equal(_bits(got[:, 1]), _bits(got[:, 7]))


def test_scorer_out_padding_and_bad_indices(case):
    """`out` is a row-strided view whose padding keeps its fill; a pair outside the tables gives a
    row of NaN, a slot outside the relations a column of NaN, and every other element keeps the bits
    of the clean run."""
    from decagon_amd import kernels

    d, h, v = case
    K = 11
    G, l, _, _ = _operands(h, v, "dedicom", K)
    base = kernels.decoder_score_cross(v["Ei"], v["Ej"], v["ri"], v["ci"], G, l)
    assert not torch.isnan(base).any()
    buf = torch.full((95, K + 5), 7.0, device="cuda")
    ri, ci = h["ri"].copy(), h["ci"].copy()
    ri[5] = -1
    ci[64] = NJ
    rel = np.arange(K, dtype=np.int32)
    rel[6] = K  # one past the relations
    got = kernels.decoder_score_cross(v["Ei"], v["Ej"], _dev(ri, np.int32), _dev(ci, np.int32), G, l,
                                      rel_idx=_dev(rel, np.int32), out=buf[:, :K])
    assert got.data_ptr() == buf.data_ptr() and got.shape == (95, K)
    full = buf.cpu().numpy()
    assert np.all(full[:, K:] == 7.0)
    g, b = full[:, :K], base.cpu().numpy()
    nan = np.zeros((95, K), bool)
    nan[5, :] = nan[64, :] = nan[:, 6] = True
    assert np.all(np.isnan(g[nan]))
    assert np.array_equal(g[~nan].view(np.uint32), b[~nan].view(np.uint32))


# ---------------------------------------------------------------- row top-k
def _lexsort_topk(x, topk):
    """numpy's selection of the fp32 matrix x: by (−value, column), −0 taken and returned as +0."""
    x = np.where(x == 0, np.float32(0.0), x).astype(np.float32)
    n, m = x.shape
    k = min(topk, m)
    vals = np.full((n, topk), -np.inf, np.float32)
    idx = np.full((n, topk), -1, np.int32)
    for r in range(n):
        order = np.lexsort((np.arange(m), -x[r].astype(np.float64)))[:k]
        vals[r, :k], idx[r, :k] = x[r, order], order
    return vals, idx, np.full(n, k, np.int32)


def _check_topk(x_dev, x_host, topk):
    from decagon_amd import kernels

    a = kernels.row_topk(x_dev, topk)
    b = kernels.row_topk(x_dev, topk)
    want = _lexsort_topk(x_host, topk)
    for g, g2, w in zip(a, b, want):
        gh = g.cpu().numpy()
        assert gh.shape == w.shape and gh.dtype == w.dtype
        assert gh.tobytes() == w.tobytes(), topk
        assert gh.tobytes() == g2.cpu().numpy().tobytes()


TOPKS = [1, 7, 64, 70, 1024]


@pytest.mark.parametrize("topk", TOPKS)
def test_row_topk_of_the_scorers_output(case, topk):
    """[95, 70] scores with repeated relations, so exact ties exist in every row."""
    from decagon_amd import kernels

    d, h, v = case
    G, l, _, _ = _operands(h, v, "dedicom", KMAX)
    rel = np.arange(KMAX)
    rel[[5, 17, 69]] = [60, 3, 3]  # relation 60 twice, relation 3 three times
    x = kernels.decoder_score_cross(v["Ei"], v["Ej"], v["ri"], v["ci"], G, l, rel_idx=_dev(rel, np.int32))
    xh = x.cpu().numpy()
    assert np.array_equal(xh[:, 3], xh[:, 17]) and np.array_equal(xh[:, 3], xh[:, 69])
    _check_topk(x, xh, topk)


@pytest.mark.parametrize("topk", TOPKS)
def test_row_topk_special_values_and_row_stride(topk):
    """+0/−0, ±inf and a row of all-equal values, in a view with ld > n_cols."""
    rng = np.random.default_rng(7)
    x = rng.standard_normal((6, 70)).astype(np.float32)
    x[0, [3, 9, 40]] = [0.0, -0.0, 0.0]
    x[0, 50:] = -np.abs(x[0, 50:])
    x[1, [2, 60]] = np.inf
    x[1, [0, 69]] = -np.inf
    x[2, :] = 1.25
    x[3, :] = -0.0
    x[4, ::2] = 0.0
    x[4, 1::2] = -0.0
    buf = _dev(np.concatenate([x, np.full((6, 9), 1e30, np.float32)], axis=1))
    _check_topk(buf[:, :70], x, topk)


@pytest.mark.parametrize("topk", TOPKS)
def test_row_topk_long_rows(topk):
    """2,000 columns: longer than one refill of the list at every topk; one row ascending (every
    wave-wide step enters the list), one descending, one of few distinct values."""
    rng = np.random.default_rng(11)
    x = rng.standard_normal((5, 2000)).astype(np.float32)
    x[1] = np.sort(x[1])
    x[2] = np.sort(x[2])[::-1]
    x[3] = rng.integers(0, 4, 2000).astype(np.float32)
    _check_topk(_dev(x), x, topk)


# ---------------------------------------------------------------- top relations, graph capture
def test_top_relations_do_not_depend_on_the_chunking(case):
    from decagon_amd import kernels

    d, h, v = case
    G, l, _, _ = _operands(h, v, "dedicom", KMAX)
    args = (v["Ei"], v["Ej"], v["ri"], v["ci"], G, l)
    small = 32 * KMAX * 4  # one 32-pair granule: 95 pairs in three chunks, the last of 31
    assert [b - a for a, b in kernels.top_relations_chunks(95, KMAX, small)] == [32, 32, 31]
    assert len(kernels.top_relations_chunks(95, KMAX, 64 << 20)) == 1
    whole = kernels.decoder_top_relations(*args, 10)
    parts = kernels.decoder_top_relations(*args, 10, max_workspace_bytes=small)
    direct = kernels.row_topk(kernels.decoder_score_cross(*args), 10)
    for a, b, c in zip(whole, parts, direct):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() == c.cpu().numpy().tobytes()
    assert whole[0].shape == (95, 10) and int(whole[2].min()) == 10


def test_scorer_and_selection_capture_in_a_graph(case):
    """Neither call reads the host or allocates: both are captured, with outputs preallocated, in
    one graph on one stream without branches, and one replay gives the eager run's outputs."""
    from decagon_amd import _lib, kernels

    d, h, v = case
    G, l, _, _ = _operands(h, v, "dedicom", KMAX)
    eager = kernels.decoder_score_cross(v["Ei"], v["Ej"], v["ri"], v["ci"], G, l)
    e_top = kernels.row_topk(eager, 10)
    out = torch.zeros((95, KMAX), device="cuda")
    vals = torch.zeros((95, 10), device="cuda")
    idx = torch.zeros((95, 10), dtype=torch.int32, device="cuda")
    cnt = torch.zeros(95, dtype=torch.int32, device="cuda")
    lib = _lib.load()
    assert lib.dg_row_topk_workspace(95, KMAX, 10) == 0
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        kernels.decoder_score_cross(v["Ei"], v["Ej"], v["ri"], v["ci"], G, l, out=out)
        _lib.check(lib.dg_row_topk_f32(out.data_ptr(), KMAX, 95, KMAX, 10, vals.data_ptr(), idx.data_ptr(),
                                       cnt.data_ptr(), None, 0, kernels._stream_ptr(None)), "dg_row_topk_f32")
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out), _bits(eager))
    for got, want in zip((vals, idx, cnt), e_top):
        assert got.cpu().numpy().tobytes() == want.cpu().numpy().tobytes()


# ---------------------------------------------------------------- through the model
@pytest.mark.parametrize("et", [(1, 1), (0, 0)], ids=["dedicom", "bilinear"])
def test_profiles_through_the_model(golden_S, et):
    """evaluate.pair_profiles / top_relations on the golden-S model against sess.run(opt.predictions)
    of every relation, the segment scorer's bits, and numpy's ordering."""
    from test_gpu_model import _setup

    from decagon_amd import evaluate, kernels
    from decagon_amd.graph import Node

    z = golden_S
    dg, ph, model, opt, feed = _setup(z)
    sess = dg.Session()
    ets = list(model.edge_types)
    first = sum(model.edge_types[t] for t in ets[:ets.index(et)])
    K = model.edge_types[et]
    ni, nj = int(z["n_nodes"][et[0]]), int(z["n_nodes"][et[1]])
    rng = np.random.default_rng(5)
    pairs = np.stack([rng.integers(0, ni, 50), rng.integers(0, nj, 50)], axis=1)
    pairs[7] = pairs[3]   # a repeated pair
    pairs[11] = (4, 4)    # a diagonal pair
    prof = evaluate.pair_profiles(sess, opt, ph, feed, pairs, et)
    assert prof.shape == (50, K) and prof.dtype == np.float32
    for r in range(K):
        fd = dict(feed)
        fd[ph["batch_edge_type_idx"]] = first + r
        fd[ph["batch_row_edge_type"]] = et[0]
        fd[ph["batch_col_edge_type"]] = et[1]
        S = np.asarray(sess.run(opt.predictions, fd), np.float64)
        want = S[pairs[:, 0], pairs[:, 1]]
        assert np.all(np.abs(prof[:, r] - want) <= tol(want)), r
    assert np.array_equal(prof[7].view(np.uint32), prof[3].view(np.uint32))

    # the bits of the scorer accuracy_scores_all uses, on the same tables
    def seg(ctx):
        row_t, col_t = opt._tables(ctx, *et)
        G, l = evaluate._stacked_latents(ctx, model.edge_type2decoder[et], row_t.shape[1])
        ri = _dev(np.tile(pairs[:, 0], K), np.int32)
        ci = _dev(np.tile(pairs[:, 1], K), np.int32)
        ptr = _dev(np.arange(K + 1) * 50, np.int32)
        return kernels.decoder_score_seg(row_t, col_t, ri, ci, ptr, G, l, seg_rel=_dev(np.arange(K), np.int32))

    fd0 = dict(feed)
    fd0[ph["dropout"]] = 0.0
    by_seg = np.asarray(sess.run(Node("test/profile_seg", seg), feed_dict=fd0), np.float32).reshape(K, 50).T
    assert np.array_equal(prof.view(np.uint32), np.ascontiguousarray(by_seg).view(np.uint32))

    # the best three relations: numpy's ordering of the profile
    k = 3
    s, rel, n = evaluate.top_relations(sess, opt, ph, feed, pairs, et, k)
    wv, wi, wn = _lexsort_topk(prof, k)
    assert s.dtype == np.float32 and rel.dtype == np.int32 and n.dtype == np.int32
    assert s.tobytes() == wv.tobytes() and np.array_equal(rel, wi) and np.array_equal(n, wn)

    # a relation list with a repeat: relation numbers come back, the tie goes to the first listing
    rl = [2, 0, 2] if K > 2 else [K - 1, 0, K - 1]
    s2, rel2, n2 = evaluate.top_relations(sess, opt, ph, feed, pairs, et, k, relations=rl)
    p2 = evaluate.pair_profiles(sess, opt, ph, feed, pairs, et, relations=rl)
    assert np.array_equal(p2.view(np.uint32), np.ascontiguousarray(prof[:, rl]).view(np.uint32))
    wv2, wi2, _ = _lexsort_topk(p2, k)
    assert set(np.unique(rel2)) <= {rl[0], rl[1]} and np.all(n2 == 3)
    assert np.array_equal(rel2, np.asarray(rl, np.int32)[wi2]) and s2.tobytes() == wv2.tobytes()
    pos0, pos2 = (wi2 == 0).argmax(axis=1), (wi2 == 2).argmax(axis=1)
    assert np.all(pos0 + 1 == pos2)  # equal scores: the first listing, then the second
    # more slots than relations listed: −inf / −1 past the count
    s3, rel3, n3 = evaluate.top_relations(sess, opt, ph, feed, pairs, et, 5, relations=rl)
    assert np.all(n3 == 3) and np.all(rel3[:, 3:] == -1) and np.all(np.isneginf(s3[:, 3:]))
    assert np.array_equal(rel3[:, :3], rel2) and s3[:, :3].tobytes() == s2.tobytes()

    # the sigmoid only transforms the returned scores
    for mode in ("main", "evaluator"):
        pm = evaluate.pair_profiles(sess, opt, ph, feed, pairs, et, sigmoid=mode)
        want = evaluate._sigmoid_host(prof, mode)
        assert pm.dtype == want.dtype and np.array_equal(pm, want)
        sm, relm, nm = evaluate.top_relations(sess, opt, ph, feed, pairs, et, 5, relations=rl, sigmoid=mode)
        assert np.array_equal(relm, rel3) and np.array_equal(nm, n3)
        assert np.array_equal(sm[:, :3], evaluate._sigmoid_host(s3[:, :3], mode)) and np.all(np.isneginf(sm[:, 3:]))

    # refusals
    with pytest.raises(ValueError, match="latent matrix is fed"):
        fdl = dict(feed)
        fdl[opt.latent_varies[first + 1]] = np.eye(int(z["dec_1_1_global_interaction"].shape[0]), dtype=np.float32)
        evaluate.pair_profiles(sess, opt, ph, fdl, pairs, et)
    for fn in (lambda **kw: evaluate.pair_profiles(sess, opt, ph, feed, **kw),
               lambda **kw: evaluate.top_relations(sess, opt, ph, feed, k=3, **kw)):
        with pytest.raises(ValueError, match="unknown edge type"):
            fn(pairs=pairs, edge_type_ij=(5, 5))
        for bad in ((ni, 0), (0, nj), (-1, 0)):
            with pytest.raises(ValueError, match="outside the embedding tables"):
                fn(pairs=np.vstack([pairs, [bad]]), edge_type_ij=et)
        with pytest.raises(ValueError, match="relation outside"):
            fn(pairs=pairs, edge_type_ij=et, relations=[0, K])
        with pytest.raises(ValueError, match="sigmoid"):
            fn(pairs=pairs, edge_type_ij=et, sigmoid="tanh")

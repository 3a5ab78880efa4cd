"""GPU: evaluation of all relations of an edge type in one pass — kernels.decoder_score_seg
(dg_decoder_score_seg_f32), evaluate.rank_metrics_seg_device (dg_rank_metrics_seg_f32) and
evaluate.accuracy_scores_all.

The contract is equality with the per-relation entry points, bit for bit: every segment's scores
against kernels.decoder_score on its slice, every metrics row against rank_metrics_device on its
segment, every row of accuracy_scores_all against evaluate.accuracy_scores.  So that agreement
with the older kernels is not the only check, the scores are also held to the float64 formula
with the project's elementwise fp32 bar tol(s) = 1e-4·|s| + 1e-6 (tests/test_gpu_topk.py), and the
metrics to oracle.accuracy_scores (sklearn) within 1e-12 (test_rank_metrics_match_sklearn's bar)."""
import numpy as np
import pytest

from oracle import decagon_oracle as orc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def tol(s):
    return 1e-4 * np.abs(s) + 1e-6


def _dev(a, dtype=np.float32):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def _ptr(lens):
    p = np.zeros(len(lens) + 1, np.int32)
    p[1:] = np.cumsum(lens)
    return p


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32 if t.dtype == torch.float32 else np.uint64)


# ---------------------------------------------------------------- scorer
SEG_LENS = [0, 1, 31, 32, 33, 64, 0, 95, 256, 257, 600]


@pytest.fixture(scope="module", params=[32, 64])
def score_case(request):
    """Tables 400×d and 300×d, 11 relations' operands, the packed pairs of SEG_LENS — uploaded once."""
    d = request.param
    rng = np.random.default_rng(100 + d)
    K, Ni, Nj = len(SEG_LENS), 400, 300

    def glorot(*shape):
        a = np.sqrt(6.0 / (shape[-2] + shape[-1])) if len(shape) > 1 else 1.0
        return rng.uniform(-a, a, shape).astype(np.float32)

    n = sum(SEG_LENS)
    host = dict(Ei=glorot(Ni, d), Ej=glorot(Nj, d), G1=glorot(d, d), GK=glorot(K, d, d),
                l1=rng.uniform(-1.5, 1.5, d).astype(np.float32), lK=rng.uniform(-1.5, 1.5, (K, d)).astype(np.float32),
                ri=rng.integers(0, Ni, n).astype(np.int32), ci=rng.integers(0, Nj, n).astype(np.int32),
                ptr=_ptr(SEG_LENS))
    dev = {k: _dev(v, v.dtype) for k, v in host.items()}
    return d, host, dev


FORMS = {
    "dedicom": ("G1", "lK"),     # shared G, one l per relation
    "bilinear": ("GK", None),    # one G per relation, identity l
    "shared": ("G1", "l1"),      # one G and one l for every relation
}


@pytest.mark.parametrize("mapped", [False, True], ids=["identity", "seg_rel"])
@pytest.mark.parametrize("form", list(FORMS))
def test_scorer_equals_per_relation_scorer(score_case, form, mapped):
    from decagon_amd import kernels

    d, h, v = score_case
    gname, lname = FORMS[form]
    n_seg = len(SEG_LENS)
    rel = np.arange(n_seg)
    seg_rel = None
    if mapped:  # not the identity, relation 2 three times, relation 0 never
        rel = np.array([3, 2, 10, 2, 7, 9, 1, 2, 4, 6, 5])
        assert rel.size == n_seg
        seg_rel = _dev(rel, np.int32)
    G, l = v[gname], (v[lname] if lname else None)
    got = kernels.decoder_score_seg(v["Ei"], v["Ej"], v["ri"], v["ci"], v["ptr"], G, l, seg_rel=seg_rel)
    torch.cuda.synchronize()
    assert got.shape == (sum(SEG_LENS),) and got.dtype == torch.float32
    ptr = h["ptr"]
    got_h = got.cpu().numpy()
    for s in range(n_seg):
        a, b = int(ptr[s]), int(ptr[s + 1])
        k = int(rel[s])
        Gk = G[k] if G.dim() == 3 else G
        lk = None if l is None else (l[k] if l.dim() == 2 else l)
        if b > a:
            want = kernels.decoder_score(v["Ei"], v["Ej"], v["ri"][a:b].contiguous(), v["ci"][a:b].contiguous(), Gk, lk)
            assert torch.equal(got[a:b], want), (s, k)
            assert np.array_equal(_bits(got[a:b]), _bits(want)), (s, k)
        # the float64 formula
        Gh = h[gname][k] if h[gname].ndim == 3 else h[gname]
        lh = np.ones(d) if lname is None else (h[lname][k] if h[lname].ndim == 2 else h[lname])
        U = h["Ei"][h["ri"][a:b]].astype(np.float64) * lh
        V = h["Ej"][h["ci"][a:b]].astype(np.float64) * lh
        ref = np.einsum("pi,ij,pj->p", U, Gh.astype(np.float64), V)
        assert np.all(np.abs(got_h[a:b] - ref) <= tol(ref)), (s, float(np.max(np.abs(got_h[a:b] - ref) - tol(ref))))


def test_scorer_out_argument_and_bad_indices(score_case):
    """`out` is written in place; a pair outside the tables and a segment whose relation is out of
    range score NaN, and every other pair keeps its bits."""
    from decagon_amd import kernels

    d, h, v = score_case
    n = sum(SEG_LENS)
    base = kernels.decoder_score_seg(v["Ei"], v["Ej"], v["ri"], v["ci"], v["ptr"], v["G1"], v["lK"])
    out = torch.full((n,), 7.0, device="cuda")
    ri = h["ri"].copy()
    ci = h["ci"].copy()
    bad = [int(h["ptr"][3]) + 5, int(h["ptr"][10]) + 599]
    ri[bad[0]] = 400
    ci[bad[1]] = -1
    rel = np.arange(len(SEG_LENS), dtype=np.int32)
    rel[7] = 11  # one past the relations
    got = kernels.decoder_score_seg(v["Ei"], v["Ej"], _dev(ri, np.int32), _dev(ci, np.int32), v["ptr"], v["G1"],
                                    v["lK"], seg_rel=_dev(rel, np.int32), out=out)
    assert got.data_ptr() == out.data_ptr()
    g, b = got.cpu().numpy(), base.cpu().numpy()
    nan = np.zeros(n, bool)
    nan[bad] = True
    nan[int(h["ptr"][7]):int(h["ptr"][8])] = True
    assert np.all(np.isnan(g[nan])) and np.array_equal(g[~nan].view(np.uint32), b[~nan].view(np.uint32))


# ---------------------------------------------------------------- metrics
SEG_PN = [(0, 0), (0, 5), (5, 0), (1, 1), (10, 3), (255, 300), (256, 256), (257, 1000), (700, 6000)]
# (the count kernel stages 256 keys at a time: 700 positives and 6000 negatives are both more than two stages)


def _logits(mode):
    """Packed positive / negative logits of SEG_PN: integer-valued (heavy ties) in the odd
    segments, spanning [−120, 120] in the even ones, a few NaN negatives under "main"."""
    rng = np.random.default_rng(7)
    pos, neg = [], []
    for s, (P, N) in enumerate(SEG_PN):
        if s % 2:
            pos.append(rng.integers(0, 20, P).astype(np.float32) + 2.0)
            neg.append(rng.integers(0, 20, N).astype(np.float32))
        else:
            pos.append(rng.uniform(-60, 120, P).astype(np.float32))
            neg.append(rng.uniform(-120, 110, N).astype(np.float32))
            if mode == "main" and N >= 256:
                neg[-1][[0, 1, 100, 255, N - 1]] = np.nan
    return pos, neg


@pytest.fixture(scope="module", params=["main", "evaluator", None], ids=["main", "evaluator", "logit"])
def metrics_case(request):
    """The logits, and the oracle's (sklearn) rows for k = 50 and k = 5 — computed once per mode."""
    mode = request.param
    pos, neg = _logits(mode)
    want = {k: [orc.accuracy_scores(p, n, k, sigmoid=mode) if len(p) and len(n) else None for p, n in zip(pos, neg)]
            for k in (50, 5)}
    return mode, pos, neg, want


@pytest.mark.parametrize("k", [50, 5])
def test_metrics_equal_per_relation_metrics(metrics_case, k):
    from decagon_amd.evaluate import rank_metrics_device, rank_metrics_seg_device

    mode, pos, neg, want = metrics_case
    dp, dn = _dev(np.concatenate(pos)), _dev(np.concatenate(neg))
    pp, npt = _ptr([len(p) for p in pos]), _ptr([len(n) for n in neg])
    got = rank_metrics_seg_device(dp, _dev(pp, np.int32), dn, _dev(npt, np.int32), k=k, sigmoid=mode)
    assert got.shape == (len(SEG_PN), 3) and got.dtype == torch.float64
    g = got.cpu().numpy()
    for s, (P, N) in enumerate(SEG_PN):
        one = rank_metrics_device(dp[pp[s]:pp[s + 1]], dn[npt[s]:npt[s + 1]], k, mode).cpu().numpy()
        assert np.array_equal(g[s], one, equal_nan=True), (s, g[s], one)
        fin = ~np.isnan(one)
        assert np.array_equal(np.isnan(g[s]), ~fin)
        assert np.array_equal(g[s][fin].view(np.uint64), one[fin].view(np.uint64)), (s, g[s], one)
        if want[k][s] is not None:
            for a, b in zip(g[s], want[k][s]):
                assert abs(a - b) <= 1e-12, (s, g[s], want[k][s])
    # the conventions for an empty class (rank_reduce_kernel's)
    assert np.isnan(g[0][0]) and np.isnan(g[0][1]) and g[0][2] == 0.0      # neither class
    assert np.isnan(g[1][0]) and np.isnan(g[1][1]) and g[1][2] == 0.0      # no positives
    assert np.isnan(g[2][0]) and g[2][1] == 1.0 and g[2][2] == 1.0         # no negatives
    assert k == 50 or SEG_PN[4][0] > k                                      # k = 5 < P is exercised


# ---------------------------------------------------------------- through the model
def _samples(z, et, K, empty, n=300, seed=5):
    """300 positives from each relation's adjacency and 300 uniform negatives; relation `empty`
    gets none (missing among the positives, empty among the negatives)."""
    rng = np.random.default_rng(seed)
    Ni, Nj = (int(x) for x in z[f"adj_{et[0]}_{et[1]}_0_shape"])
    pos, neg = {}, {}
    for r in range(K):
        if r == empty:
            neg[r] = np.zeros((0, 2), np.int64)
            continue
        co = z[f"adj_{et[0]}_{et[1]}_{r}_coords"]
        pos[r] = co[rng.choice(len(co), min(n, len(co)), replace=False)]
        neg[r] = np.stack([rng.integers(0, Ni, n), rng.integers(0, Nj, n)], 1)
    return {et: pos}, {et: neg}


@pytest.mark.parametrize("et,empty", [((1, 1), 4), ((0, 0), 0)], ids=["dedicom", "bilinear"])
def test_accuracy_scores_all_equals_the_per_relation_loop(golden_S, et, empty):
    from test_gpu_model import _setup

    from decagon_amd import evaluate, kernels

    z = golden_S
    dg, ph, model, opt, feed = _setup(z)
    sess = dg.Session()
    K = model.edge_types[et]
    flat = {}
    for i, j in model.edge_types:
        for r in range(model.edge_types[i, j]):
            flat[i, j, r] = len(flat)
    edges_pos, edges_neg = _samples(z, et, K, empty)
    got, pooled = evaluate.accuracy_scores_all(sess, opt, ph, feed, edges_pos, edges_neg, et, k=50, pooled=True)
    assert got.shape == (K, 3) and got.dtype == np.float64
    assert np.isnan(got[empty][0]) and np.isnan(got[empty][1]) and got[empty][2] == 0.0
    for r in range(K):
        if r == empty:
            continue
        one = np.array(evaluate.accuracy_scores(sess, opt, ph, feed, edges_pos, edges_neg, et + (r,), flat, k=50))
        assert np.array_equal(got[r].view(np.uint64), one.view(np.uint64)), (r, got[r], one)
        assert 0.0 <= got[r][0] <= 1.0
    # without pooled the same rows alone; a subset out of order picks its rows
    assert np.array_equal(evaluate.accuracy_scores_all(sess, opt, ph, feed, edges_pos, edges_neg, et),
                          got, equal_nan=True)
    sub = [r for r in (K - 1, 0) if r != empty]
    assert np.array_equal(evaluate.accuracy_scores_all(sess, opt, ph, feed, edges_pos, edges_neg, et, relations=sub),
                          got[sub])

    # pooled = rank_metrics on the concatenated per-relation scores
    def scores(ctx):
        row_t, col_t = opt._tables(ctx, et[0], et[1])
        out = []
        for edges in (edges_pos, edges_neg):
            per = []
            for r in range(K):
                e = edges[et].get(r)
                if e is None or not len(e):
                    continue
                G, l = opt._latent(ctx, flat[et + (r,)])
                per.append(kernels.decoder_score(row_t, col_t, _dev(e[:, 0], np.int32), _dev(e[:, 1], np.int32), G, l))
            out.append(torch.cat(per))
        return evaluate.rank_metrics_device(out[0], out[1], 50, "main")

    from decagon_amd.graph import Node

    want = sess.run(Node("test/pooled", scores), feed_dict=feed)
    assert pooled == (float(want[0]), float(want[1])), (pooled, want)


def test_accuracy_scores_all_refuses_a_fed_latent(golden_S):
    from test_gpu_model import _setup

    from decagon_amd import evaluate

    z = golden_S
    dg, ph, model, opt, feed = _setup(z)
    sess = dg.Session()
    et = (1, 1)
    edges_pos, edges_neg = _samples(z, et, model.edge_types[et], 4, n=20)
    ets = list(model.edge_types)
    first = sum(model.edge_types[t] for t in ets[:ets.index(et)])
    fd = dict(feed)
    fd[opt.latent_varies[first + 1]] = np.eye(int(z["dec_1_1_global_interaction"].shape[0]), dtype=np.float32)
    with pytest.raises(ValueError, match="latent matrix is fed"):
        evaluate.accuracy_scores_all(sess, opt, ph, fd, edges_pos, edges_neg, et)
    with pytest.raises(ValueError, match="unknown edge type"):
        evaluate.accuracy_scores_all(sess, opt, ph, feed, edges_pos, edges_neg, (5, 5))


# ---------------------------------------------------------------- graph capture
def test_scorer_and_metrics_capture_into_one_graph(score_case):
    """Neither call reads its segment pointers on the host: both capture into one graph, and two
    replays give the bits of the eager calls."""
    from decagon_amd import evaluate, kernels

    d, h, v = score_case
    lens = np.array(SEG_LENS)
    P = int(lens.sum())
    # positives: the packed pairs; negatives: a second packed set of the same segment lengths
    rj = torch.roll(v["ri"], 17)
    cj = torch.roll(v["ci"], 5)
    both_r, both_c = torch.cat([v["ri"], rj]).contiguous(), torch.cat([v["ci"], cj]).contiguous()
    seg = _dev(np.concatenate([h["ptr"], P + h["ptr"][1:]]), np.int32)
    rel = _dev(np.concatenate([np.arange(len(lens))] * 2), np.int32)
    ptr = v["ptr"]

    def run():
        s = kernels.decoder_score_seg(v["Ei"], v["Ej"], both_r, both_c, seg, v["G1"], v["lK"], seg_rel=rel)
        return s, evaluate.rank_metrics_seg_device(s[:P], ptr, s[P:], ptr, k=50, sigmoid="main")

    s0, m0 = run()
    torch.cuda.synchronize()
    s0, m0 = s0.clone(), m0.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        s1, m1 = run()
    for _ in range(2):
        s1.zero_()
        m1.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_bits(s1), _bits(s0))
        assert np.array_equal(_bits(m1), _bits(m0))

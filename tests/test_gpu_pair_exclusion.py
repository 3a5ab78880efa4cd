"""GPU: each row's best columns outside a per-row exclusion list — dg_row_topk_excl_f32 through
kernels.row_topk(exclude=), kernels.decoder_top_relations(exclude=) and
evaluate.top_relations(exclude=).

The selection is exact on given inputs, so every comparison is of bytes.  The expected side is
numpy: the excluded columns are deleted, the rest ordered by (−value, column) with −0 taken and
returned as +0 — tests/test_gpu_profile.py's _lexsort_topk with a mask."""
import numpy as np
import pytest

from test_gpu_profile import KMAX, _bits, _dev, _operands, case  # noqa: F401  (case: the module's fixture)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _lists(lists):
    """(ptr, slot) int32 host arrays of per-row lists."""
    ptr = np.zeros(len(lists) + 1, np.int32)
    np.cumsum([len(x) for x in lists], out=ptr[1:])
    return ptr, np.asarray([s for x in lists for s in x], np.int32)


def _masked_topk(x, lists, topk):
    """numpy's selection of the fp32 matrix x outside each row's list (entries outside the columns
    exclude nothing): by (−value, column), −0 taken and returned as +0."""
    x = np.where(x == 0, np.float32(0.0), x).astype(np.float32)
    n, m = x.shape
    vals = np.full((n, topk), -np.inf, np.float32)
    idx = np.full((n, topk), -1, np.int32)
    cnt = np.zeros(n, np.int32)
    for r in range(n):
        keep = np.setdiff1d(np.arange(m), np.asarray(lists[r], np.int64))
        order = keep[np.lexsort((keep, -x[r, keep].astype(np.float64)))][:topk]
        k = order.size
        vals[r, :k], idx[r, :k], cnt[r] = x[r, order], order, k
    return vals, idx, cnt


def _same(got, want):
    for g, w in zip(got, want):
        gh = g.cpu().numpy() if isinstance(g, torch.Tensor) else g
        assert gh.shape == w.shape and gh.dtype == w.dtype
        assert gh.tobytes() == w.tobytes()


def _check(x_dev, x_host, lists, topk, ptr_slot=None):
    from decagon_amd import kernels

    ptr, slot = _lists(lists) if ptr_slot is None else ptr_slot
    got = kernels.row_topk(x_dev, topk, exclude=(_dev(ptr, np.int32), _dev(slot, np.int32)))
    want = _masked_topk(x_host, lists, topk)
    _same(got, want)
    return got, want


def _special_matrix():
    """test_row_topk_special_values_and_row_stride's matrix: ties, ±0, ±inf, an all-equal row."""
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
    return x


@pytest.mark.parametrize("topk", [1, 7, 64, 70])
def test_special_values_row_stride_and_list_shapes(topk):
    """[6, 70] as a view with ld = 79 and 1e30 in the padding; the six lists are dealt to the rows
    in every rotation, so that each row of special values meets each list, and the all-equal row
    also loses columns 0 and 1 (its tie-break then starts at column 2)."""
    x = _special_matrix()
    buf = _dev(np.concatenate([x, np.full((6, 9), 1e30, np.float32)], axis=1))
    view = buf[:, :70]
    assert view.stride(0) == 79

    def own(r):  # the row's own three best columns
        return sorted(np.lexsort((np.arange(70), -np.where(x[r] == 0, 0.0, x[r]).astype(np.float64)))[:3].tolist())

    for rot in range(6):
        base = [[], [0], [69], [63, 64], list(range(70)), None]
        lists = [base[(r + rot) % 6] for r in range(6)]
        lists = [own(r) if l is None else l for r, l in enumerate(lists)]
        got, want = _check(view, x, lists, topk)
        full = [r for r in range(6) if len(lists[r]) == 70][0]
        assert want[2][full] == 0 and np.all(want[1][full] == -1) and np.all(np.isneginf(want[0][full]))
    lists = [[], [0], [0, 1], [63, 64], list(range(70)), [69]]
    got, want = _check(view, x, lists, topk)
    assert want[1][2, 0] == 2 and want[0][2, 0] == np.float32(1.25)
    assert np.all(buf[:, 70:].cpu().numpy() == np.float32(1e30))


def test_long_lists_entries_outside_the_columns_and_a_reversed_range():
    """[3, 200], topk = 10: a list of 130 entries (more than two 64-entry pieces) that names the
    columns on both sides of every block boundary; a list that starts with −1 and ends with 200
    and 205, which exclude nothing; a row whose range runs backwards: an empty list."""
    rng = np.random.default_rng(21)
    x = rng.standard_normal((3, 200)).astype(np.float32)
    x[0, [63, 64, 127, 128, 191, 192]] = 50.0  # they would lead the row if they were not excluded
    x[0, 199] = 40.0
    x[1, [5, 150]] = 60.0
    must = [63, 64, 127, 128, 191, 192]
    rest = rng.choice(np.setdiff1d(np.arange(199), must), 124, replace=False)
    l0 = sorted(must + rest.tolist())
    assert len(l0) == 130
    l1 = [-1, 5, 70, 150, 200, 205]
    ptr = np.array([0, 130, 136, 5], np.int32)  # row 2: excl_ptr[3] < excl_ptr[2]
    slot = np.asarray(l0 + l1, np.int32)
    x_dev = _dev(x)
    got, want = _check(x_dev, x, [l0, l1, []], 10, ptr_slot=(ptr, slot))
    assert want[1][0, 0] == 199 and not set(want[1][0].tolist()) & set(must)
    assert not set(want[1][1].tolist()) & {5, 150} and np.all(want[2] == 10)
    # the count comes from the entries in range: 197 permitted columns in row 1
    got, want = _check(x_dev, x, [l0, l1, []], 200, ptr_slot=(ptr, slot))
    assert want[2].tolist() == [70, 197, 200]


@pytest.mark.parametrize("topk", [64, 1024])
def test_long_rows_refill_the_list(topk):
    """[3, 2000]: an ascending row without its top 1,000 columns (1,000 permitted: fewer than
    topk = 1,024), a descending row without every second column, a row of four distinct values
    with a random 300-entry list."""
    rng = np.random.default_rng(11)
    x = rng.standard_normal((3, 2000)).astype(np.float32)
    x[0] = np.sort(x[0])
    x[1] = np.sort(x[1])[::-1]
    x[2] = rng.integers(0, 4, 2000).astype(np.float32)
    lists = [list(range(1000, 2000)), list(range(0, 2000, 2)),
             sorted(rng.choice(2000, 300, replace=False).tolist())]
    got, want = _check(_dev(x), x, lists, topk)
    assert want[2].tolist() == [min(topk, 1000), min(topk, 1000), topk]


@pytest.mark.parametrize("topk", [7, 70])
def test_empty_lists_and_null_pointers_are_the_unmasked_selection(topk):
    from decagon_amd import _lib, kernels

    x = _special_matrix()
    x_dev = _dev(x)
    plain = kernels.row_topk(x_dev, topk)
    zeros = _dev(np.zeros(7, np.int32), np.int32)
    for slot in (np.zeros(0, np.int32), np.array([5, 6, 7], np.int32)):  # no entries; entries no row owns
        _same(kernels.row_topk(x_dev, topk, exclude=(zeros, _dev(slot, np.int32))), [t.cpu().numpy() for t in plain])
    lib = _lib.load()
    vals = torch.zeros((6, topk), device="cuda")
    idx = torch.zeros((6, topk), dtype=torch.int32, device="cuda")
    cnt = torch.zeros(6, dtype=torch.int32, device="cuda")
    _lib.check(lib.dg_row_topk_excl_f32(x_dev.data_ptr(), 70, 6, 70, topk, None, None, 0, vals.data_ptr(),
                                        idx.data_ptr(), cnt.data_ptr(), kernels._stream_ptr(None)), "null lists")
    _same((vals, idx, cnt), [t.cpu().numpy() for t in plain])
    # no rows: nothing is launched, empty outputs
    assert lib.dg_row_topk_excl_f32(x_dev.data_ptr(), 70, 0, 70, topk, zeros.data_ptr(), zeros.data_ptr(), 7,
                                    vals.data_ptr(), idx.data_ptr(), cnt.data_ptr(),
                                    kernels._stream_ptr(None)) == _lib.DG_OK
    e = kernels.row_topk(x_dev[:0], topk, exclude=(zeros[:1], zeros))
    assert e[0].shape == (0, topk) and e[1].shape == (0, topk) and e[2].shape == (0,)


def _random_pair_lists(seed):
    """Lists for the 95 pairs × 70 slots case: one pair with all 70 excluded, non-empty lists on
    both sides of the 32-pair chunk boundary."""
    rng = np.random.default_rng(seed)
    lists = [sorted(rng.choice(KMAX, int(rng.integers(0, 30)), replace=False).tolist()) for _ in range(95)]
    lists[50] = list(range(KMAX))
    lists[31] = [0, 3, 69]
    lists[32] = [1, 2, 68]
    lists[0] = []
    return lists


def test_top_relations_with_lists_do_not_depend_on_the_chunking(case):
    from decagon_amd import kernels

    d, h, v = case
    G, l, _, _ = _operands(h, v, "dedicom", KMAX)
    args = (v["Ei"], v["Ej"], v["ri"], v["ci"], G, l)
    lists = _random_pair_lists(400 + d)
    ptr, slot = _lists(lists)
    ex = (_dev(ptr, np.int32), _dev(slot, np.int32))
    small = 32 * KMAX * 4  # one 32-pair granule: 95 pairs in three chunks, the last of 31
    assert [b - a for a, b in kernels.top_relations_chunks(95, KMAX, small)] == [32, 32, 31]
    whole = kernels.decoder_top_relations(*args, 10, exclude=ex)
    parts = kernels.decoder_top_relations(*args, 10, max_workspace_bytes=small, exclude=ex)
    scores = kernels.decoder_score_cross(*args)
    direct = kernels.row_topk(scores, 10, exclude=ex)
    for a, b, c in zip(whole, parts, direct):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() == c.cpu().numpy().tobytes()
    _same(whole, _masked_topk(scores.cpu().numpy(), lists, 10))
    cnt = whole[2].cpu().numpy()
    assert cnt[50] == 0 and np.array_equal(cnt, np.minimum(10, KMAX - np.diff(ptr)))


def test_scorer_and_masked_selection_capture_in_a_graph(case):
    """The masked selection reads nothing on the host and allocates nothing: captured after the
    scorer with preallocated outputs, one replay gives the eager run's bytes."""
    from decagon_amd import _lib, kernels

    d, h, v = case
    G, l, _, _ = _operands(h, v, "dedicom", KMAX)
    ptr, slot = _lists(_random_pair_lists(500 + d))
    ex = (_dev(ptr, np.int32), _dev(slot, np.int32))
    eager = kernels.decoder_score_cross(v["Ei"], v["Ej"], v["ri"], v["ci"], G, l)
    e_top = kernels.row_topk(eager, 10, exclude=ex)
    out = torch.zeros((95, KMAX), device="cuda")
    vals = torch.zeros((95, 10), device="cuda")
    idx = torch.zeros((95, 10), dtype=torch.int32, device="cuda")
    cnt = torch.zeros(95, dtype=torch.int32, device="cuda")
    lib = _lib.load()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        kernels.decoder_score_cross(v["Ei"], v["Ej"], v["ri"], v["ci"], G, l, out=out)
        _lib.check(lib.dg_row_topk_excl_f32(out.data_ptr(), KMAX, 95, KMAX, 10, ex[0].data_ptr(), ex[1].data_ptr(),
                                            ex[1].numel(), vals.data_ptr(), idx.data_ptr(), cnt.data_ptr(),
                                            kernels._stream_ptr(None)), "dg_row_topk_excl_f32")
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out), _bits(eager))
    for got, want in zip((vals, idx, cnt), e_top):
        assert got.cpu().numpy().tobytes() == want.cpu().numpy().tobytes()


@pytest.mark.parametrize("et", [(1, 1), (0, 0)], ids=["dedicom", "bilinear"])
def test_new_relations_through_the_model(golden_S, et):
    """evaluate.top_relations(exclude=) on the golden-S model, the exclusion being the fixture's
    own adjacency of every relation: numpy's masked ordering of pair_profiles, no known edge among
    the answers, the counts — for the per-relation list, a prebuilt PairExclusion, and a relation
    list that reorders and repeats."""
    from test_gpu_model import _setup

    from decagon_amd import evaluate
    from decagon_amd.sparse import pair_exclusion

    z = golden_S
    dg, ph, model, opt, feed = _setup(z)
    sess = dg.Session()
    K = model.edge_types[et]
    ni, nj = int(z["n_nodes"][et[0]]), int(z["n_nodes"][et[1]])
    rng = np.random.default_rng(5)
    pairs = np.stack([rng.integers(0, ni, 50), rng.integers(0, nj, 50)], axis=1)
    pairs[7] = pairs[3]   # a repeated pair
    pairs[11] = (4, 4)    # a diagonal pair
    adj = [np.asarray(z[f"adj_{et[0]}_{et[1]}_{r}_coords"], np.int64).reshape(-1, 2) for r in range(K)]
    edges = np.concatenate([adj[0][:2], adj[K - 1][-2:], adj[0][:1]])  # known edges, one of them twice
    pairs = np.concatenate([pairs, edges])
    known = [{(int(r), int(c)) for r, c in a} for a in adj]
    exclude = [(a, np.ones(len(a)), (ni, nj)) for a in adj]
    k = 3

    def want_for(rl):
        prof = evaluate.pair_profiles(sess, opt, ph, feed, pairs, et, relations=rl)
        lists = [[s for s, r in enumerate(rl) if (int(a), int(b)) in known[r]] for a, b in pairs]
        wv, wi, wn = _masked_topk(prof, lists, k)
        rel = np.where(wi >= 0, np.asarray(rl, np.int32)[np.maximum(wi, 0)], np.int32(-1)).astype(np.int32)
        return lists, wv, rel, wn

    def check(got, rl, lists, wv, rel, wn):
        s, r, n = got
        assert s.dtype == np.float32 and r.dtype == np.int32 and n.dtype == np.int32
        assert s.tobytes() == wv.tobytes() and np.array_equal(r, rel) and np.array_equal(n, wn)
        assert np.array_equal(n, np.minimum(k, len(rl) - np.asarray([len(x) for x in lists])))
        for p, (a, b) in enumerate(pairs):
            for q in range(k):
                assert (q < n[p]) == (r[p, q] >= 0)
                assert r[p, q] < 0 or (int(a), int(b)) not in known[r[p, q]], (p, q)

    rl = list(range(K))
    lists, wv, rel, wn = want_for(rl)
    assert sum(len(x) for x in lists) > 0 and all(len(lists[p]) > 0 for p in range(50, len(pairs)))
    check(evaluate.top_relations(sess, opt, ph, feed, pairs, et, k, exclude=exclude), rl, lists, wv, rel, wn)
    pe = pair_exclusion(pairs, exclude, (ni, nj))
    assert pe.nnz == sum(len(x) for x in lists)
    for _ in range(2):  # (the second call finds the lists on the device)
        check(evaluate.top_relations(sess, opt, ph, feed, pairs, et, k, exclude=pe), rl, lists, wv, rel, wn)
    assert len(pe._on_device) == 1
    assert np.all(evaluate.top_relations(sess, opt, ph, feed, pairs, et, k)[2] == min(k, K))  # (without: all full)

    rl = [2, 0, 2, 5, 1] if K > 5 else [K - 1, 0, K - 1]
    lists, wv, rel, wn = want_for(rl)
    assert sum(len(x) for x in lists) > 0
    got = evaluate.top_relations(sess, opt, ph, feed, pairs, et, k, relations=rl, exclude=exclude)
    check(got, rl, lists, wv, rel, wn)
    for mode in ("main", "evaluator"):  # the sigmoid only transforms the returned scores
        sm, rm, nm = evaluate.top_relations(sess, opt, ph, feed, pairs, et, k, relations=rl, exclude=exclude,
                                            sigmoid=mode)
        assert np.array_equal(rm, rel) and np.array_equal(nm, wn)
        valid = np.arange(k)[None, :] < wn[:, None]
        assert np.array_equal(sm[valid], evaluate._sigmoid_host(wv[valid], mode)) and np.all(np.isneginf(sm[~valid]))

    # refusals: lists of another query, the wrong number of relation entries, another shape
    with pytest.raises(ValueError, match="exclude"):
        evaluate.top_relations(sess, opt, ph, feed, pairs[:-1], et, k, exclude=pe)
    with pytest.raises(ValueError, match="exclude"):
        evaluate.top_relations(sess, opt, ph, feed, pairs, et, k, relations=rl, exclude=pe)
    with pytest.raises(ValueError):
        evaluate.top_relations(sess, opt, ph, feed, pairs, et, k, exclude=exclude[:-1])
    with pytest.raises(ValueError):
        evaluate.top_relations(sess, opt, ph, feed, pairs, et, k, exclude=[(a, np.ones(len(a)), (ni + 1, nj)) for a in adj])

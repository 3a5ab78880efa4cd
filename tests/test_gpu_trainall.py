"""GPU: the all-relation training step — the segmented decoder gradient (dg_decoder_grad_seg_f32)
and the segmented row sums (dg_segment_rows_sum_f32) against float64 numpy, and
trainall.train_step_all on the golden S model against the float64 sum over (edge type, relation)
of oracle.train_grads, against the sum of the existing per-relation path, and against TF's Adam.

Tolerances: kernels rel_err <= 1e-5 (test_gpu_train.py's kernel-level bound); gradients of the
model max|g − g_ref| <= 1e-4·max|g_ref| per tensor; the cost 1e-5 relative.
"""
import numpy as np
import pytest

import _trainall_ref as R
from conftest import rel_err
from oracle import decagon_oracle as orc
from test_gpu_model import _setup

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TOL = 1e-4


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


# ------------------------------------------------------------------ the segmented gradient kernel
N_REL, NR, NC = 5, 37, 29
SEG_REL = [4, 3, 0, 2]      # relation 1 has no segment; relation 3's is empty
SEG_PTR = [0, 32, 32, 72, 79]  # a full tile; empty; a full + a ragged tile; a sub-tile
BAD_PAIR = 50               # its row index lies outside the table: it must contribute nothing
SENTINEL = 7.5              # fills the outputs: what the call leaves untouched stays visible


def _grad_case(kind, d):
    rng = np.random.default_rng(100 + d)
    n = SEG_PTR[-1]
    U = rng.standard_normal((NR, d)).astype(np.float32)
    V = rng.standard_normal((NC, d)).astype(np.float32)
    rows, cols, negs = rng.integers(0, NR, n), rng.integers(0, NC, n), rng.integers(0, NR, n)
    rows[BAD_PAIR] = NR
    pos = rng.standard_normal(n).astype(np.float32)
    neg = rng.standard_normal(n).astype(np.float32)
    if kind == "dedicom":
        G, l = rng.standard_normal((d, d)).astype(np.float32), rng.standard_normal((N_REL, d)).astype(np.float32)
    elif kind == "bilinear":
        G, l = rng.standard_normal((N_REL, d, d)).astype(np.float32), None
    elif kind == "distmult":
        G = np.stack([np.diag(rng.standard_normal(d)) for _ in range(N_REL)]).astype(np.float32)
        l = None
    else:
        G, l = np.eye(d, dtype=np.float32), None
    return U, V, rows, cols, negs, pos, neg, G, l


def _grad_reference(kind, d, U, V, rows, cols, negs, pos, neg, G, l, margin):
    """float64 restatement (test_gpu_train.py:251-292's formulas, per segment); the hinge mask
    from the fed scores in fp32, as the kernel forms it."""
    n = len(rows)
    a = ((neg - (pos - np.float32(margin))) > 0).astype(np.float64)
    a[BAD_PAIR] = 0.0
    U64, V64 = U.astype(np.float64), V.astype(np.float64)
    rs = np.where(rows < NR, rows, 0)
    mv, gc = np.zeros((n, d)), np.zeros((n, d))
    dG = np.zeros((d, d)) if kind == "dedicom" else np.full((N_REL, d, d), SENTINEL)
    dl = np.full((N_REL, d), SENTINEL)
    dgd = np.full((N_REL, d), SENTINEL)
    for s, k in enumerate(SEG_REL):
        p = slice(SEG_PTR[s], SEG_PTR[s + 1])
        Gk = (G if G.ndim == 2 else G[k]).astype(np.float64)
        L = np.diag(l[k].astype(np.float64)) if l is not None else np.eye(d)
        M = L @ Gk @ L
        mv[p] = a[p, None] * (V64[cols[p]] @ M.T)
        gc[p] = a[p, None] * ((U64[negs[p]] - U64[rs[p]]) @ M)
        dM = (a[p, None] * (U64[negs[p]] - U64[rs[p]])).T @ V64[cols[p]]
        if kind == "dedicom":
            dG += L @ dM @ L
            dl[k] = np.diag(dM @ (Gk @ L).T + (L @ Gk).T @ dM)
        else:
            dG[k] = L @ dM @ L
            dgd[k] = np.diag(dM)
    return a, mv, gc, dG, dl, dgd


@pytest.mark.parametrize("d", [32, 64])
@pytest.mark.parametrize("kind", ["dedicom", "bilinear", "distmult", "innerproduct"])
def test_segmented_gradient_matches_float64(kind, d):
    from decagon_amd import kernels

    dev = _dev()
    margin = 0.1
    U, V, rows, cols, negs, pos, neg, G, l = _grad_case(kind, d)
    a, mv, gc, dG, dl, dgd = _grad_reference(kind, d, U, V, rows, cols, negs, pos, neg, G, l, margin)
    assert 0.3 <= a.mean() <= 0.7  # the margin leaves roughly half the pairs inactive
    T = lambda x, dt=torch.float32: torch.from_numpy(np.ascontiguousarray(x)).to(dev, dt)  # noqa: E731
    full = lambda *shape: torch.full(shape, SENTINEL, device=dev)  # noqa: E731
    outs = {}
    if kind == "dedicom":
        outs = dict(dG=full(d * d), dl=full(N_REL * d))
    elif kind == "bilinear":
        outs = dict(dG=full(N_REL * d * d))
    elif kind == "distmult":
        outs = dict(dG_diag=full(N_REL * d))
    op = kernels.PreparedDecoderGradSeg(T(U), T(V), T(rows, torch.int32), T(cols, torch.int32), T(negs, torch.int32),
                                        T(SEG_PTR, torch.int32), T(SEG_REL, torch.int32), T(pos), T(neg), T(G),
                                        T(l) if l is not None else None, margin, **outs)

    def run(stream=None):
        for t in outs.values():
            t.fill_(SENTINEL)
        op.mv.fill_(SENTINEL)
        op.grad_cols.fill_(SENTINEL)
        if stream is not None:
            stream.wait_stream(torch.cuda.current_stream())
        op(stream)
        (stream or torch.cuda.current_stream()).synchronize()
        return [op.mv.cpu().numpy().copy(), op.grad_cols.cpu().numpy().copy()] + [
            t.cpu().numpy().copy() for t in outs.values()]

    got = run()
    assert rel_err(got[0], mv) <= 1e-5
    assert rel_err(got[1], gc) <= 1e-5
    # the out-of-range pair and the inactive pairs: exact zeros
    assert not got[0][a == 0].any() and not got[1][a == 0].any()
    live = [k for s, k in enumerate(SEG_REL) if SEG_PTR[s + 1] > SEG_PTR[s]]
    if kind == "dedicom":
        assert rel_err(got[2].reshape(d, d), dG) <= 1e-5
        gl = got[3].reshape(N_REL, d)
        assert rel_err(gl[live], dl[live]) <= 1e-5
        assert not gl[3].any() and np.all(gl[1] == SENTINEL)  # empty segment: zeros; absent: untouched
    elif kind == "bilinear":
        gg = got[2].reshape(N_REL, d, d)
        assert rel_err(gg[live], dG[live]) <= 1e-5
        assert not gg[3].any() and np.all(gg[1] == SENTINEL)
    elif kind == "distmult":
        gd = got[2].reshape(N_REL, d)
        assert rel_err(gd[live], dgd[live]) <= 1e-5
        assert not gd[3].any() and np.all(gd[1] == SENTINEL)
    # fixed order: a second call, and a call on another stream, give the same bits
    for again in (run(), run(torch.cuda.Stream())):
        for x, y in zip(got, again):
            assert np.array_equal(x, y)


def test_shared_G_gradient_over_many_segments():
    """DEDICOM's shared dG is summed over slices of the segment list (16 a workgroup, 8 segments
    of a slice in flight): 150 segments give slices of 10 — a full batch and a clamped one — and
    an unfilled last slice; some segments are empty and one has an out-of-range relation."""
    from decagon_amd import kernels

    dev = _dev()
    rng = np.random.default_rng(17)
    d, n_seg, K = 32, 150, 160
    sizes = rng.integers(0, 4, n_seg)
    ptr = np.concatenate([[0], np.cumsum(sizes)])
    n = int(ptr[-1])
    rel = rng.permutation(K)[:n_seg]
    rel[77] = K  # outside [0, K): the segment contributes nothing
    U = rng.standard_normal((NR, d)).astype(np.float32)
    V = rng.standard_normal((NC, d)).astype(np.float32)
    rows, cols, negs = rng.integers(0, NR, n), rng.integers(0, NC, n), rng.integers(0, NR, n)
    pos, neg = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    G = rng.standard_normal((d, d)).astype(np.float32)
    l = rng.standard_normal((K, d)).astype(np.float32)
    a = ((neg - (pos - np.float32(0.1))) > 0).astype(np.float64)
    U64, V64 = U.astype(np.float64), V.astype(np.float64)
    dG, dl = np.zeros((d, d)), np.zeros((K, d))
    for s in range(n_seg):
        if rel[s] >= K:
            continue
        p = slice(ptr[s], ptr[s + 1])
        L = np.diag(l[rel[s]].astype(np.float64))
        dM = (a[p, None] * (U64[negs[p]] - U64[rows[p]])).T @ V64[cols[p]]
        dG += L @ dM @ L
        dl[rel[s]] = np.diag(dM @ (G.astype(np.float64) @ L).T + (L @ G.astype(np.float64)).T @ dM)
    T = lambda x, dt=torch.float32: torch.from_numpy(np.ascontiguousarray(x)).to(dev, dt)  # noqa: E731
    gG, gl = torch.zeros(d * d, device=dev), torch.zeros(K * d, device=dev)
    op = kernels.PreparedDecoderGradSeg(T(U), T(V), T(rows, torch.int32), T(cols, torch.int32), T(negs, torch.int32),
                                        T(ptr, torch.int32), T(rel, torch.int32), T(pos), T(neg), T(G), T(l), 0.1,
                                        dG=gG, dl=gl)
    op()
    torch.cuda.synchronize()
    first = gG.cpu().numpy().copy()
    assert rel_err(first.reshape(d, d), dG) <= 1e-5
    assert rel_err(gl.cpu().numpy().reshape(K, d), dl) <= 1e-5
    op()
    torch.cuda.synchronize()
    assert np.array_equal(first, gG.cpu().numpy())


# ------------------------------------------------------------------ segmented row sums
def _row_case(d, exact):
    from decagon_amd import kernels
    from decagon_amd.trainall import occurrence_list

    chunk, waves = kernels.segment_rows_chunk()
    rng = np.random.default_rng(200 + d)
    n_out, n_src = 37, 61
    idx = list(rng.integers(0, n_out, 300))
    idx = [r for r in idx if r not in (3, 5, 7, 9)]
    idx += [5]                                   # a row that occurs once (row 3: never)
    idx += [7] * (chunk + 3)                     # longer than one wave's chunk
    idx += [9] * (2 * chunk * waves + 5)         # longer than one round of the workgroup's chunks
    idx = np.asarray(idx)[rng.permutation(len(idx))]
    n = len(idx)
    item = rng.integers(0, n_src, n).astype(np.int32)
    sign = rng.choice([-1.0, 1.0], n).astype(np.float32)
    if exact:
        src = rng.integers(-8, 9, (n_src, d)).astype(np.float32)
        out0 = rng.integers(-8, 9, (n_out, d + 8)).astype(np.float32)
    else:
        src = rng.standard_normal((n_src, d)).astype(np.float32)
        out0 = rng.standard_normal((n_out, d + 8)).astype(np.float32)
    node_ptr, order = occurrence_list(idx, n_out)
    assert node_ptr[4] == node_ptr[3] and node_ptr[6] - node_ptr[5] == 1
    assert node_ptr[8] - node_ptr[7] > chunk and node_ptr[10] - node_ptr[9] > chunk * waves
    return idx, item, sign, src, out0, node_ptr, order


@pytest.mark.parametrize("d", [32, 64, 256])
def test_segment_rows_sum(d):
    from decagon_amd import kernels

    dev = _dev()
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    for exact in (False, True):
        idx, item, sign, src, out0, node_ptr, order = _row_case(d, exact)
        it, sg = item[order], sign[order]  # the list in node-major order

        def run():
            big = T(out0)
            kernels.segment_rows_sum(T(node_ptr), T(it), T(src), big[:, :d], sign=T(sg))  # ld_out = d + 8 > d
            torch.cuda.synchronize()
            return big.cpu().numpy()

        got = run()
        want = out0.astype(np.float64)
        np.add.at(want[:, :d], idx, sign[:, None].astype(np.float64) * src[item])
        assert np.array_equal(got[:, d:], out0[:, d:])   # the columns past d are not touched
        assert np.array_equal(got[3], out0[3])           # a row that never occurs
        # a fixed-order fp32 sum of n terms is within n·2^-24·Σ|terms| of the exact one (n terms: the
        # row's occurrences, the chunk tree's levels and the row's old value)
        mag = np.abs(out0[:, :d]).astype(np.float64)
        np.add.at(mag, idx, np.abs(src[item]).astype(np.float64))
        n_r = np.diff(node_ptr).astype(np.float64)[:, None] + 4
        assert np.all(np.abs(got[:, :d] - want[:, :d]) <= n_r * 2.0**-24 * mag)
        assert np.array_equal(got, run())                # two runs: the same bits
        if exact:  # small integers: every order of summation is exact — the old entry point's bits
            old = T(out0[:, :d])
            kernels.scatter_rows(T(idx.astype(np.int32)), T(sign[:, None] * src[item]), old)
            torch.cuda.synchronize()
            assert np.array_equal(got[:, :d], old.cpu().numpy())
            assert np.array_equal(got[:, :d], want[:, :d].astype(np.float32))
        # without signs: all +1
        big = T(out0)
        kernels.segment_rows_sum(T(node_ptr), T(it), T(src), big[:, :d])
        torch.cuda.synchronize()
        want = out0.astype(np.float64)
        np.add.at(want[:, :d], idx, src[item].astype(np.float64))
        mag = np.abs(out0[:, :d]).astype(np.float64)
        np.add.at(mag, idx, np.abs(src[item]).astype(np.float64))
        assert np.all(np.abs(big.cpu().numpy()[:, :d] - want[:, :d]) <= n_r * 2.0**-24 * mag)


# ------------------------------------------------------------------ end to end on the golden S model
@pytest.fixture(scope="module")
def ref_all(golden_S):
    """Batches and fed negatives of every relation, and their summed float64 reference (once)."""
    batches, negs = R.make_batches(golden_S)
    cost, grads, zs = R.reference(golden_S, batches, negs)
    return batches, negs, cost, grads, zs


def _want(model, grads):
    return R.wanted(model.edge_types, {et: list(model.edge_type2decoder[et].vars) for et in model.edge_types}, grads)


def _assert_grads(gv, want):
    assert len(gv) == len(want)
    nonzero = 0
    for (g, v), w in zip(gv, want):
        assert g.shape == w.shape
        scale = np.max(np.abs(w))
        if scale == 0:
            assert np.max(np.abs(g)) == 0.0
        else:
            nonzero += 1
            assert np.max(np.abs(g - w)) <= TOL * scale, f"gradient off by {rel_err(g, w):.2e}"
    assert nonzero > 0


def test_all_relation_gradients_match_the_summed_oracle(golden_S, ref_all):
    from decagon_amd.trainall import train_step_all

    batches, negs, cost_ref, grads, zs = ref_all
    assert np.min(np.abs(zs)) >= 1e-3  # fp32 cannot flip a relu mask (the seed was picked for this)
    assert abs(cost_ref - np.maximum(zs, 0).sum()) <= 1e-12 * cost_ref
    dg, ph, model, opt, feed = _setup(golden_S)
    sess = dg.Session()
    before = [p.eval() for p in model.vars.values()]
    cost, gv = train_step_all(sess, opt, ph, feed, batches, neg_samples=negs, apply=False)
    assert isinstance(cost, float) and abs(cost - cost_ref) <= 1e-5 * abs(cost_ref)
    _assert_grads(gv, _want(model, grads))
    for (g, v), p, b in zip(gv, model.vars.values(), before):  # the variables: returned, not updated
        assert np.array_equal(v, b) and np.array_equal(p.eval(), b)


def _per_relation_sum(sess, ph, model, opt, feed, batches, negs):
    """(Σ cost, Σ gradients in float64) of opt.grads_vars / opt.cost over one Session.run per relation."""
    total, cost_sum, e = None, 0.0, 0
    for (i, j), K in model.edge_types.items():
        for k in range(K):
            f = dict(feed)
            f.update({ph["batch"]: batches[i, j][k], ph["batch_edge_type_idx"]: e, ph["batch_row_edge_type"]: i,
                      ph["batch_col_edge_type"]: j, opt.neg_samples: negs[i, j][k]})
            gv, c = sess.run([opt.grads_vars, opt.cost], feed_dict=f)
            cost_sum += float(c)
            g64 = [np.asarray(g, np.float64) for g, _ in gv]
            total = g64 if total is None else [a + b for a, b in zip(total, g64)]
            e += 1
    return cost_sum, total


def test_accumulation_equals_the_per_relation_path(golden_S, ref_all):
    """The same quantities against Σ opt.grads_vars over one Session.run per relation."""
    from decagon_amd.trainall import train_step_all

    batches, negs, cost_ref, _, _ = ref_all
    dg, ph, model, opt, feed = _setup(golden_S)
    sess = dg.Session()
    cost_sum, total = _per_relation_sum(sess, ph, model, opt, feed, batches, negs)
    cost, gv = train_step_all(sess, opt, ph, feed, batches, neg_samples=negs, apply=False)
    assert abs(cost - cost_sum) <= 1e-5 * abs(cost_sum)
    _assert_grads(gv, total)


def test_decoders_whose_operands_are_no_views_take_the_one_path(golden_S, ref_all):
    """DistMult on (1, 1) and InnerProduct on (0, 1) — the decoders whose (G, l) are expanded per
    run, not views of the flat buffer — with the variables the model was constructed with:
    (a) the step against the per-relation path, as above; (b) the step on an EdgeBatches' host
    batches against the step on its device batches, bit for bit, twice in a row (the operands the
    step keeps across runs, with nothing applied in between)."""
    from decagon_amd import inits
    from decagon_amd.trainall import train_step_all
    from test_gpu_epochs import _edge_batches, _fed_negatives, _same

    batches, negs, _, _, _ = ref_all
    inits.set_random_seed(7)  # (the draws of the two decoders do not depend on the tests run before)
    dg, ph, model, opt, feed = _setup(golden_S, decoders_override={(1, 1): "distmult", (0, 1): "innerproduct"})
    kinds = {et: type(dec).__name__ for et, dec in model.edge_type2decoder.items()}
    assert kinds[1, 1] == "DistMultDecoder" and kinds[0, 1] == "InnerProductDecoder"
    sess = dg.Session()
    cost_sum, total = _per_relation_sum(sess, ph, model, opt, feed, batches, negs)
    cost, gv = train_step_all(sess, opt, ph, feed, batches, neg_samples=negs, apply=False)
    assert abs(cost - cost_sum) <= 1e-5 * abs(cost_sum)
    _assert_grads(gv, total)
    names = list(model.vars)
    dist = [q for q, nm in enumerate(names) if "relation_" in nm and model.vars[nm].tensor.dim() == 1]
    assert len(dist) == model.edge_types[1, 1] and all(np.any(gv[q][0] != 0) for q in dist)

    eb = _edge_batches(golden_S, model, opt, sess.device)
    hb = eb.host_batch(0, 0)
    assert (1, 1) in hb and (0, 1) in hb
    fed = _fed_negatives(golden_S, hb, 5)
    host = train_step_all(sess, opt, ph, feed, hb, neg_samples=fed, apply=False)
    for _ in range(2):
        _same(host, train_step_all(sess, opt, ph, feed, eb.batch(0, 0), neg_samples=fed, apply=False))
    assert any(np.any(g != 0) for g, _ in host[1])


def test_one_applied_step_is_tf_adam_and_shares_its_slots(golden_S, ref_all):
    """apply=True: the parameters after the step equal oracle.adam_tf (t = 1) on the summed
    gradient the device computed on the same state (apply=False; held to the oracle's sum in the
    test above — at t = 1 Adam moves every element by ≈ lr·sign(g), so a reference gradient whose
    tiny entries differ in sign would not be a check of the update).  Then one ordinary opt_op step
    is TF's step t = 2 on the SAME slots."""
    from decagon_amd.trainall import train_step_all
    from test_gpu_train import _batch_feed

    batches, negs, cost_ref, _, _ = ref_all
    dg, ph, model, opt, feed = _setup(golden_S)
    sess = dg.Session()
    params = list(model.vars.values())
    _, gv = train_step_all(sess, opt, ph, feed, batches, neg_samples=negs, apply=False)
    before = [p.eval() for p in params]
    cost = train_step_all(sess, opt, ph, feed, batches, neg_samples=negs)
    assert isinstance(cost, float) and abs(cost - cost_ref) <= 1e-5 * abs(cost_ref)
    m, v = [], []
    for (g, _), p0, prm in zip(gv, before, params):
        pw, m1, v1 = orc.adam_tf(p0, g, np.zeros_like(p0), np.zeros_like(p0), 1)
        m.append(m1)
        v.append(v1)
        assert np.max(np.abs(prm.eval() - pw)) <= 1e-6 * max(1.0, np.max(np.abs(pw))), prm.name
    f, e, rt, ct = _batch_feed(golden_S, ph, opt, feed, 3)
    gv2 = sess.run(opt.grads_vars, feed_dict=f)
    before = [p.eval() for p in params]
    sess.run(opt.opt_op, feed_dict=f)
    for i, ((g, _), p0, prm) in enumerate(zip(gv2, before, params)):
        pw, _, _ = orc.adam_tf(p0, g, m[i], v[i], 2)
        assert np.max(np.abs(prm.eval() - pw)) <= 1e-6 * max(1.0, np.max(np.abs(pw))), prm.name
    assert len([k for k in sess.caches if isinstance(k, tuple) and k[0] == "adam"]) == 1


def test_device_drawn_negatives_are_the_slot_samplers(golden_S):
    """neg_samples=None: relation k's negatives are dg_unigram_sample_slots' draws from ITS table
    for the optimizer's seed and draw counter — feeding the wrapper's draws gives the same bits —
    and the counter advances by the number of draws."""
    from decagon_amd import kernels
    from decagon_amd.trainall import train_step_all

    nk = 40
    batches, _ = R.make_batches(golden_S, sizes=[nk] * 10)
    dg, ph, model, opt, feed = _setup(golden_S)
    sess = dg.Session()
    opt.seed = 1234
    drawn = train_step_all(sess, opt, ph, feed, batches, apply=False)
    sampler = sess.caches[("sampler", id(opt))]
    assert sampler.counter == 10 * nk
    negs, first = {}, 0
    for (i, j), K in model.edge_types.items():
        tabs = torch.stack(sampler.tables[first:first + K])
        padded = torch.cat([torch.zeros_like(tabs[:1]).expand(first, -1, -1), tabs]).contiguous()  # slots 0 .. first + K
        got = kernels.unigram_sample_slots(padded, first, nk, K * nk, opt.seed).cpu().numpy()  # counter first·nk
        negs[i, j] = {k: got[k * nk:(k + 1) * nk] for k in range(K)}
        first += K
    fed = train_step_all(sess, opt, ph, feed, batches, neg_samples=negs, apply=False)
    assert sampler.counter == 10 * nk  # fed negatives draw nothing
    assert drawn[0] == fed[0]
    for (g0, _), (g1, _) in zip(drawn[1], fed[1]):
        assert np.array_equal(g0, g1)
    again = train_step_all(sess, opt, ph, feed, batches, apply=False)  # new draws: counter 400 ..
    assert sampler.counter == 20 * nk
    assert again[0] != drawn[0]


def test_step_with_dropout_matches_the_oracle_on_the_same_masks(golden_S):
    """At dropout 0.1: a batch of one relation per edge type against the float64 reference on the
    masks the device draws for step 1 (test_gpu_train.py's route)."""
    from decagon_amd.trainall import train_step_all
    from test_cpu_train_oracle import _masks

    allb, alln = R.make_batches(golden_S)
    batches = {et: {0: per[0]} for et, per in allb.items()}
    negs = {et: {0: per[0]} for et, per in alln.items()}
    ets, _, _, _, _, adj = R.oracle_inputs(golden_S)
    drop1, drop2 = _masks(ets, adj, 0.9, step=1)
    cost_ref, grads, zs = R.reference(golden_S, batches, negs, drop1, drop2)
    assert np.min(np.abs(zs)) >= 1e-3
    dg, ph, model, opt, feed = _setup(golden_S)
    f = dict(feed)
    f[ph["dropout"]] = 0.1
    sess = dg.Session()
    cost, gv = train_step_all(sess, opt, ph, f, batches, neg_samples=negs, apply=False)
    assert abs(cost - cost_ref) <= 1e-5 * abs(cost_ref)
    _assert_grads(gv, _want(model, grads))
    st = model.dropout_state(type("C", (), {"session": sess})())
    assert int(st[1]) == 1  # one forward with dropout was run


def test_error_paths(golden_S):
    from decagon_amd.trainall import train_step_all

    batches, negs = R.make_batches(golden_S)
    dg, ph, model, opt, feed = _setup(golden_S)
    sess = dg.Session()
    sess.shard = object()  # a sharded session
    with pytest.raises(NotImplementedError):
        train_step_all(sess, opt, ph, feed, batches, neg_samples=negs)
    sess.shard = None
    f = dict(feed)
    f[opt.latent_inters[0]] = np.eye(32, dtype=np.float32)  # a fed latent
    with pytest.raises(dg.InvalidArgumentError):
        train_step_all(sess, opt, ph, f, batches, neg_samples=negs)
    f = dict(feed)
    f[opt.cost] = 1.0
    with pytest.raises(dg.InvalidArgumentError):
        train_step_all(sess, opt, ph, f, batches, neg_samples=negs)
    twice = dict(batches)
    twice[1, 1] = [(0, batches[1, 1][0]), (2, batches[1, 1][2]), (0, batches[1, 1][0])]  # a repeated relation
    with pytest.raises(ValueError):
        train_step_all(sess, opt, ph, feed, twice, neg_samples=negs)
    with pytest.raises(ValueError):  # unequal batch sizes and nothing fed
        train_step_all(sess, opt, ph, feed, batches)
    # none of the refused calls trained anything
    assert not [k for k in sess.caches if isinstance(k, tuple) and k[0] == "adam"]

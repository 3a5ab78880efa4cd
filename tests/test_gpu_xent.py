"""GPU: training on the cross-entropy cost — dg_xent_loss_ws_f32, dg_decoder_grad_xent_f32 and
dg_decoder_grad_seg_xent_f32 against float64, and DecagonOptimizer(loss="xent") on the golden S
model (grads_vars, opt_op, trainall.train_step_all) against the autograd reference of
tests/_xent_ref.py, which test_cpu_xent.py holds to the oracle first.

Bars: gradients max|got − want| <= 1e-4·max|want| per output (test_gpu_trainall.py's), costs 1e-4
relative (test_gpu_kernels.py's and test_gpu_model.py's for the existing losses), the published
coefficients 1e-6 absolute.
"""
import numpy as np
import pytest

import _trainall_ref as R
import _xent_ref as X
from oracle import decagon_oracle as orc
from test_gpu_model import _setup

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TOL = 1e-4
SENTINEL = 7.5


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


def _T(x, dt=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(x)).to(_dev(), dt)


def _held(got, want, what=""):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, what
    assert np.all(np.isfinite(got)), what
    scale = np.max(np.abs(want))
    if scale == 0:
        assert np.max(np.abs(got)) == 0.0, what
    else:
        err = np.max(np.abs(got - want))
        print(f"{what}: max err {err:.3e}, scale {scale:.3e}, ratio {err / scale:.2e}")
        assert err <= TOL * scale, f"{what} off by {err / scale:.2e}"


def _sigmoid(x):
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0, e) / (1.0 + e)


# ------------------------------------------------------------------ the many-workgroup cost sum
SPECIAL = [0.0, 88.0, -88.0, 104.0, -104.0]


@pytest.mark.parametrize("w", [1.0, 0.25, 0.0])
@pytest.mark.parametrize("n", [1, 31, 256, 257, 65537])
def test_workspace_xent_sum_matches_the_oracle(n, w):
    from decagon_amd import kernels

    dev = _dev()
    rng = np.random.default_rng(n)
    pos = rng.uniform(-30, 30, n).astype(np.float32)
    neg = rng.uniform(-30, 30, n).astype(np.float32)
    for q in range(min(n, len(SPECIAL))):  # the exact values, on both sides
        pos[q], neg[q] = SPECIAL[q], SPECIAL[(q + 1) % len(SPECIAL)]
    want = orc.xent_loss(pos.astype(np.float64), neg.astype(np.float64), w)
    ws = kernels.hinge_workspace(dev)
    p, g = _T(pos), _T(neg)
    first = kernels.xent_loss(p, g, w, workspace=ws).cpu().numpy()
    assert int(ws[0]) == 0  # the workspace's first word is zero again
    second = kernels.xent_loss(p, g, w, workspace=ws).cpu().numpy()
    assert np.isfinite(first[0]) and first.tobytes() == second.tobytes()
    print(f"n={n} w={w}: got {first[0]!r}, want {want!r}, rel {abs(first[0] - want) / want:.2e}")
    assert abs(float(first[0]) - want) <= TOL * want
    # the same workspace serves the hinge sum next
    h = kernels.hinge_loss(p, g, 0.1, workspace=ws).cpu().numpy()
    want_h = orc.hinge_loss(pos.astype(np.float64), neg.astype(np.float64), 0.1)
    assert abs(float(h[0]) - want_h) <= TOL * want_h
    assert int(ws[0]) == 0


# ------------------------------------------------------------------ dg_decoder_grad_xent_f32
NR, NC = 9, 7  # table rows: rows, negatives and columns all repeat within a batch


def _pair_case(n, d, with_l, seed):
    rng = np.random.default_rng(seed)
    U = rng.standard_normal((NR, d)).astype(np.float32)
    V = rng.standard_normal((NC, d)).astype(np.float32)
    rows, cols, negs = rng.integers(0, NR, n), rng.integers(0, NC, n), rng.integers(0, NR, n)
    negs[::5] = rows[::5]  # some negative row is its positive row
    G = (rng.standard_normal((d, d)) / np.sqrt(d)).astype(np.float32)
    l = (1.0 + 0.3 * rng.standard_normal(d)).astype(np.float32) if with_l else None
    return U, V, rows, cols, negs, G, l


def _run_pairs(U, V, rows, cols, negs, pos, neg, G, l, w, outputs):
    from decagon_amd import kernels

    dev = _dev()
    d = G.shape[0]
    outs = {}
    if "dG" in outputs:
        outs["dG"] = torch.full((d, d), SENTINEL, device=dev)
    if "dl" in outputs:
        outs["dl"] = torch.full((d,), SENTINEL, device=dev)
    if "dG_diag" in outputs:
        outs["dG_diag"] = torch.full((d,), SENTINEL, device=dev)
    op = kernels.PreparedDecoderGrad(_T(U), _T(V), _T(rows, torch.int32), _T(cols, torch.int32), _T(negs, torch.int32),
                                     _T(pos), _T(neg), _T(G), _T(l) if l is not None else None, 0.1, **outs,
                                     loss="xent", neg_weight=w)
    op()
    torch.cuda.synchronize()
    return op.grad_rows.cpu().numpy(), op.grad_cols.cpu().numpy(), {k: v.cpu().numpy() for k, v in outs.items()}


def _hold_pairs(case, pos, neg, w, outputs, tag):
    U, V, rows, cols, negs, G, l = case
    gr, gc, outs = _run_pairs(U, V, rows, cols, negs, pos, neg, G, l, w, outputs)
    a, b, want_rows, want_cols, dM, dG, dl, dgd = X.closed_form(U, V, rows, cols, negs, pos, neg, G, l, w)
    _held(gr, want_rows, tag + " grad_rows")
    _held(gc, want_cols, tag + " grad_cols")
    for name, want in (("dG", dG), ("dl", dl), ("dG_diag", dgd)):
        if name in outs:
            _held(outs[name], want, tag + " " + name)
    return a, b, gr, gc, outs


@pytest.mark.parametrize("w", [1.0, 0.5])
@pytest.mark.parametrize("outputs", ["dG+dl", "dG_diag", "none"])
@pytest.mark.parametrize("with_l", [True, False])
@pytest.mark.parametrize("n,d", [(1, 32), (63, 32), (64, 64), (65, 32), (130, 96)])  # both sides of kPairChunk = 64
def test_per_relation_gradient_matches_float64(n, d, with_l, outputs, w):
    outs = {"dG+dl": ["dG", "dl"] if with_l else ["dG"], "dG_diag": ["dG_diag"], "none": []}[outputs]
    case = _pair_case(n, d, with_l, 1000 * n + d)
    rng = np.random.default_rng(n + d)
    pos = (2.0 * rng.standard_normal(n)).astype(np.float32)
    neg = (2.0 * rng.standard_normal(n)).astype(np.float32)
    _hold_pairs(case, pos, neg, w, outs, f"n={n} d={d} l={with_l} w={w}")


def test_saturated_scores_keep_their_small_coefficients():
    """(a) pos in [16, 20], neg in [−20, −16]: every coefficient lies in [2e-9, 1.2e-7], and the
    bar is relative to the outputs' own maximum — a coefficient formed as 1 − σ(pos) is 0 or a
    multiple of 6e-8 there and fails it."""
    n, d = 65, 32
    case = _pair_case(n, d, True, 77)
    rng = np.random.default_rng(78)
    pos = rng.uniform(16, 20, n).astype(np.float32)
    neg = rng.uniform(-20, -16, n).astype(np.float32)
    a, b, gr, gc, outs = _hold_pairs(case, pos, neg, 1.0, ["dG", "dl"], "saturated")
    assert 2e-9 <= a.min() and a.max() <= 1.2e-7 and 2e-9 <= b.min() and b.max() <= 1.2e-7
    assert np.max(np.abs(gr)) > 0 and np.max(np.abs(outs["dG"])) > 0


def test_fully_wrong_scores_have_unit_coefficients():
    """(b) pos = −100, neg = +100: the coefficients are exactly −1 and w; everything is finite."""
    n, d, w = 65, 32, 0.5
    case = _pair_case(n, d, True, 79)
    pos, neg = np.full(n, -100.0, np.float32), np.full(n, 100.0, np.float32)
    a, b, gr, gc, outs = _hold_pairs(case, pos, neg, w, ["dG", "dl"], "unit")
    assert np.all(a == 1.0) and np.all(b == w)
    # −1·mv and 0.5·mv of the same mv: exactly −2 apart
    assert np.array_equal(gr[:n], -2.0 * gr[n:]) and np.max(np.abs(gr)) > 0


def test_zero_negative_weight_gives_zero_negative_rows():
    """(c) w = 0: grad_rows[n:] is exactly zero."""
    n, d = 65, 32
    case = _pair_case(n, d, True, 80)
    rng = np.random.default_rng(81)
    pos, neg = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    a, b, gr, gc, outs = _hold_pairs(case, pos, neg, 0.0, ["dG", "dl"], "w=0")
    assert np.all(gr[n:] == 0.0) and np.max(np.abs(gr[:n])) > 0


# ------------------------------------------------------------------ dg_decoder_grad_seg_xent_f32
N_REL, SNR, SNC = 10, 37, 29
SEG_SIZES = [33, 40, 7, 64, 32, 0, 50]  # a sub-tile + 1, a ragged one, a sub-tile, several tiles, a full tile, empty
SEG_REL = [8, 2, 5, 0, 9, 3, 6]         # a permutation of a relation set with gaps: 1, 4, 7 have no segment
SEG_PTR = np.concatenate([[0], np.cumsum(SEG_SIZES)])
BAD_PAIR = 50                            # its row index lies outside the table


def _seg_case(kind, d):
    rng = np.random.default_rng(300 + d)
    n = int(SEG_PTR[-1])
    U = rng.standard_normal((SNR, d)).astype(np.float32)
    V = rng.standard_normal((SNC, d)).astype(np.float32)
    rows, cols, negs = rng.integers(0, SNR, n), rng.integers(0, SNC, n), rng.integers(0, SNR, n)
    rows[BAD_PAIR] = SNR
    pos = (2.0 * rng.standard_normal(n)).astype(np.float32)
    neg = (2.0 * rng.standard_normal(n)).astype(np.float32)
    if kind == "dedicom":  # a shared G with per-relation l
        G = (rng.standard_normal((d, d)) / np.sqrt(d)).astype(np.float32)
        l = (1.0 + 0.3 * rng.standard_normal((N_REL, d))).astype(np.float32)
    elif kind == "bilinear":  # per-relation dense G
        G, l = (rng.standard_normal((N_REL, d, d)) / np.sqrt(d)).astype(np.float32), None
    else:  # distmult: per-relation G with dG_diag
        G = np.stack([np.diag(rng.standard_normal(d)) for _ in range(N_REL)]).astype(np.float32)
        l = None
    return U, V, rows, cols, negs, pos, neg, G, l


def _seg_reference(kind, d, U, V, rows, cols, negs, pos, neg, G, l, w):
    n = len(rows)
    f = lambda x: np.asarray(x, np.float64)  # noqa: E731
    a, b = _sigmoid(-f(pos)), w * _sigmoid(f(neg))
    a[BAD_PAIR] = b[BAD_PAIR] = 0.0
    U64, V64 = f(U), f(V)
    rs = np.where(rows < SNR, rows, 0)
    mv, gc = np.zeros((n, d)), np.zeros((n, d))
    dG = np.zeros((d, d)) if kind == "dedicom" else np.full((N_REL, d, d), SENTINEL)
    dl, dgd = np.full((N_REL, d), SENTINEL), np.full((N_REL, d), SENTINEL)
    for s, k in enumerate(SEG_REL):
        p = slice(int(SEG_PTR[s]), int(SEG_PTR[s + 1]))
        Gk = f(G if G.ndim == 2 else G[k])
        L = np.diag(f(l[k])) if l is not None else np.eye(d)
        M = L @ Gk @ L
        mv[p] = V64[cols[p]] @ M.T
        x = b[p, None] * U64[negs[p]] - a[p, None] * U64[rs[p]]
        gc[p] = x @ M
        dM = x.T @ V64[cols[p]]
        if kind == "dedicom":
            dG += L @ dM @ L
            dl[k] = np.diag(dM @ (Gk @ L).T + (L @ Gk).T @ dM)
        else:
            dG[k] = L @ dM @ L
            dgd[k] = np.diag(dM)
    mv[BAD_PAIR] = 0.0
    return a, b, mv, gc, dG, dl, dgd


@pytest.mark.parametrize("w", [1.0, 0.5])
@pytest.mark.parametrize("d", [32, 64])
@pytest.mark.parametrize("kind", ["dedicom", "bilinear", "distmult"])
def test_segmented_gradient_matches_float64(kind, d, w):
    from decagon_amd import kernels

    dev = _dev()
    U, V, rows, cols, negs, pos, neg, G, l = _seg_case(kind, d)
    a, b, mv, gc, dG, dl, dgd = _seg_reference(kind, d, U, V, rows, cols, negs, pos, neg, G, l, w)
    n = len(rows)
    full = lambda *shape: torch.full(shape, SENTINEL, device=dev)  # noqa: E731
    outs = {}
    if kind == "dedicom":
        outs = {"dG": full(d, d), "dl": full(N_REL, d)}
    elif kind == "bilinear":
        outs = {"dG": full(N_REL, d, d)}
    else:
        outs = {"dG_diag": full(N_REL, d)}
    op = kernels.PreparedDecoderGradSeg(_T(U), _T(V), _T(rows, torch.int32), _T(cols, torch.int32),
                                        _T(negs, torch.int32), _T(SEG_PTR, torch.int32), _T(SEG_REL, torch.int32),
                                        _T(pos), _T(neg), _T(G), _T(l) if l is not None else None, 0.1, **outs,
                                        loss="xent", neg_weight=w)
    op()
    torch.cuda.synchronize()
    coef = op.coef.cpu().numpy()
    assert coef.shape == (2 * n,)
    assert np.max(np.abs(coef[:n] + a)) <= 1e-6 and np.max(np.abs(coef[n:] - b)) <= 1e-6
    assert coef[BAD_PAIR] == 0.0 and coef[n + BAD_PAIR] == 0.0  # the pair outside the tables weighs nothing
    tag = f"{kind} d={d} w={w}"
    got_mv = op.mv.cpu().numpy()
    _held(got_mv, mv, tag + " mv")
    _held(op.grad_cols.cpu().numpy(), gc, tag + " grad_cols")
    assert np.all(got_mv[BAD_PAIR] * coef[BAD_PAIR] == 0.0) and np.all(op.grad_cols.cpu().numpy()[BAD_PAIR] == 0.0)
    absent = [k for k in range(N_REL) if k not in SEG_REL]
    empty = SEG_REL[SEG_SIZES.index(0)]
    assert absent == [1, 4, 7]
    for name, want in (("dG", dG), ("dl", dl), ("dG_diag", dgd)):
        if name not in outs:
            continue
        got = outs[name].cpu().numpy()
        if got.ndim == want.ndim and got.shape[0] == N_REL:  # per-relation outputs, relation by relation
            for k in range(N_REL):
                if k in absent:
                    assert np.all(got[k] == SENTINEL), f"{name}[{k}] was written"
                elif k == empty:
                    assert np.all(got[k] == 0.0)
                else:
                    _held(got[k], want[k], f"{tag} {name}[{k}]")
        else:
            _held(got, want, tag + " " + name)


@pytest.mark.parametrize("d", [32, 64])
def test_single_segment_agrees_with_the_per_relation_kernel(d):
    from decagon_amd import kernels

    dev = _dev()
    n, w = 65, 0.5
    U, V, rows, cols, negs, G, l = _pair_case(n, d, True, 500 + d)
    rng = np.random.default_rng(d)
    pos = (2.0 * rng.standard_normal(n)).astype(np.float32)
    neg = (2.0 * rng.standard_normal(n)).astype(np.float32)
    gr, gc, outs = _run_pairs(U, V, rows, cols, negs, pos, neg, G, l, w, ["dG", "dl"])
    dG, dl = torch.full((d, d), SENTINEL, device=dev), torch.full((1, d), SENTINEL, device=dev)
    op = kernels.PreparedDecoderGradSeg(_T(U), _T(V), _T(rows, torch.int32), _T(cols, torch.int32),
                                        _T(negs, torch.int32), _T(np.array([0, n]), torch.int32), None, _T(pos),
                                        _T(neg), _T(G), _T(l[None, :]), 0.1, dG=dG, dl=dl, loss="xent", neg_weight=w)
    op()
    torch.cuda.synchronize()
    coef, mv = op.coef.cpu().numpy().astype(np.float64), op.mv.cpu().numpy().astype(np.float64)
    _held(np.concatenate([coef[:n, None] * mv, coef[n:, None] * mv]), gr, f"d={d} rows")
    _held(op.grad_cols.cpu().numpy(), gc, f"d={d} cols")
    _held(dG.cpu().numpy(), outs["dG"], f"d={d} dG")
    _held(dl.cpu().numpy()[0], outs["dl"], f"d={d} dl")


# ------------------------------------------------------------------ the model, golden S
def _setup_xent(z, w, loss="xent", **kw):
    """test_gpu_model._setup's model with a second optimizer on the cost under test."""
    dg, ph, model, opt, feed = _setup(z, **kw)
    xe = dg.DecagonOptimizer(embeddings=model.embeddings, latent_inters=model.latent_inters,
                             latent_varies=model.latent_varies, degrees=opt.degrees, edge_types=opt.edge_types,
                             edge_type2dim=opt.edge_type2dim, placeholders=ph, batch_size=512, margin=0.1,
                             neg_sample_weights=w, loss=loss)
    return dg, ph, model, opt, xe, feed


@pytest.fixture(scope="module")
def all_batches(golden_S):
    return R.make_batches(golden_S)


@pytest.fixture(scope="module")
def refs(golden_S, all_batches):
    """The float64 references, each computed once: key → (cost, grads, scores)."""
    cache = {}

    def get(w, pick=None, dropout=False):
        key = (w, pick, dropout)
        if key not in cache:
            allb, alln = all_batches
            b, ng = allb, alln
            if pick is not None:
                i, j, k = pick
                b, ng = {(i, j): {k: allb[i, j][k]}}, {(i, j): {k: alln[i, j][k]}}
            drop1 = drop2 = None
            if dropout:
                from test_cpu_train_oracle import _masks

                ets, _, _, _, _, adj = R.oracle_inputs(golden_S)
                drop1, drop2 = _masks(ets, adj, 0.9, step=1)
            cache[key] = X.reference(golden_S, b, ng, "xent", w=w, drop1=drop1, drop2=drop2)
        return cache[key]

    return get


def _want(model, grads):
    return R.wanted(model.edge_types, {et: list(model.edge_type2decoder[et].vars) for et in model.edge_types}, grads)


def _assert_grads(gv, want, tag):
    assert len(gv) == len(want)
    nonzero = 0
    for q, ((g, v), w) in enumerate(zip(gv, want)):
        assert g.shape == w.shape
        if np.max(np.abs(w)) > 0:
            nonzero += 1
        _held(g, w, f"{tag} gradient {q}")
    assert nonzero > 0


def _relation_feed(ph, opt, feed, batches, negs, i, j, k, e, dropout=0.0):
    f = dict(feed)
    f.update({ph["batch"]: batches[i, j][k], ph["batch_edge_type_idx"]: e, ph["batch_row_edge_type"]: i,
              ph["batch_col_edge_type"]: j, opt.neg_samples: negs[i, j][k], ph["dropout"]: dropout})
    return f


@pytest.mark.parametrize("w,dropout", [(1.0, False), (0.5, False), (0.5, True)])
def test_grads_vars_match_the_autograd_reference(golden_S, all_batches, refs, w, dropout):
    """One relation of each decoder kind; with dropout 0.1 on the masks the device draws for step 1
    (a fresh Session per relation: test_gpu_train.py's route)."""
    allb, alln = all_batches
    dg, ph, model, _, xe, feed = _setup_xent(golden_S, w)
    sess = dg.Session()
    for i, j, k, e in X.one_per_decoder_kind(golden_S):
        if dropout:
            sess = dg.Session()
        cost_ref, grads, _ = refs(w, (i, j, k), dropout)
        f = _relation_feed(ph, xe, feed, allb, alln, i, j, k, e, 0.1 if dropout else 0.0)
        gv, cost = sess.run([xe.grads_vars, xe.cost], feed_dict=f)
        print(f"w={w} dropout={dropout} relation {(i, j, k)}: cost {float(cost)!r} want {cost_ref!r}")
        assert abs(float(cost) - cost_ref) <= TOL * cost_ref
        _assert_grads(gv, _want(model, grads), f"w={w} dropout={dropout} {(i, j, k)}")


@pytest.mark.parametrize("w", [1.0, 0.5])
def test_all_relation_step_matches_the_summed_reference(golden_S, all_batches, refs, w):
    """train_step_all(apply=False) over a batch of every relation against the reference of the
    summed cost (the gradient of a sum is the sum of the per-relation gradients: one backward)."""
    from decagon_amd.trainall import train_step_all

    allb, alln = all_batches
    cost_ref, grads, scores = refs(w)
    assert len(scores) == 10
    dg, ph, model, _, xe, feed = _setup_xent(golden_S, w)
    sess = dg.Session()
    before = [p.eval() for p in model.vars.values()]
    cost, gv = train_step_all(sess, xe, ph, feed, allb, neg_samples=alln, apply=False)
    print(f"w={w}: cost {cost!r} want {cost_ref!r}")
    assert isinstance(cost, float) and abs(cost - cost_ref) <= TOL * cost_ref
    _assert_grads(gv, _want(model, grads), f"all relations w={w}")
    for (g, v), p, b in zip(gv, model.vars.values(), before):
        assert np.array_equal(v, b) and np.array_equal(p.eval(), b)
    # every pair trains: no relation's decoder gradient is zero (under the hinge inactive pairs drop out)
    assert all(np.any(g != 0) for g, _ in gv)


def test_device_batches_equal_host_batches_bit_for_bit(golden_S):
    from decagon_amd.trainall import train_step_all
    from test_gpu_epochs import _edge_batches, _fed_negatives, _same

    dg, ph, model, _, xe, feed = _setup_xent(golden_S, 0.5)
    sess = dg.Session()
    eb = _edge_batches(golden_S, model, xe, sess.device)
    hb = eb.host_batch(0, 0)
    fed = _fed_negatives(golden_S, hb, 5)
    host = train_step_all(sess, xe, ph, feed, hb, neg_samples=fed, apply=False)
    for _ in range(2):
        _same(host, train_step_all(sess, xe, ph, feed, eb.batch(0, 0), neg_samples=fed, apply=False))
    assert host[0] > 0 and any(np.any(g != 0) for g, _ in host[1])


def test_device_drawn_negatives_train_on_the_xent_cost(golden_S):
    """Negatives not fed: `cost` is the xent cost of the run's own outputs / neg_outputs, and the
    all-relation step on drawn negatives equals the step fed the sampler's draws."""
    from decagon_amd import kernels
    from decagon_amd.trainall import train_step_all

    w, nk = 0.5, 40
    dg, ph, model, _, xe, feed = _setup_xent(golden_S, w)
    sess = dg.Session()
    allb, alln = R.make_batches(golden_S, sizes=[nk] * 10)
    f = _relation_feed(ph, xe, feed, allb, alln, 1, 1, 0, 4)
    del f[xe.neg_samples]
    cost, pos, neg = sess.run([xe.cost, xe.outputs, xe.neg_outputs], feed_dict=f)
    want = orc.xent_loss(np.asarray(pos, np.float64), np.asarray(neg, np.float64), w)
    assert abs(float(cost) - want) <= TOL * want
    sess.run(xe.opt_op, feed_dict=f)  # trains on drawn negatives

    sess = dg.Session()
    xe.seed = 1234
    drawn = train_step_all(sess, xe, ph, feed, allb, apply=False)
    sampler = sess.caches[("sampler", id(xe))]
    assert sampler.counter == 10 * nk
    negs, first = {}, 0
    for (i, j), K in model.edge_types.items():
        tabs = torch.stack(sampler.tables[first:first + K])
        padded = torch.cat([torch.zeros_like(tabs[:1]).expand(first, -1, -1), tabs]).contiguous()
        got = kernels.unigram_sample_slots(padded, first, nk, K * nk, xe.seed).cpu().numpy()
        negs[i, j] = {k: got[k * nk:(k + 1) * nk] for k in range(K)}
        first += K
    fed = train_step_all(sess, xe, ph, feed, allb, neg_samples=negs, apply=False)
    assert drawn[0] == fed[0] and drawn[0] > 0
    for (g0, _), (g1, _) in zip(drawn[1], fed[1]):
        assert np.array_equal(g0, g1)


def test_one_applied_step_is_tf_adam_and_shares_its_slots(golden_S, all_batches, refs):
    """apply=True at t = 1 against oracle.adam_tf, then one opt_op step as TF's t = 2 on the SAME slots.

    At t = 1 Adam moves element x by lr·g/(|g| + ε'), ε' = ε/√(1 − β2) = 3.2e-7: the sign of g
    times lr wherever |g| >> ε'.  The update is therefore held (1) everywhere to adam_tf on the
    gradient the device computed on the same state (apply=False, held to the reference above), at
    test_gpu_trainall.py's 1e-6, and (2) to adam_tf on the float64 REFERENCE gradient wherever that
    gradient is resolved, |g_ref| >= 1e-3·max|g_ref|: there the device's gradient is within
    δ = 1e-4·max|g_ref| of it (the bar above) and cannot differ in sign, and the step's derivative
    lr·ε'/(|g| + ε')² bounds the difference by lr·ε'·δ/(|g_ref| − δ)², added to the 1e-6."""
    from decagon_amd.trainall import train_step_all
    from test_gpu_train import _batch_feed

    w, lr, eps1 = 0.5, 1e-3, 1e-8 / np.sqrt(1e-3)
    allb, alln = all_batches
    cost_ref, grads, _ = refs(w)
    dg, ph, model, _, xe, feed = _setup_xent(golden_S, w)
    sess = dg.Session()
    params = list(model.vars.values())
    _, gv = train_step_all(sess, xe, ph, feed, allb, neg_samples=alln, apply=False)
    before = [p.eval() for p in params]
    cost = train_step_all(sess, xe, ph, feed, allb, neg_samples=alln)
    assert isinstance(cost, float) and abs(cost - cost_ref) <= TOL * cost_ref
    m, v, resolved = [], [], 0
    for (g, _), gref, p0, prm in zip(gv, _want(model, grads), before, params):
        got = prm.eval()
        pw, m1, v1 = orc.adam_tf(p0, g, np.zeros_like(p0), np.zeros_like(p0), 1)
        m.append(m1)
        v.append(v1)
        assert np.max(np.abs(got - pw)) <= 1e-6 * max(1.0, np.max(np.abs(pw))), prm.name
        gref = np.asarray(gref, np.float64).reshape(p0.shape)
        scale = np.max(np.abs(gref))
        sel = np.abs(gref) >= 1e-3 * scale if scale > 0 else np.zeros(p0.shape, bool)
        if sel.any():
            pr, _, _ = orc.adam_tf(p0, gref, np.zeros_like(p0), np.zeros_like(p0), 1)
            delta = TOL * scale
            bound = 1e-6 * max(1.0, np.max(np.abs(pr))) + lr * eps1 * delta / (np.abs(gref[sel]) - delta) ** 2
            assert np.all(np.abs(got[sel] - pr[sel]) <= bound), prm.name
            resolved += int(sel.sum())
    assert resolved > 1000
    f, e, rt, ct = _batch_feed(golden_S, ph, xe, feed, 3)
    gv2 = sess.run(xe.grads_vars, feed_dict=f)
    before = [p.eval() for p in params]
    sess.run(xe.opt_op, feed_dict=f)
    for i, ((g, _), p0, prm) in enumerate(zip(gv2, before, params)):
        pw, _, _ = orc.adam_tf(p0, g, m[i], v[i], 2)
        assert np.max(np.abs(prm.eval() - pw)) <= 1e-6 * max(1.0, np.max(np.abs(pw))), prm.name
    assert len([k for k in sess.caches if isinstance(k, tuple) and k[0] == "adam"]) == 1


def test_explicit_hinge_is_the_default_bit_for_bit(golden_S, all_batches):
    from decagon_amd.trainall import train_step_all
    from test_gpu_train import _batch_feed

    allb, alln = all_batches
    dg, ph, model, opt, hinge, feed = _setup_xent(golden_S, 0.25, loss="hinge")  # (the weight is unused)
    assert opt.loss == hinge.loss == "hinge"
    sess = dg.Session()
    out = []
    for o in (opt, hinge):
        f, e, rt, ct = _batch_feed(golden_S, ph, o, feed, 3)
        gv, cost = sess.run([o.grads_vars, o.cost], feed_dict=f)
        step = train_step_all(sess, o, ph, feed, allb, neg_samples=alln, apply=False)
        out.append((gv, cost, step))
    (gv0, c0, s0), (gv1, c1, s1) = out
    assert np.asarray(c0).tobytes() == np.asarray(c1).tobytes() and s0[0] == s1[0]
    for (g0, _), (g1, _) in zip(list(gv0) + list(s0[1]), list(gv1) + list(s1[1])):
        assert np.array_equal(g0, g1)
    assert any(np.any(g != 0) for g, _ in gv0)


def test_error_paths(golden_S, all_batches):
    from decagon_amd.trainall import train_step_all

    allb, alln = all_batches
    dg, ph, model, opt, xe, feed = _setup_xent(golden_S, 0.5)
    sess = dg.Session()
    f = _relation_feed(ph, xe, feed, allb, alln, 1, 1, 0, 4)
    for node in (xe.cost, xe.outputs, xe.neg_outputs):
        fed = dict(f)
        fed[node] = 1.0 if node is xe.cost else np.zeros(len(allb[1, 1][0]), np.float32)
        for fetch in (xe.grads_vars, xe.opt_op):
            with pytest.raises(dg.InvalidArgumentError):
                sess.run(fetch, feed_dict=fed)
    g = dict(feed)
    g[xe.cost] = 1.0
    with pytest.raises(dg.InvalidArgumentError):
        train_step_all(sess, xe, ph, g, allb, neg_samples=alln)
    with pytest.raises(ValueError):
        _setup_xent(golden_S, 0.5, loss="bogus")
    # a sharded session is refused, not left untested
    sess.shard = object()
    for fetch in (xe.grads_vars, xe.opt_op):
        with pytest.raises(NotImplementedError):
            sess.run(fetch, feed_dict=f)
    with pytest.raises(NotImplementedError):
        train_step_all(sess, xe, ph, feed, allb, neg_samples=alln)
    sess.shard = None
    assert not [k for k in sess.caches if isinstance(k, tuple) and k[0] == "adam"]  # nothing trained

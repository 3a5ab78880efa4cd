"""GPU: the weighted wave tables (PreparedFusedTab(weighted=T): wave slots in proportion to pairs)
through the kernels that run them — gcn_tab_kernel's 16-wave instances of the plain 64 -> 64
launch, the 64 -> 64 launch with the projecting tail and the 32 -> 32 launch with decoder rows —
on _tab_weighted_cases' graph (groups of 1, 2 and 6 relations; 0 to 400 pairs a group and row, so
waves of one chunk of gathers, of a full ring, of overflow batches, and groups of 1 to 16 waves for
the finishing sum), and a config-S forward with the engine's knob on and off.

On the integer set every fp32 sum is exact in any order, so the rows equal the seg form's bit for
bit, and P and Q — computed from the stored row by arithmetic no table changes — those of the
tables that ship today.  On Gaussian data the rows are within test_gpu_tab.py's balanced bound, 1e-6 · max|y|, of
the seg form, and rows, P and Q within the project's 1e-4 (rel_err) of float64.
"""
import functools

import numpy as np
import pytest

import _tab_cases as tc
import _tab_weighted_cases as wc
from conftest import rel_err
from test_gpu_tab_instances import SENTINEL, _bits, _dev, _Launch

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TOL = 1e-4


@pytest.fixture(scope="module")
def K():
    from decagon_amd import kernels

    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return kernels


@functools.lru_cache(maxsize=None)
def _case(d, kind):
    """(targets, float64 references), built once and left unchanged."""
    targets = wc.make_targets(d, kind)
    if kind == "int":
        for t in targets:
            for g in t.groups:
                tc.assert_exact(g)
    return targets, [tc.fused_reference(t) for t in targets]


def _weighted(launch, T):
    assert launch.weighted == T and launch.balance
    assert (launch._tab.nw_stride, launch._tab.nw, launch.nw) == (16, 16, 16)
    return launch


def _check_rows(kind, got, seg, refs, what):
    for t, (a, b, ref) in enumerate(zip(got, seg, refs)):
        if kind == "int":
            assert np.array_equal(_bits(a), _bits(b)), (what, "rows against the seg form", t)
        else:
            delta = float(np.abs(a - b).max())
            print(f"{what} target {t}: max|row - seg form| = {delta:.3e} = {delta / np.abs(b).max():.3e} max|y|")
            assert delta <= 1e-6 * float(np.abs(b).max()), (what, t)
        err = rel_err(a, ref[0])
        print(f"{what} target {t}: rel_err against float64 {err:.3e}")
        assert err <= TOL, (what, t)


@pytest.mark.parametrize("kind", ["int", "gauss"])
@pytest.mark.parametrize("d,T", [(64, 16), (64, 24), (32, 32), (32, 48)])
def test_plain_rows(K, d, T, kind):
    targets, refs = _case(d, kind)
    dev = _Launch(K, targets, d)
    launch = _weighted(K.PreparedFusedTab(dev.targets, d, d, balance=True, weighted=T), T)
    assert launch._tname == "dg_gcn_fused_tab_f32"
    _check_rows(kind, dev.run(launch), dev.run(launch.seg_form), refs, f"plain {d} T {T} {kind}")


@pytest.mark.parametrize("share", [True, False])
@pytest.mark.parametrize("kind", ["int", "gauss"])
def test_projecting_tail(K, kind, share):
    """64 -> 64 with projection jobs: target 0's rows onto 3 relations (a slab map) and 2, target
    1's onto 7 — with `share`, workgroups of up to four rows, two to a job wave."""
    d, T = 64, 24
    targets, refs = _case(d, kind)
    dev = _Launch(K, targets, d)
    rng = np.random.default_rng(17)

    def jobs():
        out = []
        for t, n_rels, slab in ((0, 3, [4, 0, 2]), (0, 2, None), (1, 7, None)):
            k_slabs, rows = (5 if slab else n_rels), targets[t].n_rows
            out.append((t, n_rels, slab, k_slabs, rows))
        return out

    ws = []
    for t, n_rels, slab, k_slabs, rows in jobs():
        w = (rng.integers(-4, 5, size=(k_slabs, 64, 32)).astype(np.float32) if kind == "int"
             else (0.2 * rng.standard_normal((k_slabs, 64, 32))).astype(np.float32))
        used = slab if slab else list(range(n_rels))
        w[np.setdiff1d(np.arange(k_slabs), used)] = np.nan
        ws.append(w)

    def run(**kw):
        pjs, bufs = [], []
        for (t, n_rels, slab, k_slabs, rows), w in zip(jobs(), ws):
            buf = torch.full((k_slabs * rows * 32 + 32,), SENTINEL, device="cuda")
            pjs.append(K.TabProjSpec(t, _dev(w), buf[:k_slabs * rows * 32].view(k_slabs, rows, 32), n_rels, slab))
            bufs.append(buf)
        launch = K.PreparedFusedTab(dev.targets, d, d, projs=pjs, **kw)
        assert launch._tname == "dg_gcn_fused_tab_post_f32"
        h1 = dev.run(launch)
        ps = [b.cpu().numpy() for b in bufs]
        for p in ps:
            assert np.all(p[-32:] == SENTINEL), "the row past P"
        return launch, h1, [p[:-32].reshape(w.shape[0], -1, 32) for p, w in zip(ps, ws)]

    launch, h1, P = run(balance=True, weighted=T, share_proj=share)
    _weighted(launch, T)
    if share:
        assert max(rows for _, _, rows in launch.host_plan) > 2, "a workgroup with a second pair of rows"
    _check_rows(kind, h1, dev.run(launch.seg_form), refs, f"post share {share} {kind}")
    if kind == "int":
        # the equal-share table, jobs shared: exact sums, so the seg form's rows bit for bit
        _, h1_rel, P_rel = run(balance=True)
        for a, b in zip(h1_rel, h1):
            assert np.array_equal(_bits(a), _bits(b))
    for j, ((t, n_rels, slab, k_slabs, rows), w, p) in enumerate(zip(jobs(), ws, P)):
        used = slab if slab else list(range(n_rels))
        for sl in range(k_slabs):
            if sl not in used:
                assert np.all(p[sl] == SENTINEL), "an unused P slab"
                continue
            if kind == "int":
                assert np.array_equal(_bits(p[sl]), _bits(P_rel[j][sl])), ("P against the equal-share table", t, sl)
            want = h1[t].astype(np.float64) @ w[sl].astype(np.float64)
            err = rel_err(p[sl], want)
            assert err <= TOL, ("P against float64", t, sl, err)


@pytest.mark.parametrize("target", [0, 1])
@pytest.mark.parametrize("kind", ["int", "gauss"])
def test_decoder_rows(K, kind, target):
    d, T = 32, 32
    targets, refs = _case(d, kind)
    dev = _Launch(K, targets, d)
    rng = np.random.default_rng(23)
    if kind == "int":
        G = rng.integers(-4, 5, size=(32, 32)).astype(np.float32)
        l = rng.choice(np.float32([-2, -1, -0.5, 0.5, 1, 2]), size=32)
    else:
        G = (rng.standard_normal((32, 32)) / 6).astype(np.float32)
        l = rng.standard_normal(32).astype(np.float32)
    rows = targets[target].n_rows

    def run(**kw):
        qbuf = torch.full((16 * 32,), SENTINEL, device="cuda")
        dec = K.TabDecSpec(target, _dev(G), _dev(l), qbuf[:rows * 32].view(rows, 32))
        launch = K.PreparedFusedTab(dev.targets, d, d, dec=dec, **kw)
        assert launch._tname == "dg_gcn_fused_tab_dec_f32"
        E = dev.run(launch)
        Q = qbuf.cpu().numpy().reshape(16, 32)
        assert rows < 16 and np.all(Q[rows:] == SENTINEL), "a Q row past the flagged target's"
        return launch, E, Q[:rows]

    launch, E, Q = run(balance=True, weighted=T)
    _weighted(launch, T)
    _check_rows(kind, E, dev.run(launch.seg_form), refs, f"dec target {target} {kind}")
    if kind == "int":
        _, E_rel, Q_rel = run(balance=False)  # the per-relation table: the seg form's rows bit for bit
        assert np.array_equal(_bits(E[target]), _bits(E_rel[target]))
        assert np.array_equal(_bits(Q), _bits(Q_rel)), "Q against the per-relation table"
    e, lv = E[target].astype(np.float64), l.astype(np.float64)
    err = rel_err(Q, lv * ((e * lv) @ G.astype(np.float64)))
    assert err <= TOL, ("Q against float64", err)


def test_config_S_forward_with_the_knob_on_and_off(K, monkeypatch):
    """Config S through ForwardPlan and the fused decoder with TAB_WEIGHTED on and off; the knob
    changes the tables of both launches and nothing else.  The sampled negative rows are identical.
    Layer 1's rows differ by one launch's re-association of a group's sum: the balanced bound,
    1e-6 · max|y|.  The embeddings and the scores pass through both launches, the projections and
    the normalisations between them: the project's tolerance, 1e-4 (the figures are printed)."""
    from decagon_amd import engine, synthetic
    from test_gpu_preproject import _plan, _weights

    g = synthetic.load_S()
    w1, w2 = _weights(g, 1)
    rng = np.random.default_rng(3)
    rows = _dev(rng.integers(0, g.n_nodes[1], 512).astype(np.int32))
    cols = _dev(rng.integers(0, g.n_nodes[1], 512).astype(np.int32))
    alias = K.upload_alias(rng.integers(1, 30, g.n_nodes[1]).astype(np.float64), "cuda")
    Gd = _dev((rng.standard_normal((32, 32)) / 6).astype(np.float32))
    ld = _dev(rng.standard_normal(32).astype(np.float32))
    outs = {}
    # (both layers weighted, whatever T the engine ships for each)
    monkeypatch.setattr(engine, "TAB_WEIGHTED_T64", 24)
    monkeypatch.setattr(engine, "TAB_WEIGHTED_T32", 32)
    for on in (1, 0):
        monkeypatch.setattr(engine, "TAB_WEIGHTED", on)
        plan = _plan(g, w1, w2)
        l1, l2 = (ls[0] for ls in plan.spmm_launches)
        assert (l1.weighted, l2.weighted) == ((24, 32) if on else (0, 0))
        assert (l1.nw, l2.nw) == ((16, 16) if on else (8, 8))
        plan.run()
        E = plan.embeddings[1]
        dec = K.PreparedDecoderHinge(E, E, rows, cols, Gd, ld, 0.1, alias=alias, seed=7, offset=11)
        assert dec.attached
        assert plan.spmm_launches[1][0].weighted == l2.weighted, "the rebuilt launch keeps the table form"
        plan.run()
        dec()
        torch.cuda.synchronize()
        assert dec.entry == "dg_decoder_hinge_rows_f32"
        vals = {f"hidden1_{t}": h.cpu().numpy() for t, h in plan.hidden1.items()}
        vals.update({f"embeddings_{t}": e.cpu().numpy() for t, e in plan.embeddings.items()})
        vals.update({"pos": dec.pos.cpu().numpy(), "neg": dec.neg.cpu().numpy()})
        outs[on] = (vals, dec.neg_rows.cpu().numpy().copy())
    assert np.array_equal(outs[1][1], outs[0][1]), "decoder_neg_rows"
    for name, a in outs[1][0].items():
        b = outs[0][0][name]
        delta = float(np.abs(a - b).max()) / float(np.abs(b).max())
        print(f"{name}: max|on - off| = {delta:.3e} max|y|")
        assert delta <= (1e-6 if name.startswith("hidden1") else TOL), name

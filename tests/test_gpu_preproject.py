"""GPU: layer 2's operands made in layer 1's launch (DG_L2_PREPROJECT, the default for one-GPU
forward plans in the wave-table form): dg_gcn_fused_tab_post_f32's P stacks, the 32 -> 32
wave-table launch that gathers them, the whole forward against the float64 oracle and against
the reassociated form (knob off), and the plans that must keep the reassociated form.

Two graphs: config S itself, and a graph of config S's edge types on n = {0: 151, 1: 97} (odd
counts: the last gene workgroup has an empty row slot) whose per-row segment lengths are drawn
from {0, 1, 7, 8, 9, 63, 64, 65, 97}, capped at the column count — an empty segment, less than
one lane-group round of 8 pairs, exactly one round and one more, the 64-pair boundary, one
overflow batch — with a few rows whose every segment is empty.
"""
import numpy as np
import pytest

from conftest import rel_err

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TOL = 1e-4       # test_gpu_model.py's forward tolerance
TOL_GEMM = 1e-5  # test_gpu_gemm_paths.py's: Gaussian fp32 GEMM inputs against float64
LENS = [0, 1, 7, 8, 9, 63, 64, 65, 97]
EMPTY_ROWS = {0: [0, 75, 150], 1: [0, 48, 96]}


def _tiny_graph():
    from decagon_amd import synthetic

    base = synthetic.load_S()
    n = {0: 151, 1: 97}
    rng = np.random.default_rng(7)
    adj = {}
    for (i, j), K in base.edge_types.items():
        rels = []
        for _ in range(K):
            lens = np.minimum(rng.choice(LENS, size=n[i]), n[j])
            lens[EMPTY_ROWS[i]] = 0
            rows = np.repeat(np.arange(n[i]), lens)
            cols = np.concatenate([rng.choice(n[j], size=m, replace=False) for m in lens])
            vals = (rng.standard_normal(rows.size) * 0.1).astype(np.float32)
            rels.append((np.stack([rows, cols], 1).astype(np.int64), vals, (n[i], n[j])))
        adj[i, j] = rels
    return synthetic.SyntheticGraph("S-odd", n, dict(base.edge_types), dict(base.decoders), adj, base.degrees)


def _one_hot_graph():
    """The tiny graph's shape with identity-like adjacency: a row holds at most one pair of
    value 1 per edge type, so with one-hot W1 rows every H1 entry is 0, 1 or 2 exactly."""
    from decagon_amd import synthetic

    base = synthetic.load_S()
    n = {0: 151, 1: 97}
    rng = np.random.default_rng(11)
    adj = {}
    for (i, j), K in base.edge_types.items():
        has = rng.random(n[i]) < 0.8
        has[EMPTY_ROWS[i]] = False
        which = rng.integers(0, K, n[i])
        cols = rng.integers(0, n[j], n[i])
        rels = []
        for k in range(K):
            rows = np.nonzero(has & (which == k))[0]
            rels.append((np.stack([rows, cols[rows]], 1).astype(np.int64), np.ones(rows.size, np.float32),
                         (n[i], n[j])))
        adj[i, j] = rels
    return synthetic.SyntheticGraph("S-onehot", n, dict(base.edge_types), dict(base.decoders), adj, base.degrees)


def _weights(g, seed, integer=False):
    rng = np.random.default_rng(seed)
    n = g.n_nodes
    if integer:
        w1 = {}
        for et, K in g.edge_types.items():
            w = np.zeros((K, n[et[1]], 64), np.float32)
            hot = rng.integers(0, 64, (K, n[et[1]]))
            np.put_along_axis(w, hot[:, :, None], 1.0, axis=2)
            w1[et] = w
        w2 = {et: rng.integers(-4, 5, (K, 64, 32)).astype(np.float32) for et, K in g.edge_types.items()}
        return w1, w2
    w1 = {et: rng.uniform(-0.2, 0.2, (K, n[et[1]], 64)).astype(np.float32) for et, K in g.edge_types.items()}
    w2 = {et: rng.uniform(-0.3, 0.3, (K, 64, 32)).astype(np.float32) for et, K in g.edge_types.items()}
    return w1, w2


def _plan(g, w1, w2, preproject=True, balance=1, keep_sums=False, share=True):
    from decagon_amd import engine

    saved = engine.L2_PREPROJECT, engine.TAB_BALANCE, engine.L2_PREPROJECT_SHARE
    # (module policy read at plan build)
    engine.L2_PREPROJECT, engine.TAB_BALANCE, engine.L2_PREPROJECT_SHARE = preproject, balance, share
    try:
        dev = torch.device("cuda", 0)
        dg = engine.DeviceGraph(g.edge_types, g.csr(), dev, chunk=dict(g.edge_types))
        plan = engine.ForwardPlan(dg, {t: None for t in g.n_nodes},
                                  engine.LayerWeights({et: torch.from_numpy(w).to(dev) for et, w in w1.items()}),
                                  engine.LayerWeights({et: torch.from_numpy(w).to(dev) for et, w in w2.items()}),
                                  64, 32, keep_sums=keep_sums)
    finally:
        engine.L2_PREPROJECT, engine.TAB_BALANCE, engine.L2_PREPROJECT_SHARE = saved
    return plan


def _run(plan):
    """One forward with every output pre-filled with NaN."""
    for t in list(plan.hidden1.values()) + list(plan.embeddings.values()) + list(plan.proj.values()):
        t.fill_(float("nan"))
    plan.run()
    torch.cuda.synchronize()
    return ({t: h.cpu().numpy() for t, h in plan.hidden1.items()},
            {t: e.cpu().numpy() for t, e in plan.embeddings.items()},
            {et: p.cpu().numpy() for et, p in plan.proj.items()})


class _Case:
    """A graph, its weights, the float64 oracle, and the default (knob on) and knob-off plans'
    outputs: computed once, shared by the tests, never modified."""

    def __init__(self, g):
        from oracle import decagon_oracle as orc

        self.g = g
        self.w1, self.w2 = _weights(g, 1)
        n = g.n_nodes
        feats = {t: (np.stack([np.arange(n[t])] * 2, 1), np.ones(n[t]), (n[t], n[t])) for t in n}
        self.h1_ref, self.emb_ref = orc.decagon_forward(
            g.edge_types, g.adj, feats, {et: [x.astype(np.float64) for x in w] for et, w in self.w1.items()},
            {et: [x.astype(np.float64) for x in w] for et, w in self.w2.items()})
        self.on = _plan(g, self.w1, self.w2)
        self.h1_on, self.emb_on, self.p_on = _run(self.on)
        self.off = _plan(g, self.w1, self.w2, preproject=False)
        self.h1_off, self.emb_off, _ = _run(self.off)


@pytest.fixture(scope="module")
def cases():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    made = {}

    def get(name):
        from decagon_amd import synthetic

        if name not in made:
            made[name] = _Case(_tiny_graph() if name == "odd" else synthetic.load_S())
        return made[name]

    return get


def _forms(plan):
    from decagon_amd import kernels

    l1, l2 = plan.spmm_launches
    assert len(l1) == 1 and len(l2) == 1
    assert isinstance(l1[0], kernels.PreparedFusedTab) and isinstance(l2[0], kernels.PreparedFusedTab)
    return l1[0], l2[0]


GRAPHS = ["odd", "S"]


@pytest.mark.parametrize("name", GRAPHS)
def test_p_stacks_are_h1_times_w2(cases, name):
    """Every P_k row is the plan's own stored H1 row times W2_k (float64 restatement, the GEMM
    tolerance); the H1 rows are bitwise those of the launch without jobs; no weight changes."""
    c = cases(name)
    l1, l2 = _forms(c.on)
    assert l1.projs and (l1.d_in, l1.d_out) == (64, 64) and (l2.d_in, l2.d_out) == (32, 32)
    assert set(c.p_on) == set(c.g.edge_types)
    for et, K in c.g.edge_types.items():
        h = c.h1_on[et[1]].astype(np.float64)
        assert c.p_on[et].shape == (K, c.g.n_nodes[et[1]], 32)
        for k in range(K):
            want = h @ c.w2[et][k].astype(np.float64)
            assert np.isfinite(c.p_on[et][k]).all()
            assert rel_err(c.p_on[et][k], want) <= TOL_GEMM, (et, k)
    for t in c.h1_on:
        assert np.array_equal(c.h1_on[t], c.h1_off[t])  # (same layer-1 table: the same bits)
    for et in c.g.edge_types:  # nothing but the stacks and the rows is written
        assert np.array_equal(plan_w(c.on, 2, et), c.w2[et]) and np.array_equal(plan_w(c.on, 1, et), c.w1[et])
    if name == "odd":  # rows without a pair: H1 row 0, P rows written as zeros
        for et in c.g.edge_types:
            rows = EMPTY_ROWS[et[1]]
            assert not c.h1_on[et[1]][rows].any() and not c.p_on[et][:, rows].any()


@pytest.mark.parametrize("share", [True, False])
def test_p_stacks_exact_on_small_integers(share):
    """Both job forms — one wave projecting every row of its workgroup onto a relation (the
    default), and one (row, relation) a wave.  One-hot W1 rows and identity-like adjacency make H1 small integers (0, 1, 2); with integer
    W2 in [-4, 4] every product and partial sum is exact in fp32, so P must equal H1·W2_k exactly —
    a wrong slab, row slot, lane slice or butterfly cannot hide in rounding.  The weights the
    launch reads stay bit for bit what was uploaded."""
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    g = _one_hot_graph()
    w1, w2 = _weights(g, 3, integer=True)
    plan = _plan(g, w1, w2, share=share)
    l1, _ = _forms(plan)
    assert l1.projs
    from decagon_amd import wavetable

    desc = l1._desc_v.cpu().numpy().view(wavetable.DESC)
    jobs = [wavetable.decode_role(r).proj_slots for r in desc["role"]]
    assert any(jobs) and ((0, 1) in jobs) == share  # two gene rows in one job only when shared
    h1, _, p = _run(plan)
    n = g.n_nodes
    want_h1 = {t: np.zeros((n[t], 64), np.float64) for t in n}
    for (i, j), rels in g.adj.items():
        for k, (coords, vals, _) in enumerate(rels):
            np.add.at(want_h1[i], coords[:, 0], w1[i, j][k][coords[:, 1]].astype(np.float64))
    for t in n:
        assert np.array_equal(h1[t], want_h1[t])
        assert set(np.unique(h1[t])) <= {0.0, 1.0, 2.0} and h1[t].max() >= 1.0 and not h1[t][EMPTY_ROWS[t]].any()
    for et, K in g.edge_types.items():
        for k in range(K):
            assert np.array_equal(p[et][k], want_h1[et[1]] @ w2[et][k].astype(np.float64)), (et, k)
        assert not p[et][:, EMPTY_ROWS[et[1]]].any()
        assert np.array_equal(plan_w(plan, 2, et), w2[et]) and np.array_equal(plan_w(plan, 1, et), w1[et])


def plan_w(plan, layer, et):
    """The weight stack a plan's launches read, back from the device."""
    l1, _ = plan.spmm_launches
    if layer == 2:
        return next(pj.w for pj in l1[0].projs if pj.out is plan.proj[et]).cpu().numpy()
    spec = next(s for s, e in zip(l1[0]._keep[0], plan.launch_groups[id(l1[0])]) if e == et)
    return spec.x.cpu().numpy()


@pytest.mark.parametrize("name", GRAPHS)
def test_forward_matches_oracle_and_reassociated_form(cases, name):
    """The whole forward with the knob on against the float64 oracle by
    test_forward_matches_golden's criterion (rel_err <= 1e-4, elementwise pass-rate 1.0 of the
    embeddings), and against the knob-off plan: both forms round differently (P_k rows rounded to
    fp32 before the 32-wide sums, against 64-wide sums projected once per relation), so the bound
    is on their errors against the oracle — the new form's maximum error at most twice the
    reassociated form's.  Measured max|emb - oracle| on MI355X, knob on / knob off: the odd-sized
    graph 1.52e-7 / 1.41e-7, config S 1.19e-7 / 1.56e-7 ("Layer 2 over pre-projected
    operands")."""
    c = cases(name)
    for t in c.h1_on:
        assert rel_err(c.h1_on[t], c.h1_ref[t]) <= TOL
        assert rel_err(c.emb_on[t], c.emb_ref[t]) <= TOL
        ok = np.abs(c.emb_on[t] - c.emb_ref[t]) <= 1e-4 * np.abs(c.emb_ref[t]) + 1e-6
        assert ok.mean() == 1.0
    err_on = max(float(np.abs(c.emb_on[t] - c.emb_ref[t]).max()) for t in c.emb_on)
    err_off = max(float(np.abs(c.emb_off[t] - c.emb_ref[t]).max()) for t in c.emb_off)
    print(f"preproject {name}: max|emb - oracle| knob on {err_on:.3e}, knob off {err_off:.3e}")
    assert err_on <= 2.0 * err_off


@pytest.mark.parametrize("name", GRAPHS)
def test_narrow_wave_table_against_seg_form(cases, name):
    """The 32 -> 32 wave-table launch (layer 2 over the P stacks): one wave per relation it equals
    dg_gcn_fused_seg_f32's rows bit for bit; balanced (a group's pairs dealt over its waves: the
    group's fp32 sum re-associated) within 1e-6·max|y|, test_gpu_tab.py's bound."""
    c = cases(name)
    for balance, exact in ((0, True), (2, False)):
        plan = _plan(c.g, c.w1, c.w2, balance=balance)
        _run(plan)
        for launch in _forms(plan):
            assert launch.balance == (not exact)
            outs = launch._keep[1]
            launch()
            torch.cuda.synchronize()
            tab = [o.clone() for o in outs]
            for o in outs:
                o.fill_(float("nan"))
            launch.seg_form()
            torch.cuda.synchronize()
            for a, b in zip(tab, outs):
                assert torch.isfinite(a).all()
                if exact:
                    assert torch.equal(a, b)
                else:
                    assert float((a - b).abs().max()) <= 1e-6 * float(b.abs().max())


@pytest.mark.parametrize("name", GRAPHS)
def test_fallback_plans_keep_the_reassociated_form(cases, name):
    """Knob off, and a training plan (keep_sums): no projection jobs, no 32 -> 32 launch — the
    forms they had before the knob existed — and the knob-off forward agrees with the oracle."""
    from decagon_amd import kernels

    c = cases(name)
    l1, l2 = _forms(c.off)
    assert not l1.projs and (l1.d_in, l1.d_out) == (64, 64) and (l2.d_in, l2.d_out) == (64, 32)
    assert not c.off.preproj and not c.off.proj
    assert l1._tname == l2._tname == "dg_gcn_fused_tab_f32"
    for t in c.emb_off:
        assert rel_err(c.emb_off[t], c.emb_ref[t]) <= TOL
    train = _plan(c.g, c.w1, c.w2, keep_sums=True)
    assert not train.preproj and not train.fused_seg
    for layer in (train._layer1, train._layer2):
        for launch in layer.launches:
            assert not getattr(launch, "projs", None)
            assert not (isinstance(launch, kernels.PreparedFusedTab) and launch.d_in == 32)
    h1, emb, _ = _run(train)
    for t in emb:
        assert rel_err(h1[t], c.h1_ref[t]) <= TOL and rel_err(emb[t], c.emb_ref[t]) <= TOL

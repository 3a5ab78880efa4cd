"""GPU: the DEDICOM decoder's row operands made in layer 2's launch (DG_DEC_PREPROJECT, the default
for a decoder built on the embeddings of a one-GPU forward plan in the wave-table form):
dg_gcn_fused_tab_dec_f32's Q rows, dg_decoder_hinge_rows_f32's scores, draws and loss, the
attachment rules of ForwardPlan.attach_decoder_rows / kernels.PreparedDecoderHinge, the guard
against rows older than the attachment, graph capture, and release.

Graphs: test_gpu_preproject.py's odd-sized two-type graph (n = {0: 151, 1: 97}, with rows without
a pair) attached at node type 1 (one row a workgroup) and at node type 0 (two rows a workgroup, 151
rows: the last workgroup finishes one), and config S at node type 1.
"""
import numpy as np
import pytest

from conftest import rel_err
from test_gpu_preproject import EMPTY_ROWS, _plan, _tiny_graph, _weights

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

MARGIN = 0.1
CASES = [("odd", 1), ("odd", 0), ("S", 1)]


def _params(seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((32, 32)) / 6).astype(np.float32), rng.standard_normal(32).astype(np.float32)


def _dv(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _snapshot(plan):
    torch.cuda.synchronize()
    return ({t: h.cpu().numpy() for t, h in plan.hidden1.items()},
            {t: e.cpu().numpy() for t, e in plan.embeddings.items()})


class _Case:
    """A graph and weights, the unattached plan's outputs, and a plan attached at `node_type`
    with (G, l) and one with l = None, each run once: shared by the tests, never modified."""

    def __init__(self, name, node_type):
        from decagon_amd import synthetic

        self.g = _tiny_graph() if name == "odd" else synthetic.load_S()
        self.node_type = node_type
        self.w1, self.w2 = _weights(self.g, 1)
        self.G, self.l = _params(17)
        self.plain = _plan(self.g, self.w1, self.w2)
        self.plain.run()
        self.h1_plain, self.emb_plain = _snapshot(self.plain)
        self.Gd, self.ld = _dv(self.G), _dv(self.l)
        self.att, self.Q = self._attached(self.ld)
        self.att_ones, self.Q_ones = self._attached(None)

    def _attached(self, l):
        plan = _plan(self.g, self.w1, self.w2)
        Q = plan.attach_decoder_rows(self.node_type, self.Gd, l)
        assert Q is not None
        Q.fill_(float("nan"))
        for t in list(plan.hidden1.values()) + list(plan.embeddings.values()):
            t.fill_(float("nan"))
        plan.run()
        torch.cuda.synchronize()
        return plan, Q


@pytest.fixture(scope="module")
def cases():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    made = {}

    def get(name, node_type):
        if (name, node_type) not in made:
            made[name, node_type] = _Case(name, node_type)
        return made[name, node_type]

    return get


@pytest.mark.parametrize("with_l", [True, False])
@pytest.mark.parametrize("name,node_type", CASES)
def test_q_rows_and_untouched_outputs(cases, name, node_type, with_l):
    """Q = l ∘ ((E ∘ l)·G) in float64 from the device's own E within 1e-6·max|Q| (l = None: all
    ones); E bitwise the unattached plan's, the other node type's rows and H1 too; a row without
    a pair has E = 0 and so Q = 0; layer 2 stays a PreparedFusedTab and counts the Q rows written
    and G / l read."""
    from decagon_amd import kernels

    c = cases(name, node_type)
    plan, Q = (c.att, c.Q) if with_l else (c.att_ones, c.Q_ones)
    h1, emb = _snapshot(plan)
    for t in emb:
        assert np.array_equal(emb[t], c.emb_plain[t]) and np.array_equal(h1[t], c.h1_plain[t])
    l64 = c.l.astype(np.float64) if with_l else np.ones(32)
    want = ((emb[node_type].astype(np.float64) * l64) @ c.G.astype(np.float64)) * l64
    got = Q.cpu().numpy()
    assert got.shape == want.shape and np.isfinite(got).all()
    err = float(np.abs(got - want).max() / np.abs(want).max())
    print(f"dec preproject {name}/{node_type} l={with_l}: max|Q - Q64| / max|Q| = {err:.3e}")
    assert err <= 1e-6
    if name == "odd":
        rows = EMPTY_ROWS[node_type]
        assert not emb[node_type][rows].any() and not got[rows].any()
    (l2,), (p2,) = plan.spmm_launches[1], c.plain.spmm_launches[1]
    assert isinstance(l2, kernels.PreparedFusedTab) and l2._tname == "dg_gcn_fused_tab_dec_f32"
    assert p2._tname == "dg_gcn_fused_tab_f32" and (l2.d_in, l2.d_out) == (32, 32)
    extra = 4 * (32 * 32 + (32 if with_l else 0) + 32 * c.g.n_nodes[node_type])
    assert plan.layer_bytes(2) - c.plain.layer_bytes(2) == extra
    assert plan.launch_bytes(l2, 2) - c.plain.launch_bytes(p2, 2) == extra
    assert plan.layer_bytes(1) == c.plain.layer_bytes(1)


def _rows_hinge(Q, E, rows, cols, n, alias=None, negs=None, seed=5, offset=1000):
    """dg_decoder_hinge_rows_f32 on fresh buffers: (pos, neg, neg_rows, loss bits)."""
    from decagon_amd import _lib

    pos, neg = torch.full((n,), float("nan"), device="cuda"), torch.full((n,), float("nan"), device="cuda")
    nro = torch.full((n,), -1, device="cuda", dtype=torch.int32)
    loss = torch.full((1,), float("nan"), device="cuda")
    ws = torch.zeros(4 + -(-n // 8), device="cuda")
    losses = []
    for _ in range(3):  # the same workspace: each launch leaves it zero for the next
        _lib.check(_lib.load().dg_decoder_hinge_rows_f32(
            Q.data_ptr(), Q.shape[1], E.data_ptr(), E.shape[1], rows.data_ptr(), cols.data_ptr(),
            negs.data_ptr() if negs is not None else None, alias.data_ptr() if alias is not None else None,
            alias.shape[0] if alias is not None else 0, seed, offset, n, 32, MARGIN, pos.data_ptr(), neg.data_ptr(),
            nro.data_ptr(), loss.data_ptr(), ws.data_ptr(), torch.cuda.current_stream().cuda_stream), "rows")
        torch.cuda.synchronize()
        losses.append(loss.cpu().numpy().view(np.uint32)[0])
    assert not ws.any()
    return pos.cpu().numpy(), neg.cpu().numpy(), nro.cpu().numpy(), losses


# 4100 pairs: 257 workgroups of 16 pairs, the ticket path (more than 255)
@pytest.mark.parametrize("n", [1, 31, 32, 33, 100, 512, 4100])
def test_scores_draws_and_loss(cases, n):
    """Config S's attached plan at every pair count: sampled negatives are dg_unigram_sample's
    draws; both score vectors match orc.batch_predict on the device's own E (rel_err <= 1e-5) and
    the loss the oracle's hinge (1e-4·|loss|): test_decoder_hinge_fused's tolerances; the new
    form's max error is at most twice dg_decoder_hinge_f32's on the same inputs, or 4 ulp of the
    largest |score|; given negatives give the sampled path's bits; three launches one loss."""
    from decagon_amd import kernels as K
    from oracle import decagon_oracle as orc

    c = cases("S", 1)
    E = c.att.embeddings[1]
    n_rows = E.shape[0]
    rng = np.random.default_rng(100 + n)
    rows, cols = rng.integers(0, n_rows, n).astype(np.int32), rng.integers(0, n_rows, n).astype(np.int32)
    tab = K.upload_alias(rng.integers(0, 30, n_rows).astype(np.float64), "cuda")
    rows_d, cols_d = _dv(rows), _dv(cols)
    pos, neg, negs, losses = _rows_hinge(c.Q, E, rows_d, cols_d, n, alias=tab)
    assert np.array_equal(negs, K.unigram_sample(tab, n, 5, 1000).cpu().numpy())
    assert len(set(losses)) == 1
    negs_d = _dv(negs)
    pos2, neg2, negs2, losses2 = _rows_hinge(c.Q, E, rows_d, cols_d, n, negs=negs_d)
    assert np.array_equal(pos2.view(np.uint32), pos.view(np.uint32)) and np.array_equal(negs2, negs)
    assert np.array_equal(neg2.view(np.uint32), neg.view(np.uint32)) and losses2 == losses
    emb = [E.cpu().numpy().astype(np.float64)] * 2
    L = np.diag(c.l.astype(np.float64))
    pos64 = orc.batch_predict(emb, 0, 1, c.G.astype(np.float64), L, rows, cols)
    neg64 = orc.batch_predict(emb, 0, 1, c.G.astype(np.float64), L, negs, cols)
    old = K.PreparedDecoderHinge(E, E, rows_d, cols_d, c.Gd, c.ld, MARGIN, neg_rows=negs_d, preproject=False)
    old()
    torch.cuda.synchronize()
    assert old.entry == "dg_decoder_hinge_f32" and not old.attached
    err_new = max(np.abs(pos - pos64).max(), np.abs(neg - neg64).max())
    err_old = max(np.abs(old.pos.cpu().numpy() - pos64).max(), np.abs(old.neg.cpu().numpy() - neg64).max())
    big = np.float32(max(np.abs(pos64).max(), np.abs(neg64).max()))
    print(f"dec preproject n={n}: max score error new {err_new:.3e}, old {err_old:.3e}, ulp {np.spacing(big):.3e}")
    assert rel_err(pos, pos64) <= 1e-5 and rel_err(neg, neg64) <= 1e-5
    want = orc.hinge_loss(pos64, neg64, MARGIN)
    got = float(np.array(losses[:1], np.uint32).view(np.float32)[0])
    assert abs(got - want) <= 1e-4 * abs(want)
    assert err_new <= max(2.0 * err_old, 4.0 * float(np.spacing(big)))


def _batch(g, n, seed=3):
    from decagon_amd import kernels as K

    rng = np.random.default_rng(seed)
    rows = rng.integers(0, g.n_nodes[1], n).astype(np.int32)
    cols = rng.integers(0, g.n_nodes[1], n).astype(np.int32)
    tab = K.upload_alias(rng.integers(1, 30, g.n_nodes[1]).astype(np.float64), "cuda")
    return _dv(rows), _dv(cols), tab


def _outs(dec):
    torch.cuda.synchronize()
    return [x.cpu().numpy().copy().view(np.uint32) for x in (dec.pos, dec.neg, dec.neg_rows, dec.loss)]


def test_guard_then_row_path_and_graph_capture(cases):
    """A decoder attached after the plan's last run scores the old way, bitwise
    PreparedDecoderHinge(..., preproject=False); after plan.run() it takes the row-operand entry
    point.  A step (plan.run(); dec()) captured in a graph and replayed gives the eager step's
    bits."""
    from decagon_amd import kernels as K

    c = cases("S", 1)
    plan = _plan(c.g, c.w1, c.w2)
    plan.run()
    E = plan.embeddings[1]
    rows, cols, tab = _batch(c.g, 512)
    dec = K.PreparedDecoderHinge(E, E, rows, cols, c.Gd, c.ld, MARGIN, alias=tab, seed=7, offset=11)
    assert dec.attached and dec.Q is not None
    ref = K.PreparedDecoderHinge(E, E, rows, cols, c.Gd, c.ld, MARGIN, alias=tab, seed=7, offset=11,
                                 preproject=False)
    assert not ref.attached
    dec()
    ref()
    assert dec.entry == ref.entry == "dg_decoder_hinge_f32"
    for a, b in zip(_outs(dec), _outs(ref)):
        assert np.array_equal(a, b)
    plan.run()
    dec()
    assert dec.entry == "dg_decoder_hinge_rows_f32"
    eager = _outs(dec)
    assert np.array_equal(eager[2], _outs(ref)[2])  # the same draws
    assert rel_err(dec.pos.cpu().numpy(), ref.pos.cpu().numpy()) <= 1e-5
    e_eager, q_eager = E.cpu().numpy().copy(), dec.Q.cpu().numpy().copy()
    assert np.array_equal(e_eager, c.emb_plain[1])
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        plan.run()
        dec()
        stream.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream, capture_error_mode="thread_local"):
            plan.run()
            dec()
        assert dec.entry == "dg_decoder_hinge_rows_f32"
        for t in (E, dec.Q, dec.pos, dec.neg, dec.loss):
            t.fill_(float("nan"))
        dec.neg_rows.fill_(-1)
        graph.replay()
        stream.synchronize()
    for a, b in zip(_outs(dec), eager):
        assert np.array_equal(a, b)
    assert np.array_equal(E.cpu().numpy(), e_eager) and np.array_equal(dec.Q.cpu().numpy(), q_eager)
    dec.release()


def test_attachment_rules_and_release(cases, monkeypatch):
    """One attachment a plan: the same (G, l) shares Q, another (G, l) scores the old way.  No
    attachment with keep_sums, dropout, a sharded plan, either knob off, preproject=False or
    2n < rows.  Releasing restores the plain layer-2 launch and bitwise the same E."""
    from decagon_amd import engine, kernels as K
    from decagon_amd.sharding import RelationShard, _no_op_reduce

    c = cases("S", 1)
    g = c.g
    rows, cols, tab = _batch(g, 512)

    def make(plan, G=None, l=None, n=512, **kw):
        return K.PreparedDecoderHinge(plan.embeddings[1], plan.embeddings[1], rows[:n], cols[:n],
                                      c.Gd if G is None else G, c.ld if l is None else l, MARGIN, alias=tab, **kw)

    plan = _plan(g, c.w1, c.w2)
    first = make(plan)
    assert first.attached and plan.spmm_launches[1][0]._tname == "dg_gcn_fused_tab_dec_f32"
    same = make(plan)
    assert same.attached and same.Q is first.Q
    G2, l2 = (_dv(x) for x in _params(23))
    other = make(plan, G=G2, l=l2)
    assert not other.attached
    assert not make(plan, n=10).attached and not make(plan, preproject=False).attached  # 20 < 400 rows
    plan.run()
    other()
    first()
    assert other.entry == "dg_decoder_hinge_f32" and first.entry == "dg_decoder_hinge_rows_f32"
    # release: the last holder restores the plain launch
    same.release()
    assert plan.spmm_launches[1][0]._tname == "dg_gcn_fused_tab_dec_f32"
    first.release()
    assert not first.attached and plan.spmm_launches[1][0]._tname == "dg_gcn_fused_tab_f32"
    for t in plan.embeddings.values():
        t.fill_(float("nan"))
    plan.run()
    first()
    assert first.entry == "dg_decoder_hinge_f32"
    _, emb = _snapshot(plan)
    for t in emb:
        assert np.array_equal(emb[t], c.emb_plain[t])
    assert make(plan, G=G2, l=l2).attached  # free again
    # plans that never attach
    dev = torch.device("cuda", 0)
    assert not make(_plan(g, c.w1, c.w2, keep_sums=True)).attached
    assert not make(_plan(g, c.w1, c.w2, preproject=False)).attached  # DG_L2_PREPROJECT=0
    lw = lambda ws: engine.LayerWeights({et: torch.from_numpy(w).to(dev) for et, w in ws.items()})
    drop = (0.9, torch.tensor([20180701, 0], dtype=torch.int64, device=dev))
    dg1 = engine.DeviceGraph(g.edge_types, g.csr(), dev, chunk=dict(g.edge_types))
    dropped = engine.ForwardPlan(dg1, {t: None for t in g.n_nodes}, lw(c.w1), lw(c.w2), 64, 32, dropout=drop)
    assert not dropped.preproj and not make(dropped).attached
    nnz = {et: [len(x[1]) for x in rels] for et, rels in g.adj.items()}
    shard = RelationShard.lpt(g.edge_types, nnz, 0, 2, _no_op_reduce)
    dg2 = engine.DeviceGraph(g.edge_types, shard.local_csr(g.csr()), dev, shard.local, row_block=shard.row_block)
    sharded = engine.ForwardPlan(dg2, {t: None for t in g.n_nodes}, lw(c.w1), lw(c.w2), 64, 32, shard=shard)
    assert not sharded.preproj and not make(sharded).attached
    monkeypatch.setenv("DG_DEC_PREPROJECT", "0")
    off = _plan(g, c.w1, c.w2)
    assert not make(off).attached and off.attach_decoder_rows(1, c.Gd, c.ld) is None
    monkeypatch.delenv("DG_DEC_PREPROJECT")
    assert make(off).attached

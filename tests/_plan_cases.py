"""Case generator of the forward-plan form tests (test_cpu_plan_forms.py on the form decision,
test_gpu_plan_forms.py and golden/make_plan_forms.py on the built plans): one case per launch
form that engine.ForwardPlan serves — config S on one GPU under its policy switches, training
plans, config S's row blocks at N GPUs, a scaled-down config P (windowed PPI, 120 staged
relations) whole and split, the peer exchange in loopback, sparse features.

Sharded cases are one process standing in for one rank: the collectives are the no-ops of
sharding.py, as bench.py --simulate-world runs them.  `manifest` describes a built plan from
attributes only (no addresses): what test_gpu_plan_forms.py compares with
golden/plan_forms.json.
"""
import contextlib
import hashlib
from dataclasses import dataclass, field
from typing import Dict, Optional, Tuple

import numpy as np

H1, H2 = 64, 32
SEED, DROP_SEED = 5, 20180701
FEAT_COLS, FEAT_NNZ = 40, 3  # the sparse features of node type 1


@dataclass
class Case:
    name: str
    graph: str = "S"                  # "S", "S-sets" (world relation sets) or "P-small"
    knobs: Dict[str, object] = field(default_factory=dict)  # engine module policy at plan build
    keep_sums: bool = False
    keep: float = 1.0                 # dropout keep probability
    shard: Optional[str] = None       # "weak-seg", "weak-fused", "lpt", "split"
    world: int = 1
    rank: int = 0
    split: Tuple = ()                 # "split": deal_rows
    peer: Optional[str] = None        # a loopback PeerConfig's mode
    sparse: bool = False              # sparse features on node type 1

    @property
    def sharded(self) -> bool:
        return self.shard is not None


def cases():
    out = [
        Case("S"),
        Case("S-no-preproject", knobs={"L2_PREPROJECT": False}),
        Case("S-no-wave-table", knobs={"WAVE_TABLE": False}),
        Case("S-no-fused-seg", knobs={"FUSED_SEG": False}),
        Case("S-partial", knobs={"FUSED_SEG": False, "FUSED_MAX_ROWS": 0}),
        Case("S-keep-sums", keep_sums=True),
        Case("S-keep-sums-dropout", keep_sums=True, keep=0.9),
        Case("P-small", graph="P-small"),
        Case("P-small-keep-sums", graph="P-small", keep_sums=True),
        Case("S-sets-2-seg", graph="S-sets", shard="weak-seg", world=2, rank=1),
        Case("S-sets-8-seg", graph="S-sets", shard="weak-seg", world=8, rank=3),
        Case("S-sets-2-fused", graph="S-sets", shard="weak-fused", world=2, rank=0),
        Case("S-lpt-2", shard="lpt", world=2, rank=0),
        Case("P-small-split-3", graph="P-small", shard="split", world=3, rank=2, split=((1, 0),)),
        Case("P-small-split-2-keep-sums", graph="P-small", shard="split", world=2, rank=0, keep_sums=True),
    ]
    by = {c.name: c for c in out}
    for base in ("S-sets-2-seg", "P-small-split-3"):
        for mode in ("fused", "kernel"):
            c = by[base]
            out.append(Case(f"{base}-peer-{mode}", c.graph, shard=c.shard, world=c.world, rank=c.rank,
                            split=c.split, peer=mode))
    out.append(Case("S-sparse-features", sparse=True))
    return out


_GRAPHS: dict = {}


def graph(case: Case):
    """The case's graph (built once a process, never modified)."""
    from decagon_amd import synthetic

    key = (case.graph, case.world if case.graph == "S-sets" else 1)
    if key not in _GRAPHS:
        if case.graph == "S":
            g = synthetic.load_S()
        elif case.graph == "S-sets":
            g = synthetic.replicate_sets(synthetic.load_S(), case.world)
        else:
            g = synthetic.make_P(seed=3, n_proteins=1500, n_drugs=150, n_side_effects=60, ppi_edges=12000,
                                 target_edges=1200)
        _GRAPHS[key] = g
    return _GRAPHS[key]


def features(case: Case, g):
    """{node type: HostCSR or None (identity)}: FEAT_NNZ distinct columns a row of node type 1."""
    from decagon_amd.sparse import HostCSR

    feats = {t: None for t in g.n_nodes}
    if case.sparse:
        rng = np.random.default_rng(SEED + 1)
        n1 = g.n_nodes[1]
        col = np.concatenate([np.sort(rng.choice(FEAT_COLS, FEAT_NNZ, replace=False)) for _ in range(n1)])
        val = rng.uniform(0.5, 1.5, n1 * FEAT_NNZ).astype(np.float32)
        feats[1] = HostCSR(np.arange(0, n1 * FEAT_NNZ + 1, FEAT_NNZ, dtype=np.int32), col.astype(np.int32), val,
                           (n1, FEAT_COLS))
    return feats


def weights(case: Case, g):
    rng = np.random.default_rng(SEED)
    n = g.n_nodes
    rows = lambda j: FEAT_COLS if case.sparse and j == 1 else n[j]  # noqa: E731
    w1 = {et: rng.uniform(-0.1, 0.1, (K, rows(et[1]), H1)).astype(np.float32) for et, K in g.edge_types.items()}
    w2 = {et: rng.uniform(-0.3, 0.3, (K, H1, H2)).astype(np.float32) for et, K in g.edge_types.items()}
    return w1, w2


def shard_of(case: Case, g):
    from decagon_amd.sharding import RelationShard, _no_op, _no_op_reduce

    if not case.sharded:
        return None
    nnz = {et: [len(c[1]) for c in rels] for et, rels in g.adj.items()}
    if case.shard in ("weak-seg", "weak-fused"):
        sh = RelationShard.weak_sets(g.edge_types, g.n_nodes, case.rank, case.world, _no_op_reduce, _no_op,
                                     form=case.shard[5:])
    elif case.shard == "lpt":
        sh = RelationShard.lpt(g.edge_types, nnz, case.rank, case.world, _no_op_reduce)
    else:
        sh = RelationShard.split(g.edge_types, g.n_nodes, nnz, case.rank, case.world, _no_op_reduce, _no_op,
                                 row_split_min=1000, deal_rows=list(case.split))
    if case.peer is not None:
        from decagon_amd.peer import PeerConfig

        sh.peer = PeerConfig(mode=case.peer, loopback=True)
    return sh


@contextlib.contextmanager
def policy(case: Case):
    """The case's engine module policy, restored afterwards."""
    from decagon_amd import engine

    saved = {k: getattr(engine, k) for k in case.knobs}
    for k, v in case.knobs.items():
        setattr(engine, k, v)
    try:
        yield
    finally:
        for k, v in saved.items():
            setattr(engine, k, v)


def plan_args(case: Case, device):
    """(DeviceGraph, ForwardPlan's positional arguments after it, its keyword arguments), the
    graph uploaded as bench.py uploads it.  Call inside policy(case)."""
    import torch

    from decagon_amd.engine import DeviceGraph, LayerWeights

    g = graph(case)
    sh = shard_of(case, g)
    csr = g.csr()
    if sh is not None:
        csr = sh.local_csr(csr)
    # (the "fused" row-block form keeps its projection GEMM: uploaded without segment starts, as
    # test_gpu_sharded.py uploads it)
    dg = DeviceGraph(g.edge_types, csr, device, None if sh is None else sh.local,
                     chunk=None if sh is None else sh.chunks, row_block=None if sh is None else sh.row_block,
                     segments=sh is None or not sh.fused_rows)
    w1, w2 = weights(case, g)
    up = lambda w: LayerWeights({et: torch.from_numpy(x).to(device) for et, x in w.items()})  # noqa: E731
    drop = None
    if case.keep < 1.0:
        drop = (case.keep, torch.tensor([DROP_SEED, 0], dtype=torch.int64, device=device))
    return dg, (features(case, g), up(w1), up(w2), H1, H2), dict(shard=sh, keep_sums=case.keep_sums, dropout=drop)


def build_plan(case: Case, device):
    from decagon_amd.engine import ForwardPlan

    with policy(case):
        dg, args, kw = plan_args(case, device)
        return ForwardPlan(dg, *args, **kw)


def oracle(case: Case):
    """(hidden1, embeddings) of the case's whole graph in float64 (oracle/decagon_oracle.py's
    restatement of the reference forward; with dropout, under the masks the device draws in
    its first step): computed once a process, shared, never modified."""
    key = (case.graph, case.world if case.graph == "S-sets" else 1, case.keep, case.sparse)
    if key not in _ORACLES:
        _ORACLES[key] = _oracle(case)
    return _ORACLES[key]


_ORACLES: dict = {}


def _oracle(case: Case):
    from oracle import decagon_oracle as orc

    g = graph(case)
    w1, w2 = weights(case, g)
    n = g.n_nodes
    adj = {et: [(c, v.astype(np.float32).astype(np.float64), s) for c, v, s in mats] for et, mats in g.adj.items()}
    feats = {}
    for t, f in features(case, g).items():
        if f is None:
            feats[t] = (np.stack([np.arange(n[t])] * 2, 1), np.ones(n[t]), (n[t], n[t]))
        else:
            rows = np.repeat(np.arange(f.shape[0]), np.diff(f.rowptr))
            feats[t] = (np.stack([rows, f.col], 1), f.val.astype(np.float64), tuple(f.shape))
    w1 = {et: [x.astype(np.float64) for x in w] for et, w in w1.items()}
    w2 = {et: [x.astype(np.float64) for x in w] for et, w in w2.items()}
    if case.keep >= 1.0:
        return orc.decagon_forward(g.edge_types, adj, feats, w1, w2)
    from decagon_amd.engine import drop_tag

    hid: dict = {}
    for gi, ((i, j), K) in enumerate(g.edge_types.items()):  # (identity features: rows of W1_k masked)
        m = orc.dropout_scale(DROP_SEED, 1, drop_tag(1, gi), K * n[j], case.keep).reshape(K, n[j])
        outs = [orc.sparse_dense_matmul(adj[i, j][k], m[k][:, None] * w1[i, j][k]) for k in range(K)]
        hid.setdefault(i, []).append(orc.l2_normalize_rows(np.sum(outs, axis=0)))
    h1 = {i: np.maximum(np.sum(v, axis=0), 0.0) for i, v in hid.items()}
    emb: dict = {}
    for gi, ((i, j), K) in enumerate(g.edge_types.items()):
        m = orc.dropout_scale(DROP_SEED, 1, drop_tag(2, gi), K * n[j] * H1, case.keep).reshape(K, n[j], H1)
        outs = [orc.sparse_dense_matmul(adj[i, j][k], (m[k] * h1[j]) @ w2[i, j][k]) for k in range(K)]
        emb.setdefault(i, []).append(orc.l2_normalize_rows(np.sum(outs, axis=0)))
    return h1, [np.sum(emb[i], axis=0) for i in sorted(emb)]


# ---------------------------------------------------------------------------- the manifest
FLAGS = ("seg_mode", "fused_seg", "flat_mode", "sums_mode", "peer_reduce", "tab_weighted")
SETS = ("preproj", "seg_proj", "staged_proj", "fused")


def _ets(v):
    return sorted([list(x) if isinstance(x, tuple) else x for x in v])


def _names(fns):
    return [type(f).__name__ for f in fns]


def _table(launch):
    def plain(x):  # (numpy integers as ints; a workgroup without rows is None)
        return [plain(y) for y in x] if isinstance(x, (list, tuple)) else None if x is None else int(x)

    plan = hashlib.sha256(repr(plain(launch.host_plan)).encode()).hexdigest()
    return {"class": type(launch).__name__, "tname": getattr(launch, "_tname", None),
            "d_in": launch.d_in, "d_out": launch.d_out, "n_blocks": int(launch.n_blocks), "nw": int(launch.nw),
            "slot_pairs": int(launch.slot_pairs), "balance": getattr(launch, "balance", None),
            "weighted": getattr(launch, "weighted", None), "host_plan": plan}


def manifest(plan) -> dict:
    """A JSON-able description of a built ForwardPlan: its forms, its launches by class and
    order, its wave tables' parameters and its byte accounting."""
    out = {k: bool(getattr(plan, k)) for k in FLAGS}
    out.update({k: _ets(getattr(plan, k)) for k in SETS})
    out["pre"] = len(plan._pre)
    out["gemm2"] = _names(plan._gemm2)
    l1, l2 = plan.spmm_launches
    for no, L, spmm in ((1, plan._layer1, l1), (2, plan._layer2, l2)):
        out[f"layer{no}"] = {
            "launches": _names(L.launches),
            "launch_groups": [_ets(plan.launch_groups.get(id(f), [])) for f in L.launches],
            "local_epilogues": _names(L.local_epilogues), "epilogues": _names(L.epilogues),
            "flat": 0 if L.flat is None else int(L.flat.numel()), "need_zero": bool(L.need_zero),
            "has_exchange": bool(L.has_exchange), "gathers": len(L.gathers),
            "gather_all": L.gather_all is not None, "fused_targets": [int(i) for i in L.fused_targets],
            "tables": [_table(f) for f in L.launches if hasattr(f, "host_plan")],
            "layer_bytes": int(plan.layer_bytes(no)),
            "launch_bytes": [int(plan.launch_bytes(f, no)) for f in spmm]}
    return out


def own_rows(plan, t: int, x):
    """This rank's finished rows of node type t's output x (a row-split type: its block)."""
    if t in plan.row_block:
        a, b, _ = plan.row_block[t]
        return x[a:b]
    return x


def output_hashes(plan) -> dict:
    """SHA-256 of every hidden1, embeddings and kept sum tensor after a run (sharded: the rank's
    own finished rows)."""
    def h(x):
        return hashlib.sha256(x.detach().cpu().contiguous().numpy().tobytes()).hexdigest()

    out = {}
    for name, d in (("hidden1", plan.hidden1), ("embeddings", plan.embeddings)):
        for t, x in d.items():
            out[f"{name}[{t}]"] = h(own_rows(plan, t, x))
    for no, L in ((1, plan._layer1), (2, plan._layer2)):
        for et, v in L.views.items():
            out[f"views{no}[{et[0]},{et[1]}]"] = h(v)
    return out

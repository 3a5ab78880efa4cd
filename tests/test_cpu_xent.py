"""CPU: the reference the cross-entropy training tests are held to, and the host surface of the cost.

(1) tests/_xent_ref.py's autograd reference in hinge mode reproduces oracle.train_grads — cost and
every gradient to 1e-10 relative, with and without dropout masks — before anything is held to it
in xent mode; (2) its xent cost is oracle.xent_loss on the same scores; (3) the closed formulas
of the kernels' header comments, restated in numpy float64, equal autograd; (4) the optimizer's
`loss` keyword and the new C symbols.
"""
import re
from pathlib import Path

import numpy as np
import pytest

import _trainall_ref as R
import _xent_ref as X
from oracle import decagon_oracle as orc

torch = pytest.importorskip("torch")

ROOT = Path(__file__).resolve().parents[1]
REL = 1e-10
NEW_SYMBOLS = ("dg_xent_loss_ws_f32", "dg_decoder_grad_xent_f32", "dg_decoder_grad_seg_xent_f32")


def _close(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape
    scale = np.max(np.abs(want))
    if scale == 0:
        assert np.max(np.abs(got)) == 0.0
    else:
        assert np.max(np.abs(got - want)) <= REL * scale


def _assert_same_grads(ets, got, want):
    for et, K in ets.items():
        for k in range(K):
            _close(got["w1"][et][k], want["w1"][et][k])
            _close(got["w2"][et][k], want["w2"][et][k])
        assert set(got["dec"][et]) == set(want["dec"][et])
        for name in want["dec"][et]:
            _close(got["dec"][et][name], want["dec"][et][name])


@pytest.fixture(scope="module")
def batches(golden_S):
    return R.make_batches(golden_S)  # SEED = 2


@pytest.mark.parametrize("dropout", [False, True])
def test_autograd_reference_in_hinge_mode_is_the_oracle(golden_S, batches, dropout):
    from test_cpu_train_oracle import _masks

    allb, alln = batches
    ets, decoders, w1, w2, dec, adj = R.oracle_inputs(golden_S)
    drop1, drop2 = _masks(ets, adj, 0.9, step=1) if dropout else (None, None)
    picks = X.one_per_decoder_kind(golden_S)
    assert len(picks) == len(set(decoders.values())) >= 2
    nonzero = 0
    for i, j, k, e in picks:
        b, ng = {(i, j): {k: allb[i, j][k]}}, {(i, j): {k: alln[i, j][k]}}
        cost, grads, _ = X.reference(golden_S, b, ng, "hinge", drop1=drop1, drop2=drop2)
        want_cost, want = orc.train_grads(ets, adj, {0: None, 1: None}, w1, w2, decoders, dec, 32, allb[i, j][k],
                                          alln[i, j][k], e, i, j, R.MARGIN, drop1=drop1, drop2=drop2)
        assert want_cost > 0 and abs(cost - want_cost) <= REL * want_cost
        _assert_same_grads(ets, grads, want)
        nonzero += sum(np.any(v != 0) for v in want["dec"][i, j].values())
    assert nonzero > 0  # some decoder variable's gradient was held, not only zeros


@pytest.mark.parametrize("w", [1.0, 0.5])
def test_reference_xent_cost_is_the_oracles_on_the_same_scores(golden_S, batches, w):
    allb, alln = batches
    cost, _, scores = X.reference(golden_S, allb, alln, "xent", w=w)
    assert len(scores) == len(R.SIZES)
    want = sum(orc.xent_loss(pos, neg, w) for pos, neg in scores.values())
    assert abs(cost - want) <= REL * want
    # and the scores are those of the hinge reference's pairs: z = neg − (pos − margin)
    _, _, zs = R.reference(golden_S, allb, alln)
    got = np.concatenate([neg - (pos - R.MARGIN) for pos, neg in scores.values()])
    assert np.max(np.abs(got - zs)) <= 1e-12


def test_closed_formulas_equal_autograd():
    """n = 37 pairs, d = 32, w = 0.5 over small tables (rows, negatives and columns repeat)."""
    n, d, w, nr, nc = 37, 32, 0.5, 11, 9
    rng = np.random.default_rng(5)
    U, V = rng.standard_normal((nr, d)), rng.standard_normal((nc, d))
    G, l = rng.standard_normal((d, d)) / np.sqrt(d), 1.0 + 0.3 * rng.standard_normal(d)
    rows, cols, negs = rng.integers(0, nr, n), rng.integers(0, nc, n), rng.integers(0, nr, n)
    tU, tV, tG, tl = (torch.tensor(x, requires_grad=True) for x in (U, V, G, l))
    M = torch.diag(tl) @ tG @ torch.diag(tl)
    pos = torch.sum((tU[rows] @ M) * tV[cols], dim=1)
    neg = torch.sum((tU[negs] @ M) * tV[cols], dim=1)
    cost = X.cost_of(pos, neg, "xent", w)
    cost.backward()
    c = float(cost.detach())
    assert abs(c - orc.xent_loss(pos.detach().numpy(), neg.detach().numpy(), w)) <= REL * c

    a, b, grad_rows, grad_cols, dM, dG, dl, dgd = X.closed_form(U, V, rows, cols, negs, pos.detach().numpy(),
                                                                neg.detach().numpy(), G, l, w)
    assert np.all((a > 0) & (a < 1)) and np.all((b > 0) & (b < w))
    dU = np.zeros_like(U)
    np.add.at(dU, np.concatenate([rows, negs]), grad_rows)
    dV = np.zeros_like(V)
    np.add.at(dV, cols, grad_cols)
    _close(dU, tU.grad.numpy())
    _close(dV, tV.grad.numpy())
    _close(dG, tG.grad.numpy())
    _close(dl, tl.grad.numpy())
    _close(dgd, np.diag(tG.grad.numpy()))
    # the hinge is the special case a = b = [z > 0] of the same formulas
    z = (neg - (pos - 0.1)).detach().numpy()
    act = (z > 0).astype(np.float64)
    x = act[:, None] * (U[negs] - U[rows])
    Mn = np.diag(l) @ G @ np.diag(l)
    for t in (tU, tV, tG, tl):
        t.grad = None
    M = torch.diag(tl) @ tG @ torch.diag(tl)
    pos = torch.sum((tU[rows] @ M) * tV[cols], dim=1)
    neg = torch.sum((tU[negs] @ M) * tV[cols], dim=1)
    X.cost_of(pos, neg, "hinge").backward()
    _close(np.diag(l) @ (x.T @ V[cols]) @ np.diag(l), tG.grad.numpy())
    dV = np.zeros_like(V)
    np.add.at(dV, cols, x @ Mn)
    _close(dV, tV.grad.numpy())


def _optimizer(**kw):
    import decagon_amd as dg

    et = {(0, 0): 2, (0, 1): 1, (1, 0): 1, (1, 1): 6}
    dec = {(0, 0): "bilinear", (0, 1): "bilinear", (1, 0): "bilinear", (1, 1): "dedicom"}
    ph = dg.construct_placeholders(et)
    m = dg.DecagonModel(ph, {0: 500, 1: 400}, {0: 500, 1: 400}, et, dec)
    return dg.DecagonOptimizer(m.embeddings, m.latent_inters, m.latent_varies,
                               {0: [np.ones(500)] * 2, 1: [np.ones(400)] * 6}, et,
                               {e: [(500 if e[0] == 0 else 400, 0)] * k for e, k in et.items()}, ph, **kw)


def test_optimizer_loss_keyword():
    import inspect

    import decagon_amd as dg

    assert list(inspect.signature(dg.DecagonOptimizer.__init__).parameters)[-1] == "loss"
    opt = _optimizer()
    assert opt.loss == "hinge" and opt.cost.name == "optimizer/cost"
    xe = _optimizer(loss="xent", neg_sample_weights=0.5)
    assert xe.loss == "xent" and xe.neg_sample_weights == 0.5
    assert xe.cost.name == "optimizer/xent_cost" and xe.opt_op is not None and xe.grads_vars.training
    with pytest.raises(ValueError):
        _optimizer(loss="bogus")


def test_prepared_gradients_take_the_loss_after_the_existing_arguments():
    import inspect

    from decagon_amd import kernels

    for cls in (kernels.PreparedDecoderGrad, kernels.PreparedDecoderGradSeg):
        p = inspect.signature(cls.__init__).parameters
        names = list(p)
        assert names[-2:] == ["loss", "neg_weight"] and names[-5:-2] == ["dG", "dl", "dG_diag"]
        assert p["loss"].default == "hinge" and p["neg_weight"].default == 1.0
    assert list(inspect.signature(kernels.xent_loss).parameters)[-1] == "workspace"
    with pytest.raises(ValueError):
        kernels.loss_param("bogus", 0.1, 1.0)
    assert kernels.loss_param("hinge", 0.1, 0.5) == 0.1 and kernels.loss_param("xent", 0.1, 0.5) == 0.5


def test_new_symbols_are_in_the_header_and_the_signature_table():
    from decagon_amd import _lib

    header = (ROOT / "include" / "decagon_hip.h").read_text()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _lib.SIGNATURES
    # additive to the ABI: the hinge forms keep their signatures, the xent forms differ as documented
    sig = _lib.SIGNATURES
    assert sig["dg_xent_loss_ws_f32"] == sig["dg_hinge_loss_ws_f32"]
    assert sig["dg_decoder_grad_xent_f32"] == sig["dg_decoder_grad_f32"]
    seg, xseg = sig["dg_decoder_grad_seg_f32"][1], sig["dg_decoder_grad_seg_xent_f32"][1]
    assert len(xseg) == len(seg) + 1  # one more output: coef
    assert _lib.ABI_VERSION == 39

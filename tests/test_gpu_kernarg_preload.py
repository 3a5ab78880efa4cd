"""GPU: the fused decoders after their first-trip operands became leading kernel parameters
(rows, cols, neg_given, alias, n, range, seed, offset: what the build's kernel-argument preload
places in SGPRs at wave launch, decoder.hip) — every value must still land in its parameter.

dg_decoder_hinge_f32 through kernels.PreparedDecoderHinge and through the plain call, and
dg_decoder_hinge_rows_f32 on row operands made on the host, on a 40 x 32 table at
n in {1, 15, 16, 17, 130}: one lane group, one short of the row-operand kernel's 16 pairs a
workgroup, exactly one workgroup, one over, several workgroups with a ragged last one — with
sampled and with given negatives.  One attached case: the odd-sized plan of
test_gpu_dec_preproject.py with the decoder attached at node type 1.
"""
import numpy as np
import pytest

from conftest import rel_err
from test_gpu_preproject import _plan, _tiny_graph, _weights

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

MARGIN = 0.1
D, N_ROWS = 32, 40
NS = [1, 15, 16, 17, 130]
SEED, OFFSET = 3, 77
SEED2, OFFSET2 = 2**40 + 11, 2**33 + 5  # (both halves of each 64-bit counter in use)


def _dv(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class _Inputs:
    """The table, decoder parameters, sampler and per-n index arrays, on the host and on the
    device: made once, never modified."""

    def __init__(self):
        from decagon_amd import kernels as K

        rng = np.random.default_rng(20)
        self.E = rng.standard_normal((N_ROWS, D)).astype(np.float32)
        self.G = (rng.standard_normal((D, D)) / 6).astype(np.float32)
        self.l = rng.standard_normal(D).astype(np.float32)
        l64 = self.l.astype(np.float64)
        # the row operands dg_decoder_hinge_rows_f32 takes: Q[r] = l ∘ ((E[r] ∘ l)·G), rounded once
        self.Q = (((self.E.astype(np.float64) * l64) @ self.G.astype(np.float64)) * l64).astype(np.float32)
        self.tab = K.upload_alias(rng.integers(0, 30, N_ROWS).astype(np.float64), "cuda")
        self.Ed, self.Gd, self.ld, self.Qd = _dv(self.E), _dv(self.G), _dv(self.l), _dv(self.Q)
        self.idx = {}
        for n in NS:
            rows, cols = rng.integers(0, N_ROWS, n).astype(np.int32), rng.integers(0, N_ROWS, n).astype(np.int32)
            self.idx[n] = (rows, cols, _dv(rows), _dv(cols))


@pytest.fixture(scope="module")
def inputs():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return _Inputs()


def _check(E, G, l, rows, cols, pos, neg, negs, loss, want_negs, groups):
    """Scores against the float64 restatement (test_decoder_hinge_fused's tolerance), the draws,
    and the loss against the float64 hinge of the returned scores.

    The loss bound: each fp32 term max(neg - (pos - m), 0) carries two roundings of values below
    |pos| + |neg| + m (2·2^-24 of that); the fp32 sum of n terms in any order, and its final
    rounding, at most (n + 1)·2^-24 of the sum; the packed hand-off rounds each of `groups`
    workgroup partials to the nearest 2^-32 (2^-33 each)."""
    from oracle import decagon_oracle as orc

    assert np.array_equal(negs, want_negs)
    emb = [E.astype(np.float64)] * 2
    L = np.diag(l.astype(np.float64))
    pos64 = orc.batch_predict(emb, 0, 1, G.astype(np.float64), L, rows, cols)
    neg64 = orc.batch_predict(emb, 0, 1, G.astype(np.float64), L, negs, cols)
    assert np.isfinite(pos).all() and np.isfinite(neg).all()
    assert rel_err(pos, pos64) <= 1e-5 and rel_err(neg, neg64) <= 1e-5
    p, q, m = pos.astype(np.float64), neg.astype(np.float64), float(np.float32(MARGIN))
    own = float(np.maximum(q - (p - m), 0.0).sum())
    n = len(rows)
    tol = 2.0 ** -24 * (2.0 * float((np.abs(p) + np.abs(q) + m).sum()) + (n + 1) * own) + groups * 2.0 ** -33
    print(f"n={n}: loss {loss!r} float64 hinge of the returned scores {own!r} bound {tol:.3e}")
    assert abs(float(loss) - own) <= tol


def _direct(name, inp, n, negs_d, seed, offset, **table):
    """One plain call of a fused decoder entry point on fresh buffers."""
    from decagon_amd import _lib

    _, _, rows_d, cols_d = inp.idx[n]
    pos, neg = torch.full((n,), float("nan"), device="cuda"), torch.full((n,), float("nan"), device="cuda")
    nro = torch.full((n,), -1, device="cuda", dtype=torch.int32)
    loss = torch.full((1,), float("nan"), device="cuda")
    ws = torch.zeros(4 + -(-n // 8), device="cuda")
    sampled = negs_d is None
    args = _lib.pack(name, col_table=inp.Ed.data_ptr(), ld_col=D, rows=rows_d.data_ptr(), cols=cols_d.data_ptr(),
                     neg_rows=None if sampled else negs_d.data_ptr(),
                     alias_table=inp.tab.data_ptr() if sampled else None,
                     range=inp.tab.shape[0] if sampled else 0, seed=seed, offset=offset, n=n, d=D, margin=MARGIN,
                     pos=pos.data_ptr(), neg=neg.data_ptr(), neg_rows_out=nro.data_ptr(), loss=loss.data_ptr(),
                     workspace=ws.data_ptr(), stream=torch.cuda.current_stream().cuda_stream, **table)
    _lib.check(getattr(_lib.load(), name)(*args), name)
    torch.cuda.synchronize()
    assert not ws.any()  # the launch leaves its workspace zero for the next
    return pos.cpu().numpy(), neg.cpu().numpy(), nro.cpu().numpy(), float(loss[0])


@pytest.mark.parametrize("given", [False, True], ids=["sampled", "given"])
@pytest.mark.parametrize("n", NS)
def test_prepared_decoder(inputs, n, given):
    """kernels.PreparedDecoderHinge on a plain table (dg_decoder_hinge_f32); a second call with
    another seed and offset gives that call's draws."""
    from decagon_amd import kernels as K

    rows, cols, rows_d, cols_d = inputs.idx[n]
    draws = K.unigram_sample(inputs.tab, n, SEED, OFFSET).cpu().numpy()
    kw = dict(neg_rows=_dv(draws)) if given else dict(alias=inputs.tab)
    op = K.PreparedDecoderHinge(inputs.Ed, inputs.Ed, rows_d, cols_d, inputs.Gd, inputs.ld, MARGIN, seed=SEED,
                                offset=OFFSET, **kw)
    assert not op.attached
    op.neg_rows.fill_(-1)
    op()
    torch.cuda.synchronize()
    assert op.entry == "dg_decoder_hinge_f32"
    _check(inputs.E, inputs.G, inputs.l, rows, cols, op.pos.cpu().numpy(), op.neg.cpu().numpy(),
           op.neg_rows.cpu().numpy(), float(op.loss[0]), draws, -(-n // 32))
    op.seed, op.offset = SEED2, OFFSET2
    op()
    torch.cuda.synchronize()
    want = draws if given else K.unigram_sample(inputs.tab, n, SEED2, OFFSET2).cpu().numpy()
    _check(inputs.E, inputs.G, inputs.l, rows, cols, op.pos.cpu().numpy(), op.neg.cpu().numpy(),
           op.neg_rows.cpu().numpy(), float(op.loss[0]), want, -(-n // 32))


@pytest.mark.parametrize("given", [False, True], ids=["sampled", "given"])
@pytest.mark.parametrize("n", NS)
def test_plain_calls(inputs, n, given):
    """dg_decoder_hinge_f32 and dg_decoder_hinge_rows_f32 called directly, at two (seed, offset)."""
    from decagon_amd import kernels as K

    rows, cols, _, _ = inputs.idx[n]
    for seed, offset in ((SEED, OFFSET), (SEED2, OFFSET2)):
        draws = K.unigram_sample(inputs.tab, n, seed, offset).cpu().numpy()
        negs_d = _dv(draws) if given else None
        pos, neg, negs, loss = _direct("dg_decoder_hinge_f32", inputs, n, negs_d, seed, offset,
                                       row_table=inputs.Ed.data_ptr(), ld_row=D, G=inputs.Gd.data_ptr(),
                                       l=inputs.ld.data_ptr())
        _check(inputs.E, inputs.G, inputs.l, rows, cols, pos, neg, negs, loss, draws, -(-n // 32))
        pos, neg, negs, loss = _direct("dg_decoder_hinge_rows_f32", inputs, n, negs_d, seed, offset,
                                       Q=inputs.Qd.data_ptr(), ld_q=D)
        _check(inputs.E, inputs.G, inputs.l, rows, cols, pos, neg, negs, loss, draws, -(-n // 16))


def test_attached_decoder():
    """The odd-sized plan (32 -> 32 table form) with the decoder attached at node type 1: after
    one plan.run() the call takes dg_decoder_hinge_rows_f32; scores against float64 on the
    device's own embeddings, draws and loss as above, and again at another seed and offset."""
    from decagon_amd import kernels as K

    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    g = _tiny_graph()
    w1, w2 = _weights(g, 1)
    rng = np.random.default_rng(17)
    G, l = (rng.standard_normal((32, 32)) / 6).astype(np.float32), rng.standard_normal(32).astype(np.float32)
    plan = _plan(g, w1, w2)
    E = plan.embeddings[1]
    n, n_rows = 130, g.n_nodes[1]
    rows, cols = rng.integers(0, n_rows, n).astype(np.int32), rng.integers(0, n_rows, n).astype(np.int32)
    tab = K.upload_alias(rng.integers(1, 30, n_rows).astype(np.float64), "cuda")
    dec = K.PreparedDecoderHinge(E, E, _dv(rows), _dv(cols), _dv(G), _dv(l), MARGIN, alias=tab, seed=SEED,
                                 offset=OFFSET)
    assert dec.attached
    plan.run()
    for seed, offset in ((SEED, OFFSET), (SEED2, OFFSET2)):
        dec.seed, dec.offset = seed, offset
        dec.neg_rows.fill_(-1)
        dec()
        torch.cuda.synchronize()
        assert dec.entry == "dg_decoder_hinge_rows_f32"
        _check(E.cpu().numpy(), G, l, rows, cols, dec.pos.cpu().numpy(), dec.neg.cpu().numpy(),
               dec.neg_rows.cpu().numpy(), float(dec.loss[0]), K.unigram_sample(tab, n, seed, offset).cpu().numpy(),
               -(-n // 16))
    dec.release()

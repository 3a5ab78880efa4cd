"""Kernel-level tests of every site that applies a dropout mask, path by path.  The reference of every
comparison is oracle.dropout_scale (pinned on its own in test_cpu_dropout_stream.py) plus float64 numpy:

    dropout_rows_kernel / dropout_elems_kernel / dropout_rows_map_kernel / dropout_elems_map_kernel
                                 (dropout.hip)  out = src · scale: one fp32 multiply, np.array_equal
    gemm_f32_reduce_k32<1>, gemm_f32_reduce_k32<2>, gemm_f32_generic with a dropout descriptor
                                 (gemm.hip)     mask element (map(b)·m + row)·n + col
    spmm_groups_kernel<LP, U> with DG_GROUP_DROPOUT: range_head and range_body's prefetch
                                 (spmm.hip)     mask element c·nnz + (drop_index[p] or p)

Each case names the kernel, the lanes per row (LP) or the unroll the dispatcher gives it, so a change to a
dispatch heuristic shows which case lost its purpose.

The GEMM and SpMM cases run on the two input kinds of test_gpu_gemm_paths.py:
  exact — integers in [-3, 3] as fp32, keep 0.5 or 0.25 (1/keep a power of two), float64 reference, every
          partial sum far below 2^24: one wrong mask bit moves an element by a whole integer, np.array_equal.
  gauss — standard_normal, keep 0.7 and 0.9, rel_err <= 1e-5 (test_gpu_gemm_paths.TOL, the bar the masked
          GEMM tests of test_gpu_train.py hold these kernels to).
Outputs start as NaN; whatever a launch must not write keeps that NaN bit for bit."""
import numpy as np
import pytest
import scipy.sparse as sp

from conftest import rel_err
from oracle import decagon_oracle as orc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

KINDS = ["exact", "gauss"]
KEEPS = {"exact": (0.5, 0.25), "gauss": (0.7, 0.9)}
NAN_BITS = np.float32(np.nan).view(np.uint32)
TOL = 1e-5
# (seed, step, tag): test_cpu_dropout_stream.TRIPLES — every field past its device width, and a training tag
BIG = (2 ** 64 - 1, 2 ** 32 + 3, 0xFFFFFFFF)
MID = (123456789012, 5, 77)
TRAIN = (20180701, 1, (2 << 16) | 3)


@pytest.fixture(scope="module")
def K():
    from decagon_amd import kernels

    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return kernels


def _state(seed, step):
    """The device's {seed, step} as uint64, held in an int64 tensor."""
    s64 = lambda v: v - (1 << 64) if v >= (1 << 63) else v  # noqa: E731
    return torch.tensor([s64(seed), s64(step)], dtype=torch.int64, device="cuda")


def _draw(rng, kind, shape, lim=3):
    if kind == "exact":
        return rng.integers(-lim, lim + 1, size=shape).astype(np.float32)
    return rng.standard_normal(shape).astype(np.float32)


def _src(rng, shape):
    """Gauss with negatives and some exact zeros."""
    x = rng.standard_normal(shape).astype(np.float32)
    x[rng.random(shape) < 0.1] = 0.0
    return x


def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda", dtype=torch.float32)


def _is_nan_sentinel(x):
    x = np.ascontiguousarray(x)
    return np.array_equal(x.view(np.uint32), np.full(x.shape, NAN_BITS, np.uint32))


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


# ------------------------------------------------------------------------------ dropout_rows_kernel
@pytest.mark.parametrize("triple", [MID, BIG], ids=["mid", "big"])
@pytest.mark.parametrize("d", [1, 8, 12, 64, 65, 200])  # the column loop strides by 64
def test_rows(K, d, triple):
    """dropout_rows_kernel: four rows a block (n_rows = 1, 3, 4, 5 and 4·37 + 1), out of place and in place
    (as train.py calls it); the rows of the buffer past n_rows keep their NaN."""
    seed, step, tag = triple
    st = _state(seed, step)
    rng = np.random.default_rng(d)
    for n_rows in (1, 3, 4, 5, 4 * 37 + 1):
        for keep in (0.8, 0.5):
            src = _src(rng, (n_rows, d))
            want = src * orc.dropout_scale(seed, step, tag, n_rows, keep)[:, None]
            out = _nan(n_rows + 3, d)
            K.dropout_rows(_dev(src), out[:n_rows], st, tag, keep)
            buf = _nan(n_rows + 3, d)
            buf[:n_rows] = _dev(src)
            K.dropout_rows(buf[:n_rows], buf[:n_rows], st, tag, keep)
            torch.cuda.synchronize()
            for got in (out.cpu().numpy(), buf.cpu().numpy()):
                assert np.array_equal(got[:n_rows], want), (n_rows, d, keep)
                assert _is_nan_sentinel(got[n_rows:])
        # keep 1.0 is the identity, bit for bit
        src = _src(rng, (n_rows, d))
        out = _nan(n_rows + 3, d)
        K.dropout_rows(_dev(src), out[:n_rows], st, tag, 1.0)
        torch.cuda.synchronize()
        assert _same_bits(out.cpu().numpy()[:n_rows], src) and _is_nan_sentinel(out.cpu().numpy()[n_rows:])


# ------------------------------------------------------------------------------ dropout_elems_kernel
@pytest.mark.parametrize("Kr,n,d", [
    (1, 1, 1), (3, 5, 3), (7, 50, 64),  # one trip of the grid-stride loop, a partial last block
    (3, 683, 512),  # 1,049,088 elements > 4096·256: the grid-stride loop makes a second trip (4 MB)
])
def test_elems(K, Kr, n, d):
    seed, step, tag = BIG if n == 5 else MID
    st = _state(seed, step)
    rng = np.random.default_rng(Kr * n * d)
    src = _src(rng, (n, d))
    for keep in (0.8, 1.0):
        out = _nan(Kr + 1, n, d)
        K.dropout_elems(_dev(src), out[:Kr], st, tag, keep)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        want = src[None] * orc.dropout_scale(seed, step, tag, Kr * n * d, keep).reshape(Kr, n, d)
        assert np.array_equal(got[:Kr], want), keep
        assert _is_nan_sentinel(got[Kr])
        if keep == 1.0:
            assert _same_bits(got[:Kr], np.broadcast_to(src, (Kr, n, d)))


# ------------------------------------------------------------------------------ dropout_rows_map_kernel
@pytest.mark.parametrize("flags", [0, 1, 2, 3])
@pytest.mark.parametrize("rps", [1, 5, 37])  # no multiple of 4: one block spans two slabs
def test_rows_map(K, rps, flags):
    """dropout_rows_map_kernel against the oracle itself: local slab b of a non-monotone map [5, 0, 3] into 7
    global slabs draws global row map[b]·rps + j; in / out addressed globally (flags bit 1 / 2) or locally.
    A globally addressed output keeps NaN in the slabs the map does not name; a globally addressed input
    holds NaN there (never read)."""
    seed, step, tag = BIG
    st = _state(seed, step)
    rmap = np.array([5, 0, 3], np.int32)
    G, L = 7, len(rmap)
    in_glob, out_glob = bool(flags & 1), bool(flags & 2)
    rng = np.random.default_rng(10 * rps + flags)
    for d in (12, 65):
        for keep in (0.7, 0.5):
            src = _src(rng, (L, rps, d))
            scale = orc.dropout_scale(seed, step, tag, G * rps, keep).reshape(G, rps)
            want = src * scale[rmap][:, :, None]
            inp = np.full((G, rps, d), np.nan, np.float32)
            inp[rmap] = src
            out = _nan((G if out_glob else L) + 1, rps, d)
            K.dropout_rows_map(_dev(inp if in_glob else src), out[:-1], _dev(rmap), rps, st, tag, keep, in_glob,
                               out_glob)
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            if out_glob:
                assert np.array_equal(got[rmap], want), (d, keep)
                assert _is_nan_sentinel(np.delete(got, rmap, axis=0))
            else:
                assert np.array_equal(got[:L], want), (d, keep)
                assert _is_nan_sentinel(got[L:])


# ------------------------------------------------------------------------------ dropout_elems_map_kernel
@pytest.mark.parametrize("rmap,n,d", [
    ([5, 0, 3], 5, 3),      # plane 15: no multiple of 256, several slabs in one block
    ([5, 0, 3], 37, 12),    # plane 444: a block spans two slabs
    ([4, 0, 2], 683, 512),  # 1,049,088 elements > 4096·256: the grid-stride loop makes a second trip
])
def test_elems_map(K, rmap, n, d):
    seed, step, tag = TRAIN if n == 37 else BIG
    st = _state(seed, step)
    rmap = np.array(rmap, np.int32)
    L, G = len(rmap), int(rmap.max()) + 2
    rng = np.random.default_rng(n * d)
    src = _src(rng, (n, d))
    keep = 0.7
    out = _nan(L + 1, n, d)
    K.dropout_elems_map(_dev(src), out[:L], _dev(rmap), st, tag, keep)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    want = src[None] * orc.dropout_scale(seed, step, tag, G * n * d, keep).reshape(G, n, d)[rmap]
    assert np.array_equal(got[:L], want)
    assert _is_nan_sentinel(got[L])


# ------------------------------------------------------------------------------ dropout_advance_kernel
@pytest.mark.parametrize("seed,step", [(20180701, 0), (2 ** 64 - 1, 2 ** 32 - 1)])
def test_advance(K, seed, step):
    """After dg_dropout_advance the next draw is the oracle's at step + 1 (the counter is 64-bit; the key
    takes its low 32 bits, as the oracle does)."""
    st = _state(seed, step)
    src = _src(np.random.default_rng(1), (33, 8))
    for s in (step, step + 1, step + 2):
        out = _nan(33, 8)
        K.dropout_rows(_dev(src), out, st, 9, 0.5)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), src * orc.dropout_scale(seed, s, 9, 33, 0.5)[:, None]), s
        K.dropout_advance(st)
    torch.cuda.synchronize()
    assert int(st[1]) == step + 3 and int(st[0]) & (2 ** 64 - 1) == seed


# ------------------------------------------------------------------------------ refused before launch
def test_dropout_refusals(K):
    """keep 0, keep 1.5, keep NaN and d = 0 are refused by all four kernels' entry points, and the output
    keeps its NaN; empty shapes return cleanly."""
    from decagon_amd import _lib

    lib = _lib.load()
    st = _state(1, 1)
    rmap = _dev(np.array([1, 0], np.int32))
    src2, src3 = _dev(np.ones((10, 8), np.float32)), _dev(np.ones((5, 8), np.float32))
    refused = (_lib.KernelError, ValueError)
    for keep in (0.0, 1.5, float("nan"), -0.5):
        out2, out3 = _nan(10, 8), _nan(2, 5, 8)
        with pytest.raises(refused):
            K.dropout_rows(src2, out2, st, 3, keep)
        with pytest.raises(refused):
            K.dropout_rows_map(src2, out2, rmap, 5, st, 3, keep, False, False)
        with pytest.raises(refused):
            K.dropout_elems(src3, out3, st, 3, keep)
        with pytest.raises(refused):
            K.dropout_elems_map(src3, out3, rmap, st, 3, keep)
        torch.cuda.synchronize()
        assert _is_nan_sentinel(out2.cpu().numpy()) and _is_nan_sentinel(out3.cpu().numpy())
    # d = 0: the wrappers on zero-width tensors, and the entry points on real buffers
    e2, e3 = torch.empty((10, 0), device="cuda"), torch.empty((2, 5, 0), device="cuda")
    with pytest.raises(refused):
        K.dropout_rows(e2, e2, st, 3, 0.5)
    with pytest.raises(refused):
        K.dropout_rows_map(e2, e2, rmap, 5, st, 3, 0.5, False, False)
    with pytest.raises(refused):
        K.dropout_elems(e2[:5], e3, st, 3, 0.5)
    with pytest.raises(refused):
        K.dropout_elems_map(e2[:5], e3, rmap, st, 3, 0.5)
    out2, out3 = _nan(10, 8), _nan(2, 5, 8)
    p = lambda t: t.data_ptr()  # noqa: E731
    assert lib.dg_dropout_rows_f32(p(src2), p(out2), 10, 0, p(st), 3, 0.5, None) == _lib.DG_EINVAL
    assert lib.dg_dropout_rows_map_f32(p(src2), p(out2), p(rmap), 2, 5, 0, 0, p(st), 3, 0.5, None) == _lib.DG_EINVAL
    assert lib.dg_dropout_rows_map_f32(p(src2), p(out2), p(rmap), 2, 5, 8, 4, p(st), 3, 0.5, None) == _lib.DG_EINVAL
    assert lib.dg_dropout_elems_f32(p(src3), p(out3), 2, 5, 0, p(st), 3, 0.5, None) == _lib.DG_EINVAL
    assert lib.dg_dropout_elems_map_f32(p(src3), p(out3), p(rmap), 2, 5, 0, p(st), 3, 0.5, None) == _lib.DG_EINVAL
    torch.cuda.synchronize()
    assert _is_nan_sentinel(out2.cpu().numpy()) and _is_nan_sentinel(out3.cpu().numpy())
    # nothing to do: no launch, no error
    z2 = torch.empty((0, 8), device="cuda")
    K.dropout_rows(z2, z2, st, 3, 0.5)
    K.dropout_rows_map(z2, z2, rmap[:0], 5, st, 3, 0.5, False, False)
    K.dropout_elems(z2, torch.empty((2, 0, 8), device="cuda"), st, 3, 0.5)
    K.dropout_elems(src3, torch.empty((0, 5, 8), device="cuda"), st, 3, 0.5)
    K.dropout_elems_map(src3, torch.empty((0, 5, 8), device="cuda"), rmap[:0], st, 3, 0.5)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------ masked batch-reduce GEMM
GB = 11  # batches of the masked reduce cases


def _compare(kind, got, want, what):
    """got [..., m, n] against want (float64), matrix by matrix."""
    if kind == "exact":
        # at most 64 terms of magnitude <= 3·3, scaled by 1/keep <= 4, summed over <= 11 batches
        assert np.abs(want).max() * 2 < 2 ** 24 and 64 * 9 * 4 * GB * 2 < 2 ** 24
        assert np.array_equal(got, want), what
    else:
        got = got.reshape((-1,) + got.shape[-2:])
        want = want.reshape(got.shape)
        for q in range(len(want)):
            assert rel_err(got[q], want[q]) <= TOL, (what, q, rel_err(got[q], want[q]))


class _Masked:
    """One batch-reduce descriptor in the backward's layout (A [batch][m][k]; B [slabs][n][k] read transposed,
    strides (n·k, 1, k)) with its inputs and float64 reference
        out[q] = Σ_{b in run q} M_{map(b)} ∘ (A_b · B_{map(b)}),  M = dropout_scale(...).reshape(slabs, m, n);
    drop = None: the unmasked sum."""

    def __init__(self, K, rng, kind, m, n, k, R, mapped, drop, a_off=0, batch=GB, ones=False):
        self.kind, self.R = kind, R
        slabs = batch + 3 if mapped else batch
        if ones:  # A_b = e_0 rows, B_b = e_0 columns: every product is 1
            A = np.zeros((batch, m, k), np.float32)
            B = np.zeros((slabs, n, k), np.float32)
            A[:, :, 0] = 1.0
            B[:, :, 0] = 1.0
        else:
            A = _draw(rng, kind, (batch, m, k))
            B = _draw(rng, kind, (slabs, n, k))
        bmap = rng.permutation(slabs)[:batch].astype(np.int32) if mapped else np.arange(batch, dtype=np.int32)
        self.bmap = bmap
        a_flat = torch.empty(A.size + a_off, device="cuda")
        a_flat[a_off:] = _dev(A.ravel())
        self.runs = -(-batch // R)
        self.C = _nan(self.runs + 1, m, n)
        st = None
        prod = A.astype(np.float64) @ B[bmap].astype(np.float64).transpose(0, 2, 1)  # [batch][m][n]
        if drop is not None:
            (seed, step, tag), keep = drop
            st = _state(seed, step)
            M = orc.dropout_scale(seed, step, tag, slabs * m * n, keep).reshape(slabs, m, n).astype(np.float64)
            self.mask = M[bmap]
            prod = prod * self.mask
        self.want = np.stack([prod[q * R:(q + 1) * R].sum(axis=0) for q in range(self.runs)])
        self.gemm = K.PreparedGemm(a_flat[a_off:], (m * k, k, 1), _dev(B), (n * k, 1, k), self.C, (m * n, n, 1), m, n, k,
                                   batch, b_map=_dev(bmap) if mapped else None, b_batches=slabs,
                                   b_map_max=int(bmap.max()) if mapped else None, reduce=R,
                                   drop=None if drop is None else (st, tag, keep))

    def check(self, what):
        got = self.C.cpu().numpy()
        _compare(self.kind, got[:self.runs], self.want, what)
        assert _is_nan_sentinel(got[self.runs]), what


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,k,a_off", [
    (32, 32, 0),   # gemm_f32_reduce_k32<1>
    (16, 32, 0),   # gemm_f32_reduce_k32<1>, partial tile
    (48, 32, 0),   # gemm_f32_reduce_k32<2>, partial second tile
    (64, 32, 0),   # gemm_f32_reduce_k32<2> (the model's shape)
    (96, 32, 0),   # gemm_f32_generic with a dropout descriptor: n > 64, three column tiles
    (40, 19, 0),   # gemm_f32_generic with a dropout descriptor: odd k
    (32, 64, 0),   # gemm_f32_generic with a dropout descriptor: k != 32
    (32, 32, 1),   # gemm_f32_generic with a dropout descriptor: A not 16-byte aligned
])
def test_masked_batch_reduce(K, kind, n, k, a_off):
    """m = 37 (two row tiles) and 161 (six: a second block, tm = tb·4 + wave inside the mask index), 11 batches
    in runs of R = 1, 4 (a short last run) and 11 (bpw = R), unmapped and with a permuting map into 14 slabs:
    the mask follows the mapped slab, A and the run index do not."""
    rng = np.random.default_rng(2000 + n + k + a_off)
    triple = BIG if kind == "exact" else TRAIN
    for m in (37, 161):
        for R in (1, 4, GB):
            for mapped in (False, True):
                for keep in KEEPS[kind]:
                    g = _Masked(K, rng, kind, m, n, k, R, mapped, (triple, keep), a_off)
                    g.gemm()
                    torch.cuda.synchronize()
                    g.check((m, n, k, R, mapped, keep))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", ["reduce_k32<1>", "reduce_k32<2>", "generic"])
def test_masked_multi(K, kind, case):
    """One PreparedGemmMulti with a masked descriptor, an unmasked one and a second masked one of another tag
    and keep: each keeps its own mask (or none).  n = 32, 16, 32 at k = 32: gemm_f32_reduce_k32<1>; n = 32, 64,
    48: gemm_f32_reduce_k32<2> (the n = 32 descriptor's second column tile idle); k = 19: gemm_f32_generic."""
    rng = np.random.default_rng(2100 + len(case))
    ns = {"reduce_k32<1>": (32, 16, 32), "reduce_k32<2>": (32, 64, 48), "generic": (32, 64, 48)}[case]
    k = 19 if case == "generic" else 32
    k0, k1 = KEEPS[kind]
    ds = [_Masked(K, rng, kind, 37, ns[0], k, 4, True, ((20180701, 4, (2 << 16) | 1), k0)),
          _Masked(K, rng, kind, 70, ns[1], k, 3, True, None),
          _Masked(K, rng, kind, 161, ns[2], k, GB, False, ((20180701, 4, (2 << 16) | 2), k1))]
    K.PreparedGemmMulti([d.gemm for d in ds])()
    torch.cuda.synchronize()
    for i, d in enumerate(ds):
        d.check((case, i))


@pytest.mark.parametrize("n,k", [
    (32, 32),  # gemm_f32_reduce_k32<1>
    (64, 32),  # gemm_f32_reduce_k32<2>
    (96, 32),  # gemm_f32_generic
])
def test_masked_gemm_agrees_with_dropout_elems(K, n, k):
    """The forward's masks (dropout_elems_kernel / dropout_elems_map_kernel on ones) and the backward's
    (the masked batch-reduce GEMM on all-ones products) on the device: out[q] is the sum over run q of the
    forward's masked ones, bit for bit (keep 0.5: every sum exact), and both are the oracle's."""
    seed, step, tag = TRAIN
    rng = np.random.default_rng(n)
    m, keep = 161, 0.5
    for mapped in (False, True):
        g = _Masked(K, rng, "exact", m, n, k, 4, mapped, (TRAIN, keep), ones=True)
        g.gemm()
        slabs = GB + 3 if mapped else GB
        el = _nan(GB, m, n)
        ones = torch.ones((m, n), device="cuda")
        if mapped:
            K.dropout_elems_map(ones, el, _dev(g.bmap), _state(seed, step), tag, keep)
        else:
            K.dropout_elems(ones, el, _state(seed, step), tag, keep)
        torch.cuda.synchronize()
        fwd = el.cpu().numpy()
        assert np.array_equal(fwd, g.mask), slabs
        got = g.C.cpu().numpy()
        want = np.stack([fwd[q * 4:(q + 1) * 4].sum(axis=0, dtype=np.float32) for q in range(g.runs)])
        assert _same_bits(got[:g.runs], want)
        g.check(mapped)


# ------------------------------------------------------------------------------ masked shared-pattern SpMM
def _pattern(rng, kind, lens, n_cols):
    """A CSR with the given row lengths: distinct sorted columns per row, values of `kind`."""
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    col = np.concatenate([np.sort(rng.choice(n_cols, l, replace=False)) for l in lens] + [np.zeros(0, np.int64)])
    val = _draw(rng, kind, len(col))
    if kind == "exact":
        val[val == 0] = 1.0  # (a zero value would hide its mask bit)
    return rowptr, col.astype(np.int32), val


def _masked_spmm_want(rowptr, col, val, X, drop, index):
    """out[c] = (val ∘ M[c·nnz + idx]) as CSR @ X_c in float64."""
    n_chunks, F = X.shape[0], X.shape[1]
    nnz = len(val)
    if drop is None:
        M = np.ones((n_chunks, nnz))
    else:
        (seed, step, tag), keep = drop
        M = orc.dropout_scale(seed, step, tag, n_chunks * nnz, keep).reshape(n_chunks, nnz).astype(np.float64)
        if index is not None:
            M = M[:, index]
    return np.stack([sp.csr_matrix((val.astype(np.float64) * M[c], col, rowptr), shape=(len(rowptr) - 1, F))
                     @ X[c].astype(np.float64) for c in range(n_chunks)])


def _shared_spec(K, rowptr, col, val, X, out, drop, index):
    n_chunks, F, d = X.shape
    dd = None
    if drop is not None:
        (seed, step, tag), keep = drop
        dd = (_state(seed, step), tag, keep)
    return K.RelGroupSpec(_dev(rowptr), _dev(col), _dev(val), _dev(X), out, len(rowptr) - 1, n_chunks, d, F,
                          vcol_max=int(col.max()) if len(col) else -1, shared=True, drop=dd,
                          drop_index=_dev(index.astype(np.int32)) if index is not None else None)


def _spmm_compare(kind, got, want, what):
    if kind == "exact":
        # at most 200 terms of magnitude <= 3·3·4
        assert np.abs(want).max() * 2 < 2 ** 24 and 200 * 36 * 2 < 2 ** 24
        assert np.array_equal(got, want), what
    else:
        assert rel_err(got, want) <= TOL, (what, rel_err(got, want))


# rows of 0, 1, 63, 64, 65, 130 and 200 nonzeros: the first, second and third batches of 64 (range_head, and
# range_body's prefetch with its read past the end predicated off), a short row after the long ones and an
# empty last row; 11 rows: a remainder mod 8 (two rows a wave, eight a block), the last wave holding one row
LENS = [0, 1, 63, 64, 65, 130, 200, 3, 17, 64, 0]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("indexed", [False, True], ids=["plain", "drop_index"])
@pytest.mark.parametrize("d", [4, 12, 32, 64, 256])  # spmm_groups_kernel<LP, 8>, LP = 1, 4, 8, 16, 64
def test_masked_spmm(K, kind, indexed, d):
    """3 chunks of one shared pattern, each masking the pattern's values with its own draw: element
    c·nnz + p, or c·nnz + drop_index[p] with drop_index a random permutation."""
    rng = np.random.default_rng(3000 + d + indexed)
    F = 210
    rowptr, col, val = _pattern(rng, kind, LENS, F)
    index = rng.permutation(len(val)) if indexed else None
    X = _draw(rng, kind, (3, F, d))
    for keep in KEEPS[kind]:
        drop = (BIG if kind == "exact" else TRAIN, keep)
        out = _nan(4, len(LENS), d)
        K.spmm_groups([_shared_spec(K, rowptr, col, val, X, out, drop, index)], d)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        _spmm_compare(kind, got[:3], _masked_spmm_want(rowptr, col, val, X, drop, index), (d, keep))
        assert _is_nan_sentinel(got[3])
        assert not got[:3, [0, -1]].any()  # the empty rows are written, as zeros


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("indexed", [False, True], ids=["plain", "drop_index"])
def test_masked_spmm_short_unroll(K, kind, indexed):
    """16 chunks x 1024 rows: 16·ceil(1024/8) = 2048 workgroups = DG_GROUP_U4_BLOCKS, spmm_groups_kernel<8, 4>
    (the launches above stay below and run <LP, 8>): rows of about 3 nonzeros, and a few of 70, 130 and 200
    so the shorter unroll steps several times a batch.  Equal to the same reference: 'same bits either way'."""
    rng = np.random.default_rng(3100 + indexed)
    F, d, n_rows, n_chunks = 210, 32, 1024, 16
    lens = rng.integers(0, 7, n_rows)
    lens[[5, 300, 1022]] = (70, 130, 200)
    lens[-1] = 0
    rowptr, col, val = _pattern(rng, kind, lens, F)
    index = rng.permutation(len(val)) if indexed else None
    X = _draw(rng, kind, (n_chunks, F, d))
    drop = (TRAIN, KEEPS[kind][0])
    out = _nan(n_chunks + 1, n_rows, d)
    K.spmm_groups([_shared_spec(K, rowptr, col, val, X, out, drop, index)], d)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    _spmm_compare(kind, got[:n_chunks], _masked_spmm_want(rowptr, col, val, X, drop, index), "U4")
    assert _is_nan_sentinel(got[n_chunks])


@pytest.mark.parametrize("kind", KINDS)
def test_masked_spmm_beside_unmasked_merged(K, kind):
    """One launch with a masked shared group, an unmasked merged group of the same pattern and a second masked
    shared group of another tag: the unmasked one is untouched by its neighbours' states."""
    from decagon_amd.sparse import HostCSR, merge_chunks

    rng = np.random.default_rng(3200)
    F, d, nrel = 210, 32, 3
    rowptr, col, val = _pattern(rng, kind, LENS, F)
    X = _draw(rng, kind, (nrel, F, d))
    k0, k1 = KEEPS[kind]
    drops = [(TRAIN, k0), None, ((20180701, 1, (1 << 16) | 2), k1)]
    outs = [_nan(nrel + 1, len(LENS), d) for _ in drops]
    index = rng.permutation(len(val))
    h = HostCSR(rowptr, col, val, (len(LENS), F))
    mm = merge_chunks([h] * nrel, np.arange(nrel), 1, nrel)
    merged = K.RelGroupSpec(_dev(mm.rowptr), _dev(mm.vcol), _dev(mm.val), _dev(X), outs[1], len(LENS), nrel, d,
                            nrel * F, vcol_max=int(mm.vcol.max()))
    K.spmm_groups([_shared_spec(K, rowptr, col, val, X, outs[0], drops[0], None), merged,
                   _shared_spec(K, rowptr, col, val, X, outs[2], drops[2], index)], d)
    torch.cuda.synchronize()
    for i, (drop, idx) in enumerate(zip(drops, (None, None, index))):
        got = outs[i].cpu().numpy()
        _spmm_compare(kind, got[:nrel], _masked_spmm_want(rowptr, col, val, X, drop, idx), i)
        assert _is_nan_sentinel(got[nrel])


def test_masked_spmm_forward_backward_transposition(K):
    """As the engine uses the masks: the forward is X (no index), the backward Xᵀ from
    transpose_csr(X, with_perm=True) with drop_index = perm.  Fed identity operands (columns padded to a
    multiple of 4), each returns its masked matrix densely: exact transposes of one another per chunk, and
    the oracle's."""
    from decagon_amd.sparse import HostCSR
    from decagon_amd.train import transpose_csr

    rng = np.random.default_rng(3300)
    n_r, F, n_chunks, keep = 37, 50, 3, 0.7
    lens = rng.integers(0, 9, n_r)
    lens[3] = F  # a full row
    rowptr, col, val = _pattern(rng, "gauss", lens, F)
    xt, perm = transpose_csr(HostCSR(rowptr, col, val, (n_r, F)), with_perm=True)
    drop = (TRAIN, keep)
    Fp, rp = -(-F // 4) * 4, -(-n_r // 4) * 4
    eye_f = np.broadcast_to(np.eye(F, Fp, dtype=np.float32), (n_chunks, F, Fp)).copy()
    eye_r = np.broadcast_to(np.eye(n_r, rp, dtype=np.float32), (n_chunks, n_r, rp)).copy()
    out_f, out_b = _nan(n_chunks, n_r, Fp), _nan(n_chunks, F, rp)
    K.spmm_groups([_shared_spec(K, rowptr, col, val, eye_f, out_f, drop, None)], Fp)
    K.spmm_groups([_shared_spec(K, xt.rowptr, xt.col, xt.val, eye_r, out_b, drop, perm)], rp)
    torch.cuda.synchronize()
    fwd, bwd = out_f.cpu().numpy(), out_b.cpu().numpy()
    M = orc.dropout_scale(*TRAIN, n_chunks * len(val), keep).reshape(n_chunks, -1)
    for c in range(n_chunks):
        want = sp.csr_matrix((val * M[c], col, rowptr), shape=(n_r, F)).toarray()  # one fp32 multiply: exact
        assert np.array_equal(fwd[c, :, :F], want), c
        assert np.array_equal(bwd[c, :, :n_r], want.T), c
        assert np.array_equal(fwd[c, :, :F], bwd[c, :, :n_r].T), c
        assert not fwd[c, :, F:].any() and not bwd[c, :, n_r:].any()
    assert M.min() == 0 and 0 < (M == 0).mean() < 1  # (some dropped, some kept)


def test_masked_spmm_refusals(K):
    """DG_GROUP_DROPOUT without the shared flag, keep 0 (1.5, NaN) and n_chunks·drop_stride > 2^32 - 1 are
    refused by the wrapper and by the entry point; the output keeps its NaN."""
    from decagon_amd import _lib

    rng = np.random.default_rng(3400)
    F, d = 210, 32
    rowptr, col, val = _pattern(rng, "gauss", LENS, F)
    X = _draw(rng, "gauss", (3, F, d))
    out = _nan(3, len(LENS), d)
    good = _shared_spec(K, rowptr, col, val, X, out, (TRAIN, 0.5), None)
    lib = _lib.load()

    def raw(edit):
        arr = (_lib.DgRelGroup * 1)()
        K._fill_group(arr[0], good)
        edit(arr[0])
        return lib.dg_spmm_groups_f32(arr, 1, d, None)

    def set_(**kw):
        def edit(g):
            for name, v in kw.items():
                setattr(g, name, v)
        return edit

    assert raw(set_(flags=_lib.DG_GROUP_DROPOUT)) == _lib.DG_EINVAL
    for keep in (0.0, 1.5, float("nan")):
        assert raw(set_(drop_keep=keep)) == _lib.DG_EINVAL
        with pytest.raises(ValueError):
            K.spmm_groups([_shared_spec(K, rowptr, col, val, X, out, (TRAIN, keep), None)], d)
    assert raw(set_(drop_stride=2 ** 31 - 1)) == _lib.DG_EINVAL  # 3·(2^31 - 1) > 2^32 - 1
    assert raw(set_(drop_stride=-1)) == _lib.DG_EINVAL
    assert raw(set_(drop_state=None)) == _lib.DG_EINVAL
    unshared = _shared_spec(K, rowptr, col, val, X[:1], out, (TRAIN, 0.5), None)  # (one chunk: a valid plain CSR)
    unshared.shared = False
    with pytest.raises(ValueError, match="shared pattern"):
        K.spmm_groups([unshared], d)
    torch.cuda.synchronize()
    assert _is_nan_sentinel(out.cpu().numpy())
    assert raw(set_()) == _lib.DG_OK  # (the unedited descriptor is accepted)
    torch.cuda.synchronize()
    assert not np.isnan(out.cpu().numpy()).any()

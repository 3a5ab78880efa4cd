"""Kernel-level tests of every dispatch path of dg_gemm_f32 and every instantiation of
dg_gemm_tn_f32 (csrc/gemm.hip).

Each case names the kernel and the batches per block (`bpb`, projection kernel) or per wave
(`bpw`, resident-A / generic kernels) that the dispatcher gives it:
    tiles_m = ceil(m/32), tiles_n = ceil(n/32)
    resident-A / generic:  tile_blocks = ceil(tiles_m·tiles_n / 4);
                           bpw doubles (from 1, up to 16) while tile_blocks·4·ceil(batch/(2·bpw)) >= 8192
    projection:            nbm = ceil(tiles_m/8), wpb = max(4, ceil(tiles_m/nbm)), tile_blocks = ceil(tiles_m/wpb);
                           bpb doubles (from 1, up to 64) while tile_blocks·ceil(batch/(2·bpb)) >= 512
    batch-reduce:          bpw = R (the run length)
so a change to those heuristics shows which case lost its purpose.

Every shape runs on two kinds of input:
  exact — small integers stored as fp32, reference in float64 (exact on integers this small).  Every
          partial sum stays far below 2^24, where the fp32 MFMA / fmaf chains are exact, so any indexing,
          stale-operand or tail error is an inequality whatever its magnitude: np.array_equal.
  gauss — seeded standard_normal fp32 against the float64 product, rel_err <= 1e-5 (a float32 numpy
          restatement of these products meets that bar on these inputs).
Outputs start as NaN; whatever the launch must not write keeps that NaN bit for bit."""
import numpy as np
import pytest

from conftest import rel_err

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

KINDS = ["exact", "gauss"]
NAN_BITS = np.float32(np.nan).view(np.uint32)
TOL = 1e-5


@pytest.fixture(scope="module")
def K():
    from decagon_amd import kernels

    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return kernels


def _draw(rng, kind, shape, lim=3):
    """exact: integers in [-lim, lim]; gauss: standard normal.  fp32."""
    if kind == "exact":
        return rng.integers(-lim, lim + 1, size=shape).astype(np.float32)
    return rng.standard_normal(shape).astype(np.float32)


def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda", dtype=torch.float32)


def _is_nan_sentinel(x):
    return np.array_equal(np.ascontiguousarray(x).view(np.uint32), np.full(x.shape, NAN_BITS, np.uint32))


def _compare(kind, got, want, what=""):
    """got [..., m, n] against want (float64), matrix by matrix."""
    if kind == "exact":
        # at most 4,800 terms (75 batches x 64) of magnitude <= 3·3·2 (a·b·sa), times sc <= 2
        assert np.abs(want).max() * 2 < 2 ** 24 and 4800 * 18 * 2 < 2 ** 24
        assert np.array_equal(got, want), what
    else:
        got = got.reshape((-1,) + got.shape[-2:])
        want = want.reshape(got.shape)
        den = np.abs(want).max(axis=(1, 2))
        err = np.abs(got - want).max(axis=(1, 2))
        assert np.all(den > 0)
        assert float((err / den).max()) <= TOL, (what, float((err / den).max()))


def _plain(K, kind, seed, m, n, k, batch, *, per_batch_a=False, sa=False, sc=False, c_t=False, a_off=0,
           b_pad=0, extra=3):
    """C[map(b)] = diag-scaled A(_b) · B[map(b)] through PreparedGemm, with a batch map into batch + extra
    slabs; checks every mapped slab, and that the unmapped ones (and B's padding, never read) left no trace."""
    rng = np.random.default_rng(seed)
    slabs = batch + extra
    A = _draw(rng, kind, (batch if per_batch_a else 1, m, k))
    ldb = n + b_pad
    Bw = np.full((slabs, k, ldb), np.nan, np.float32)  # (b_sk > n: the padding is never read)
    Bw[:, :, :n] = _draw(rng, kind, (slabs, k, n))
    bmap = rng.permutation(slabs)[:batch].astype(np.int32)
    sa_h = _draw(rng, kind, k, 2) if sa else None
    sc_h = _draw(rng, kind, n, 2) if sc else None
    a_flat = torch.empty(A.size + a_off, device="cuda")
    a_flat[a_off:] = torch.from_numpy(A.ravel()).cuda()
    C = _nan(slabs, n, m) if c_t else _nan(slabs, m, n)
    K.PreparedGemm(a_flat[a_off:], (m * k if per_batch_a else 0, k, 1), torch.from_numpy(Bw).cuda(), (k * ldb, ldb, 1),
                   C, (m * n, 1, m) if c_t else (m * n, n, 1), m, n, k, batch,
                   torch.from_numpy(sa_h).cuda() if sa else None, torch.from_numpy(sc_h).cuda() if sc else None,
                   b_map=torch.from_numpy(bmap).cuda(), b_batches=slabs, b_map_max=int(bmap.max()))()
    torch.cuda.synchronize()
    got = C.cpu().numpy()
    if c_t:
        got = got.transpose(0, 2, 1)
    A64 = A.astype(np.float64) * (sa_h.astype(np.float64) if sa else 1.0)
    want = A64 @ Bw[bmap, :, :n].astype(np.float64)  # [1 or batch, m, k] @ [batch, k, n]
    if sc:
        want = want * sc_h.astype(np.float64)
    _compare(kind, got[bmap], want, (m, n, k, batch))
    untouched = np.setdiff1d(np.arange(slabs), bmap)
    assert len(untouched) == extra and _is_nan_sentinel(got[untouched])


# ------------------------------------------------------------------------------ projection kernel
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("m,k,batch", [
    # gemm_f32_proj<64>: 9 tiles, nbm 2, wpb 5 (320 threads), tile_blocks 2; 2·ceil(1030/2) = 1030,
    # 2·ceil(1030/4) = 516 >= 512, 2·ceil(1030/8) = 258 < 512: bpb 4, last run 2 (1030 = 257·4 + 2)
    (257, 64, 1030),
    # gemm_f32_proj<32>: the same plan; (tid + 320) & 255 wraps in the staging of B
    (257, 32, 1030),
    # gemm_f32_proj<64>: 1 tile, wpb 4, tile_blocks 1; ceil(1024/2) = 512 >= 512, ceil(1024/4) = 256: bpb 2
    (32, 64, 1024),
])
def test_projection_several_batches_per_block(K, kind, m, k, batch):
    """The double-buffered steady state of gemm_f32_proj (put_b / load_b two batches ahead / the batch
    map through readlane) only iterates when a block owns more than one batch."""
    _plain(K, kind, 100 + m + k, m, 32, k, batch)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k", [32, 64])
@pytest.mark.parametrize("n", [4, 12, 28])
def test_projection_general_n(K, kind, k, n):
    """gemm_f32_proj<k> MODE 2 (n < 32), bpb 1: m = 1, 31, 33 — 1 or 2 tiles, wpb 4; m = 353 — 12 tiles,
    nbm 2, wpb 6 (384 threads), tile_blocks 2."""
    for m in (1, 31, 33, 353):
        _plain(K, kind, 200 + n + k + m, m, n, k, 3)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k", [32, 64])
def test_projection_last_tile_shuffle(K, kind, k):
    """gemm_f32_proj<k> MODE 1 (n = 32), bpb 1, wpb 4: the lanes past the last row of a partial tile store
    row m-1's values, shuffled in from the lane that owns it."""
    for m in (1, 31, 32, 33):
        _plain(K, kind, 300 + k + m, m, 32, k, 3)


# ------------------------------------------------------------------------------ resident-A / generic
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k", [32, 64])
@pytest.mark.parametrize("why", ["n30", "n33", "n70", "sa", "sc", "c_transposed", "a_unaligned", "b_sk_odd"])
def test_projection_fall_through(K, kind, k, why):
    """One disqualifier of the projection shape at a time: gemm_f32_resident_a<k>, bpw 1 (m = 37: 2 or 6
    tiles, tile_blocks 1 or 2, 4·2·ceil(3/2) << 8192)."""
    n = {"n30": 30, "n33": 33, "n70": 70}.get(why, 32)
    _plain(K, kind, 400 + k + n + len(why), 37, n, k, 3, sa=why == "sa", sc=why == "sc",
           c_t=why == "c_transposed", a_off=1 if why == "a_unaligned" else 0, b_pad=1 if why == "b_sk_odd" else 0)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k", [19, 32, 64])
def test_per_batch_a(K, kind, k):
    """a_bs = m·k (A is [batch][m][k], the dropout forward's operand): gemm_f32_resident_a<32/64>, or
    gemm_f32_generic at k = 19; bpw 1."""
    _plain(K, kind, 500 + k, 37, 32, k, 5, per_batch_a=True)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("per_batch_a", [True, False])
@pytest.mark.parametrize("k", [64, 19])
def test_two_batches_per_wave(K, kind, per_batch_a, k):
    """m = n = 20, sa set, batch = 4101: tile_blocks 1, 4·ceil(4101/2) = 8204 >= 8192 and
    4·ceil(4101/4) = 4104 < 8192: bpw 2, last run 1.  gemm_f32_resident_a<64> (k = 64; per-batch A: the
    only way to its load_a(b) for b != b0) or gemm_f32_generic (k = 19), per-batch and shared A."""
    _plain(K, kind, 600 + k + per_batch_a, 20, 20, k, 4101, per_batch_a=per_batch_a, sa=True)


# ------------------------------------------------------------------------------ batch-reduce
KR = 70  # batches of the reduce cases


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,k,a_off", [
    (32, 32, 0),   # gemm_f32_reduce_k32<1>
    (16, 32, 0),   # gemm_f32_reduce_k32<1>, partial tile
    (48, 32, 0),   # gemm_f32_reduce_k32<2>, partial second tile
    (96, 64, 0),   # gemm_f32_generic in batch-reduce mode (k != 32, n > 64)
    (32, 32, 1),   # gemm_f32_generic in batch-reduce mode (A not 16-byte aligned)
])
def test_batch_reduce(K, kind, n, k, a_off):
    """The backward's layout (A [K][m][k]; B [K+3][n][k] read transposed, strides (n·k, 1, k)), runs of
    R = 1, 16 and K + 5 batches (bpw = R), m = 1 and 33, with a batch map: B is mapped, A and the run
    index are not."""
    rng = np.random.default_rng(700 + n + k + a_off)
    for m in (1, 33):
        A = _draw(rng, kind, (KR, m, k))
        B = _draw(rng, kind, (KR + 3, n, k))
        bmap = rng.permutation(KR + 3)[:KR].astype(np.int32)
        a_flat = torch.empty(A.size + a_off, device="cuda")
        a_flat[a_off:] = torch.from_numpy(A.ravel()).cuda()
        prod = A.astype(np.float64) @ B[bmap].astype(np.float64).transpose(0, 2, 1)  # [K][m][n]
        for R in (1, 16, KR + 5):
            runs = -(-KR // R)
            C = _nan(runs + 1, m, n)
            K.PreparedGemm(a_flat[a_off:], (m * k, k, 1), torch.from_numpy(B).cuda(), (n * k, 1, k), C, (m * n, n, 1),
                           m, n, k, KR, b_map=torch.from_numpy(bmap).cuda(), b_batches=KR + 3,
                           b_map_max=int(bmap.max()), reduce=R)()
            torch.cuda.synchronize()
            got = C.cpu().numpy()
            want = np.stack([prod[q * R:q * R + R].sum(axis=0) for q in range(runs)])
            _compare(kind, got[:runs], want, (m, n, k, R))
            assert _is_nan_sentinel(got[runs])


# ------------------------------------------------------------------------------ several descriptors
class _Desc:
    """One descriptor of a multi-GEMM launch with its inputs and float64 reference."""

    def __init__(self, K, rng, kind, m, n, k, batch, reduce=0):
        self.kind, self.m, self.n, self.batch, self.reduce = kind, m, n, batch, reduce
        slabs = batch + 2
        if reduce:  # the backward's layout
            A = _draw(rng, kind, (batch, m, k))
            B = _draw(rng, kind, (slabs, n, k))
            a_str, b_str = (m * k, k, 1), (n * k, 1, k)
            Bm = B.transpose(0, 2, 1)
        else:
            A = _draw(rng, kind, (1, m, k))
            B = _draw(rng, kind, (slabs, k, n))
            a_str, b_str = (0, k, 1), (k * n, n, 1)
            Bm = B
        self.bmap = rng.permutation(slabs)[:batch].astype(np.int32)
        self.n_out = -(-batch // reduce) if reduce else slabs
        self.C = _nan(self.n_out + 1, m, n)
        prod = A.astype(np.float64) @ Bm[self.bmap].astype(np.float64) if batch and m and n else None
        if prod is None:
            self.want = None
        elif reduce:
            self.want = np.stack([prod[q * reduce:(q + 1) * reduce].sum(axis=0) for q in range(self.n_out)])
        else:
            self.want = prod
        dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731
        self.gemm = K.PreparedGemm(dev(A) if A.size else torch.zeros(4, device="cuda"), a_str,
                                   dev(B) if B.size else torch.zeros(4, device="cuda"), b_str, self.C, (m * n, n, 1),
                                   m, n, k, batch, b_map=dev(self.bmap) if batch else None, b_batches=slabs,
                                   b_map_max=int(self.bmap.max()) if batch else None, reduce=reduce)

    def check(self, what):
        got = self.C.cpu().numpy()
        if self.want is None:
            assert _is_nan_sentinel(got), what
        elif self.reduce:
            _compare(self.kind, got[:self.n_out], self.want, what)
            assert _is_nan_sentinel(got[self.n_out:]), what
        else:
            _compare(self.kind, got[self.bmap], self.want, what)
            assert _is_nan_sentinel(np.delete(got, self.bmap, axis=0)), what


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", ["proj", "mixed_k", "reduce", "reduce_and_plain"])
def test_multi(K, kind, case):
    """PreparedGemmMulti: block_begin / pick over several descriptors, each against its own reference.
      proj             three projection-eligible descriptors (k = 64; m = 33, 257, 100; n = 32, 16, 32), an
                       empty batch and an m = 0 descriptor between them: gemm_f32_proj<64> with the common
                       wpb 5 of the largest tiles_m (9), MODE 1 and MODE 2 in one launch, bpb 1
      mixed_k          k = 32 and k = 64 (and an n = 0 descriptor): kd falls to 0, gemm_f32_generic, bpw 1
      reduce           two batch-reduce descriptors, n = 32 and 64: gemm_f32_reduce_k32<2> for both
      reduce_and_plain a batch-reduce and a plain k = 32 descriptor: not all reduce, kd 0: gemm_f32_generic"""
    rng = np.random.default_rng(800 + len(case))
    D = lambda *a, **kw: _Desc(K, rng, kind, *a, **kw)  # noqa: E731
    if case == "proj":
        ds = [D(33, 32, 64, 3), D(40, 32, 64, 0), D(257, 16, 64, 2), D(0, 32, 64, 2), D(100, 32, 64, 4)]
    elif case == "mixed_k":
        ds = [D(33, 32, 32, 3), D(50, 0, 64, 2), D(70, 32, 64, 2)]
    elif case == "reduce":
        ds = [D(33, 32, 32, 9, reduce=4), D(70, 64, 32, 5, reduce=8)]
    else:
        ds = [D(33, 32, 32, 9, reduce=4), D(40, 32, 32, 3)]
    K.PreparedGemmMulti([d.gemm for d in ds])()
    torch.cuda.synchronize()
    for i, d in enumerate(ds):
        d.check((case, i))


@pytest.mark.parametrize("kind", KINDS)
def test_multi_max_groups(K, kind):
    """DG_MAX_GROUPS small descriptors in one launch (k = 19: gemm_f32_generic, bpw 1); one more is refused."""
    from decagon_amd import _lib

    rng = np.random.default_rng(900)
    ds = [_Desc(K, rng, kind, 5 + 9 * i, 3 + 11 * i, 19, 1 + i % 3) for i in range(_lib.DG_MAX_GROUPS + 1)]
    K.PreparedGemmMulti([d.gemm for d in ds[:-1]])()
    torch.cuda.synchronize()
    for i, d in enumerate(ds[:-1]):
        d.check(i)
    assert _is_nan_sentinel(ds[-1].C.cpu().numpy())
    with pytest.raises(ValueError):
        K.PreparedGemmMulti([d.gemm for d in ds])
    with pytest.raises(ValueError):
        K.PreparedGemmMulti([])


# ------------------------------------------------------------------------------ dg_gemm_tn_f32
TN_SHAPES = [(32, 32), (64, 32), (32, 64), (64, 64), (128, 32), (32, 128), (96, 32), (32, 96)]
TN_ROWS = (0, 1, 2, 7, 645)


def _tn_inputs(rng, kind, rows, M, N, batch, batched_a):
    A = _draw(rng, kind, (batch if batched_a else 1, rows, M))
    B = _draw(rng, kind, (batch, rows, N))
    want = np.einsum("brm,brn->bmn", np.broadcast_to(A, (batch, rows, M)).astype(np.float64), B.astype(np.float64))
    return A, B, want


def _tn_compare(kind, got, want, what):
    if not want.any():  # rows = 0 (or an all-zero product): exact zeros
        assert np.array_equal(got, want), what
    elif kind == "exact":
        # 645 terms of magnitude <= 3·3
        assert np.abs(want).max() * 2 < 2 ** 24 and 645 * 9 * 2 < 2 ** 24
        assert np.array_equal(got, want), what
    else:
        for b in range(want.shape[0]):
            assert rel_err(got[b], want[b]) <= TOL, (what, b)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("M,N", TN_SHAPES)
def test_gemm_tn_tile_shapes(K, kind, M, N):
    """gemm_tn_kernel<M/32, N/32>: c[b] = a(_b)ᵀ·b[b] for a shared [rows][M] and a batched [batch][rows][M],
    rows = 0 (exact zeros), 1 and 2 (one row pair, the second half of the lanes idle or not), 7 and 645;
    one row range (n_split 1), the default split, several ranges, and ranges of 2 rows."""
    rng = np.random.default_rng(1000 + M + 2 * N)
    for rows in TN_ROWS:
        for batch in (1, 3):
            for batched_a in (False, True):
                A, B, want = _tn_inputs(rng, kind, rows, M, N, batch, batched_a)
                Ad = torch.from_numpy(A if batched_a else A[0]).cuda()
                Bd = torch.from_numpy(B).cuda()
                for rps in ((1024, 0, 100, 2) if rows == 645 else (1024, 2)):
                    if rows == 645 and rps == 2 and (batch, batched_a) != (3, True):
                        continue  # (323 ranges: once per shape is enough)
                    C = _nan(batch, M, N)
                    op = K.PreparedGemmTN(Ad, Bd, C, rows_per_split=rps)
                    if rps == 1024 or rows <= 2:
                        assert op.n_split == 1
                    elif rows == 645:
                        assert op.n_split == {0: 11, 100: 7, 2: 323}[rps]
                    else:
                        assert op.n_split == 4
                    op()
                    torch.cuda.synchronize()
                    _tn_compare(kind, C.cpu().numpy(), want, (rows, batch, batched_a, rps))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("M,N", TN_SHAPES)
def test_gemm_tn_padded_rows_and_empty_ranges(K, kind, M, N):
    """Through the C entry point: lda = M + 4 and ldb = N + 8 with NaN in the padding (never read), and more
    row ranges than row pairs — rows = 7 in 8 ranges of 2 rows leaves four ranges empty, rows = 0 in 3 ranges
    leaves all of them empty: their partials are zeros."""
    from decagon_amd import _lib

    lib = _lib.load()
    rng = np.random.default_rng(1100 + M + 2 * N)
    lda, ldb = M + 4, N + 8
    for rows, n_split in ((0, 3), (1, 1), (2, 2), (7, 1), (7, 8), (645, 5)):
        for batch, batched_a in ((1, False), (3, False), (3, True)):
            A, B, want = _tn_inputs(rng, kind, rows, M, N, batch, batched_a)
            Aw = np.full((A.shape[0], max(rows, 1), lda), np.nan, np.float32)
            Bw = np.full((batch, max(rows, 1), ldb), np.nan, np.float32)
            Aw[:, :rows, :M] = A
            Bw[:, :rows, :N] = B
            Ad, Bd = torch.from_numpy(Aw).cuda(), torch.from_numpy(Bw).cuda()
            C = _nan(batch, M, N)
            part = _nan(n_split, batch, M, N)
            rc = lib.dg_gemm_tn_f32(Ad.data_ptr(), lda, Aw.shape[1] * lda if batched_a else 0, Bd.data_ptr(), ldb,
                                    Bw.shape[1] * ldb, C.data_ptr(), rows, M, N, batch, n_split,
                                    part.data_ptr() if n_split > 1 else None,
                                    torch.cuda.current_stream().cuda_stream)
            assert rc == _lib.DG_OK
            torch.cuda.synchronize()
            _tn_compare(kind, C.cpu().numpy(), want, (rows, n_split, batch, batched_a))
            if n_split == 8:  # ranges 4..7 start past the last row
                assert not part[4:].cpu().numpy().any()

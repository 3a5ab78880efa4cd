"""Kernel-level tests of the training-step kernels (csrc/train.hip) across the shapes their header
documents: dg_decoder_grad_f32, dg_scatter_rows_f32, dg_l2norm_grad_f32 and dg_adam_f32.

Every shape runs on two kinds of input:
  exact — small integers (or powers of two) stored as fp32, chosen so that every product and partial sum
          is an integer (or dyadic) far below 2^24: the fp32 chains are exact, the float64 reference is
          exact, and any indexing, stale-operand or tail error is an inequality whatever its magnitude.
  gauss — seeded standard_normal fp32 against a float64 restatement at the suite's fp32 bar (a float32
          numpy restatement of the same formulas meets that bar on these inputs).
Outputs start as NaN wherever the kernel must write everything, and what it must not write (padding
columns, rows no index names) keeps its bits."""
import numpy as np
import pytest

from conftest import rel_err
from oracle import decagon_oracle as orc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

KINDS = ["exact", "gauss"]
TOL = 1e-5


@pytest.fixture(scope="module")
def K():
    from decagon_amd import kernels

    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return kernels


def _T(x, dt=None):
    t = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    return t if dt is None else t.to(dt)


def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda", dtype=torch.float32)


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------ dg_decoder_grad_f32
MARGIN = 0.5
NR, NC = 9, 7  # table rows: with n > 9 pairs the row, negative and column indices all repeat


def _hinge_scores(rng, n, pattern):
    """pos / neg (multiples of 0.5) with z = neg - (pos - 0.5) drawn from the pattern's set; z == 0 is
    inactive (the kernel tests z > 0).  Every value is exact in fp32, and so is the kernel's z."""
    zs = {"mixed": [-1.0, -0.5, 0.0, 0.5, 1.0], "inactive": [-1.0, -0.5, 0.0], "active": [0.5, 1.0, 2.5]}[pattern]
    z = np.array([zs[(3 * p + p // 5) % len(zs)] for p in range(n)])
    pos = rng.integers(-6, 7, n) * 0.5
    neg = pos - MARGIN + z
    return pos.astype(np.float32), neg.astype(np.float32), (z > 0).astype(np.float64)


def _decoder_case(K, kind, seed, d, n, dec, pattern, padded):
    from decagon_amd import _lib

    rng = np.random.default_rng(seed)
    if kind == "exact":
        draw = lambda *s: rng.integers(-2, 3, size=s).astype(np.float32)  # noqa: E731
    else:
        draw = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    U, V = draw(NR, d), draw(NC, d)
    rows, cols, negs = (rng.integers(0, hi, n).astype(np.int32) for hi in (NR, NC, NR))
    if dec in ("dedicom", "bilinear"):
        G = draw(d, d)
    elif dec == "distmult":
        G = np.diag(draw(d)).astype(np.float32)
    else:
        G = np.eye(d, dtype=np.float32)
    l = draw(d) if dec == "dedicom" else None
    pos, neg, act = _hinge_scores(rng, n, pattern)
    # every output the decoder kind can ask for (dedicom: all three)
    dG = _nan(d * d) if dec in ("dedicom", "bilinear") else None
    dl = _nan(d) if dec == "dedicom" else None
    dgd = _nan(d) if dec in ("dedicom", "distmult") else None
    idx = [_T(x) for x in (rows, cols, negs)]
    if padded:  # ld_row = d + 4, ld_col = d + 8: the padding (NaN) is never read
        ldr, ldc = d + 4, d + 8
        Uw, Vw = np.full((NR, ldr), np.nan, np.float32), np.full((NC, ldc), np.nan, np.float32)
        Uw[:, :d], Vw[:, :d] = U, V
        lib = _lib.load()
        gr, gc = _nan(2 * n, d), _nan(n, d)
        nbytes = int(lib.dg_decoder_grad_workspace(n, d))
        ws = torch.empty(nbytes // 4, device="cuda")
        keep = (_T(Uw), _T(Vw), _T(pos), _T(neg), _T(G), _T(l) if l is not None else None)
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        rc = lib.dg_decoder_grad_f32(keep[0].data_ptr(), ldr, keep[1].data_ptr(), ldc, idx[0].data_ptr(),
                                     idx[1].data_ptr(), idx[2].data_ptr(), n, keep[2].data_ptr(), keep[3].data_ptr(),
                                     keep[4].data_ptr(), ptr(keep[5]), d, MARGIN, gr.data_ptr(), gc.data_ptr(),
                                     ptr(dG), ptr(dl), ptr(dgd), ws.data_ptr(), nbytes, _stream())
        assert rc == _lib.DG_OK
    else:
        op = K.PreparedDecoderGrad(_T(U), _T(V), *idx, _T(pos), _T(neg), _T(G), _T(l) if l is not None else None,
                                   MARGIN, dG=dG, dl=dl, dG_diag=dgd)
        op.grad_rows.fill_(float("nan"))
        op.grad_cols.fill_(float("nan"))
        op()
        gr, gc = op.grad_rows, op.grad_cols
    torch.cuda.synchronize()
    # the header's formulas, in float64
    U6, V6, G6 = U.astype(np.float64), V.astype(np.float64), G.astype(np.float64)
    l6 = l.astype(np.float64) if l is not None else np.ones(d)
    M = l6[:, None] * G6 * l6[None, :]
    mv = V6[cols] @ M.T
    x = act[:, None] * (U6[negs] - U6[rows])
    dM = x.T @ V6[cols]
    want = {"grad_rows[:n]": (gr[:n], -act[:, None] * mv), "grad_rows[n:]": (gr[n:], act[:, None] * mv),
            "grad_cols": (gc, x @ M)}
    if dG is not None:
        want["dG"] = (dG.view(d, d), l6[:, None] * dM * l6[None, :])
    if dl is not None:
        want["dl"] = (dl, (dM * G6) @ l6 + (dM * G6).T @ l6)
    if dgd is not None:
        want["dG_diag"] = (dgd, l6 * np.diag(dM) * l6)
    if kind == "exact":
        # |u|, |v|, |G|, |l| <= 2 and |un - u| <= 4.  M·v: d terms of |G·l·v| <= 8, times l: 16·d.  Mᵀ·x: d
        # terms of |G·l·x| <= 16, times l: 32·d.  dM: n terms of |x·v| <= 8; dG = l·dM·l <= 32·n.  dl: 2d
        # terms of |dM·G·l| <= 8n·4.  All far below 2^24 at d <= 256, n <= 65.
        assert 32 * d < 2 ** 24 and 32 * n < 2 ** 24 and 2 * d * 32 * n < 2 ** 24
    for name, (got, ref) in want.items():
        got = got.cpu().numpy()
        if kind == "exact" or pattern == "inactive":
            assert np.abs(ref).max() < 2 ** 24
            assert np.array_equal(got, ref), (name, d, n, dec, pattern)
        else:
            assert rel_err(got, ref) <= TOL, (name, d, n, dec, pattern, rel_err(got, ref))
    if pattern == "inactive":  # every requested output is exact zeros
        assert all(not got.cpu().numpy().any() for got, _ in want.values())


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("d,n", [(32, 1), (32, 63), (32, 64), (32, 65), (64, 65), (128, 65), (256, 65)])
def test_decoder_grad_shapes(K, kind, padded, d, n):
    """DEDICOM (dG, dl and dG_diag all requested) over d % 32 == 0 up to 256 — d >= 64 gives
    decoder_grad_dm_kernel more than one 32x32 tile — and n around the 64-pair chunk of the dM partials; the
    hinge pattern mixes active pairs, inactive ones and z == 0; padded: ld_row = d + 4, ld_col = d + 8
    through the C entry point."""
    _decoder_case(K, kind, 10 * d + n, d, n, "dedicom", "mixed", padded)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("pattern", ["mixed", "inactive", "active"])
@pytest.mark.parametrize("dec", ["dedicom", "distmult", "bilinear", "innerproduct"])
def test_decoder_grad_kinds_and_hinge_patterns(K, kind, pattern, dec):
    """All four decoder kinds at d = 64, n = 65, with a batch where every pair is inactive (z <= 0: every
    output is exact zeros) and one where every pair is active."""
    _decoder_case(K, kind, 77 + len(dec) + len(pattern), 64, 65, dec, pattern, False)


# ------------------------------------------------------------------------------ dg_scatter_rows_f32
N_OUT = 7
BAD = (-1, N_OUT, 2 ** 31 - 1)  # indices outside the table update nothing


def _scatter_indices(rng, n, case):
    """n indices into N_OUT rows.  'dense': every row many times, so one row's occurrences span 64-index
    chunks and (n > 1024) 1,024-index scan rounds.  'late': row 6 first appears in the second scan round
    (index 1030) and rows 4 and 5 are named by no index.  'bad': as dense, with out-of-range entries
    interleaved (every 5th index)."""
    if case == "late":
        idx = rng.integers(0, 4, n).astype(np.int32)
        idx[[p for p in (1030, 1100, 2100, n - 1) if p < n]] = 6
        return idx
    idx = rng.integers(0, N_OUT, n).astype(np.int32)
    if case == "bad":
        idx[::5] = np.resize(np.array(BAD, np.int64), len(idx[::5])).astype(np.int32)
    return idx


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("d", [1, 3, 32, 65, 200, 256])
def test_scatter_rows(K, kind, d):
    """out[idx[q]] += Σ src[q'] for d around the 64-column steps of the accumulators, n = 1, 64, 65 (one
    chunk and a second one), 1025 and 2500 (two and three scan rounds), through the wrapper (ld_out = d) and
    through the C entry point with ld_out = d + 4 (NaN padding kept)."""
    from decagon_amd import _lib

    lib = _lib.load()
    rng = np.random.default_rng(2000 + d)
    for n, case in ((1, "dense"), (64, "dense"), (65, "bad"), (1025, "dense"), (2500, "dense"), (2500, "late"),
                    (2500, "bad")):
        idx = _scatter_indices(rng, n, case)
        if kind == "exact":
            src = rng.integers(-8, 9, (n, d)).astype(np.float32)
            out0 = rng.integers(-8, 9, (N_OUT, d)).astype(np.float32)
        else:
            src = rng.standard_normal((n, d)).astype(np.float32)
            out0 = rng.standard_normal((N_OUT, d)).astype(np.float32)
        ok = (idx >= 0) & (idx < N_OUT)
        assert (case == "bad") == (not ok.all())
        ref = out0.astype(np.float64)
        np.add.at(ref, idx[ok], src[ok].astype(np.float64))
        mag = np.abs(out0).astype(np.float64)
        np.add.at(mag, idx[ok], np.abs(src[ok]).astype(np.float64))
        occ = np.bincount(idx[ok], minlength=N_OUT)
        if case == "late":
            assert occ[4] == occ[5] == 0 and occ[6] >= 3 and np.flatnonzero(idx == 6)[0] == 1030
        # the wrapper, and a padded output through the C entry point
        out_a = _T(out0.copy())
        K.scatter_rows(_T(idx), _T(src), out_a)
        wide = np.full((N_OUT, d + 4), np.nan, np.float32)
        wide[:, :d] = out0
        out_b = _T(wide)
        i_d, s_d = _T(idx), _T(src)
        assert lib.dg_scatter_rows_f32(i_d.data_ptr(), n, s_d.data_ptr(), d, out_b.data_ptr(), d + 4, N_OUT,
                                       _stream()) == _lib.DG_OK
        torch.cuda.synchronize()
        got_b = out_b.cpu().numpy()
        assert _same_bits(got_b[:, d:], wide[:, d:])
        for got in (out_a.cpu().numpy(), got_b[:, :d]):
            assert _same_bits(got[occ == 0], out0[occ == 0]), (n, case)  # rows no index names
            if kind == "exact":
                # 2,501 terms of magnitude <= 8
                assert mag.max() < 2 ** 24
                assert np.array_equal(got, ref), (n, case)
            else:
                # k sequential roundings of partial sums bounded by |out0| + Σ|src| (the occurrences are
                # summed first, then added to the row)
                bound = (occ[:, None] + 1) * 2.0 ** -24 * mag
                assert np.all(np.abs(got - ref) <= bound), (n, case, float((np.abs(got - ref) / bound).max()))


# ------------------------------------------------------------------------------ dg_l2norm_grad_f32
def _row_rel(got, want):
    """max|Δ| of each row over max|want| of that row (a row whose reference is all zero must be zero)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err = np.abs(got - want).max(axis=1)
    den = np.abs(want).max(axis=1)
    return np.where(den > 0, err / np.where(den > 0, den, 1.0), np.where(err > 0, np.inf, 0.0))


def _differs_from_group0(got, want, g, n_rows):
    """Wherever group g's reference row differs from group 0's, so does the kernel's: a kernel that read group
    0's S for every group would repeat group 0's result.  (An all-zero row and a row below ε have the same
    gradient, dy'·1e6, so not every row differs.)"""
    if g == 0:
        return
    rows = np.any(want[g] != want[0], axis=1)
    assert n_rows < 5 or rows.any()
    assert np.all(np.any(got[g] != got[0], axis=1)[rows]), g


@pytest.mark.parametrize("n_groups", [1, 3, 8])
@pytest.mark.parametrize("d", [4, 12, 32, 100, 128, 256])  # lanes per row 1, 4, 8, 32, 32, 64
def test_l2norm_grad_gauss(K, n_groups, d):
    """ds_g for several groups with their own S, rows of four kinds — all zero, Σs² ≈ 0.5e-12 and ≈ 2e-12
    (either side of the ε switch; the factor 2 keeps fp32 and float64 on the same side), ordinary — compared
    row by row: the near-ε rows are 10^6 times larger and must not hide the ordinary ones."""
    rng = np.random.default_rng(3000 + 10 * d + n_groups)
    for n_rows in (1, 5, 90):
        for use_mask in (True, False):
            dy = rng.standard_normal((n_rows, d)).astype(np.float32)
            mask = rng.standard_normal((n_rows, d)).astype(np.float32) if use_mask else None
            S = rng.standard_normal((n_groups, n_rows, d)).astype(np.float32)
            for g in range(n_groups):
                for r in range(n_rows):
                    kind = (r + g) % 4
                    if kind == 0:
                        S[g, r] = 0.0
                    elif kind in (1, 2):
                        ss = float(np.sum(S[g, r].astype(np.float64) ** 2))
                        S[g, r] *= np.float32(np.sqrt((0.5e-12 if kind == 1 else 2e-12) / ss))
            ss64 = np.sum(S.astype(np.float64) ** 2, axis=2)
            ss32 = np.sum(S * S, axis=2, dtype=np.float32)
            assert np.array_equal(ss32 >= np.float32(1e-12), ss64 >= 1e-12)
            assert np.all((ss64 == 0) | (np.abs(ss64 / 1e-12 - 1) > 0.4))
            ds = [_nan(n_rows, d) for _ in range(n_groups)]
            K.PreparedL2Grad([(_T(S[g]), ds[g]) for g in range(n_groups)], _T(dy), _T(mask) if use_mask else None,
                             n_rows, d)()
            torch.cuda.synchronize()
            dym = (dy * (mask > 0) if use_mask else dy).astype(np.float64)
            got = [x.cpu().numpy() for x in ds]
            want = [orc.l2_normalize_rows_grad(S[g].astype(np.float64), dym) for g in range(n_groups)]
            for g in range(n_groups):
                rr = _row_rel(got[g], want[g])
                assert float(rr.max()) <= TOL, (n_rows, use_mask, g, int(rr.argmax()), float(rr.max()))
                _differs_from_group0(got, want, g, n_rows)


@pytest.mark.parametrize("n_groups", [1, 3, 8])
@pytest.mark.parametrize("d", [4, 12, 32, 100, 128, 256])
def test_l2norm_grad_exact(K, n_groups, d):
    """Rows with c ∈ {1, 4, 16, 64} non-zero entries of magnitude 2^j: Σs² = c·4^j is a power of 4, so inv and
    inv³ are powers of two, s·dy is a small integer and every step of ds = dy·inv − s·inv³·(s·dy) is exact
    in fp32: equality with the float64 formula."""
    rng = np.random.default_rng(3500 + 10 * d + n_groups)
    for n_rows in (1, 5, 90):
        for use_mask in (True, False):
            dy = rng.integers(-4, 5, (n_rows, d)).astype(np.float32)
            mask = rng.integers(-1, 2, (n_rows, d)).astype(np.float32) if use_mask else None
            S = np.zeros((n_groups, n_rows, d), np.float32)
            for g in range(n_groups):
                for r in range(n_rows):
                    c = [c for c in (1, 4, 16, 64) if c <= d][(r + g) % len([c for c in (1, 4, 16, 64) if c <= d])]
                    where = rng.choice(d, c, replace=False)
                    S[g, r, where] = rng.choice([-1.0, 1.0], c) * 2.0 ** ((r + 2 * g) % 3)
            ds = [_nan(n_rows, d) for _ in range(n_groups)]
            K.PreparedL2Grad([(_T(S[g]), ds[g]) for g in range(n_groups)], _T(dy), _T(mask) if use_mask else None,
                             n_rows, d)()
            torch.cuda.synchronize()
            dym = (dy * (mask > 0) if use_mask else dy).astype(np.float64)
            got = [x.cpu().numpy() for x in ds]
            want = [orc.l2_normalize_rows_grad(S[g].astype(np.float64), dym) for g in range(n_groups)]
            for g in range(n_groups):
                # with c entries of magnitude a: |dy·inv| <= 4 and |s·inv³·(s·dy)| <= a·(c·a·4)/(c·a²)^1.5 <= 4,
                # both on a grid no finer than 2^-15: at most 19 significant bits
                assert np.abs(want[g]).max() <= 8 and np.array_equal(want[g] * 2 ** 15, np.round(want[g] * 2 ** 15))
                assert np.array_equal(got[g], want[g]), (n_rows, use_mask, g)
                _differs_from_group0(got, want, g, n_rows)


# ------------------------------------------------------------------------------ dg_adam_f32
ADAM_SIZES = [4, 4096, 4098, 4100, 8191, 8192 + 1024 * 4 + 3]  # float4 counts around the 1,024 of a block


def _adam_segments(rng, full):
    """(size, has_grad) per segment: the sizes above — or DG_MAX_ADAM_SEGS segments, empty ones and
    grad=None ones among them."""
    from decagon_amd import _lib

    if not full:
        return [(n, True) for n in ADAM_SIZES]
    sizes = (ADAM_SIZES + [0, 1, 2, 3, 5, 7, 0, 1023, 1024, 4095, 4097, 0] + [int(x) for x in rng.integers(1, 3000, 32)])
    sizes = sizes[:_lib.DG_MAX_ADAM_SEGS]
    return [(n, i % 4 != 1) for i, n in enumerate(sizes)]


@pytest.mark.parametrize("full", [False, True])
def test_adam_segments_three_steps(K, full):
    """p, m and v of every segment against the float32 TF restatement over three steps: segments whose float4
    count is a multiple of a block's 1,024 with and without a tail, and a launch of DG_MAX_ADAM_SEGS segments
    with empty and gradient-less ones."""
    from decagon_amd import _lib, train

    rng = np.random.default_rng(4000 + full)
    segs = _adam_segments(rng, full)
    assert not full or (len(segs) == _lib.DG_MAX_ADAM_SEGS and sum(n == 0 for n, _ in segs) >= 3
                        and sum(not hg for _, hg in segs) >= 3)
    p = [rng.standard_normal(n).astype(np.float32) for n, _ in segs]
    g = [rng.standard_normal(n).astype(np.float32) for n, _ in segs]
    dp = [_T(x.copy()) for x in p]
    st = train.AdamState(dp, lr=0.01)
    grads = [_T(x) if hg else None for x, (_, hg) in zip(g, segs)]
    op = st.prepared(grads)
    assert len(op._arrs) == 1  # one launch
    m = [np.zeros(n, np.float32) for n, _ in segs]
    v = [np.zeros(n, np.float32) for n, _ in segs]
    for t in (1, 2, 3):
        st.apply(op)
        for i, (_, hg) in enumerate(segs):
            p[i], m[i], v[i] = orc.adam_tf(p[i], g[i] if hg else np.zeros_like(g[i]), m[i], v[i], t, lr=0.01)
    torch.cuda.synchronize()
    for i, (n, hg) in enumerate(segs):
        if n == 0:
            continue
        assert np.max(np.abs(dp[i].cpu().numpy() - p[i])) <= 1e-6, (i, n, hg)
        assert np.max(np.abs(st.m[i].cpu().numpy() - m[i])) <= 1e-6, (i, n, hg)
        assert np.max(np.abs(st.v[i].cpu().numpy() - v[i])) <= 1e-6, (i, n, hg)


def test_adam_exact(K):
    """One step from m = v = 0 with β1 = 0.5, β2 = 0.75, ε = 1, alpha = 0.5 and g ∈ {±2, ±6, ±14} (or none):
    m = g/2, v = g²/4, sqrt(v) + ε ∈ {1, 2, 4, 8} and p − (g/4)/(sqrt(v) + ε) are all dyadic: every element of
    every segment — block tails and the n % 4 tail included — is an equality."""
    rng = np.random.default_rng(4100)
    segs = [(n, i != 2) for i, n in enumerate(ADAM_SIZES + [1, 3, 1024 * 4])]
    p = [rng.integers(-8, 9, n).astype(np.float32) for n, _ in segs]
    g = [(rng.choice([2.0, 6.0, 14.0], n) * rng.choice([-1.0, 1.0], n)).astype(np.float32) for n, _ in segs]
    dp = [_T(x.copy()) for x in p]
    dm = [torch.zeros(n, device="cuda") for n, _ in segs]
    dv = [torch.zeros(n, device="cuda") for n, _ in segs]
    K.PreparedAdam([(dp[i], _T(g[i]) if hg else None, dm[i], dv[i]) for i, (_, hg) in enumerate(segs)])(
        0.5, 0.5, 0.75, 1.0)
    torch.cuda.synchronize()
    for i, (n, hg) in enumerate(segs):
        g6 = g[i].astype(np.float64) if hg else np.zeros(n)
        m6, v6 = g6 * 0.5, g6 * g6 * 0.25
        p6 = p[i] - (m6 * 0.5) / (np.sqrt(v6) + 1.0)
        assert np.array_equal(p6 * 32, np.round(p6 * 32))  # on a 2^-5 grid, |p| < 16
        assert np.array_equal(dm[i].cpu().numpy(), m6), (i, n)
        assert np.array_equal(dv[i].cpu().numpy(), v6), (i, n)
        assert np.array_equal(dp[i].cpu().numpy(), p6), (i, n)

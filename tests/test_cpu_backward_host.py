"""CPU: the host side of the GEMM family (gemm.hip) and the training-step kernels (train.hip) —
every argument rejection that returns before a launch, so it runs without a device, and the
decoder gradient's workspace formula.  The pointers are fakes: no call below reaches a kernel."""
import ctypes

import pytest

P = 4096  # a non-null, 16-byte aligned fake device pointer (never dereferenced)


@pytest.fixture(scope="module")
def L():
    from decagon_amd import _lib

    return _lib, _lib.load()


def _tn(lib, **over):
    """dg_gemm_tn_f32 with arguments that would be valid, except for `over`."""
    a = dict(a=P, lda=64, a_bs=0, b=P, ldb=32, b_bs=100 * 32, c=P, rows=100, M=64, N=32, batch=3, n_split=1,
             partial=None, stream=None)
    assert set(over) <= set(a), over
    a.update(over)
    return lib.dg_gemm_tn_f32(*a.values())


def test_gemm_tn_rejections(L):
    _lib, lib = L
    EINVAL, EALIGN = _lib.DG_EINVAL, _lib.DG_EALIGN
    # M or N not a multiple of 32 (or below one tile)
    for M, N in ((48, 32), (32, 40), (0, 32), (32, 0), (33, 32), (64, 31)):
        assert _tn(lib, M=M, N=N, lda=256, ldb=256) == EINVAL, (M, N)
    # more than four 32x32 tiles: 5x1, 1x5, 3x2, 2x3, 4x2
    for M, N in ((160, 32), (32, 160), (96, 64), (64, 96), (128, 64)):
        assert _tn(lib, M=M, N=N, lda=256, ldb=256) == EINVAL, (M, N)
    # leading dimensions below the row length
    assert _tn(lib, lda=63) == EINVAL
    assert _tn(lib, ldb=31) == EINVAL
    # sizes
    assert _tn(lib, rows=-1) == EINVAL
    assert _tn(lib, batch=-1) == EINVAL
    for ns in (0, -1):
        assert _tn(lib, n_split=ns, partial=P) == EINVAL, ns
    # the split partials: required, and 16-byte aligned
    assert _tn(lib, n_split=2, partial=None) == EINVAL
    assert _tn(lib, n_split=2, partial=P + 4) == EALIGN
    assert _tn(lib, n_split=2, partial=P + 8) == EALIGN
    # null operands
    for nm in ("a", "b", "c"):
        assert _tn(lib, **{nm: None}) == EINVAL, nm
    # an empty batch is no work — even before the pointers are looked at
    assert _tn(lib, batch=0) == _lib.DG_OK
    assert _tn(lib, batch=0, a=None, b=None, c=None) == _lib.DG_OK
    # ... but not before the shape is: a bad tile shape is refused at batch 0 too
    assert _tn(lib, batch=0, M=96, N=64, lda=256, ldb=256) == EINVAL


def _desc(_lib, **over):
    d = _lib.DgGemmDesc()
    a = dict(a=P, b=P, c=P, sa=None, sc=None, b_map=None, a_bs=0, a_sm=64, a_sk=1, b_bs=64 * 32, b_sk=32, b_sn=1,
             c_bs=100 * 32, c_sm=32, c_sn=1, m=100, n=32, k=64, batch=3, reduce=0, drop_tag=0, drop_state=None,
             drop_keep=0.0)
    assert set(over) <= set(a), over
    a.update(over)
    for k, v in a.items():
        setattr(d, k, v)
    return d


def _gemm(_lib, lib, *descs):
    arr = (_lib.DgGemmDesc * len(descs))(*descs)
    return lib.dg_gemm_f32(arr, len(descs), None)


def test_gemm_rejections(L):
    _lib, lib = L
    EINVAL = _lib.DG_EINVAL
    for nm in ("m", "n", "k", "batch"):
        assert _gemm(_lib, lib, _desc(_lib, **{nm: -1})) == EINVAL, nm
    assert _gemm(_lib, lib, _desc(_lib, reduce=-1)) == EINVAL
    # null operands (a and b only matter when k > 0, c always)
    for nm in ("a", "b", "c"):
        assert _gemm(_lib, lib, _desc(_lib, **{nm: None})) == EINVAL, nm
    # a dropout descriptor belongs to batch-reduce mode, with keep in (0, 1]
    assert _gemm(_lib, lib, _desc(_lib, drop_state=P, drop_keep=0.5, reduce=0)) == EINVAL
    for keep in (0.0, -0.25, 1.5, float("nan"), float("inf")):
        assert _gemm(_lib, lib, _desc(_lib, drop_state=P, drop_keep=keep, reduce=4)) == EINVAL, keep
    # unmapped mask indices are 32-bit
    assert _gemm(_lib, lib, _desc(_lib, drop_state=P, drop_keep=0.5, reduce=4, m=1 << 16, n=1 << 15,
                                  batch=2)) == EINVAL
    # a bad descriptor behind a good empty one is still seen
    assert _gemm(_lib, lib, _desc(_lib, batch=0), _desc(_lib, m=-1)) == EINVAL
    # descriptor count
    assert lib.dg_gemm_f32(None, 1, None) == EINVAL
    one = _desc(_lib, batch=0)
    assert lib.dg_gemm_f32(ctypes.byref(one), 0, None) == EINVAL
    many = [_desc(_lib, batch=0) for _ in range(_lib.DG_MAX_GROUPS + 1)]
    assert _gemm(_lib, lib, *many) == _lib.DG_ETOOMANY
    # nothing but empty descriptors: no launch
    assert _gemm(_lib, lib, *many[:_lib.DG_MAX_GROUPS]) == _lib.DG_OK
    assert _gemm(_lib, lib, _desc(_lib, m=0), _desc(_lib, n=0, c=None)) == _lib.DG_OK


def _dgrad(lib, **over):
    a = dict(row_table=P, ld_row=64, col_table=P, ld_col=64, rows=P, cols=P, neg_rows=P, n=100, pos=P, neg=P,
             G=P, l=P, d=64, margin=0.1, grad_rows=P, grad_cols=P, dG=P, dl=P, dG_diag=P, ws=P, ws_bytes=1 << 40,
             stream=None)
    assert set(over) <= set(a), over
    a.update(over)
    return lib.dg_decoder_grad_f32(*a.values())


def test_decoder_grad_rejections_and_workspace(L):
    _lib, lib = L
    EINVAL = _lib.DG_EINVAL
    for d in (0, 16, 48, 288, -32):
        assert _dgrad(lib, d=d, ld_row=512, ld_col=512) == EINVAL, d
    assert _dgrad(lib, n=-1) == EINVAL
    assert _dgrad(lib, ld_row=63) == EINVAL
    assert _dgrad(lib, ld_col=60) == EINVAL
    assert _dgrad(lib, l=None) == EINVAL  # dl without l
    for nm in ("row_table", "col_table", "rows", "cols", "neg_rows", "pos", "neg", "G", "grad_rows", "grad_cols",
               "ws"):
        assert _dgrad(lib, **{nm: None}) == EINVAL, nm
    need = lib.dg_decoder_grad_workspace(100, 64)
    assert _dgrad(lib, ws_bytes=need - 1) == EINVAL
    assert _dgrad(lib, ws_bytes=0) == EINVAL
    assert _dgrad(lib, ws=P + 8) in (EINVAL, _lib.DG_EALIGN)
    assert _dgrad(lib, ws=P + 4) in (EINVAL, _lib.DG_EALIGN)
    # an empty batch is no work
    assert _dgrad(lib, n=0) == _lib.DG_OK
    assert _dgrad(lib, n=0, ws=None, ws_bytes=0) == _lib.DG_OK
    # xw and vw ([n][d] each), one d×d partial per chunk of 64 pairs, and dM
    for n in (1, 63, 64, 65, 300, 4096):
        for d in (32, 64, 128, 256):
            assert lib.dg_decoder_grad_workspace(n, d) == 4 * (2 * n * d + -(-n // 64) * d * d + d * d), (n, d)
    assert lib.dg_decoder_grad_workspace(0, 64) == 0
    assert lib.dg_decoder_grad_workspace(10, 0) == 0


def test_scatter_rows_rejections(L):
    _lib, lib = L
    EINVAL = _lib.DG_EINVAL

    def call(idx=P, n=10, src=P, d=32, out=P, ld_out=32, n_out=5):
        return lib.dg_scatter_rows_f32(idx, n, src, d, out, ld_out, n_out, None)

    for d in (0, -1, 257):
        assert call(d=d, ld_out=512) == EINVAL, d
    assert call(ld_out=31) == EINVAL
    assert call(n=-1) == EINVAL
    assert call(n_out=-1) == EINVAL
    for nm in ("idx", "src", "out"):
        assert call(**{nm: None}) == EINVAL, nm
    assert call(n=0) == _lib.DG_OK
    assert call(n=0, idx=None, src=None, out=None) == _lib.DG_OK


def test_l2norm_grad_rejections(L):
    _lib, lib = L
    EINVAL, EALIGN = _lib.DG_EINVAL, _lib.DG_EALIGN

    def call(n_groups=2, s=P, ds=P, dy=P, mask=P, n_rows=10, d=32, bad_group=0):
        arr = (_lib.DgL2gGroup * max(1, n_groups))()
        for g in arr:
            g.s, g.ds = P, P
        arr[bad_group].s, arr[bad_group].ds = s, ds
        return lib.dg_l2norm_grad_f32(arr, n_groups, dy, mask, n_rows, d, None)

    for d in (0, 2, 6, 260, 258, -4):
        assert call(d=d) == EINVAL, d
    assert call(n_rows=-1) == EINVAL
    assert call(n_groups=0) == EINVAL
    assert lib.dg_l2norm_grad_f32(None, 1, P, P, 10, 32, None) == EINVAL
    assert call(n_groups=_lib.DG_MAX_GROUPS + 1) == _lib.DG_ETOOMANY
    assert call(dy=None) == EINVAL
    assert call(s=None) == EINVAL
    assert call(ds=None, bad_group=1) == EINVAL
    # every row is read and written as float4s
    for off in (4, 8, 12):
        assert call(dy=P + off) == EALIGN, off
        assert call(mask=P + off) == EALIGN, off
        assert call(s=P + off) == EALIGN, off
        assert call(ds=P + off) == EALIGN, off
        assert call(s=P + off, bad_group=1) == EALIGN, off
        assert call(n_groups=_lib.DG_MAX_GROUPS, ds=P + off, bad_group=_lib.DG_MAX_GROUPS - 1) == EALIGN, off
    assert call(n_rows=0) == _lib.DG_OK


def test_adam_rejections(L):
    _lib, lib = L
    EINVAL, EALIGN = _lib.DG_EINVAL, _lib.DG_EALIGN

    def call(n_segs=2, bad=0, **over):
        arr = (_lib.DgAdamSeg * max(1, n_segs))()
        for s in arr:
            s.param, s.grad, s.m, s.v, s.n = P, P, P, P, 0  # n = 0: skipped, so nothing launches
        for k, v in over.items():
            setattr(arr[bad], k, v)
        return lib.dg_adam_f32(arr, n_segs, 0.001, 0.9, 0.999, 1e-8, None, None)

    assert call() == _lib.DG_OK  # only empty segments
    assert call(n_segs=0) == _lib.DG_OK
    assert call(n_segs=_lib.DG_MAX_ADAM_SEGS) == _lib.DG_OK
    assert call(n_segs=_lib.DG_MAX_ADAM_SEGS + 1) == _lib.DG_ETOOMANY
    assert call(n_segs=-1) == EINVAL
    assert lib.dg_adam_f32(None, 1, 0.001, 0.9, 0.999, 1e-8, None, None) == EINVAL
    assert call(n=-1) == EINVAL
    assert call(n=-1, bad=1) == EINVAL
    for nm in ("param", "m", "v"):
        assert call(n=8, **{nm: None}) == EINVAL, nm
    for nm in ("param", "grad", "m", "v"):
        for off in (4, 8):
            assert call(n=8, **{nm: P + off}) == EALIGN, (nm, off)
            assert call(n=8, bad=1, **{nm: P + off}) == EALIGN, (nm, off)

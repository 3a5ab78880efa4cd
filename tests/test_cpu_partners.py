"""CPU: the host side of a node's best partners (dg_decoder_node_topk_f32 and its workspace size,
declared in include/decagon_hip_ext2.h; additive to ABI 39) — the second extension header's parse,
export and binding, every argument rejection (they run before any HIP call, so they work without
a device), evaluate.pack_node_queries and the Python wrappers' validation."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

P = 4096  # a non-null, 16-byte aligned fake device pointer (never dereferenced: every call below is rejected)
NAME = "dg_decoder_node_topk_f32"
WS = "dg_decoder_node_topk_workspace"
# 500 queries in 3 segments against 8,000 columns at topk 10: 18 query tiles of 250 column tiles,
# so the columns are dealt over waves and splits and the workspace is not empty
SHAPE = dict(n_queries=500, n_seg=3, n_cols=8000, topk=10)


def _call(lib, **over):
    """dg_decoder_node_topk_f32 with arguments that would be valid, except for `over`."""
    from decagon_amd import _lib

    a = dict(row_table=P, ld_row=32, n_rows=100, col_table=P, ld_col=32, row_idx=P, seg_ptr=P, seg_rel=None,
             G=P, g_stride=0, l=P, l_stride=32, n_rel=3, d=32, excl_rowptr=P, excl_col=P, flags=0, out_score=P,
             out_col=P, out_count=P, workspace=P, workspace_bytes=None, stream=None, **SHAPE)
    assert set(over) <= set(a), over
    a.update(over)
    if a["workspace_bytes"] is None:
        a["workspace_bytes"] = int(getattr(lib, WS)(a["n_queries"], a["n_seg"], a["n_cols"], a["topk"]))
    return getattr(lib, NAME)(*_lib.pack(NAME, **a))


def test_second_extension_header_parses_into_its_own_table():
    from decagon_amd import _lib, abi

    assert list(abi.EXT2.prototypes) == [WS, NAME] and not abi.EXT2.structs
    assert abi.EXT2.constants == {"DG_NODE_TOPK_MAX_K": 128, "DG_NODE_TOPK_NO_SELF": 1, "DG_NODE_TOPK_NO_SPLIT": 2}
    # the earlier tables are what they were
    assert list(abi.EXT.prototypes) == ["dg_decoder_edge_rank_f32"] and not abi.EXT.structs
    assert abi.EXT.constants == {"DG_EDGE_RANK_NO_SELF": 1, "DG_EDGE_RANK_NO_SPLIT": 2}
    assert len(abi.PROTOTYPES) == 78 and len(abi.ABI.structs) == 15
    assert not {NAME, WS} & (set(abi.PROTOTYPES) | set(abi.EXT.prototypes))
    assert not set(abi.EXT2.constants) & (set(abi.CONSTANTS) | set(abi.EXT.constants))
    assert abi.EXTENSIONS == [abi.EXT, abi.EXT2]
    assert set(abi.ALL_PROTOTYPES) == set(abi.PROTOTYPES) | set(abi.EXT.prototypes) | set(abi.EXT2.prototypes)
    assert len(abi.ALL_PROTOTYPES) == 81
    p = abi.EXT2.prototypes[NAME]
    assert p.restype is ctypes.c_int32 and len(p.argtypes) == len(p.names) == 27
    assert p.names[:3] == ("row_table", "ld_row", "n_rows")
    assert p.names[-6:] == ("out_score", "out_col", "out_count", "workspace", "workspace_bytes", "stream")
    assert "col_idx" not in p.names
    by_name = dict(zip(p.names, p.argtypes))
    assert by_name["ld_row"] is by_name["g_stride"] is by_name["workspace_bytes"] is ctypes.c_int64
    assert by_name["n_queries"] is by_name["flags"] is by_name["topk"] is ctypes.c_int32
    assert all(by_name[n] is ctypes.c_void_p for n in ("row_table", "seg_ptr", "excl_col", "out_col", "workspace", "stream"))
    w = abi.EXT2.prototypes[WS]
    assert w.restype is ctypes.c_int64 and w.argtypes == [ctypes.c_int32] * 4
    assert w.names == ("n_queries", "n_seg", "n_cols", "topk")
    assert _lib.DG_NODE_TOPK_MAX_K == 128 and _lib.DG_NODE_TOPK_NO_SPLIT == 2 and _lib.DG_EDGE_RANK_NO_SELF == 1
    assert _lib.arg_index(NAME, "topk") == 17 and _lib.arg_index("dg_decoder_edge_rank_f32", "flags") == 20
    # both earlier headers' names are in scope of the third parse
    text = "#ifndef DECAGON_HIP_EXT2_H\n#define DECAGON_HIP_EXT2_H\n" \
           "#define DG_X (DG_MAX_GROUPS + DG_EDGE_RANK_NO_SPLIT)\n#endif\n"
    scope = abi.Abi({**abi.CONSTANTS, **abi.EXT.constants}, dict(abi.ABI.structs), {})
    assert abi.parse(text, "x.h", base=scope).constants == {"DG_X": 10}
    with pytest.raises(abi.AbiError, match="DG_EDGE_RANK_NO_SPLIT"):
        abi.parse(text, "x.h", base=abi.ABI)


def test_symbols_exported_bound_and_typed():
    from decagon_amd import _lib, abi

    lib = _lib.load()
    for nm in (WS, NAME):
        assert hasattr(lib, nm) and nm in _lib.SIGNATURES
        p = abi.EXT2.prototypes[nm]
        fn = getattr(lib, nm)
        assert fn.restype is p.restype and list(fn.argtypes) == p.argtypes
        assert _lib.SIGNATURES[nm] == (p.restype, p.argtypes)
    assert all(s in _lib.SIGNATURES for s in abi.PROTOTYPES) and "dg_decoder_edge_rank_f32" in _lib.SIGNATURES
    assert lib.dg_abi_version() == _lib.ABI_VERSION == 39


def test_workspace_size():
    from decagon_amd import _lib

    ws = getattr(_lib.load(), WS)
    need = ws(*SHAPE.values())
    assert need > 0 and need % (500 * 10 * 8) == 0 and need // (500 * 10 * 8) > 1  # whole lists of every query
    assert ws(500, 3, 8000, 20) == 2 * need
    # few column tiles, or query tiles enough to fill the device: one list per query, written in place
    assert ws(500, 3, 80, 10) == 0 and ws(645 * 1928, 1928, 645, 10) == 0
    for bad in ((0, 3, 80, 10), (500, 0, 80, 10), (500, 3, 0, 10), (500, 3, 80, 0), (500, 3, 80, 129)):
        assert ws(*bad) == 0, bad


def test_rejections_without_a_device():
    from decagon_amd import _lib

    lib = _lib.load()
    EINVAL, EALIGN = _lib.DG_EINVAL, _lib.DG_EALIGN
    need = int(getattr(lib, WS)(*SHAPE.values()))
    for nm in ("row_table", "col_table", "row_idx", "seg_ptr", "G", "out_score", "out_col", "out_count", "workspace"):
        assert _call(lib, **{nm: None}) == EINVAL, nm
    assert _call(lib, excl_rowptr=None) == EINVAL and _call(lib, excl_col=None) == EINVAL  # one alone
    for n_seg in (0, -1):
        assert _call(lib, n_seg=n_seg) == EINVAL, n_seg
    assert _call(lib, n_queries=-1) == EINVAL
    for d in (0, -32, 16, 48, 96, 128):
        assert _call(lib, d=d, ld_row=512, ld_col=512, l_stride=d) == EINVAL, d
    assert _call(lib, ld_row=28) == EINVAL and _call(lib, ld_col=31) == EINVAL
    assert _call(lib, n_rows=0) == EINVAL and _call(lib, n_cols=0) == EINVAL
    # strides: 0 or d·d for G, 0 or d for l
    for over in (dict(g_stride=32), dict(g_stride=-1024), dict(l_stride=16), dict(l_stride=1024)):
        assert _call(lib, **over) == EINVAL, over
    # a relation map needs a relation count; without a map per-relation operands and the exclusion bound n_seg
    assert _call(lib, seg_rel=P, n_rel=0) == EINVAL and _call(lib, seg_rel=P, n_rel=-3) == EINVAL
    assert _call(lib, n_seg=4, n_rel=3) == EINVAL
    assert _call(lib, n_seg=4, n_rel=3, g_stride=1024, l=None) == EINVAL
    assert _call(lib, n_seg=4, n_rel=3, l_stride=0) == EINVAL  # (the exclusion is per relation)
    # topk
    for topk in (0, -1, 129, 2**20):
        assert _call(lib, topk=topk, workspace_bytes=2**40) == EINVAL, topk
    # the workspace: one byte short, absent bytes, misaligned
    assert _call(lib, workspace_bytes=need - 1) == EINVAL and _call(lib, workspace_bytes=0) == EINVAL
    assert _call(lib, workspace_bytes=-1) == EINVAL
    assert _call(lib, workspace=P + 8) == EALIGN
    # flags
    assert _call(lib, flags=4) == EINVAL and _call(lib, flags=-1) == EINVAL
    assert _call(lib, flags=_lib.DG_NODE_TOPK_NO_SELF) == EINVAL  # 100 x 8000 tables
    assert _call(lib, flags=_lib.DG_NODE_TOPK_NO_SELF, n_cols=80, workspace_bytes=2**40) == EINVAL  # 100 x 80
    # 32-bit query offsets
    assert _call(lib, n_queries=2**31 - 1, n_seg=1, workspace_bytes=2**60) == EINVAL
    assert _call(lib, n_queries=2**31 - 96, n_seg=3, workspace_bytes=2**60) == EINVAL
    assert _call(lib, n_queries=0, n_seg=2**26, l_stride=0, seg_rel=P) == EINVAL
    # alignment: 16-byte tables, ld % 4 == 0
    assert _call(lib, row_table=P + 4) == EALIGN and _call(lib, col_table=P + 8) == EALIGN
    assert _call(lib, ld_row=34) == EALIGN and _call(lib, ld_col=33) == EALIGN
    # nothing to list is not an error (and launches nothing: no device here)
    nothing = dict(n_queries=0, row_idx=None, out_score=None, out_col=None, out_count=None, workspace=None,
                   workspace_bytes=0)
    assert _call(lib, **nothing) == _lib.DG_OK
    assert _call(lib, excl_rowptr=None, excl_col=None, n_seg=4, l_stride=0, **nothing) == _lib.DG_OK
    assert _call(lib, n_rows=8000, flags=_lib.DG_NODE_TOPK_NO_SELF | _lib.DG_NODE_TOPK_NO_SPLIT, **nothing) == _lib.DG_OK
    assert _call(lib, topk=128, **nothing) == _lib.DG_OK and _call(lib, topk=129, **nothing) == EINVAL


def test_pack_node_queries():
    from decagon_amd.evaluate import pack_node_queries

    idx, ptr, rels = pack_node_queries(np.array([5, 0, 9, 5]), 3, 10)
    assert idx.dtype == ptr.dtype == rels.dtype == np.int32
    assert idx.tolist() == [5, 0, 9, 5] * 3 and ptr.tolist() == [0, 4, 8, 12] and rels.tolist() == [0, 1, 2]
    idx, ptr, rels = pack_node_queries([7, 1], 4, 10, relations=[3, 0])
    assert idx.tolist() == [7, 1, 7, 1] and ptr.tolist() == [0, 2, 4] and rels.tolist() == [3, 0]
    # a mapping: relations out of order, one empty, one missing, one None; a key that is not listed is refused
    per = {2: [4, 4, 1], 0: np.array([9], np.int64), 1: [], 4: None, 5: [3]}
    with pytest.raises(ValueError, match=r"relations \[5\], which are not among those listed"):
        pack_node_queries(per, 6, 10, relations=[2, 1, 0, 3, 4, 2])
    idx, ptr, rels = pack_node_queries({r: v for r, v in per.items() if r != 5}, 6, 10, relations=[2, 1, 0, 3, 4, 2])
    assert rels.tolist() == [2, 1, 0, 3, 4, 2] and ptr.tolist() == [0, 3, 3, 4, 4, 4, 7]
    assert idx.tolist() == [4, 4, 1, 9, 4, 4, 1]
    idx, ptr, rels = pack_node_queries(per, 6, 10)
    assert rels.tolist() == list(range(6)) and ptr.tolist() == [0, 1, 1, 4, 4, 4, 5] and idx.tolist() == [9, 4, 4, 1, 3]
    idx, ptr, rels = pack_node_queries(np.zeros(0, np.int64), 2, 10)
    assert idx.size == 0 and ptr.tolist() == [0, 0, 0]
    with pytest.raises(ValueError, match="outside the embedding table"):
        pack_node_queries([0, 10], 3, 10)
    with pytest.raises(ValueError, match="outside the embedding table"):
        pack_node_queries({1: [-1]}, 3, 10)
    with pytest.raises(ValueError, match=r"relation outside \[0, 3\)"):
        pack_node_queries([0], 3, 10, relations=[0, 3])
    with pytest.raises(ValueError, match=r"relation outside \[0, 3\)"):
        pack_node_queries({3: [0]}, 3, 10)
    with pytest.raises(ValueError, match="no relations"):
        pack_node_queries([0], 3, 10, relations=[])
    with pytest.raises(ValueError, match="1-D integer"):
        pack_node_queries(np.zeros((2, 2), np.int64), 3, 10)
    with pytest.raises(ValueError, match="1-D integer"):
        pack_node_queries([0.5], 3, 10)


def test_wrappers_validate_before_touching_the_library(monkeypatch):
    from decagon_amd import _lib, evaluate, kernels
    from decagon_amd.sparse import exclusion_csr

    def no_library(*a, **k):
        raise AssertionError("the library was loaded before the arguments were checked")

    monkeypatch.setattr(_lib, "load", no_library)
    E = torch.zeros(10, 32)
    G = torch.zeros(32, 32)
    l = torch.zeros(3, 32)
    idx = torch.zeros(8, dtype=torch.int32)
    ptr = torch.tensor([0, 3, 3, 8], dtype=torch.int32)
    f = kernels.decoder_node_topk
    with pytest.raises(TypeError, match="dtype"):
        f(E.double(), E, idx, ptr, G, l, 5)
    with pytest.raises(TypeError, match="dtype"):
        f(E, E, idx.long(), ptr, G, l, 5)
    with pytest.raises(TypeError, match="dtype"):
        f(E, E, idx, ptr, G, l, 5, seg_rel=torch.zeros(3))
    with pytest.raises(TypeError, match="torch.Tensor"):
        f(E, E, idx, ptr.numpy(), G, l, 5)
    with pytest.raises(ValueError, match="contiguous"):
        f(torch.zeros(10, 64)[:, ::2], E, idx, ptr, G, l, 5)
    with pytest.raises(ValueError, match="d mismatch"):
        f(torch.zeros(10, 64), E, idx, ptr, G, l, 5)
    with pytest.raises(ValueError, match="unsupported"):  # the register-resident tiles: 32 or 64
        f(torch.zeros(10, 96), torch.zeros(10, 96), idx, ptr, torch.zeros(96, 96), None, 5)
    for topk in (0, 129, -3):
        with pytest.raises(ValueError, match=r"topk must be in \[1, 128\]"):
            f(E, E, idx, ptr, G, l, topk)
    with pytest.raises(ValueError, match="seg_ptr"):
        f(E, E, idx, ptr[:1], G, l, 5)
    with pytest.raises(ValueError, match="seg_rel"):
        f(E, E, idx, ptr, G, l, 5, seg_rel=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError, match="disagree"):
        f(E, E, idx, ptr, torch.zeros(2, 32, 32), l, 5)
    with pytest.raises(ValueError, match="pass seg_rel"):
        f(E, E, idx, ptr, G, l[:2], 5)
    with pytest.raises(ValueError, match="square"):
        f(E, torch.zeros(9, 32), idx, ptr, G, l, 5, no_self=True)
    with pytest.raises(ValueError, match="exclusion shape"):
        f(E, E, idx, ptr, G, l, 5, exclude=exclusion_csr([None] * 3, (10, 9)))
    with pytest.raises(ValueError, match="disagree"):
        f(E, E, idx, ptr, G, l, 5, exclude=exclusion_csr([None] * 4, (10, 10)))
    with pytest.raises(ValueError, match="pass seg_rel"):  # the exclusion's relations bound the segments too
        f(E, E, idx, ptr, G, None, 5, exclude=exclusion_csr([None] * 2, (10, 10)))
    with pytest.raises(ValueError, match="rowptr"):
        f(E, E, idx, ptr, G, l, 5, exclude=(torch.zeros(32, dtype=torch.int32), idx))
    # everything else right, but host tensors: the device check
    with pytest.raises(ValueError, match="device"):
        f(E, E, idx, ptr, G, l, 5, exclude=exclusion_csr([None] * 3, (10, 10)))

    with pytest.raises(ValueError, match="side"):
        evaluate.top_partners(None, None, {}, {}, [0], (0, 0), 5, side="column")

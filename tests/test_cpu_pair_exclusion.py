"""CPU: the host side of ranking a pair's relations outside a per-pair exclusion set —
sparse.pair_exclusion / PairExclusion against a brute-force set lookup, their ValueErrors,
evaluate.top_relations' check of a prebuilt PairExclusion, and dg_row_topk_excl_f32 (additive to
ABI 39): exported, declared, bound, its argument rejections (they run before any HIP call, so they
work without a device) and kernels.row_topk(exclude=...)'s validation."""
import re
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp

torch = pytest.importorskip("torch")

ROOT = Path(__file__).resolve().parents[1]
NI, NJ, K = 7, 5, 6
P = 4096  # a non-null, 16-byte aligned fake device pointer (never dereferenced: every call below is rejected)


def _sets(seed=3):
    """One edge set per relation: relation 2 empty, the others random with duplicates."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(K):
        n = 0 if k == 2 else int(rng.integers(4, 15))
        out.append(np.stack([rng.integers(0, NI, n), rng.integers(0, NJ, n)], axis=1).astype(np.int64))
    return out


def _pairs(sets, seed=4):
    """40 pairs with repeats, edges of several relations, and one pair found in no relation."""
    rng = np.random.default_rng(seed)
    pairs = np.stack([rng.integers(0, NI, 40), rng.integers(0, NJ, 40)], axis=1).astype(np.int64)
    pairs[5] = pairs[2]
    pairs[17] = pairs[2]
    pairs[9] = sets[1][0]
    pairs[10] = sets[4][1]
    pairs[30] = pairs[10]
    member = {(int(r), int(c)) for e in sets for r, c in e}
    free = [(r, c) for r in range(NI) for c in range(NJ) if (r, c) not in member]
    assert free, "every cell is an edge of some relation: draw sparser sets"
    pairs[21] = free[0]
    return pairs


def _entries(sets, form):
    """The per-relation entries in one of the forms exclusion_csr takes."""
    out = []
    for k, e in enumerate(sets):
        f = ("scipy", "coo", "array", "none")[k % 4] if form == "mixed" else form
        if f == "none" and len(e):
            f = "array"
        if f == "scipy":
            out.append(sp.coo_matrix((np.ones(len(e)), (e[:, 0], e[:, 1])), shape=(NI, NJ)).tocsr())
        elif f == "coo":
            out.append((e.reshape(-1, 2), np.ones(len(e)), (NI, NJ)))
        elif f == "array":
            out.append(e if len(e) else None)
        else:
            out.append(None)
    return out


def _brute(pairs, sets, rels):
    member = [{(int(r), int(c)) for r, c in e} for e in sets]
    lists = [[s for s, k in enumerate(rels) if (int(r), int(c)) in member[k]] for r, c in pairs]
    ptr = np.zeros(len(pairs) + 1, np.int64)
    np.cumsum([len(x) for x in lists], out=ptr[1:])
    return ptr, np.asarray([s for x in lists for s in x], np.int64)


def _check(pe, pairs, sets, rels):
    ptr, slot = _brute(pairs, sets, rels)
    assert pe.ptr.dtype == np.int32 and pe.slot.dtype == np.int32
    assert pe.n_pairs == len(pairs) and pe.n_sel == len(rels)
    assert pe.ptr.shape == (len(pairs) + 1,) and pe.ptr[0] == 0 and pe.ptr[-1] == pe.slot.size == pe.nnz
    assert np.array_equal(pe.ptr, ptr) and np.array_equal(pe.slot, slot)
    for p in range(len(pairs)):
        own = pe.slot[pe.ptr[p]:pe.ptr[p + 1]]
        assert np.all(np.diff(own) > 0), p  # ascending and unique
        assert own.size == 0 or (own[0] >= 0 and own[-1] < pe.n_sel)


@pytest.mark.parametrize("relations", [None, [4, 1, 1, 5], [3, 5, 0, 4, 2, 1]], ids=["all", "repeat", "permuted"])
@pytest.mark.parametrize("form", ["scipy", "coo", "array", "mixed"])
def test_builder_equals_a_set_lookup(form, relations):
    from decagon_amd.sparse import exclusion_csr, pair_exclusion

    sets = _sets()
    pairs = _pairs(sets)
    rels = list(range(K)) if relations is None else relations
    pe = pair_exclusion(pairs, _entries(sets, form), (NI, NJ), relations)
    _check(pe, pairs, sets, rels)
    assert pe.nnz > 0 and pe.ptr[22] == pe.ptr[21]  # the pair found in no relation has an empty list
    for a, b in ((2, 5), (2, 17), (10, 30)):  # a repeated pair: its own, equal, list
        assert np.array_equal(pe.slot[pe.ptr[a]:pe.ptr[a + 1]], pe.slot[pe.ptr[b]:pe.ptr[b + 1]])
    # the stacked form gives the same object
    pe2 = pair_exclusion(pairs, exclusion_csr(_entries(sets, form), (NI, NJ)), (NI, NJ), relations)
    assert np.array_equal(pe2.ptr, pe.ptr) and np.array_equal(pe2.slot, pe.slot)
    assert (pe2.n_pairs, pe2.n_sel) == (pe.n_pairs, pe.n_sel) and pe2.ptr.dtype == pe2.slot.dtype == np.int32


def test_builder_repeated_relation_is_excluded_at_both_positions():
    from decagon_amd.sparse import pair_exclusion

    sets = _sets()
    pairs = _pairs(sets)
    pe = pair_exclusion(pairs, _entries(sets, "array"), (NI, NJ), [4, 1, 1, 5])
    own = pe.slot[pe.ptr[9]:pe.ptr[10]].tolist()  # pairs[9] is an edge of relation 1
    assert 1 in own and 2 in own


def test_builder_without_pairs_and_without_edges():
    from decagon_amd.sparse import pair_exclusion

    sets = _sets()
    for empty in (np.zeros((0, 2), np.int64), []):
        pe = pair_exclusion(empty, _entries(sets, "array"), (NI, NJ))
        assert pe.n_pairs == 0 and pe.n_sel == K and pe.nnz == 0
        assert pe.ptr.dtype == np.int32 and pe.slot.dtype == np.int32 and pe.ptr.tolist() == [0]
    pairs = _pairs(sets)
    pe = pair_exclusion(pairs, [None] * K, (NI, NJ), [0, 3])
    assert pe.nnz == 0 and pe.n_sel == 2 and np.array_equal(pe.ptr, np.zeros(41, np.int32))


def test_builder_value_errors():
    from decagon_amd.sparse import exclusion_csr, pair_exclusion

    sets = _sets()
    pairs = _pairs(sets)
    ent = _entries(sets, "array")
    for bad in ((NI, 0), (0, NJ), (-1, 0), (0, -1)):  # a pair out of range
        with pytest.raises(ValueError):
            pair_exclusion(np.vstack([pairs, [bad]]), ent, (NI, NJ))
    with pytest.raises(ValueError):
        pair_exclusion(pairs.reshape(-1), ent, (NI, NJ))
    for bad in ((NI, 0), (0, NJ), (-1, 0)):  # an exclusion index out of range
        with pytest.raises(ValueError):
            pair_exclusion(pairs, ent[:3] + [np.array([bad])] + ent[4:], (NI, NJ))
    for rl in ([0, K], [-1], []):  # a relation out of range, none listed
        with pytest.raises(ValueError):
            pair_exclusion(pairs, ent, (NI, NJ), rl)
    # the wrong number of relation entries
    for n in (K - 1, K + 1):
        with pytest.raises(ValueError):
            pair_exclusion(pairs, (ent + [None])[:n], (NI, NJ), num_relations=K)
        with pytest.raises(ValueError):
            pair_exclusion(pairs, exclusion_csr((ent + [None])[:n], (NI, NJ)), (NI, NJ), num_relations=K)
    with pytest.raises(ValueError):
        pair_exclusion(pairs, [], (NI, NJ))
    with pytest.raises(ValueError):  # K − 1 entries: relation K − 1 does not exist
        pair_exclusion(pairs, ent[:K - 1], (NI, NJ), [K - 1])
    # a stacked exclusion, or a matrix, of another shape
    with pytest.raises(ValueError):
        pair_exclusion(pairs, exclusion_csr(ent, (NI, NJ + 1)), (NI, NJ))
    with pytest.raises(ValueError):
        pair_exclusion(pairs, [sp.csr_matrix((NI + 1, NJ))] * K, (NI, NJ))
    assert pair_exclusion(pairs, ent, (NI, NJ), num_relations=K).n_sel == K


def test_top_relations_checks_a_prebuilt_exclusion():
    from decagon_amd import evaluate
    from decagon_amd.sparse import pair_exclusion

    sets = _sets()
    pairs = _pairs(sets)
    ent = _entries(sets, "array")
    pe = pair_exclusion(pairs, ent, (NI, NJ))
    assert evaluate._pair_exclusion(None, pairs, None, K, (NI, NJ)) is None
    assert evaluate._pair_exclusion(pe, pairs, None, K, (NI, NJ)) is pe
    with pytest.raises(ValueError, match="exclude"):  # the wrong P
        evaluate._pair_exclusion(pe, pairs[:39], None, K, (NI, NJ))
    with pytest.raises(ValueError, match="exclude"):  # the wrong n_sel
        evaluate._pair_exclusion(pe, pairs, [0, 1, 2], K, (NI, NJ))
    pe3 = pair_exclusion(pairs, ent, (NI, NJ), [4, 1, 1, 5])
    assert evaluate._pair_exclusion(pe3, pairs, [4, 1, 1, 5], K, (NI, NJ)) is pe3
    with pytest.raises(ValueError, match="exclude"):
        evaluate._pair_exclusion(pe3, pairs, None, K, (NI, NJ))
    # anything else is built against the call's pairs and relations, with the table sizes
    built = evaluate._pair_exclusion(ent, pairs, [4, 1, 1, 5], K, (NI, NJ))
    assert np.array_equal(built.ptr, pe3.ptr) and np.array_equal(built.slot, pe3.slot)
    with pytest.raises(ValueError):  # the wrong number of relation entries for the edge type
        evaluate._pair_exclusion(ent[:-1], pairs, None, K, (NI, NJ))
    with pytest.raises(ValueError):  # a shape that is not the tables'
        evaluate._pair_exclusion(ent, pairs, None, K, (NI - 1, NJ))


# ---------------------------------------------------------------- the symbol
def _excl(lib, **over):
    """dg_row_topk_excl_f32 with arguments that would be valid, except for `over`."""
    a = dict(x=P, ld=70, n_rows=95, n_cols=70, topk=10, excl_ptr=P, excl_slot=P, excl_nnz=300, out_val=P, out_idx=P,
             out_count=P, stream=None)
    assert set(over) <= set(a), over
    a.update(over)
    return lib.dg_row_topk_excl_f32(*a.values())


def test_symbol_exported_declared_and_bound():
    from decagon_amd import _lib

    lib = _lib.load()
    assert hasattr(lib, "dg_row_topk_excl_f32")
    assert "dg_row_topk_excl_f32" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["dg_row_topk_excl_f32"][1]) == 12
    hdr = (ROOT / "include" / "decagon_hip.h").read_text()
    assert re.search(r"^int dg_row_topk_excl_f32\(const float\* x, int64_t ld,", hdr, re.M)
    assert lib.dg_abi_version() == _lib.ABI_VERSION == 39  # additive: the number stays


def test_rejections_without_a_device():
    from decagon_amd import _lib

    lib = _lib.load()
    EINVAL = _lib.DG_EINVAL
    # exactly one of the two exclusion pointers NULL, with rows and without
    for n_rows in (95, 0):
        assert _excl(lib, excl_ptr=None, n_rows=n_rows) == EINVAL
        assert _excl(lib, excl_slot=None, n_rows=n_rows) == EINVAL
    for nnz in (-1, -2**31):
        assert _excl(lib, excl_nnz=nnz) == EINVAL
        assert _excl(lib, excl_nnz=nnz, excl_ptr=None, excl_slot=None) == EINVAL
    # everything dg_row_topk_f32 rejects, with lists and without
    for lists in ({}, dict(excl_ptr=None, excl_slot=None, excl_nnz=0)):
        for nm in ("x", "out_val", "out_idx", "out_count"):
            assert _excl(lib, **{nm: None}, **lists) == EINVAL, nm
        for topk in (0, -1, _lib.DG_TOPK_MAX_K + 1):
            assert _excl(lib, topk=topk, **lists) == EINVAL, topk
        assert _excl(lib, n_cols=0, **lists) == EINVAL
        assert _excl(lib, n_rows=-1, **lists) == EINVAL
        assert _excl(lib, ld=69, **lists) == EINVAL
        # nothing to select is not an error (and launches nothing: no device here)
        assert _excl(lib, n_rows=0, x=None, out_val=None, out_idx=None, out_count=None, **lists) == _lib.DG_OK


def test_row_topk_exclude_validation():
    from decagon_amd import kernels

    x = torch.zeros(3, 4)
    ptr, slot = torch.zeros(4, dtype=torch.int32), torch.zeros(5, dtype=torch.int32)
    for bad in (ptr, (ptr,), (ptr, slot, slot), "ab", (ptr.numpy(), slot), (ptr, slot.numpy()), (ptr, None)):
        with pytest.raises(TypeError):
            kernels.row_topk(x, 2, exclude=bad)
    for bad in ((ptr.long(), slot), (ptr, slot.long()), (ptr.float(), slot)):
        with pytest.raises(TypeError, match="dtype"):
            kernels.row_topk(x, 2, exclude=bad)
    for bad in ((torch.zeros(3, dtype=torch.int32), slot), (torch.zeros(5, dtype=torch.int32), slot),
                (torch.zeros(8, dtype=torch.int32)[::2], slot), (ptr, torch.zeros(10, dtype=torch.int32)[::2]),
                (ptr.view(2, 2), slot), (ptr, slot.view(5, 1))):
        with pytest.raises(ValueError, match="exclude"):
            kernels.row_topk(x, 2, exclude=bad)
    with pytest.raises(ValueError, match="topk"):
        kernels.row_topk(x, 0, exclude=(ptr, slot))
    with pytest.raises(ValueError, match="device"):  # all else valid: the device check is the last
        kernels.row_topk(x, 2, exclude=(ptr, slot))
    with pytest.raises(ValueError, match="device"):
        kernels.row_topk(x, 2, exclude=(ptr, torch.zeros(0, dtype=torch.int32)))


def test_decoder_top_relations_exclude_validation():
    from decagon_amd import kernels

    f = torch.zeros
    a = dict(row_table=f(20, 32), col_table=f(30, 32), row_idx=f(10, dtype=torch.int32),
             col_idx=f(10, dtype=torch.int32), G=f(32, 32), l=f(5, 32), topk=3)
    ptr, slot = f(11, dtype=torch.int32), f(4, dtype=torch.int32)
    with pytest.raises(TypeError):
        kernels.decoder_top_relations(**a, exclude=ptr)
    with pytest.raises(TypeError, match="dtype"):
        kernels.decoder_top_relations(**a, exclude=(ptr.long(), slot))
    with pytest.raises(ValueError, match="exclude"):  # one list per pair, and one entry more
        kernels.decoder_top_relations(**a, exclude=(f(10, dtype=torch.int32), slot))
    with pytest.raises(ValueError, match="device"):
        kernels.decoder_top_relations(**a, exclude=(ptr, slot))

"""CPU: the host wave-table builder (decagon_amd/wavetable.py), which needs neither torch nor a GPU.

* tests/golden/wave_tables.npz holds the tables the previous, launch-welded builder
  (kernels.PreparedFusedTab / PreparedSegTab before wavetable.py existed) made for the cases of
  `cases(0)`; the pure builder must reproduce them byte for byte.  Pointer-valued fields are kept
  as (buffer index, byte offset); `role` of a fused table is compared under bits 21-30 (the
  earlier builder also wrote bits 0-20 and 31, which no fused kernel reads).
* Read-back: every wave's pairs, decoded from the compact slots and overflow batches, give back
  each row's CSR, relation by relation in order, and the finishing waves' words describe them.
* The Python descriptor dtype and bit-field constants agree with include/decagon_hip.h and the
  offsets asserted in segspmm.hip.
"""
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
FIXTURE = ROOT / "tests" / "golden" / "wave_tables.npz"

# Two node types, four edge types with 1/2/2/5 relations: 3 and 7 relations a row, config S's.
N = {0: 7, 1: 131}            # type 0: an odd row count at 2 rows a workgroup; type 1: >= 130 columns
EDGE_TYPES = [((0, 0), 1), ((0, 1), 2), ((1, 0), 2), ((1, 1), 5)]
SLABS = {(1, 1): (6, [5, 0, 3, 1, 2])}  # (K, relation -> slab): the one non-identity slab map
FAKE_BASE = 0x100 << 32       # buffer b of a case sits at FAKE_BASE + (b << 32)


def _rows(rng, n_r, n_c, planted=None):
    """One relation's rows: (cols, vals) per row, lengths mostly 0-9, `planted` {row: length}."""
    out = []
    for r in range(n_r):
        n = int(rng.choice([0, 0, 1, 2, 3, 5, 9]))
        if planted and r in planted:
            n = planted[r]
        n = min(n, n_c)
        cols = rng.choice(n_c, size=n, replace=False).astype(np.int64)
        vals = (rng.integers(1, 64, size=n) / 64.0).astype(np.float32)
        out.append((cols, vals))
    return out


def _merge(rels, slabs, n_r, n_c, chunk):
    """The chunk-merged CSR and segment starts of sparse.merge_chunks / chunk_segments."""
    n_chunks = -(-len(rels) // chunk)
    rowptr, seg, vcol, val = [0], [], [], []
    for c in range(n_chunks):
        for r in range(n_r):
            for t in range(chunk):
                seg.append(len(vcol))
                k = c * chunk + t
                if k < len(rels):
                    cols, vals = rels[k][r]
                    vcol += [int(slabs[k]) * n_c + int(x) for x in cols]
                    val += [float(v) for v in vals]
            rowptr.append(len(vcol))
    return (np.array(rowptr, np.int32), np.array(seg, np.int32), np.array(vcol, np.int32),
            np.array(val, np.float32), n_chunks)


def _spec(rels, n_r, n_c, chunk, K=None, slab=None):
    K = len(rels) if K is None else K
    slabs = list(range(len(rels))) if slab is None else slab
    rowptr, seg, vcol, val, n_chunks = _merge(rels, slabs, n_r, n_c, chunk)
    return dict(rels=rels, rowptr=rowptr, seg=seg, vcol=vcol, val=val, K=K,
                slab=None if slab is None else np.array(slab, np.int32), n_rows=n_r, n_cols=n_c,
                chunk=chunk, n_chunks=n_chunks, n_rels=len(rels))


def cases(seed):
    """The table cases: dicts of plain data, from which both builders can be driven."""
    rng = np.random.default_rng(seed)
    specs = []
    for (i, j), k_rels in EDGE_TYPES:
        K, slab = SLABS.get((i, j), (None, None))
        rels = []
        for k in range(k_rels):
            planted = None
            if (i, j) == (1, 1):  # waves of S, S + 1, S + 65 pairs, and a 600-pair group
                planted = {6: 120}
                if k == 0:
                    planted.update({3: 16, 4: 17, 5: 81})
            rels.append(_rows(rng, N[i], N[j], planted))
        specs.append(_spec(rels, N[i], N[j], k_rels, K, slab))
    targets = [(N[0], [0, 1], True), (N[1], [2, 3], False)]
    # projection specs, one per edge type sourced from the target's node type: (target, n_rels, K, slab)
    projs = [(0, 1, 1, None), (0, 2, 2, None), (1, 2, 2, None), (1, 5, 6, [5, 0, 3, 1, 2])]

    def fused(name, d_in, d_out, balance, projs=(), share=True, dec=None, peer=False):
        return dict(name=name, kind="fused", d_in=d_in, d_out=d_out, balance=balance, projs=list(projs), share=share,
                    dec=dec, peer=peer, targets=targets, specs=specs)

    out = [fused("l1", 64, 64, False),
           fused("l1_bal_shared", 64, 64, True, projs, True),
           fused("l1_bal_unshared", 64, 64, True, projs, False),
           fused("l2_reassoc", 64, 32, False),
           fused("l2_reassoc_bal", 64, 32, True),
           fused("l2_narrow_bal", 32, 32, True),
           fused("l2_narrow_bal_dec", 32, 32, True, dec=0),
           fused("l1_bal_peer", 64, 64, True, peer=True)]
    a = _spec([_rows(rng, 9, N[0]) for _ in range(3)], 9, N[0], 2)
    b = _spec([_rows(rng, 5, N[1], {1: 90}) for _ in range(2)], 5, N[1], 1)
    out.append(dict(name="seg_chunk2", kind="seg", d_in=64, d_out=64, specs=[a, b]))
    return out


def buffers(case):
    """The case's device buffers, in a fixed order: {name: index}."""
    names = [f"x{g}" for g in range(len(case["specs"]))] + [f"w{g}" for g in range(len(case["specs"]))]
    if case["kind"] == "seg":
        names += [f"out{g}" for g in range(len(case["specs"]))]
    else:
        names += [f"tout{t}" for t in range(len(case["targets"]))]
        names += [f"pw{p}" for p in range(len(case["projs"]))] + [f"pout{p}" for p in range(len(case["projs"]))]
        names += ["q"]
    return {n: b for b, n in enumerate(names)}


def x_ld(case, g):
    return case["d_in"] + (4 if g == 1 else 0)


def split_pointers(desc, locate):
    """A table's descriptors with every pointer-valued field replaced by (buffer index, byte
    offset) — `locate(address) -> (index, offset)`, (-1, 0) for NULL: (descriptors with those
    fields zeroed, [n, 4, 2] index and offset of x, w, orow and the auxiliary address).  The
    auxiliary words are an address on a projecting wave and on a flagged decoder-row wave (the
    low and high word are then zeroed in `raw`); elsewhere they stay as stored."""
    from decagon_amd import wavetable as wt

    raw = np.zeros(len(desc), wt.DESC)
    for f in wt.DESC.names:
        raw[f] = desc[f]
    ptr = np.zeros((len(desc), 4, 2), np.int64)
    for i in range(len(desc)):
        role = wt.decode_role(desc["role"][i])
        for c, f in enumerate(("x", "w", "orow")):
            a = int(desc[f][i])
            ptr[i, c] = locate(a) if a else (-1, 0)
            raw[f][i] = 0
        if role.proj_slots or (role.dec and desc["orow"][i]):
            ptr[i, 3] = locate(wt.join_addr(desc["aux_lo"][i], desc["aux_hi"][i]))
            raw["aux_lo"][i] = raw["aux_hi"][i] = 0
        else:
            ptr[i, 3] = (-1, 0)
    return raw, ptr


def _locate_fake(a):
    return (a - FAKE_BASE) >> 32, a & 0xffffffff


def build(case):
    """The case through the pure builder, its buffers at the fake bases."""
    from decagon_amd import wavetable as wt

    buf = buffers(case)
    addr = {n: FAKE_BASE + (b << 32) for n, b in buf.items()}
    reassoc = case["d_out"] != case["d_in"]
    data = [wt.SegData(s["rowptr"], s["seg"], s["vcol"], s["val"], s["slab"], addr[f"x{g}"],
                       addr[f"w{g}"] if reassoc else None, addr[f"out{g}"] if case["kind"] == "seg" else None,
                       x_ld(case, g), s["n_rows"], s["n_cols"], s["chunk"], s["n_chunks"], s["n_rels"])
            for g, s in enumerate(case["specs"])]
    if case["kind"] == "seg":
        return wt.seg_table(data, case["d_in"], case["d_out"])
    return wt.fused_table(
        [(addr[f"tout{t}"], n_rows, [data[g] for g in gs], relu) for t, (n_rows, gs, relu) in enumerate(case["targets"])],
        case["d_in"], case["d_out"], balance=case["balance"],
        projs=[wt.ProjData(t, addr[f"pw{p}"], addr[f"pout{p}"], n_rels, slab)
               for p, (t, n_rels, _, slab) in enumerate(case["projs"])],
        share_proj=case["share"], dec=None if case["dec"] is None else wt.DecData(case["dec"], addr["q"]),
        peer=case["peer"])


@pytest.fixture(scope="module")
def built():
    return {seed: [(c, build(c)) for c in cases(seed)] for seed in (0, 1)}


FUSED_ROLE_MASK = np.uint32(0x7fe00000)  # bits 21-30


def test_tables_equal_the_previous_builders(built):
    z = np.load(FIXTURE, allow_pickle=False)
    cnts, S = [], None
    for case, tab in built[0]:
        n = case["name"]
        raw, ptr = split_pointers(tab.desc, _locate_fake)
        want = z[f"{n}.desc"].view(raw.dtype).reshape(-1)  # [n, 64] bytes: every field keeps its offset
        assert [int(v) for v in z[f"{n}.counts"]] == [tab.n_blocks, tab.nw, tab.stride, tab.slot_pairs], n
        assert len(want) == len(raw), n
        for f in raw.dtype.names:
            got_f, want_f = raw[f], want[f]
            if f == "role" and case["kind"] == "fused":
                got_f, want_f = got_f & FUSED_ROLE_MASK, want_f & FUSED_ROLE_MASK
                assert not (raw[f] & ~FUSED_ROLE_MASK).any(), "a fused table writes only the live role bits"
            assert np.array_equal(got_f, want_f), (n, f)
        assert np.array_equal(ptr, z[f"{n}.ptr"]), n
        assert tab.pairs.dtype == np.int32 and tab.ovf.dtype == np.int32
        assert tab.pairs.tobytes() == z[f"{n}.pairs"].tobytes(), n
        assert tab.ovf.tobytes() == z[f"{n}.ovf"].tobytes(), n
        if n == "l1":
            cnts, S = tab.desc["cnt"], tab.slot_pairs
            t0 = [(r0, rpb) for t, r0, rpb in tab.plan if t == 0]
            assert all(rpb == 2 for _, rpb in t0) and case["targets"][0][0] % 2 == 1
    # the conditions the fixture was made to meet
    assert max(N.values()) >= 130
    assert (cnts == 0).any() and (cnts == S).any() and (cnts == S + 1).any() and (cnts >= S + 65).any()
    assert any((tab.desc["cnt"] >= tab.slot_pairs + 65).any() for c, tab in built[0] if c.get("balance"))
    assert FIXTURE.stat().st_size <= 256 * 1024


def _row_pairs(spec, k, r, reassoc):
    cols, vals = spec["rels"][k][r]
    sl = k if spec["slab"] is None else int(spec["slab"][k])
    vc = cols if reassoc else cols + sl * spec["n_cols"]
    return np.stack([vc.astype(np.int32), vals.view(np.int32)], 1).reshape(-1, 2)


@pytest.mark.parametrize("seed", [0, 1])
def test_tables_read_back_to_the_rows_they_were_built_from(built, seed):
    from decagon_amd import wavetable as wt

    for case, tab in built[seed]:
        d, lp, reassoc = tab.desc, case["d_in"] // 4, case["d_out"] != case["d_in"]
        addr = {n: FAKE_BASE + (b << 32) for n, b in buffers(case).items()}
        assert len(d) == tab.n_blocks * tab.stride == len(tab.plan) * tab.stride
        if case["kind"] == "seg":
            for b, blk in enumerate(tab.plan):
                i0 = b * tab.stride
                if blk is None:
                    assert not d["cnt"][i0:i0 + tab.stride].any() and not d["orow"][i0:i0 + tab.stride].any()
                    continue
                g, c, r0, rpb = blk
                s = case["specs"][g]
                for w in range(tab.nw):
                    slot, t = divmod(w, s["chunk"])
                    r, k = r0 + slot, c * s["chunk"] + t
                    live = slot < rpb and r < s["n_rows"]
                    want = _row_pairs(s, k, r, False) if live and k < s["n_rels"] else np.zeros((0, 2), np.int32)
                    assert np.array_equal(wt.wave_pairs(tab, i0 + w, lp), want)
                    if live and t == 0:
                        assert d["orow"][i0 + w] == addr[f"out{g}"] + (c * s["n_rows"] + r) * case["d_out"] * 4
                        assert wt.decode_role(d["role"][i0 + w]) == wt.Role((), False, s["chunk"])
                    else:
                        assert d["orow"][i0 + w] == 0
            continue
        covered = {}  # (target, row, projection relation) -> times projected
        for b, (t, r0, rpb) in enumerate(tab.plan):
            n_rows, gs, relu = case["targets"][t]
            i0, used = b * tab.stride, set()
            for slot in range(rpb):
                r, i = r0 + slot, i0 + slot
                if r >= n_rows:
                    assert d["orow"][i] == 0
                    continue
                assert d["orow"][i] == addr[f"tout{t}"] + r * case["d_out"] * 4
                assert wt.decode_wr(d["wr"][i]) == wt.Wr(len(gs), relu, slot)
                counts, w = wt.decode_gwaves(d["gwaves"][i], len(gs)), int(d["first_wave"][i])
                for g, cnt in zip(gs, counts):
                    s = case["specs"][g]
                    waves = list(range(w, w + cnt))
                    assert not used & set(waves) and waves[-1] < tab.nw
                    used |= set(waves)
                    got = [wt.wave_pairs(tab, i0 + x, lp) for x in waves]
                    want = [_row_pairs(s, k, r, reassoc) for k in range(s["n_rels"])]
                    assert np.array_equal(np.concatenate(got), np.concatenate(want)), (case["name"], t, r, g)
                    for x, p in zip(waves, got):
                        if len(p):
                            assert d["x"][i0 + x] == addr[f"x{g}"] and d["x_ld"][i0 + x] == x_ld(case, g)
                        if reassoc and len(p):  # the wave's W slab names the one relation it holds
                            sl, rem = divmod(int(d["w"][i0 + x]) - addr[f"w{g}"], wt.W_SLAB_BYTES)
                            k = sl if s["slab"] is None else list(s["slab"]).index(sl)
                            assert rem == 0 and (_row_pairs(s, k, r, True)[:, None] == p[None]).all(2).any(0).all()
                    if reassoc:  # relation by relation, in order: the waves' relations do not go back
                        ks = [int(d["w"][i0 + x]) for x, p in zip(waves, got) if len(p)]
                        order = [addr[f"w{g}"] + (k if s["slab"] is None else int(s["slab"][k])) * wt.W_SLAB_BYTES
                                 for k in range(s["n_rels"])]
                        assert [order.index(a) for a in ks] == sorted(order.index(a) for a in ks)
                    w += cnt
            for x in range(tab.stride):  # the waves no finishing wave names gather nothing
                if x not in used:
                    assert d["cnt"][i0 + x] == 0
            rels = [(p, k) for p, pj in enumerate(case["projs"]) if pj[0] == t for k in range(pj[1])]
            for x in range(tab.stride):
                role = wt.decode_role(d["role"][i0 + x])
                assert role.dec == (case["dec"] == t and x < rpb and r0 + x < n_rows)
                if role.dec:
                    assert wt.join_addr(d["aux_lo"][i0 + x], d["aux_hi"][i0 + x]) == addr["q"] + (r0 + x) * 128
                if not role.proj_slots:
                    continue
                assert rels and all(sl < rpb and r0 + sl < n_rows for sl in role.proj_slots)
                hit = [(p, k) for p, k in rels
                       if int(d["w"][i0 + x]) == addr[f"pw{p}"] + _slab(case, p, k) * wt.W_SLAB_BYTES]
                assert len(hit) == 1
                p, k = hit[0]
                assert (wt.join_addr(d["aux_lo"][i0 + x], d["aux_hi"][i0 + x])
                        == addr[f"pout{p}"] + (_slab(case, p, k) * n_rows + r0) * 128)
                for sl in role.proj_slots:
                    covered[t, r0 + sl, p, k] = covered.get((t, r0 + sl, p, k), 0) + 1
        want = {(pj[0], r, p, k): 1 for p, pj in enumerate(case["projs"]) for k in range(pj[1])
                for r in range(case["targets"][pj[0]][0])}
        assert covered == want


def _slab(case, p, k):
    slab = case["projs"][p][3]
    return k if slab is None else slab[k]


def test_descriptor_dtype_and_constants_agree_with_the_header():
    from decagon_amd import wavetable as wt

    header = (ROOT / "include" / "decagon_hip.h").read_text()
    kernel = (ROOT / "decagon_amd" / "csrc" / "segspmm.hip").read_text()
    macros = {m[0]: int(m[1], 0) for m in re.findall(r"^#define (DG_TAB_\w+) +(\w+)", header, re.M)}
    assert len(macros) >= 11
    for name, value in macros.items():
        assert getattr(wt, name) == value, name
    assert {n for n in vars(wt) if n.startswith("DG_TAB_")} == set(macros)
    offsets = {m[0]: int(m[1]) for m in
               re.findall(r"static_assert\(offsetof\(dg_tab_desc, (\w+)\) == (\d+)", kernel)}
    assert offsets == {f: wt.DESC.fields[f][1] for f in wt.DESC.names}
    body = header[header.index("typedef struct dg_tab_desc {"):header.index("} dg_tab_desc;")]
    assert re.findall(r"(\w+);", body) == list(wt.DESC.names)  # the same fields in the same order
    assert wt.DESC.itemsize == 64
    # the codec round-trips every field
    assert wt.decode_role(wt.encode_role((0, 3), True, 0)) == wt.Role((0, 3), True, 0)
    assert wt.decode_role(wt.encode_role(seg_waves=16)) == wt.Role((), False, 16)
    assert wt.encode_role((1,)) == 0x42000000 and wt.encode_role(dec=True) == 0x20000000
    assert wt.decode_wr(wt.encode_wr(8, True, 3)) == wt.Wr(8, True, 3) and wt.encode_wr(3, True, 1) == 3 | 256 | 65536
    assert wt.decode_gwaves(wt.encode_gwaves([16, 1, 7, 2, 1, 1, 1, 16]), 8) == [16, 1, 7, 2, 1, 1, 1, 16]
    a = 0x7f12_8000_fff0
    assert wt.join_addr(*wt.split_addr(a)) == a and wt.split_addr(a) == (-2147418128, 0x7f12)

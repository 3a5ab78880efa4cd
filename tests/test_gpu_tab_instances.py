"""GPU: every one-GPU template instance of the wave-table kernels (segspmm.hip: gcn_tab_kernel,
seg_tab_kernel) and the 16-wave fused-seg instances, launched from PreparedFusedTab / PreparedSegTab
objects built here (tests/_tab_cases.py), against float64 at every element of every output.

Who reaches what (the template arguments are <PROJ, NW, PEER, LP, POST, DEC>):
  gcn_tab_kernel<false,  8, false>                  64->64, stride 8     fused, order, slots, POST's plain run
  gcn_tab_kernel<false, 16, false>                  64->64, stride 16    (nw = 11 < 16 unbalanced, 16 balanced)
  gcn_tab_kernel<true,   8, false>                  64->32, stride 8     fused, order, slots
  gcn_tab_kernel<true,  16, false>                  64->32, stride 16    (nw = 11 and 16)
  gcn_tab_kernel<false,  8, false, 8>               32->32, stride 8     fused, order, slots, DEC's plain run
  gcn_tab_kernel<false, 16, false, 8>               32->32, stride 16
  gcn_tab_kernel<false,  8 / 16, false, 16, true>   dg_gcn_fused_tab_post_f32    test_post_*
  gcn_tab_kernel<false,  8 / 16, false, 8, false, true>  dg_gcn_fused_tab_dec_f32  test_dec_*
  gcn_fused_seg_kernel<16 / 16 / 8, PROJ, 16, false>  seg_form() of the stride-16 launches (order, slots)
  seg_tab_kernel<PROJ, 8>                           chunk 1, 3, 8        test_seg_tab_*
  seg_tab_kernel<PROJ, 16>                          chunk 9, 16
The peer instances (PEER = true) need an exchange region and are test_gpu_peer.py's; their NW = 16
forms are not launched here.  Each test asserts the entry point, wave-slot stride, waves per
workgroup and slot size of the launch it built.  A fused launch takes at most 8 groups, so the
32-wide geometries run as two launches (three targets; the 8-group target alone).

Finishing-wave group logic: rows of 1, 2, 4 (d_out = 64) and 8 (d_out = 32) groups; a group of 16
waves (the "one" geometry, balanced); rows per workgroup 1 to 4 with absent row slots; nw < stride.

Data.  integer: val in {±1, ±2, ±3}, operand in {±1, ±2}, weight stacks in [-4, 4] — every
aggregate and projected value is an integer below 2^24 (asserted on the float64 reference), so
the fp32 sums are exact in any order and a dropped, doubled or misrouted pair moves its whole
row.  tiny: the same with val · 2^-30, so Σx² falls under the 1e-12 clamp (with weight stacks,
whose sums run to 10^6, on either side of it), and val · 2^-50, where every row is clamped; the
sums stay exact and the reference applies the clamp.  gaussian: for the bitwise cross-form claims
only, which integer data cannot see.

The bound of a finished row, per element e, on exact sums:  |got − ref| ≤ (8 + gc)·2^-24·Σ_g |n_g[e]|,
n_g the float64 normalised vector of group g, gc the row's groups.  Roundings, from the source
(-O3 alone: contraction may fuse the squares' adds, correctly rounded sqrtf and divide):
  Σx²      4 per lane (x·x, then three adds or fmas) + log2(d_out/4) butterfly adds = 8 (d_out 64) / 7 (32),
           all terms non-negative: relative 8·u, halved by the square root           4   u = 2^-24
  sqrtf, 1.0f / ·, sum · inv   one each                                              3
  the gc − 1 ordered adds of the groups, each within u of a partial sum ≤ Σ|n_g|     gc − 1
so 6 + gc to first order; the 2 left over in 8 + gc cover the second-order terms, the clamp
constant's own rounding (1e-12f) and the float64 reference.  relu moves nothing further apart.
Each test prints its worst ratio; on the MI355X the largest over all cases is 0.25 of the bound
(0.017 of POST's, 0.031 of DEC's).  Dropping any single pair of the integer set moves some element
of its row's float64 reference by more than 1000 bounds (test_cpu_tab_cases.py asserts it).

POST: a P element passes 8 fmaf and 3 butterfly adds; the bound allows one rounding per term of
the 64-term product and the butterfly's three, (64 + 3)·2^-24·Σ|terms|.
DEC: one product, 4 fmaf, 3 butterfly adds, one product; bound (32 + 3 + 2)·2^-24·Σ|terms|.
"""
import functools

import numpy as np
import pytest

import _tab_cases as tc
from conftest import rel_err

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SENTINEL = -12345.0
FUSED = [(shape, stride, balance) for shape in tc.SHAPES for stride in (8, 16, "one") for balance in (False, True)
         if balance or stride != "one"]


@pytest.fixture(scope="module")
def K():
    from decagon_amd import kernels

    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return kernels


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _spec(K, g, out=None):
    m = g.m
    return K.SegSpec(_dev(m.rowptr), _dev(g.seg), _dev(m.vcol), _dev(m.val), _dev(g.x), out, g.n_rows, tc.N_COLS,
                     m.n_chunks, g.chunk, g.n_rels, g.x.shape[1], g.n_slabs * tc.N_COLS,
                     vcol_max=int(m.vcol.max()) if m.nnz else -1,  # (a group may be empty throughout)
                     w=None if g.w is None else _dev(g.w), slab=_dev(g.slabs), slab_max=int(g.slabs.max()))


@functools.lru_cache(maxsize=None)
def _case(shape, stride, kind):
    """The launches of a geometry: (spec, targets, float64 references), built once and left unchanged."""
    d_in, d_out = shape
    out = []
    for li, spec in enumerate(tc.geometry(stride, d_out)):
        targets = tc.make_launch(spec, d_in, d_out, "gauss" if kind == "gauss" else "int", 100 + li)
        scale = {"tiny": tc.TINY, "tinier": tc.TINIER}.get(kind, 1.0)
        if scale != 1.0:
            targets = [tc.Target(t.n_rows, [tc.scaled(g, scale) for g in t.groups], t.relu) for t in targets]
        if kind != "gauss":
            for t in targets:
                for g in t.groups:
                    tc.assert_exact(g, scale)
        out.append((spec, targets, [tc.fused_reference(t) for t in targets]))
    return out


class _Launch:
    """A launch's tensors on the device; every output has one more row than its target, a guard."""

    def __init__(self, K, targets, d_out):
        self.bufs = [torch.empty((t.n_rows + 1, d_out), device="cuda") for t in targets]
        self.targets = [(b, t.n_rows, [_spec(K, g) for g in t.groups], t.relu) for b, t in zip(self.bufs, targets)]

    def run(self, fn):
        """The target rows fn() leaves in NaN-filled outputs; the guard rows must keep their sentinel."""
        for b in self.bufs:
            b.fill_(float("nan"))
            b[-1] = SENTINEL
        fn()
        torch.cuda.synchronize()
        outs = [b.cpu().numpy() for b in self.bufs]
        for o in outs:
            assert np.all(o[-1] == SENTINEL), "a row past the target was written"
            assert np.isfinite(o).all(), "a row was not written, or gathered from a spare slab"
        return [o[:-1].copy() for o in outs]


def _tab(K, monkeypatch, dev, shape, balance, slot, **kw):
    if slot:
        monkeypatch.setenv("DG_TAB_SLOT", str(slot))
    else:
        monkeypatch.delenv("DG_TAB_SLOT", raising=False)
    return K.PreparedFusedTab(dev.targets, shape[0], shape[1], balance=balance, **kw)


def _reached(launch, tname, spec, balance, slot):
    nw, stride, _ = tc.expected_geometry(spec, balance)
    assert launch._tname == tname
    assert (launch._tab.nw_stride, launch.nw, launch._tab.nw) == (stride, nw, nw)
    assert launch.slot_pairs == launch._tab.slot_pairs and launch.slot_pairs in (16, 32, 48, 64)
    assert not slot or launch.slot_pairs == slot


def _within(got, want, bound, what):
    """|got − want| ≤ bound at every element, none of them NaN or infinite; returns the worst ratio
    (0 where the bound is 0)."""
    assert np.isfinite(got).all(), f"{what}: {np.count_nonzero(~np.isfinite(got))} elements not finite"
    err = np.abs(got.astype(np.float64) - want)
    ratio = float(np.max(np.divide(err, bound, out=np.zeros_like(err), where=bound > 0), initial=0.0))
    bad = np.argwhere(~(err <= bound))
    assert not len(bad), f"{what}: {len(bad)} elements outside the bound, first {bad[0]}, worst ratio {ratio:.3f}"
    return ratio


def _check_rows(got, ref, gc, what):
    want, A, empty = ref
    assert np.all(_bits(got[empty]) == 0), f"{what}: a row without pairs is exactly 0"
    return _within(got, want, (8 + gc) * tc.U24 * A, what)


# ------------------------------------------------------------------------------ 1: fused instances
@pytest.mark.parametrize("shape,stride,balance", FUSED)
def test_fused_instances_against_float64(K, monkeypatch, shape, stride, balance):
    """Assertion 1: act(Σ_g l2norm(Σ_k Â_k·X_k)), with weight stacks Σ_g l2norm(Σ_k (Â_k·H)·W[slab_k]),
    within (8 + gc)·2^-24·Σ_g|n_g| of float64 at every element, on the integer set and its two tiny
    copies, at every slot size; rows without pairs exactly 0."""
    worst = 0.0
    for kind in ("int", "tiny", "tinier"):
        for li, (spec, targets, refs) in enumerate(_case(shape, stride, kind)):
            dev = _Launch(K, targets, shape[1])
            for slot in tc.SLOTS:
                launch = _tab(K, monkeypatch, dev, shape, balance, slot)
                _reached(launch, "dg_gcn_fused_tab_f32", spec, balance, slot)
                for t, (got, tg, ref) in enumerate(zip(dev.run(launch), targets, refs)):
                    what = f"{kind} launch {li} slot {slot} target {t}"
                    worst = max(worst, _check_rows(got, ref, len(tg.groups), what))
    print(f"fused {shape} stride {stride} balance {balance}: worst |got - ref| / B = {worst:.3f}")


# ------------------------------------------------------------------------------ 2: order independence
@pytest.mark.parametrize("stride", [8, 16])
@pytest.mark.parametrize("shape", tc.SHAPES)
def test_exact_sums_do_not_depend_on_dealing_or_batching(K, monkeypatch, shape, stride):
    """Assertion 2: on the integer set both balance settings, every slot size and seg_form() give
    the same bits — exact sums leave nothing for the dealing or the batching to change."""
    for spec, targets, _ in _case(shape, stride, "int"):
        dev = _Launch(K, targets, shape[1])
        base = None
        for balance in (False, True):
            for slot in tc.SLOTS:
                launch = _tab(K, monkeypatch, dev, shape, balance, slot)
                _reached(launch, "dg_gcn_fused_tab_f32", spec, balance, slot)
                outs = dev.run(launch)
                base = outs if base is None else base
                for t, (a, b) in enumerate(zip(outs, base)):
                    assert np.array_equal(_bits(a), _bits(b)), (balance, slot, t)
        for t, (a, b) in enumerate(zip(dev.run(launch.seg_form), base)):
            assert np.array_equal(_bits(a), _bits(b)), ("seg_form", t)


# ------------------------------------------------------------------------------ 3: the bitwise claims
@pytest.mark.parametrize("stride", [8, 16])
@pytest.mark.parametrize("shape", tc.SHAPES)
def test_gaussian_rows_bitwise_across_slot_sizes_and_seg_form(K, monkeypatch, shape, stride):
    """Assertion 3, on inexact data: the four fixed slot sizes give the same bits, unbalanced and
    balanced (a lane group adds the same pairs in the same order whatever the first batch's size);
    the unbalanced table equals seg_form() bit for bit; and seg_form() — at stride 16
    gcn_fused_seg_kernel<.., 16, false> — is within rel_err 1e-5 of float64."""
    for spec, targets, refs in _case(shape, stride, "gauss"):
        dev = _Launch(K, targets, shape[1])
        for balance in (False, True):
            base = None
            for slot in tc.SLOTS[1:]:
                launch = _tab(K, monkeypatch, dev, shape, balance, slot)
                _reached(launch, "dg_gcn_fused_tab_f32", spec, balance, slot)
                outs = dev.run(launch)
                base = outs if base is None else base
                for t, (a, b) in enumerate(zip(outs, base)):
                    assert np.array_equal(_bits(a), _bits(b)), (balance, slot, t)
            if balance:
                continue
            assert (tc.expected_geometry(spec, False)[0] > 8) == (stride == 16)  # the seg form's 16-wave instance
            seg = dev.run(launch.seg_form)
            for t, (a, b, ref) in enumerate(zip(seg, base, refs)):
                assert np.array_equal(_bits(a), _bits(b)), ("seg_form", t)
                assert rel_err(a, ref[0]) <= 1e-5, ("seg_form against float64", t)


# ------------------------------------------------------------------------------ 4: POST
@pytest.mark.parametrize("balance", [False, True])
@pytest.mark.parametrize("share", [True, False])
@pytest.mark.parametrize("stride", [8, 16])
def test_post_projection_rows_against_float64(K, monkeypatch, stride, share, balance):
    """Assertion 4 (dg_gcn_fused_tab_post_f32): every P row within (64 + 3)·2^-24·Σ|terms| of the
    float64 product of the H1 row as stored and its W2 slab; H1 bitwise the launch without jobs;
    unused P slabs and the guard rows untouched.  Relation counts for which the jobs of a full
    workgroup fit its wave slots in both modes: two specs of 3 + 2 relations on the one-row-a-
    workgroup target, 2, 1 and 3 on the others (3 or 4, 4, 1 or 2 rows a workgroup, the last
    workgroup of each with an absent row slot)."""
    shape = (64, 64)
    (spec, targets, _), = _case(shape, stride, "int")
    dev = _Launch(K, targets, 64)
    plain = dev.run(_tab(K, monkeypatch, dev, shape, balance, 0))
    rng = np.random.default_rng(7 + stride)
    jobs = []
    for t, counts in enumerate(((3, 2), (2,), (1,), (3,))):
        for n_rels in counts:
            k_slabs, rows = n_rels + 2, targets[t].n_rows
            slab = rng.permutation(k_slabs)[:n_rels]
            w = rng.integers(-4, 5, size=(k_slabs, 64, 32)).astype(np.float32)
            w[np.setdiff1d(np.arange(k_slabs), slab)] = np.nan
            buf = torch.empty(k_slabs * rows * 32 + 32, device="cuda")
            pj = K.TabProjSpec(t, _dev(w), buf[:k_slabs * rows * 32].view(k_slabs, rows, 32), n_rels,
                               [int(s) for s in slab])
            jobs.append((pj, buf, w, slab))
    launch = _tab(K, monkeypatch, dev, shape, balance, 0, projs=[j[0] for j in jobs], share_proj=share)
    _reached(launch, "dg_gcn_fused_tab_post_f32", spec, balance, 0)
    for _, buf, _, _ in jobs:
        buf.fill_(SENTINEL)
    h1 = dev.run(launch)
    for a, b in zip(h1, plain):
        assert np.array_equal(_bits(a), _bits(b)), "H1 rows of the projecting launch"
    worst = 0.0
    for pj, buf, w, slab in jobs:
        P = buf.cpu().numpy()
        assert np.all(P[-32:] == SENTINEL), "the row past P"
        P = P[:-32].reshape(w.shape[0], -1, 32)
        h = h1[pj.target].astype(np.float64)
        for sl in range(w.shape[0]):
            if sl not in slab:
                assert np.all(P[sl] == SENTINEL), "an unused P slab"
                continue
            wk = w[sl].astype(np.float64)
            bound = 67 * tc.U24 * (np.abs(h) @ np.abs(wk))
            worst = max(worst, _within(P[sl], h @ wk, bound, f"P target {pj.target} slab {sl}"))
    print(f"post stride {stride} share {share} balance {balance}: worst |P - ref| / bound = {worst:.3f}")


# ------------------------------------------------------------------------------ 5: DEC
@pytest.mark.parametrize("balance", [False, True])
@pytest.mark.parametrize("has_l", [True, False])
@pytest.mark.parametrize("stride", [8, 16])
def test_dec_row_operands_against_float64(K, monkeypatch, stride, has_l, balance):
    """Assertion 5 (dg_gcn_fused_tab_dec_f32): Q rows within (32 + 3 + 2)·2^-24·Σ|terms| of the
    float64 l∘((E∘l)·G) of the stored E row, with l and without; E bitwise the plain launch's; the
    Q rows past the target's — where a finishing wave of another, longer target would write — keep
    their sentinel.  The three-target launch flags its second target (3 or 4 rows a workgroup); the
    8-group launch has one target, which it flags."""
    shape = (32, 32)
    rng = np.random.default_rng(11 + stride)
    G = rng.integers(-4, 5, size=(32, 32)).astype(np.float32)
    l = rng.choice(np.float32([-2, -1, -0.5, 0.5, 1, 2]), size=32) if has_l else None
    worst = 0.0
    for (spec, targets, _), target in zip(_case(shape, stride, "int"), (1, 0)):
        dev = _Launch(K, targets, 32)
        plain = dev.run(_tab(K, monkeypatch, dev, shape, balance, 0))
        rows = targets[target].n_rows
        qbuf = torch.full((16 * 32,), SENTINEL, device="cuda")
        dec = K.TabDecSpec(target, _dev(G), None if l is None else _dev(l), qbuf[:rows * 32].view(rows, 32))
        launch = _tab(K, monkeypatch, dev, shape, balance, 0, dec=dec)
        _reached(launch, "dg_gcn_fused_tab_dec_f32", spec, balance, 0)
        E = dev.run(launch)
        for a, b in zip(E, plain):
            assert np.array_equal(_bits(a), _bits(b)), "E rows of the launch that stores Q"
        Q = qbuf.cpu().numpy().reshape(16, 32)
        assert rows < 16 and np.all(Q[rows:] == SENTINEL), "a Q row past the flagged target's"
        e, g64 = E[target].astype(np.float64), G.astype(np.float64)
        lv = np.ones(32) if l is None else l.astype(np.float64)
        want = lv * ((e * lv) @ g64)
        terms = np.abs(lv) * ((np.abs(e) * np.abs(lv)) @ np.abs(g64))
        worst = max(worst, _within(Q[:rows], want, 37 * tc.U24 * terms, f"Q target {target}"))
    print(f"dec stride {stride} l {has_l} balance {balance}: worst |Q - ref| / bound = {worst:.3f}")


# ------------------------------------------------------------------------------ 6: PreparedSegTab
@pytest.mark.parametrize("chunk", [1, 3, 8, 9, 16])
@pytest.mark.parametrize("shape", [(64, 64), (64, 32)])
def test_seg_tab_chunk_partials_exact(K, monkeypatch, shape, chunk):
    """Assertion 6 (dg_spmm_seg_tab_f32 from a PreparedSegTab built here): on the integer set the
    chunk partials are the float64 values themselves and bitwise seg_form()'s, at every slot size;
    two groups, one with a short last chunk (at chunk = 1 no chunk can be short); the row past
    each output untouched."""
    d_in, d_out = shape
    groups = tc.make_seg_groups(chunk, d_in, d_out, "int", 200 + chunk)
    for g in groups:
        tc.assert_exact(g)
    want = [tc.group_sums(g)[0] for g in groups]
    bufs = [torch.empty(w.size + d_out, device="cuda") for w in want]
    specs = [_spec(K, g, out=b) for g, b in zip(groups, bufs)]

    def run(fn):
        for b in bufs:
            b.fill_(float("nan"))
            b[-d_out:] = SENTINEL
        fn()
        torch.cuda.synchronize()
        outs = [b.cpu().numpy() for b in bufs]
        assert all(np.all(o[-d_out:] == SENTINEL) for o in outs), "the row past an output"
        return [o[:-d_out].reshape(w.shape) for o, w in zip(outs, want)]

    for slot in tc.SLOTS[1:]:
        monkeypatch.setenv("DG_TAB_SLOT", str(slot))
        launch = K.PreparedSegTab(specs, d_in, d_out)
        # (PreparedSegTab has the one entry point, dg_spmm_seg_tab_f32: the stride picks the instance)
        assert (launch._tab.nw_stride, launch.nw, launch.slot_pairs) == (8 if chunk <= 8 else 16, chunk, slot)
        tab = run(launch)
        seg = run(launch.seg_form)
        for a, b, w in zip(tab, seg, want):
            assert np.array_equal(a.astype(np.float64), w), (slot, "against float64")
            assert np.array_equal(_bits(a), _bits(b)), (slot, "against seg_form")

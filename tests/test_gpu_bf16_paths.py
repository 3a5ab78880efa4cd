"""GPU: every dispatch path of the bf16 decoders (decoder_bf16.hip) at small shapes, against a
float64 restatement, pair by pair.

The four kernels and who reaches them here:
  decoder_bf16_kernel<D, HAS_L>                       dg_decoder_score_bf16, d = 64 / 128 / 256
  decoder_bf16_colshared_kernel<D, HAS_L, 768, false> dg_decoder_score_bf16_paired at d = 64 / 128, and at
                                                      d = 256 on a table past 2^31 bytes
  decoder_bf16_colshared_kernel<256, true, 768, true> dg_slot_score_hinge_bf16 when batch % 32 != 0, or
                                                      on a table past 2^31 bytes
  decoder_bf16_cs16_kernel<768, FUSED>                dg_slot_score_hinge_bf16 when batch % 32 == 0 (FUSED),
                                                      dg_decoder_score_bf16_paired at d = 256 (not FUSED)

Two data sets make fp32 arithmetic exact in ANY order, so a kernel must return the float64 value
itself, on every pair (compared with ==; no tolerance):
  integer   E in [-2, 2], D_k in {±1, ±2}, R in {-1, 0, 1}: every product and partial sum is an
            integer below 2^20 — a dropped, doubled or misrouted product changes the score;
  rounding  the side whose product with D_k is rounded to bf16 (the MFMA's B operand: D_k∘v for
            the column-shared kernels, u∘D_k for dg_decoder_score_bf16) and D_k are ±k/128,
            k in [128, 256): ≈ 97 % of the products need rounding and ≈ 2.5 % are ties, so
            truncation (or rounding ties away) changes the scores; R has two ±1 per row and the
            other side 32 ±1 per row, so every term is a multiple of 2^-14 with Σ|terms| < 2^9.
The preconditions (Σ|terms| below 2^24 units) are asserted on the host before each launch.
A third, random-normal set is inexact; there every pair must lie within 2d·2^-23·A_p of the
float64 value, A_p = Σ_i Σ_n |u_i D_k[i] R[i][n] b_n|: a term passes through at most 2d rounded
additions (d in the MFMA chain, fewer than d in the epilogue and its butterfly), each off by at
most 2^-23 of its result even in a truncating accumulator.

The fused step's loss is compared with the float64 sum of relu(neg − (pos − margin)) formed in
fp32 from the device's own scores: within N·2^-24 of it, N = 6 (the tile's butterfly) + rounds
(the wave's tiles) + 12 (the workgroup's waves) + 10 (the block-order sum).  (That last sum is
serial, a term of block 0 passing through every later block's addition — up to 255 of them in
the 3,077- and 3,079-tile cases; the bound stays at the smaller figure, tighter than a serial
sum's worst case.  On the MI355X the largest error seen over all cases is 9.1·2^-24 of the sum,
in a 3,079-tile case, against N = 30.)  On random data the largest score error is 4e-4 of its
bound, and with batch % 32 != 0 the fused and three-launch scores differ in bits on ≈ 86 % of
pairs (another kernel template); they are bit-equal in every other case.
"""
from dataclasses import dataclass

import numpy as np
import pytest

from conftest import alias_draws

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SEED = 11            # the sampler's
D256 = 256
U23 = 2.0 ** -23
KINDS = ("integer", "rounding", "random")


def _device():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda")


# ------------------------------------------------------------------------------ data sets
def _bf16_rne(x):
    """float32 array -> nearest bf16 (ties to even) as float64, by torch's CPU cast."""
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    return t.to(torch.bfloat16).double().numpy()


def _signed_picks(rng, n, d, per_row):
    """[n, d] with exactly per_row entries ±1 in each row, the rest 0."""
    out = np.zeros((n, d), np.float32)
    cols = rng.permuted(np.tile(np.arange(d), (n, 1)), axis=1)[:, :per_row]
    out[np.arange(n)[:, None], cols] = rng.choice(np.float32([-1, 1]), size=(n, per_row))
    return out


def _k128(rng, shape):
    """±k/128, k in [128, 256): 8 significant bits, so exact in bf16."""
    return (rng.choice(np.float32([-1, 1]), size=shape) * rng.integers(128, 256, size=shape) / 128).astype(np.float32)


def _dataset(kind, seed, n_r, n_c, n_rel, d, side="col"):
    """Er [n_r, d] (row side), Ec [n_c, d] (column side), R [d, d], D [n_rel, d]: float32 arrays
    of bf16-representable values.  side: whose product with D_k the kernel rounds to bf16."""
    rng = np.random.default_rng(seed)
    if kind == "integer":
        Er = rng.integers(-2, 3, (n_r, d)).astype(np.float32)
        Ec = rng.integers(-2, 3, (n_c, d)).astype(np.float32)
        D = rng.choice(np.float32([-2, -1, 1, 2]), size=(n_rel, d))
        R = rng.integers(-1, 2, (d, d)).astype(np.float32)
    elif kind == "rounding":
        D = _k128(rng, (n_rel, d))
        R = _signed_picks(rng, d, d, 2)
        if side == "col":
            Er, Ec = _signed_picks(rng, n_r, d, 32), _k128(rng, (n_c, d))
        else:
            Er, Ec = _k128(rng, (n_r, d)), _signed_picks(rng, n_c, d, 32)
    else:
        Er, Ec, D = (_bf16_rne(rng.standard_normal(s)).astype(np.float32) for s in ((n_r, d), (n_c, d), (n_rel, d)))
        R = _bf16_rne(rng.standard_normal((d, d)) / 16).astype(np.float32)
    for x in (Er, Ec, D, R):
        assert np.array_equal(_bf16_rne(x), x)  # the upload to bf16 changes nothing
    return dict(kind=kind, Er=Er, Ec=Ec, R=R, D=D, side=side)


def _assert_rounds(ds):
    """The rounding set does what it is for: most operand products are not bf16 values, some are
    ties, and truncation would give other operands."""
    D = ds["D"][:8].astype(np.float64)
    prod = (D[:, None, :] * (ds["Ec"] if ds["side"] == "col" else ds["Er"])[None].astype(np.float64)).ravel()
    rne = _bf16_rne(prod.astype(np.float32))  # (the products have 16 significant bits: exact in fp32)
    trunc = (prod.astype(np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    assert np.mean(rne != prod) > 0.9
    assert np.mean(rne != trunc) > 0.4
    ulp = 2.0 ** (np.floor(np.log2(np.abs(prod))) - 7)
    assert np.mean(np.abs(rne - prod) == ulp / 2) > 0.01  # exact ties


def _chunks(n, step=1 << 14):
    return [slice(s, min(n, s + step)) for s in range(0, n, step)]


def _ref_colshared(ds, rows_p, rows_n, cols, rel, use_l=True):
    """Column-shared kernels (paired and fused): y = Σ_i u_i·D_k[i]·Σ_n R[i][n]·b_n with
    b = bf16_rne(D_k∘v), for the positive rows and the negative rows of the same (v, k); float64.
    Returns (y_pos, A_pos, y_neg, A_neg), A = Σ|terms|."""
    R = ds["R"].astype(np.float64)
    Ra = np.abs(R)
    n = len(cols)
    out = [np.empty(n) for _ in range(4)]
    for c in _chunks(n):
        dk = ds["D"][rel[c]] if use_l else np.ones((len(cols[c]), R.shape[0]), np.float32)
        b = _bf16_rne(dk * ds["Ec"][cols[c]])  # the fp32 product of two bf16 values is exact
        T, Ta = b @ R.T, np.abs(b) @ Ra.T
        for k, rows in enumerate((rows_p, rows_n)):
            a = ds["Er"][rows[c]].astype(np.float64) * dk
            out[2 * k][c] = np.einsum("pi,pi->p", a, T)
            out[2 * k + 1][c] = np.einsum("pi,pi->p", np.abs(a), Ta)
    return out


def _ref_rowside(ds, rows, cols, rel, use_l=True):
    """dg_decoder_score_bf16: the bf16 rounding sits on u∘D_k; y = Σ_n (Σ_i a_i R[i][n])·D_k[n]·v_n."""
    R = ds["R"].astype(np.float64)
    dk = ds["D"][rel] if use_l else np.ones((len(rows), R.shape[0]), np.float32)
    a = _bf16_rne(ds["Er"][rows] * dk)
    c = dk.astype(np.float64) * ds["Ec"][cols]
    return np.einsum("pn,pn->p", a @ R, c), np.einsum("pn,pn->p", np.abs(a) @ np.abs(R), np.abs(c))


def _assert_exact_precondition(kind, y, A):
    """fp32 sums of the terms are exact in any order: all terms are multiples of one unit and
    every partial sum stays below 2^24 units."""
    unit = 1.0 if kind == "integer" else 2.0 ** -14
    assert np.all(A / unit < 2.0 ** 24)
    assert np.array_equal(np.round(y / unit) * unit, y)
    assert np.array_equal(y.astype(np.float32).astype(np.float64), y)


def _assert_scores(kind, d, got, y, A, what):
    got = got.astype(np.float64)
    if kind == "random":
        err, tol = np.abs(got - y), 2 * d * U23 * A
        bad = np.flatnonzero(~(err <= tol))
        assert bad.size == 0, (what, bad[:8], err[bad[:8]], tol[bad[:8]])
    else:
        _assert_exact_precondition(kind, y, A)
        bad = np.flatnonzero(got != y)
        assert bad.size == 0, (what, bad.size, bad[:8], got[bad[:8]], y[bad[:8]])


def _up(x, dev):
    return torch.from_numpy(x).to(torch.bfloat16).to(dev)


# ------------------------------------------------------------------------------ the fused step
@dataclass(frozen=True)
class Fused:
    batch: int
    n_slots: int
    slot0: int
    alias: str           # "slot": [n, range, 2]; "shared": one [range, 2]
    range: int
    one_table: bool = False   # E_row is E_col
    id: str = ""


FUSED_CASES = [
    # the 16x16x32 kernel (batch % 32 == 0): every tile in one slot
    Fused(32, 3, 0, "slot", 5, id="cs16-32x3-range5"),              # 3 tiles, 9 idle waves
    Fused(32, 13, 2, "slot", 40, id="cs16-32x13-slot0-2"),          # 2 workgroups, round-major order
    Fused(64, 7, 3, "shared", 20, True, id="cs16-64x7-shared-onetable"),
    Fused(32, 3077, 0, "slot", 8, id="cs16-32x3077-second-round"),  # 3,077 tiles > 256·12
    Fused(32, 2, 0, "slot", 1, id="cs16-32x2-range1"),              # every negative is row 0
    # the 32x32x16 column-shared kernel (batch % 32 != 0): tiles straddle slots, ragged last tile
    Fused(1, 70, 0, "slot", 40, id="colshared-1x70"),               # a relation per pair, tail 6
    Fused(37, 5, 2, "slot", 17, id="colshared-37x5-slot0-2"),       # tail 25
    Fused(7, 1, 0, "shared", 40, id="colshared-7x1-shared"),        # one partial tile
    Fused(500, 3, 0, "shared", 33, id="colshared-500x3-shared"),
    Fused(33, 2985, 0, "slot", 8, id="colshared-33x2985-second-round"),  # 3,079 tiles
]


def _alias_tables(rng, n, rng_):
    from decagon_amd.sampling import alias_table

    deg = rng.integers(0, 50, (n, rng_)).astype(np.float64)
    deg[:, rng.integers(0, rng_)] += 1  # (a positive sum; zero-degree rows are never drawn)
    return np.stack([alias_table(x) for x in deg])


class FusedProblem:
    """One fused case on one data set: host arrays, device tensors, and the layout that says
    which table rows are row-side rows (rows_r; the first `range` of them are the sampler's
    rows 0 .. range−1) and which column-side rows (rows_c)."""

    def __init__(self, c, kind, dev, seed, big=None):
        self.c, self.kind, self.dev = c, kind, dev
        rng = np.random.default_rng(seed)
        self.total = c.slot0 + c.n_slots + 1  # one more relation behind the launch's last
        if big is not None:
            self.rows_r, self.rows_c = np.array(BIG_ROWS_R), np.array(BIG_ROWS_C)
        elif c.one_table:
            self.rows_r, self.rows_c = np.arange(20), np.arange(20, 40)
        else:
            self.rows_r, self.rows_c = np.arange(40), np.arange(30)
        assert c.range <= len(self.rows_r) and np.array_equal(self.rows_r[:c.range], np.arange(c.range))
        self.ds = _dataset(kind, seed + 1, len(self.rows_r), len(self.rows_c), self.total, D256)
        if kind == "rounding":
            _assert_rounds(self.ds)
        B, nt = c.batch, self.total * c.batch
        self.ri = rng.integers(0, len(self.rows_r), nt)  # positions in rows_r / rows_c
        self.ci = rng.integers(0, len(self.rows_c), nt)
        if big is not None:  # the last row of the table, and a row just past 2^31 bytes, are among the pairs
            at = c.slot0 * c.batch
            self.ci[at], self.ri[at], self.ri[at + 1] = len(self.rows_c) - 1, len(self.rows_r) - 1, len(self.rows_r) - 4
        if big is not None or c.one_table:
            if big is not None:
                self.E_row = self.E_col = big
            else:
                self.E_row = self.E_col = torch.empty((40, D256), dtype=torch.bfloat16, device=dev)
            self.E_row[torch.from_numpy(self.rows_r).to(dev)] = _up(self.ds["Er"], dev)
            self.E_row[torch.from_numpy(self.rows_c).to(dev)] = _up(self.ds["Ec"], dev)
        else:
            self.E_row, self.E_col = _up(self.ds["Er"], dev), _up(self.ds["Ec"], dev)
        self.R, self.D = _up(self.ds["R"], dev), _up(self.ds["D"], dev)
        self.pos_rows = torch.from_numpy(self.rows_r[self.ri].astype(np.int32)).to(dev)
        self.pos_cols = torch.from_numpy(self.rows_c[self.ci].astype(np.int32)).to(dev)
        n_tab = self.total if c.alias == "slot" else 1
        self.tables = _alias_tables(rng, n_tab, c.range)           # uint32 [n_tab, range, 2]
        t = torch.from_numpy(self.tables.view(np.int32)).to(dev)
        self.alias = t if c.alias == "slot" else t[0].contiguous()
        self.n = c.n_slots * B
        self.lo, self.hi = c.slot0 * B, (c.slot0 + c.n_slots) * B
        self.rel = np.repeat(np.arange(c.slot0, c.slot0 + c.n_slots), B)

    def launch(self, margin):
        from decagon_amd import kernels

        n = self.n
        out = torch.full((2 * n + 64,), float("nan"), dtype=torch.float32, device=self.dev)
        neg = torch.full((n + 64,), -1, dtype=torch.int32, device=self.dev)
        loss = torch.full((1,), float("nan"), dtype=torch.float32, device=self.dev)
        ws = kernels.hinge_workspace(self.dev)
        c = self.c

        def go():
            # (the pairs of the relation behind the last follow in memory: never read)
            kernels.slot_score_hinge_bf16(self.E_row, self.E_col, self.pos_rows[self.lo:],
                                          self.pos_cols[self.lo:], self.alias, c.slot0, c.n_slots, c.batch,
                                          SEED, self.R, self.D, margin, out, neg, loss, ws)
            torch.cuda.synchronize()
            return out.cpu().numpy(), neg.cpu().numpy(), loss.cpu().numpy()[0], int(ws[0])

        return go

    def want_draws(self):
        c, B = self.c, self.c.batch
        want = np.empty(self.n, np.int32)
        for s in range(c.n_slots):
            k = c.slot0 + s
            tab = self.tables[k if c.alias == "slot" else 0]
            want[s * B:(s + 1) * B] = alias_draws(tab, SEED, k * B + np.arange(B))
        return want

    def loss_terms_n(self):
        """Additions on a loss term's path: 6 (tile butterfly) + rounds + 12 (waves) + 10."""
        from decagon_amd import _lib

        n_tiles = -(-self.n // 32)
        blocks = min(-(-n_tiles // 12), (_lib.DG_HINGE_WS_BYTES - 16) // 4)
        return 6 + -(-n_tiles // (blocks * 12)) + 12 + 10


def _check_loss(loss, out, n, margin, N):
    pos, neg = out[:n], out[n:2 * n]
    terms = np.maximum(neg - (pos - np.float32(margin)), np.float32(0))  # fp32, as the kernel forms them
    assert terms.dtype == np.float32
    s = terms.astype(np.float64).sum()
    assert abs(float(loss) - s) <= N * 2.0 ** -24 * s, (float(loss), s, N)


def _check_fused(p):
    from decagon_amd import kernels
    from decagon_amd.scorer import SlotScorer

    c, n, d = p.c, p.n, D256
    go = p.launch(0.125)
    out, neg, loss, ticket = go()
    # every entry written, nothing behind them touched
    assert np.all(np.isnan(out[2 * n:])) and np.all(neg[n:] == -1)
    assert not np.any(np.isnan(out[:2 * n]))
    assert neg[:n].min() >= 0 and neg[:n].max() < c.range
    # the draws: slot k's table at counter k·batch + i, and the stand-alone sampler's, bit for bit
    assert np.array_equal(neg[:n], p.want_draws())
    alone = kernels.unigram_sample_slots(p.alias, c.slot0, c.batch, n, SEED)
    assert np.array_equal(neg[:n], alone.cpu().numpy())
    if c.range == 1:
        assert np.all(neg[:n] == 0)
    # the scores of every pair
    yp, Ap, yn, An = _ref_colshared(p.ds, p.ri[p.lo:p.hi], neg[:n], p.ci[p.lo:p.hi], p.rel)
    _assert_scores(p.kind, d, out[:n], yp, Ap, "pos")
    _assert_scores(p.kind, d, out[n:2 * n], yn, An, "neg")
    # the loss, on the device's own scores; the same bits on every launch; the ticket reset
    N = p.loss_terms_n()
    _check_loss(loss, out, n, 0.125, N)
    assert ticket == 0
    for _ in range(3):
        out2, neg2, loss2, ticket2 = go()
        assert np.float32(loss2).tobytes() == np.float32(loss).tobytes()
        assert np.array_equal(out2[:2 * n], out[:2 * n]) and np.array_equal(neg2, neg) and ticket2 == 0
        assert np.all(np.isnan(out2[2 * n:]))
    out15, _, loss15, _ = p.launch(1.5)()
    assert np.array_equal(out15[:2 * n], out[:2 * n])
    _check_loss(loss15, out15, n, 1.5, N)
    assert np.all(yn - yp < 9e5)  # (so every term at margin −1e6 is negative before the relu)
    _, _, loss_far, _ = p.launch(-1e6)()
    assert np.float32(loss_far).tobytes() == np.float32(0.0).tobytes()
    # the three-launch form of the same step
    three = SlotScorer(p.E_row, p.E_col, p.R, p.D, p.pos_rows, p.pos_cols, p.alias, c.batch, 0.125, seed=SEED,
                       slots=(c.slot0, c.slot0 + c.n_slots), fused=False)
    three()
    torch.cuda.synchronize()
    assert np.array_equal(three.neg_rows.cpu().numpy(), neg[:n])
    out3 = three.out.cpu().numpy()
    big = p.E_row.shape[0] > 1 << 22
    if p.kind != "random" or big or c.batch % 32 == 0:
        # exact sets: both equal the reference.  Random data: the same bits where both forms run
        # one kernel template (the 16x16x32 one, or on the big table the 32x32x16 one)
        assert np.array_equal(out3, out[:2 * n])
    else:
        # the fused call runs the 32x32x16 kernel, the paired call the 16x16x32 one: another
        # accumulation order, each within its own bound of the float64 value
        tol = 2 * (2 * d * U23 * np.concatenate([Ap, An]))
        assert np.all(np.abs(out3.astype(np.float64) - out[:2 * n]) <= tol)
        _assert_scores(p.kind, d, out3[:n], yp, Ap, "pos, three launches")
        _assert_scores(p.kind, d, out3[n:], yn, An, "neg, three launches")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", FUSED_CASES, ids=lambda c: c.id)
def test_fused_step_every_pair(case, kind):
    dev = _device()
    _check_fused(FusedProblem(case, kind, dev, seed=100 + FUSED_CASES.index(case)))


def test_fused_step_no_slots():
    """n_slots == 0: the loss becomes 0, nothing else is written."""
    dev = _device()
    p = FusedProblem(Fused(32, 0, 1, "slot", 5), "integer", dev, seed=7)
    out, neg, loss, ticket = p.launch(0.125)()
    assert np.float32(loss).tobytes() == np.float32(0.0).tobytes()
    assert np.all(np.isnan(out)) and np.all(neg == -1) and ticket == 0


# ------------------------------------------------------------------------------ a table past 2^31 bytes
BIG_N = 4_200_000                 # rows of 512 bytes: 2.15 GB
_HI = (1 << 31) // (2 * D256)     # the first row whose byte offset needs bit 31
BIG_ROWS_R = list(range(20)) + [20, 1_000_003, _HI // 2 - 1, _HI - 1, _HI, _HI + 2, BIG_N - 1000, BIG_N - 2]
BIG_ROWS_C = [21, 22, 23, 24, 777_777, _HI // 2, 3_000_001, _HI + 1, _HI + 3, BIG_N - 999, BIG_N - 3, BIG_N - 1]


@pytest.fixture(scope="module")
def big_table():
    """One bf16 [4,200,000, 256] table (uninitialised: the tests write the ≈ 40 rows they use,
    the last row among them), row and column table at once."""
    dev = _device()
    free, _ = torch.cuda.mem_get_info()
    if free < 8 << 30:
        pytest.skip("under 8 GiB of device memory free")
    t = torch.empty((BIG_N, D256), dtype=torch.bfloat16, device=dev)
    assert t.numel() * 2 > 1 << 31
    yield t
    del t
    torch.cuda.empty_cache()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", [Fused(32, 3, 0, "slot", 20, id="big-32x3"),
                                  Fused(37, 5, 2, "slot", 20, id="big-37x5")], ids=lambda c: c.id)
def test_fused_step_big_table(big_table, case, kind):
    """Tables past 32-bit byte offsets: the fused call runs the 64-bit addressed 32x32x16 kernel
    whatever the batch, and so does the three-launch form."""
    _check_fused(FusedProblem(case, kind, big_table.device, seed=300 + case.batch, big=big_table))


@pytest.mark.parametrize("use_l", [True, False], ids=["l_table", "identity"])
@pytest.mark.parametrize("kind", KINDS)
def test_paired_big_table(big_table, kind, use_l):
    """dg_decoder_score_bf16_paired at d = 256 on the big table: decoder_bf16_colshared_kernel<256, *, 768, false>."""
    dev, nh, n_rel = big_table.device, 45, 5
    rows_r, rows_c = np.array(BIG_ROWS_R), np.array(BIG_ROWS_C)
    ds = _dataset(kind, 400 + use_l, len(rows_r), len(rows_c), n_rel, D256)
    big_table[torch.from_numpy(rows_r).to(dev)] = _up(ds["Er"], dev)
    big_table[torch.from_numpy(rows_c).to(dev)] = _up(ds["Ec"], dev)
    rng = np.random.default_rng(401)
    ri, ci, rel = rng.integers(0, len(rows_r), 2 * nh), rng.integers(0, len(rows_c), nh), rng.integers(0, n_rel, nh)
    ri[:2], ci[:2] = (len(rows_r) - 1, len(rows_r) - 4), (len(rows_c) - 1, len(rows_c) - 5)  # rows past 2^31 bytes
    got = _run_paired(dev, big_table, big_table, rows_r[ri], rows_c[ci], rel, ds, use_l)
    yp, Ap, yn, An = _ref_colshared(ds, ri[:nh], ri[nh:], ci, rel, use_l)
    _assert_scores(kind, D256, got[:nh], yp, Ap, "pos")
    _assert_scores(kind, D256, got[nh:2 * nh], yn, An, "neg")
    assert np.all(np.isnan(got[2 * nh:]))


# ------------------------------------------------------------------------------ the score-only entry points
def _run_paired(dev, E_row, E_col, rows, cols, rel, ds, use_l):
    from decagon_amd import kernels

    nh = len(cols)
    i32 = lambda x: torch.from_numpy(np.asarray(x, np.int32)).to(dev)  # noqa: E731
    out = torch.full((2 * nh + 64,), float("nan"), dtype=torch.float32, device=dev)
    # (cols / rel are read for the first half only; the second half here would give other scores)
    cols2 = i32(np.concatenate([cols, np.zeros(nh)]))
    rel2 = i32(np.concatenate([rel, np.zeros(nh)]))
    kernels.decoder_score_bf16(E_row, E_col, i32(rows), cols2, _up(ds["R"], dev), _up(ds["D"], dev) if use_l else None,
                               rel2 if use_l else None, out=out, paired=True)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("use_l", [True, False], ids=["l_table", "identity"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("d", [64, 128, 256])
def test_paired_every_pair(d, kind, use_l):
    """dg_decoder_score_bf16_paired, n_half = 45 (a ragged second tile), relations mixed inside a
    tile: the 32x32x16 column-shared kernel at d = 64 / 128, the 16x16x32 one at d = 256."""
    dev = _device()
    nh, n_rel = 45, 5
    ds = _dataset(kind, 500 + d + use_l, 40, 30, n_rel, d)
    if kind == "rounding":
        _assert_rounds(ds)
    rng = np.random.default_rng(501 + d)
    ri, ci, rel = rng.integers(0, 40, 2 * nh), rng.integers(0, 30, nh), rng.integers(0, n_rel, nh)
    got = _run_paired(dev, _up(ds["Er"], dev), _up(ds["Ec"], dev), ri, ci, rel, ds, use_l)
    yp, Ap, yn, An = _ref_colshared(ds, ri[:nh], ri[nh:], ci, rel, use_l)
    _assert_scores(kind, d, got[:nh], yp, Ap, "pos")
    _assert_scores(kind, d, got[nh:2 * nh], yn, An, "neg")
    assert np.all(np.isnan(got[2 * nh:]))


@pytest.mark.parametrize("use_l", [True, False], ids=["l_table", "identity"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("d", [64, 128, 256])
def test_rowside_every_pair(d, kind, use_l):
    """dg_decoder_score_bf16 (decoder_bf16_kernel<D, HAS_L>), n = 77 (three tiles, the last of 13
    pairs), relations mixed inside a tile; the bf16 rounding sits on u∘D_k, so the rounding
    set's roles of E_row and E_col are swapped."""
    from decagon_amd import kernels

    dev = _device()
    n, n_rel = 77, 5
    ds = _dataset(kind, 600 + d + use_l, 40, 30, n_rel, d, side="row")
    if kind == "rounding":
        _assert_rounds(ds)
    rng = np.random.default_rng(601 + d)
    ri, ci, rel = rng.integers(0, 40, n), rng.integers(0, 30, n), rng.integers(0, n_rel, n)
    i32 = lambda x: torch.from_numpy(np.asarray(x, np.int32)).to(dev)  # noqa: E731
    out = torch.full((n + 64,), float("nan"), dtype=torch.float32, device=dev)
    kernels.decoder_score_bf16(_up(ds["Er"], dev), _up(ds["Ec"], dev), i32(ri), i32(ci), _up(ds["R"], dev),
                               _up(ds["D"], dev) if use_l else None, i32(rel) if use_l else None, out=out)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    y, A = _ref_rowside(ds, ri, ci, rel, use_l)
    _assert_scores(kind, d, got[:n], y, A, "score")
    assert np.all(np.isnan(got[n:]))

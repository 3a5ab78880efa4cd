"""CPU: oracle.dropout_scale — the restatement every dropout test compares the device with — pinned on
its own: against a scalar restatement in Python integers written from the comment at the top of
csrc/dropout.h (not from the oracle's numpy code), at the edges of keep, and for the property
dropout.hip's header says the hash restates (every element kept independently with probability keep,
a fresh draw per step, group and layer).

The statistical bounds are conditions, not measurements: 5 standard deviations for a kept fraction
(sd = sqrt(keep·(1 - keep)/n)) and 5/sqrt(n) for a correlation coefficient of n samples (sd 1/sqrt(n)
under independence), over about 200 comparisons at n = 2^20 with fixed seeds — deterministic."""
import itertools

import numpy as np
import pytest

from oracle import decagon_oracle as orc

M32 = 0xFFFFFFFF
# (seed, step, tag): zeros; the values test_gpu_train uses; every field past its device width (the device
# truncates step and tag to 32 bits and splits the 64-bit seed into halves); a training tag (layer 2, group 3)
TRIPLES = [(0, 0, 0), (123456789012, 5, 77), (2 ** 64 - 1, 2 ** 32 + 3, 0xFFFFFFFF), (20180701, 1, (2 << 16) | 3)]


def _lowbias32(x: int) -> int:
    x &= M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x


def _key(seed: int, step: int, tag: int) -> int:
    seed_lo, seed_hi = seed & M32, (seed >> 32) & M32
    step, tag = step & M32, tag & M32
    return _lowbias32(_lowbias32(seed_lo ^ ((tag * 0x9E3779B9) & M32)) ^ ((seed_hi + step * 0x85EBCA6B) & M32))


def _scalar_scale(seed: int, step: int, tag: int, n: int, keep: float) -> np.ndarray:
    """Element by element in Python integers: kept iff the top 24 bits of lowbias32(key ^ idx) are below
    keep·2^24 (keep as float32; the product by 2^24 is exact), a kept element scaled by the float32 1/keep."""
    key = _key(seed, step, tag)
    thr = int(float(np.float32(keep)) * 16777216.0)
    inv = np.float32(1.0) / np.float32(keep)
    return np.array([inv if (_lowbias32(key ^ idx) >> 8) < thr else np.float32(0.0) for idx in range(n)], np.float32)


@pytest.mark.parametrize("seed,step,tag", TRIPLES)
def test_scalar_restatement(seed, step, tag):
    n = 3001
    for keep in (0.9, 0.5, 0.1):
        got = orc.dropout_scale(seed, step, tag, n, keep)
        assert got.dtype == np.float32
        assert np.array_equal(got, _scalar_scale(seed, step, tag, n, keep)), (seed, step, tag, keep)


def test_truncation_is_the_devices():
    """step and tag enter in their low 32 bits only, the seed in both halves."""
    n = 4096
    a = orc.dropout_scale(2 ** 64 - 1, 2 ** 32 + 3, 0xFFFFFFFF, n, 0.5)
    assert np.array_equal(a, orc.dropout_scale(2 ** 64 - 1, 3, 0xFFFFFFFF, n, 0.5))
    assert not np.array_equal(a, orc.dropout_scale(2 ** 32 - 1, 3, 0xFFFFFFFF, n, 0.5))  # the high half counts
    assert not np.array_equal(a, orc.dropout_scale(2 ** 64 - 1, 4, 0xFFFFFFFF, n, 0.5))


def test_keep_edges():
    n = 1 << 16
    for seed, step, tag in TRIPLES:
        one = orc.dropout_scale(seed, step, tag, n, 1.0)
        assert np.array_equal(one.view(np.uint32), np.full(n, np.float32(1.0).view(np.uint32)))
        for tiny in (2.0 ** -25, 2.0 ** -24 * 0.999, 1e-30):  # keep·2^24 < 1: the threshold is 0
            assert not orc.dropout_scale(seed, step, tag, n, tiny).any()
        s = orc.dropout_scale(seed, step, tag, n, 0.8)
        inv = np.float32(1) / np.float32(0.8)
        assert s.dtype == np.float32 and set(np.unique(s).tolist()) == {0.0, float(inv)}
        assert np.array_equal(np.unique(s)[1:].view(np.uint32), np.array([inv]).view(np.uint32))


# the streams of one training run — two consecutive steps, two groups of one layer, layer 1 against
# layer 2 — and the three edge triples
STREAMS = {
    "step1": (20180701, 1, (1 << 16) | 0),
    "step2": (20180701, 2, (1 << 16) | 0),
    "group1": (20180701, 1, (1 << 16) | 1),
    "layer2": (20180701, 1, (2 << 16) | 0),
    "zeros": TRIPLES[0],
    "mid": TRIPLES[1],
    "wide": TRIPLES[2],
}
N = 1 << 20
BOUND = 5.0


def _corr(a, b):
    a = a - a.mean()
    b = b - b.mean()
    return float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum()))


@pytest.mark.parametrize("keep", [0.9, 0.7, 0.5, 0.1])
def test_distribution(keep):
    kept = {name: (orc.dropout_scale(*t, N, keep) != 0).astype(np.float64) for name, t in STREAMS.items()}
    worst_f = worst_c = 0.0
    sd = np.sqrt(keep * (1.0 - keep) / N)
    for name, x in kept.items():
        z = abs(x.mean() - keep) / sd
        worst_f = max(worst_f, z)
        assert z <= BOUND, ("fraction", name, keep, z)
    lim = BOUND / np.sqrt(N)
    for a, b in itertools.combinations(kept, 2):
        c = _corr(kept[a], kept[b])
        worst_c = max(worst_c, abs(c) * np.sqrt(N))
        assert abs(c) <= lim, ("correlation", a, b, keep, c * np.sqrt(N))
    for name, x in kept.items():
        for lag in (1, 64, 4096, N // 4):
            c = _corr(x[:-lag], x[lag:])
            worst_c = max(worst_c, abs(c) * np.sqrt(N))
            assert abs(c) <= lim, ("autocorrelation", name, lag, keep, c * np.sqrt(N))
    print(f"keep {keep}: worst fraction {worst_f:.2f} sd, worst correlation {worst_c:.2f}/sqrt(n)")

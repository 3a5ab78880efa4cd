// A stateless keyed permutation of [0, n): the per-epoch shuffle of a relation's training edges,
// computed per element where it is needed (epochs.hip) — no shuffled copy is kept.
//
// perm(n, key, x), 1 <= n < 2^31, 0 <= x < n: an 8-round Feistel network over the w = bit_length(n − 1)
// bits that cover [0, n), with cycle walking (re-encrypt while the result is >= n).  The halves are
// unequal where w is odd — the low ⌊w/2⌋ bits and the high ⌈w/2⌉ bits — and the rounds alternate
// between them (hi ^= F(lo), lo ^= F(hi), …: every round is its own inverse, so the network is a
// bijection on [0, 2^w) for any widths, a zero-width half included), so the domain 2^w is below 2n
// and an element walks fewer than two times on average.  Round r's function is
// F_r(v) = lowbias32(v ^ rk_r), rk_r = lowbias32(key + (r + 1)·0x9E3779B9), truncated to the half it
// is added to.  n = 1 has the one permutation.
//
// epoch_key(seed, epoch, slot): the key of global relation slot `slot` in epoch `epoch`, mixed as
// dropout.h's drop_key mixes (seed, step, tag).
//
// The numpy restatement is decagon_amd/epochs.py (perm, epoch_key); tests/test_cpu_epochs.py holds
// the two to the same integers through dg_epoch_perm_host / dg_epoch_key_host.
#pragma once

#include <stdint.h>

#include "dropout.h"

namespace dg {

constexpr int kPermRounds = 8;

__host__ __device__ __forceinline__ uint32_t epoch_key(uint64_t seed, uint32_t epoch, uint32_t slot) {
    return lowbias32(lowbias32(static_cast<uint32_t>(seed) ^ (slot * 0x9E3779B9U)) ^
                     (static_cast<uint32_t>(seed >> 32) + epoch * 0x85EBCA6BU));
}

// bits that cover [0, n): the smallest w with 2^w >= n (0 for n = 1)
__host__ __device__ __forceinline__ int perm_bits(uint32_t n) {
    int w = 0;
    while (w < 31 && (1u << w) < n) ++w;
    return w;
}

__host__ __device__ __forceinline__ uint32_t perm(uint32_t n, uint32_t key, uint32_t x) {
    if (n <= 1) return 0;
    const int w = perm_bits(n);
    const int lw = w >> 1, hw = w - lw;
    const uint32_t lmask = (1u << lw) - 1u, hmask = (1u << hw) - 1u;
    uint32_t rk[kPermRounds];
#pragma unroll
    for (int r = 0; r < kPermRounds; ++r) rk[r] = lowbias32(key + static_cast<uint32_t>(r + 1) * 0x9E3779B9U);
    uint32_t y = x;
    do {
        uint32_t lo = y & lmask, hi = y >> lw;
#pragma unroll
        for (int r = 0; r < kPermRounds; ++r) {
            if ((r & 1) == 0)
                hi ^= lowbias32(lo ^ rk[r]) & hmask;
            else
                lo ^= lowbias32(hi ^ rk[r]) & lmask;
        }
        y = (hi << lw) | lo;
    } while (y >= n);
    return y;
}

}  // namespace dg

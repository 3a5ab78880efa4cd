// One wave's running top-k list in LDS and its total-order 64-bit keys, shared by topk.hip (the
// best pairs of every relation), profile.hip (the best columns of every row) and nodetopk.hip (the
// keys of its per-row lists, WaveTopK in its merge); rank_walk.h takes wave_lds_sync from here.
//
// A candidate is one key, (monotone map of the score's bits) << 32 | ~index: unsigned comparison
// orders by higher score, then smaller index (−0 is made +0 first).  Keys are unique, and a key is
// only ever dropped when topk larger keys exist, so a selection is unique whatever the tiling.
#pragma once
#include "common.h"

namespace dg {

// List capacity: twice the power of two ≥ max(topk, 64), so that after a truncation to topk at
// least 64 slots (one wave-wide append) are free.
inline int list_cap(int topk) {
    int kp = 64;
    while (kp < topk) kp <<= 1;
    return 2 * kp;
}

// Orders one wave's LDS accesses: its DS instructions execute in issue order, so all this has to
// do is complete them and keep the compiler from moving accesses across.
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ uint64_t make_key(float s, uint32_t lin) {
    uint32_t b = __float_as_uint(s);
    if (b == 0x80000000u) b = 0u;  // −0 → +0
    const uint32_t mono = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    return ((uint64_t)mono << 32) | (uint32_t)~lin;
}

__device__ __forceinline__ float key_score(uint64_t key) {
    const uint32_t mono = (uint32_t)(key >> 32);
    return __uint_as_float((mono & 0x80000000u) ? (mono ^ 0x80000000u) : ~mono);
}

// Bitonic sort, descending, of cap (a power of two ≥ 128) keys in LDS by one wave.
__device__ __forceinline__ void wave_sort_desc(uint64_t* buf, int cap, int lane) {
#pragma unroll 1
    for (int k = 2; k <= cap; k <<= 1) {
#pragma unroll 1
        for (int j = k >> 1; j > 0; j >>= 1) {
#pragma unroll 1
            for (int t = lane; t < cap / 2; t += dg::kWave) {
                const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const int hi = lo | j;
                const bool desc = (lo & k) == 0;
                const uint64_t x = buf[lo], y = buf[hi];
                if (desc ? (x < y) : (x > y)) {
                    buf[lo] = y;
                    buf[hi] = x;
                }
            }
            wave_lds_sync();
        }
    }
}

// One wave's running top-k: an unsorted list of n ≤ cap keys in LDS, all above thr.  n and thr are
// wave-uniform.  Valid keys are ≥ 1 (the index half is never 0: lin < 2³² − 1), so 0 is padding
// and thr = 0 admits everything.
struct WaveTopK {
    uint64_t* buf;
    uint64_t thr;
    int cap, topk, n, lane;

    __device__ __forceinline__ void init(uint64_t* b, int cap_, int topk_, int lane_) {
        buf = b;
        thr = 0;
        cap = cap_;
        topk = topk_;
        n = 0;
        lane = lane_;
    }

    // sort, keep the topk largest; afterwards buf[0 .. cap) is descending with zeros past n
    __device__ __forceinline__ void compact() {
        for (int t = n + lane; t < cap; t += dg::kWave) buf[t] = 0;
        wave_lds_sync();
        wave_sort_desc(buf, cap, lane);
        if (n >= topk) {
            n = topk;
            thr = buf[topk - 1];
        }
    }

    // append the keys of the lanes with pred (wave-uniform call)
    __device__ __forceinline__ void push(uint64_t key, bool pred) {
        pred = pred && key > thr;
        uint64_t m = __ballot(pred);
        if (m == 0) return;
        if (n + __popcll(m) > cap) {
            compact();
            pred = pred && key > thr;
            m = __ballot(pred);
            if (m == 0) return;
        }
        const int pos = n + __popcll(m & ((1ull << lane) - 1ull));
        if (pred) buf[pos] = key;
        n += __popcll(m);
    }
};

}  // namespace dg

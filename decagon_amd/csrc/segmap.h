// Virtual tiles over segments (evalseg.hip): a launch over n_seg segments of a packed array
// (segment s = [ptr[s], ptr[s+1]), ptr on the device) in tiles of T elements that never straddle
// a segment, without a prefix sum over the tile counts and without reading ptr on the host.
//
// Segment s owns the virtual tiles starting at start(s) = ptr[s]/T + s.  start is strictly
// increasing in s (ptr is ascending and s adds 1), and
//   start(s+1) − start(s) = ⌊ptr[s+1]/T⌋ − ⌊ptr[s]/T⌋ + 1 ≥ ⌊len/T⌋ + 1 ≥ ⌈len/T⌉,
// so the range always holds the segment's tiles.  start(n_seg) = n_total/T + n_seg is the grid,
// which the host knows from the totals alone; at most n_seg + (segments' tails) virtual tiles
// are empty and exit at once.  A workgroup (or wave) finds its segment by binary search for the
// last s with start(s) ≤ vt.
//
// The same function runs on the host (dg_seg_tile_lookup) so that the map is tested without a
// device.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DG_HD __host__ __device__
#else
#define DG_HD
#endif

namespace dg {

DG_HD inline int64_t seg_tile_grid(int64_t n_total, int64_t n_seg, int tile) { return n_total / tile + n_seg; }

// Virtual tile vt < seg_tile_grid(ptr[n_seg], n_seg, tile) → its segment s and its tile index
// inside the segment; false when that tile lies past the segment's end (an empty slot).
DG_HD inline bool seg_tile_find(const int32_t* ptr, int n_seg, int tile, int vt, int& s, int& local) {
    int lo = 0, hi = n_seg - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (ptr[mid] / tile + mid <= vt)
            lo = mid;
        else
            hi = mid - 1;
    }
    s = lo;
    local = vt - (ptr[lo] / tile + lo);
    return (int64_t)local * tile < (int64_t)ptr[lo + 1] - (int64_t)ptr[lo];
}

#if defined(__HIPCC__)
// [beg, end) of segment s, end clamped to the element count; false for an empty or malformed one
__device__ __forceinline__ bool seg_bounds(const int32_t* ptr, int n_total, int s, int& beg, int& end) {
    beg = ptr[s];
    end = ptr[s + 1];
    if (end > n_total) end = n_total;
    return beg >= 0 && beg < end;
}

// relation of slot s (map[s], or s itself without a map), wave-uniform; false when it lies
// outside [0, n_rel)
__device__ __forceinline__ bool seg_relation(const int32_t* map, int n_rel, int s, int& k) {
    k = map ? map[s] : s;
    k = __builtin_amdgcn_readfirstlane(k);
    return k >= 0 && k < n_rel;
}
#endif

}  // namespace dg

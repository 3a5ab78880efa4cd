// The per-relation decoder operands of the "every relation of an edge type in one pass" entry
// points (evalseg.hip, gradseg.hip, profile.hip, topk.hip, and through rank_walk.h edgerank.hip
// and nodetopk.hip) — include/decagon_hip.h,
// "Per-relation operands":
//   G is [d, d] shared by every relation (g_stride 0) or [K, d, d] (g_stride d·d);
//   l is absent, [d] (l_stride 0) or [K, d] (l_stride d);
//   slot s (a segment, a selected column, a relation of the grid) is relation map[s], or s itself
//   without a map; a relation outside [0, n_rel) has no operands.
// The host fills one RelOps from the raw ABI arguments; the kernels select from it.
#pragma once
#include "common.h"

namespace dg {

struct RelOps {
    const float* G;  // relation 0's
    const float* l;  // relation 0's, or NULL
    int64_t g_stride, l_stride;
    int32_t n_rel;  // relations a slot may name
};

// DG_EINVAL for a stride that is neither 0 nor the operand's size, for a map without a relation
// count, and for per-relation operands that are fewer than the slots that index them directly.
// Without a map slot s is relation s, so every slot is in range: n_rel = n_slots.
inline int rel_ops(const float* G, int64_t g_stride, const float* l, int64_t l_stride, int32_t n_rel, int32_t d,
                   bool has_map, int32_t n_slots, RelOps& o) {
    if (g_stride != 0 && g_stride != (int64_t)d * d) return DG_EINVAL;
    if (l && l_stride != 0 && l_stride != d) return DG_EINVAL;
    const bool per_rel = g_stride != 0 || (l && l_stride != 0);
    if (has_map ? n_rel <= 0 : (per_rel && n_slots > n_rel)) return DG_EINVAL;
    o = RelOps{G, l, g_stride, l ? l_stride : 0, has_map ? n_rel : n_slots};
    return DG_OK;
}

__device__ __forceinline__ const float* rel_G(const RelOps& o, int k) { return o.G + (int64_t)k * o.g_stride; }

__device__ __forceinline__ const float* rel_l(const RelOps& o, int k) {
    return o.l ? o.l + (int64_t)k * o.l_stride : nullptr;
}

}  // namespace dg

// One query tile against every column of a table: the routines topk.hip, edgerank.hip and
// nodetopk.hip share, so that a pair's score
//   s_k[r, c] = (E_i[r] ∘ l_k)ᵀ · G_k · (l_k ∘ E_j[c])
// carries the same bits from dg_decoder_topk_f32, dg_decoder_edge_rank_f32 and
// dg_decoder_node_topk_f32 by construction: there is one A block and one tile product.
//
// All three take the half-row load and the A block.  The two segmented kernels (edgerank.hip,
// nodetopk.hip) also take the walk: a workgroup owns one 32-query tile of one segment (segmap.h)
// and one column split; the split's column tiles are dealt to the waves in contiguous runs, so
// each lane's cursor into its query's sorted exclusion row starts at one lower bound and never
// skips another wave's columns.  A wave takes its run in blocks of kBlock tiles.  First the lane
// that owns query row i builds the row's 32-bit masks of countable columns of the whole block in
// LDS, fetching the exclusion row kBatch entries per round trip — one dependent load per entry
// beside the tiles, topk.hip's own walk, cost more than the MFMAs.  Then it walks the
// tiles, the next tile's rows in flight behind the current MFMAs; what a tile's accumulator and
// row masks feed is the kernel's own: a ballot count in edgerank.hip, a threshold test and a list
// append in nodetopk.hip.  The two nested loops of that walk stay in the kernels, built from the
// routines here, and nodetopk.hip writes its prologue out (query_tile, tile_run and excl_cursor
// below serve edgerank.hip): DESIGN §21, "One walk", has the measurements that decided both.
//
// MFMA s of a 32×32 tile takes k = H·h + s from lane half h (the contraction order is free as
// long as A and B agree), so each lane's operands are H = D/2 contiguous floats of its row.
#pragma once
#include "common.h"
#include "rel_operands.h"
#include "segmap.h"
#include "topk_list.h"

namespace dg {

constexpr int kBlock = 16;        // column tiles whose row masks a wave builds at once (2 KiB of LDS a wave)
constexpr int kBatch = 8;         // exclusion entries a lane fetches per round trip
constexpr int kSplitGrid = 1024;  // workgroups a call wants before it stops splitting (4 per CU)

// Row stride of A in LDS, padded: 16-byte rows that do not all start on one bank.
constexpr int a_ld(int d) { return d + 4; }

template <int H>
__device__ __forceinline__ void load_half_row(const float* p, bool ok, float (&x)[H]) {
#pragma unroll
    for (int s4 = 0; s4 < H / 4; ++s4) {
        const float4 v = ok ? *reinterpret_cast<const float4*>(p + 4 * s4) : make_float4(0.f, 0.f, 0.f, 0.f);
        x[4 * s4] = v.x;
        x[4 * s4 + 1] = v.y;
        x[4 * s4 + 2] = v.z;
        x[4 * s4 + 3] = v.w;
    }
}

// Columns [32·nb, 32·nb + 32) of A = ((U ∘ l)·G) ∘ l for 32 rows, lane (i, h) holding the half row
// `u` of row i, into `As` (the first of the 32 rows, stride a_ld(D)).  (Through LDS: the MFMA leaves
// a row's 32 columns on 32 lanes, the next product wants them in one lane.)
template <int D>
__device__ __forceinline__ void a_block(const float (&u)[D / 2], const float* G, const float* l, int nb, int i, int h,
                                        float* As) {
    constexpr int H = D / 2;
    f32x16 acc = {};
#pragma unroll
    for (int t = 0; t < H; ++t) {
        const int kk = H * h + t;
        const float av = l ? u[t] * l[kk] : u[t];
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, G[kk * D + nb * 32 + i], acc, 0, 0, 0);
    }
    const float lj = l ? l[nb * 32 + i] : 1.0f;
#pragma unroll
    for (int q = 0; q < 16; ++q) As[acc_row(q, h) * a_ld(D) + nb * 32 + i] = acc[q] * lj;
}

// The 32×32 scores of a tile: lane (i, h) gives half row `af` of A's row i and `b` of column i.
template <int H>
__device__ __forceinline__ f32x16 tile_scores(const float (&af)[H], const float (&b)[H]) {
    f32x16 acc = {};
#pragma unroll
    for (int u = 0; u < H; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af[u], b[u], acc, 0, 0, 0);
    return acc;
}

// The 32-query tile a workgroup of a segmented grid owns: segment s = [.., end), its relation k
// (dead: outside [0, n_rel), k is then not a relation), the tile's first query p0, and lane i's
// query p with in_seg = p < end.
struct QueryTile {
    int s, k, p0, end, p;
    bool dead, in_seg;
};

// False where virtual tile `vt` holds no query.
__device__ __forceinline__ bool query_tile(const int32_t* seg_ptr, const int32_t* seg_rel, int n_seg, int n_queries,
                                           int n_rel, int vt, int i, QueryTile& q) {
    int s, local;
    if (!seg_tile_find(seg_ptr, n_seg, 32, vt, s, local)) return false;
    q.s = __builtin_amdgcn_readfirstlane(s);
    int beg;
    if (!seg_bounds(seg_ptr, n_queries, q.s, beg, q.end)) return false;
    q.p0 = beg + local * 32;
    if (q.p0 >= q.end) return false;
    q.p = q.p0 + i;
    q.in_seg = q.p < q.end;
    q.dead = !seg_relation(seg_rel, n_rel, q.s, q.k);
    return true;
}

// The contiguous run [t0, t1) of the n_ct 32-column tiles that wave slot `slot` of `n_slots` takes.
__device__ __forceinline__ void tile_run(int n_cols, int slot, int n_slots, int& n_ct, int& t0, int& t1) {
    n_ct = (int)(((int64_t)n_cols + 31) >> 5);
    t0 = (int)((int64_t)n_ct * slot / n_slots);
    t1 = (int)((int64_t)n_ct * (slot + 1) / n_slots);
}

// Cursor [pc, pe) into exclusion row q (columns ascending), at the first entry of tile t0 or later.
__device__ __forceinline__ void excl_cursor(const int32_t* ex_rowptr, const int32_t* ex_col, int64_t q, int t0,
                                            int& pc, int& pe) {
    pc = ex_rowptr[q];
    pe = ex_rowptr[q + 1];
    if (t0 > 0) {
        int lo = pc, hi = pe;
        while (lo < hi) {
            const int mid = lo + ((hi - lo) >> 1);
            if ((ex_col[mid] >> 5) < t0)
                lo = mid + 1;
            else
                hi = mid;
        }
        pc = lo;
    }
}

// Half rows of column tile t for lane (i, h); zeroes past the table (t = n_ct: no tile).
template <int H>
__device__ __forceinline__ void load_col_tile(const float* col_table, int64_t ld_col, int n_cols, int n_ct, int t,
                                              int i, int h, float (&x)[H]) {
    const uint32_t col = (uint32_t)t * 32u + (uint32_t)i;
    const bool in = t < n_ct && col < (uint32_t)n_cols;
    load_half_row<H>(col_table + (int64_t)(in ? col : 0u) * ld_col + H * h, in, x);
}

// Row i's masks of tiles [tb, tb + nt) into s_mask[t][i] (run by the lanes of half 0): the columns
// inside the table, less what clear(ct, m) drops of tile ct, less the excluded ones — kBatch
// entries of the sorted row per round trip, until one lies past the block.  Advances the cursor.
template <class Clear>
__device__ __forceinline__ void build_masks(uint32_t* s_mask, int i, int tb, int nt, int n_cols,
                                            const int32_t* ex_col, int& pc, int pe, Clear clear) {
#pragma unroll 1
    for (int t = 0; t < nt; ++t) {
        const int ct = tb + t;
        const uint32_t left = (uint32_t)n_cols - (uint32_t)ct * 32u;  // ≥ 1: columns from the tile's first on
        s_mask[t * 32 + i] = clear(ct, left >= 32u ? ~0u : (1u << left) - 1u);
    }
    bool more = pc < pe;
    while (more) {
        int e[kBatch];
#pragma unroll
        for (int j = 0; j < kBatch; ++j) e[j] = ex_col[pc + j < pe ? pc + j : pe - 1];
        int used = 0;
#pragma unroll
        for (int j = 0; j < kBatch; ++j) {
            const int t = (e[j] >> 5) - tb;
            const bool live = pc + j < pe && t < nt;
            if (live && t >= 0) atomicAnd(&s_mask[t * 32 + i], ~(1u << (e[j] & 31)));
            used += live;
        }
        pc += used;
        more = used == kBatch && pc < pe;
    }
}

// mr[q]: the mask of tile row acc_row(q, h) = (q & 3) + 8·(q >> 2) + 4·h, from one tile's 32 masks
__device__ __forceinline__ void row_masks(const uint32_t* tile_mask, int h, uint32_t (&mr)[16]) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const uint4 v = *reinterpret_cast<const uint4*>(tile_mask + 8 * g + 4 * h);
        mr[4 * g] = v.x;
        mr[4 * g + 1] = v.y;
        mr[4 * g + 2] = v.z;
        mr[4 * g + 3] = v.w;
    }
}

// Column splits of a call whose query tiles alone give fewer than kSplitGrid workgroups: as many
// as reach it, while each of a workgroup's `waves` waves keeps `wave_min_tiles` column tiles.
inline int column_splits(int64_t n_tiles, int n_ct, int waves, int wave_min_tiles, bool split) {
    int64_t n_split = 1;
    if (split && n_tiles < kSplitGrid) {
        n_split = (kSplitGrid + n_tiles - 1) / n_tiles;
        const int64_t most = n_ct / (waves * wave_min_tiles);
        if (n_split > most) n_split = most;
        if (n_split < 1) n_split = 1;
    }
    return (int)n_split;
}

// The argument checks of the segmented ranking entry points, after their own DG_EINVAL checks;
// fills `ops`.  `no_self` and `no_split` are the entry point's flag bits.
inline int check_rank_call(const float* row_table, int64_t ld_row, int32_t n_rows, const float* col_table,
                           int64_t ld_col, int32_t n_cols, const int32_t* row_idx, const int32_t* seg_ptr,
                           const int32_t* seg_rel, int32_t n_seg, int32_t n_queries, const float* G, int64_t g_stride,
                           const float* l, int64_t l_stride, int32_t n_rel, int32_t d, const int32_t* excl_rowptr,
                           const int32_t* excl_col, int32_t flags, int32_t no_self, int32_t no_split, RelOps& ops) {
    if (n_seg <= 0 || n_queries < 0 || (d != 32 && d != 64)) return DG_EINVAL;
    if (!row_table || !col_table || !seg_ptr || !G) return DG_EINVAL;
    if (n_queries > 0 && !row_idx) return DG_EINVAL;
    if (n_rows < 1 || n_cols < 1 || ld_row < d || ld_col < d) return DG_EINVAL;
    if (rel_ops(G, g_stride, l, l_stride, n_rel, d, seg_rel != nullptr, n_seg, ops) != DG_OK) return DG_EINVAL;
    if ((excl_rowptr == nullptr) != (excl_col == nullptr)) return DG_EINVAL;
    if (excl_rowptr && !seg_rel && n_seg > n_rel) return DG_EINVAL;  // segment s reads exclusion relation s
    if (flags & ~(no_self | no_split)) return DG_EINVAL;
    if ((flags & no_self) && n_rows != n_cols) return DG_EINVAL;
    if ((int64_t)n_queries + 32LL * n_seg >= (1ll << 31)) return DG_EINVAL;  // 32-bit query offsets
    if (!aligned16(row_table) || !aligned16(col_table) || (ld_row & 3) || (ld_col & 3)) return DG_EALIGN;
    return DG_OK;
}

}  // namespace dg

// A node's best partners per relation: for every query (row node r of a relation k) the `topk`
// highest-scoring permitted columns c' of
//   s_k[r, c'] = (E_i[r] ∘ l_k)ᵀ · G_k · (l_k ∘ E_j[c'])
// — "given drug u and side effect k, which drugs are u's likeliest partners outside the known
// ones?" — without ever forming an N_i×N_j matrix, or a chunk of one.
//
// Replaces (paths relative to the reference root):
//   session.run(predictions) of one relation, a dense mask of the known edges and a sort of each
//   wanted row on the host, once per relation          main/Predictor/NpPredictor.py:293-313
//
// Form.  Launch 1: one workgroup per 32-query tile of one segment (segmap.h) and per column split.
// It forms A = ((U ∘ l)·G) ∘ l of its 32 query rows once on v_mfma_f32_32x32x2_f32 into LDS
// (rank_walk.h's A block, the one topk.hip and edgerank.hip form, so that a score has the bits
// dg_decoder_topk_f32 and dg_decoder_edge_rank_f32 give for the pair).  The waves then take
// rank_walk.h's walk over the split's column tiles, edgerank.hip's: contiguous runs, in blocks of
// 16 tiles whose per-row masks of permitted columns (inside the table, not excluded, not r under
// NO_SELF) are built first.  What this file adds to the walk, in place of edgerank's count, is
// one running list of topk_list.h's keys PER QUERY ROW that a wave keeps in LDS.  The
// fast path is straight-line: each of a lane's 16 accumulator elements is compared with its row's
// threshold score held in a register and masked by the row's bit; one ballot over the tile decides
// whether the exact path runs at all.  The exact path appends the passing 64-bit keys to their
// rows' lists (a row's 32 columns sit in one lane half, so an append is at most 32 keys) and,
// where a list has fewer than 32 free slots left, sorts it (bitonic, two rows at once: one per
// lane half), truncates it to topk and raises the row's threshold.  Past the first few tiles
// almost nothing passes.  The list capacity — the power of two ≥ topk + 32 — and with it the
// waves a workgroup can hold are sized by the call's topk (dynamic LDS).
//
// Where a tile has one wave and one split the wave writes the decoded lists itself.  Otherwise
// the waves' sorted partial lists go to the workspace, and launch 2 merges them with one wave per
// query, as topk.hip's second launch does per relation.
//
// Ordering: topk_list.h's keys with the column as the index — higher fp32 score first, equal
// scores by smaller column, −0 as +0.  Keys of one query are unique and a key is only dropped
// when topk larger ones exist, so the result is the unique top-k of the row whatever the tiling,
// the grid or the order in which waves run.
#include "common.h"
#include "decagon_hip_ext2.h"
#include "rank_walk.h"

namespace {

using dg::f32x16;
using dg::kBlock;
using dg::key_score;
using dg::load_half_row;
using dg::make_key;
using dg::wave_lds_sync;

constexpr int kMaxWaves = 4;       // waves per workgroup at most: column runs per split
constexpr int kWaveMinTiles = 16;  // column tiles a wave of a workgroup keeps at least (one mask block)
constexpr int kSplitMinTiles = 4;  // column tiles a wave keeps at least when the columns are split
constexpr int kMergeWaves = 4;     // queries per workgroup of the merge

struct NodeTopkArgs {
    const float* row_table;
    const float* col_table;
    dg::RelOps ops;
    const int32_t* row_idx;
    const int32_t* seg_ptr;
    const int32_t* seg_rel;
    const int32_t* ex_rowptr;
    const int32_t* ex_col;
    float* out_score;
    int32_t* out_col;
    int32_t* out_count;
    uint64_t* lists;  // [n_queries][n_split · waves][topk] partial lists (unused with one slot)
    int64_t ld_row, ld_col;
    int32_t n_rows, n_cols, n_seg, n_queries, n_split, topk, cap, flags;
};

// Capacity of a row's list: the power of two ≥ topk + 32, so that after a truncation to topk one
// append (at most 32 keys: a tile's columns of the row) always fits.
inline int row_cap(int topk) {
    int c = 64;
    while (c < topk + 32) c <<= 1;
    return c;
}

// Waves a workgroup holds at that capacity: 16 / 32 / 64 KiB of lists a wave.
inline int max_waves(int cap) { return cap <= 64 ? kMaxWaves : cap <= 128 ? 2 : 1; }

inline int lds_bytes(int waves, int cap, int d) {
    return waves * 32 * cap * 8 + waves * 32 * 8 + 32 * dg::a_ld(d) * 4 + waves * kBlock * 32 * 4 + waves * 32 * 4 * 2;
}

struct Plan {
    int waves, n_split;
};

// Waves per workgroup and column splits of a call (host; from the totals alone).
inline Plan plan(int64_t n_queries, int64_t n_seg, int n_cols, int topk, bool split) {
    const int n_ct = dg::ceil_div(n_cols, 32);
    int waves = n_ct / kWaveMinTiles;
    const int most_w = max_waves(row_cap(topk));
    if (waves > most_w) waves = most_w;
    if (waves < 1) waves = 1;
    const int64_t n_tiles = dg::seg_tile_grid(n_queries, n_seg, 32);
    return Plan{waves, dg::column_splits(n_tiles, n_ct, waves, kSplitMinTiles, split)};
}

// One wave's per-row lists: 32 rows of cap keys, unsorted, n[row] of them live and all above
// thr[row]; ts[row] is thr's score (−inf while the list holds fewer than topk keys).
struct RowLists {
    uint64_t* keys;  // [32][cap]
    uint64_t* thr;   // [32]
    float* ts;       // [32]
    int* n;          // [32]
    int cap, topk;
};

// Sort, and truncate to topk, the lists of two rows at once: lane half h takes `row` (its own) when
// `active` (uniform over the half).  Bitonic, descending, the half's 32 lanes on cap/2 comparators.
__device__ __forceinline__ void compact_pair(const RowLists& L, int row, bool active, int i) {
    uint64_t* buf = L.keys + row * L.cap;
    const int n = active ? L.n[row] : 0;
    if (active)
        for (int t = n + i; t < L.cap; t += 32) buf[t] = 0;
    wave_lds_sync();
#pragma unroll 1
    for (int k = 2; k <= L.cap; k <<= 1) {
#pragma unroll 1
        for (int j = k >> 1; j > 0; j >>= 1) {
            if (active) {
#pragma unroll 1
                for (int t = i; t < L.cap / 2; t += 32) {
                    const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                    const int hi = lo | j;
                    const bool desc = (lo & k) == 0;
                    const uint64_t x = buf[lo], y = buf[hi];
                    if (desc ? (x < y) : (x > y)) {
                        buf[lo] = y;
                        buf[hi] = x;
                    }
                }
            }
            wave_lds_sync();
        }
    }
    if (active && i == 0 && n >= L.topk) {
        const uint64_t t = buf[L.topk - 1];
        L.n[row] = L.topk;
        L.thr[row] = t;
        L.ts[row] = key_score(t);
    }
    wave_lds_sync();
}

// compact_pair over the rows of `rows` (a wave-uniform 32-bit set), two per pass
__device__ __forceinline__ void compact_rows(const RowLists& L, uint32_t rows, int i, int h) {
#pragma unroll 1
    while (rows) {
        const int ra = __builtin_ctz(rows);
        rows &= rows - 1;
        const int rb = rows ? __builtin_ctz(rows) : -1;
        rows &= rows - 1;  // (0 & … stays 0)
        compact_pair(L, h == 0 ? ra : (rb < 0 ? 0 : rb), h == 0 || rb >= 0, i);
    }
}

// Launch 1.  blockDim.x = 64 · waves; grid (virtual query tiles, column splits); dynamic LDS
// lds_bytes(waves, cap, D).
template <int D>
__global__ __launch_bounds__(256) void node_topk_kernel(const NodeTopkArgs a) {
    constexpr int H = D / 2;
    constexpr int LDA = dg::a_ld(D);
    extern __shared__ __attribute__((aligned(16))) unsigned char node_smem[];

    const int lane = threadIdx.x & 63;
    const int W = (int)(blockDim.x >> 6);
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int i = lane & 31, h = lane >> 5;
    const int split = blockIdx.y;
    const int cap = a.cap, topk = a.topk;

    uint64_t* keys_all = reinterpret_cast<uint64_t*>(node_smem);     // [W][32][cap]
    uint64_t* thr_all = keys_all + W * 32 * cap;                     // [W][32]
    float* As = reinterpret_cast<float*>(thr_all + W * 32);          // [32][LDA]
    uint32_t* mask_all = reinterpret_cast<uint32_t*>(As + 32 * LDA);  // [W][kBlock][32]
    float* ts_all = reinterpret_cast<float*>(mask_all + W * kBlock * 32);
    int* n_all = reinterpret_cast<int*>(ts_all + W * 32);
    uint32_t* s_mask = mask_all + w * kBlock * 32;  // this wave's row masks of one block of tiles
    RowLists L{keys_all + w * 32 * cap, thr_all + w * 32, ts_all + w * 32, n_all + w * 32, cap, topk};

    // (the prologue below — tile, run, cursor — is rank_walk.h's query_tile, tile_run and
    // excl_cursor written out: DESIGN §21, "One walk", says why)
    int s, local;
    if (!dg::seg_tile_find(a.seg_ptr, a.n_seg, 32, (int)blockIdx.x, s, local)) return;
    s = __builtin_amdgcn_readfirstlane(s);
    int beg, end;
    if (!dg::seg_bounds(a.seg_ptr, a.n_queries, s, beg, end)) return;
    const int p0 = beg + local * 32;
    if (p0 >= end) return;
    const int p = p0 + i;
    const bool in_seg = p < end;
    int k;
    const bool dead = !dg::seg_relation(a.seg_rel, a.ops.n_rel, s, k);  // the whole segment: empty lists
    if (dead) k = 0;
    const float* G = dg::rel_G(a.ops, k);
    const float* l = dg::rel_l(a.ops, k);

    int r = in_seg ? a.row_idx[p] : 0;
    const bool ok = !dead && in_seg && r >= 0 && r < a.n_rows;
    if (!ok) r = 0;

    // this wave's contiguous run of column tiles inside the split's (none in a dead segment)
    const int n_ct = (int)(((int64_t)a.n_cols + 31) >> 5);
    const int slot = split * W + w, n_slots = a.n_split * W;
    const int t0 = (int)((int64_t)n_ct * slot / n_slots);
    const int t1 = dead ? t0 : (int)((int64_t)n_ct * (slot + 1) / n_slots);

    // this lane's cursor into the exclusion row of query row i (columns ascending), at the run's
    // first tile; and the first tile's rows — both in flight behind the A stripe
    int pc = 0, pe = 0;
    if (a.ex_rowptr && ok && h == 0) {  // (lane half 0 owns the rows' masks)
        const int64_t q = (int64_t)k * a.n_rows + r;
        pc = a.ex_rowptr[q];
        pe = a.ex_rowptr[q + 1];
        if (t0 > 0) {
            int lo = pc, hi = pe;
            while (lo < hi) {
                const int mid = lo + ((hi - lo) >> 1);
                if ((a.ex_col[mid] >> 5) < t0)
                    lo = mid + 1;
                else
                    hi = mid;
            }
            pc = lo;
        }
    }
    float b[H];
    dg::load_col_tile<H>(a.col_table, a.ld_col, a.n_cols, n_ct, t0 < t1 ? t0 : n_ct, i, h, b);

    // A of the 32 query rows, 32 columns at a time
    if (w < D / 32) {  // (the waves that form a block of the stripe)
        float u[H];
        load_half_row<H>(a.row_table + (int64_t)r * a.ld_row + H * h, ok, u);
#pragma unroll 1
        for (int nb = w; nb < D / 32; nb += W) dg::a_block<D>(u, G, l, nb, i, h, As);
    }
    if (h == 0) {
        L.n[i] = 0;
        L.thr[i] = 0;
        L.ts[i] = -__builtin_inff();
    }
    __syncthreads();

    float af[H];
    load_half_row<H>(As + i * LDA + H * h, true, af);

    float ts[16];  // threshold score of the 16 tile rows this lane's accumulator registers hold
#pragma unroll
    for (int q = 0; q < 16; ++q) ts[q] = -__builtin_inff();

    const bool no_self = (a.flags & DG_NODE_TOPK_NO_SELF) != 0;
    float bn[H];
#pragma unroll 1
    for (int tb = t0; tb < t1; tb += kBlock) {  // the run in blocks of kBlock tiles: masks first, then the walk
        const int nt = t1 - tb < kBlock ? t1 - tb : kBlock;
        wave_lds_sync();  // the previous block's masks have been read
        if (h == 0)
            dg::build_masks(s_mask, i, tb, nt, a.n_cols, a.ex_col, pc, pe, [&](int ct, uint32_t m) {
                if (no_self && (r >> 5) == ct) m &= ~(1u << (r & 31));  // not r under NO_SELF
                return ok ? m : 0u;                                      // nothing of a query outside the table
            });
        wave_lds_sync();
#pragma unroll 1
        for (int t = 0; t < nt; ++t) {
            const int ct = tb + t;
            // next tile's rows in flight behind this tile's MFMAs
            dg::load_col_tile<H>(a.col_table, a.ld_col, a.n_cols, n_ct, ct + 1 < t1 ? ct + 1 : n_ct, i, h, bn);
            const f32x16 acc = dg::tile_scores<H>(af, b);
            uint32_t mr[16];
            dg::row_masks(s_mask + t * 32, h, mr);
            // the fast path: does any element reach its row's threshold?  (−0 == +0 in fp32 and a
            // list's threshold is never above its topk-th key, so this admits a superset)
            bool any = false;
#pragma unroll
            for (int q = 0; q < 16; ++q) any |= (acc[q] >= ts[q]) & (((mr[q] >> i) & 1u) != 0);
            if (__ballot(any) != 0) {
                // the exact path: append the keys above their row's threshold key
                const uint32_t col = (uint32_t)ct * 32u + (uint32_t)i;
                const uint32_t below = (1u << i) - 1u;
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const bool adm = (acc[q] >= ts[q]) & (((mr[q] >> i) & 1u) != 0);
                    if (__ballot(adm) == 0) continue;
                    const int row = dg::acc_row(q, h);
                    const uint64_t key = make_key(acc[q], col);
                    const bool pred = adm && key > L.thr[row];
                    const uint64_t m = __ballot(pred);
                    const uint32_t mh = h ? (uint32_t)(m >> 32) : (uint32_t)m;
                    const int n = L.n[row];
                    const int pos = n + __popc(mh & below);
                    if (pred && pos < cap) L.keys[row * cap + pos] = key;
                    if (i == 0 && mh != 0) L.n[row] = n + __popc(mh);  // ≤ cap: n ≤ cap − 32 before a tile
                }
                wave_lds_sync();
                // lists with fewer than 32 free slots: sort, keep topk, raise the threshold
                const uint32_t full = (uint32_t)__ballot(h == 0 && L.n[i] > cap - 32);
                if (full != 0) {
                    compact_rows(L, full, i, h);
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const float4 v = *reinterpret_cast<const float4*>(&L.ts[8 * g + 4 * h]);
                        ts[4 * g] = v.x;
                        ts[4 * g + 1] = v.y;
                        ts[4 * g + 2] = v.z;
                        ts[4 * g + 3] = v.w;
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < H; ++u) b[u] = bn[u];
        }
    }

    // every non-empty list sorted and cut to topk; then out: decoded where this wave saw all the
    // columns, as keys for the merge otherwise
    wave_lds_sync();
    compact_rows(L, (uint32_t)__ballot(h == 0 && L.n[i] > 0), i, h);
    const float ninf = -__builtin_inff();
#pragma unroll 1
    for (int row = 0; row < 32; ++row) {
        const int q = p0 + row;
        if (q >= end) break;
        const int n = L.n[row] < topk ? L.n[row] : topk;
        for (int t = lane; t < topk; t += dg::kWave) {
            const uint64_t key = t < n ? L.keys[row * cap + t] : 0;
            if (n_slots > 1) {
                a.lists[((int64_t)q * n_slots + slot) * topk + t] = key;
            } else {
                a.out_score[(int64_t)q * topk + t] = key ? key_score(key) : ninf;
                a.out_col[(int64_t)q * topk + t] = key ? (int32_t)~(uint32_t)key : -1;
            }
        }
        if (n_slots == 1 && lane == 0) a.out_count[q] = n;
    }
}

// Launch 2.  One wave per query: the top-k of its n_slots descending partial lists, decoded.
__global__ __launch_bounds__(64 * kMergeWaves) void node_topk_merge_kernel(const uint64_t* lists, int n_slots,
                                                                           int n_queries, int topk, int cap,
                                                                           float* out_score, int32_t* out_col,
                                                                           int32_t* out_count) {
    extern __shared__ __attribute__((aligned(16))) unsigned char node_smem[];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t q = (int64_t)blockIdx.x * kMergeWaves + w;
    if (q >= n_queries) return;  // (no workgroup barrier below)
    dg::WaveTopK tk;
    tk.init(reinterpret_cast<uint64_t*>(node_smem) + w * cap, cap, topk, lane);
#pragma unroll 1
    for (int L = 0; L < n_slots; ++L) {
        const uint64_t* src = lists + (q * n_slots + L) * topk;
#pragma unroll 1
        for (int t0 = 0; t0 < topk; t0 += dg::kWave) {
            const int t = t0 + lane;
            const uint64_t key = t < topk ? src[t] : 0;
            const bool ok = key > tk.thr;  // (padding is 0)
            if (__ballot(ok) == 0) break;  // descending: nothing further can enter
            tk.push(key, ok);
        }
    }
    tk.compact();
    for (int t = lane; t < topk; t += dg::kWave) {
        const uint64_t key = t < tk.n ? tk.buf[t] : 0;
        out_score[q * topk + t] = key ? key_score(key) : -__builtin_inff();
        out_col[q * topk + t] = key ? (int32_t)~(uint32_t)key : -1;
    }
    if (lane == 0) out_count[q] = tk.n;
}

template <int D>
int launch_walk(const NodeTopkArgs& a, int waves, int64_t n_tiles, hipStream_t st) {
    static std::atomic<uint64_t> optin{0};
    const int bytes = lds_bytes(waves, a.cap, D);
    if (bytes > 65536) {  // the opt-in covers the largest form: the most waves of every capacity
        int most = 0;
        for (int cap = 64; cap <= row_cap(DG_NODE_TOPK_MAX_K); cap <<= 1)
            if (lds_bytes(max_waves(cap), cap, D) > most) most = lds_bytes(max_waves(cap), cap, D);
        dg::lds_optin(reinterpret_cast<const void*>(&node_topk_kernel<D>), most, optin);
    }
    hipLaunchKernelGGL(node_topk_kernel<D>, dim3((unsigned)n_tiles, (unsigned)a.n_split), dim3(64 * waves), bytes, st, a);
    return dg::launch_status();
}

}  // namespace

extern "C" int64_t dg_decoder_node_topk_workspace(int32_t n_queries, int32_t n_seg, int32_t n_cols, int32_t topk) {
    if (n_queries < 1 || n_seg < 1 || n_cols < 1 || topk < 1 || topk > DG_NODE_TOPK_MAX_K) return 0;
    const Plan pl = plan(n_queries, n_seg, n_cols, topk, true);
    const int64_t n_slots = (int64_t)pl.waves * pl.n_split;
    return n_slots > 1 ? (int64_t)n_queries * n_slots * topk * 8 : 0;
}

extern "C" int dg_decoder_node_topk_f32(const float* row_table, int64_t ld_row, int32_t n_rows,
                                        const float* col_table, int64_t ld_col, int32_t n_cols,
                                        const int32_t* row_idx, const int32_t* seg_ptr, const int32_t* seg_rel,
                                        int32_t n_seg, int32_t n_queries, const float* G, int64_t g_stride,
                                        const float* l, int64_t l_stride, int32_t n_rel, int32_t d, int32_t topk,
                                        const int32_t* excl_rowptr, const int32_t* excl_col, int32_t flags,
                                        float* out_score, int32_t* out_col, int32_t* out_count, void* workspace,
                                        int64_t workspace_bytes, void* stream) {
    if (n_queries > 0 && (!out_score || !out_col || !out_count)) return DG_EINVAL;
    if (topk < 1 || topk > DG_NODE_TOPK_MAX_K) return DG_EINVAL;
    const int64_t need = dg_decoder_node_topk_workspace(n_queries, n_seg, n_cols, topk);
    if (workspace_bytes < need || (need > 0 && !workspace)) return DG_EINVAL;
    NodeTopkArgs a{};
    const int rc0 = dg::check_rank_call(row_table, ld_row, n_rows, col_table, ld_col, n_cols, row_idx, seg_ptr, seg_rel,
                                        n_seg, n_queries, G, g_stride, l, l_stride, n_rel, d, excl_rowptr, excl_col,
                                        flags, DG_NODE_TOPK_NO_SELF, DG_NODE_TOPK_NO_SPLIT, a.ops);
    if (rc0 != DG_OK) return rc0;
    if (need > 0 && !dg::aligned16(workspace)) return DG_EALIGN;
    if (n_queries == 0) return DG_OK;

    const Plan pl = plan(n_queries, n_seg, n_cols, topk, !(flags & DG_NODE_TOPK_NO_SPLIT));
    a.row_table = row_table;
    a.col_table = col_table;
    a.row_idx = row_idx;
    a.seg_ptr = seg_ptr;
    a.seg_rel = seg_rel;
    a.ex_rowptr = excl_rowptr;
    a.ex_col = excl_col;
    a.out_score = out_score;
    a.out_col = out_col;
    a.out_count = out_count;
    a.lists = static_cast<uint64_t*>(workspace);
    a.ld_row = ld_row;
    a.ld_col = ld_col;
    a.n_rows = n_rows;
    a.n_cols = n_cols;
    a.n_seg = n_seg;
    a.n_queries = n_queries;
    a.n_split = pl.n_split;
    a.topk = topk;
    a.cap = row_cap(topk);
    a.flags = flags;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int64_t n_tiles = dg::seg_tile_grid(n_queries, n_seg, 32);
    const int rc = d == 32 ? launch_walk<32>(a, pl.waves, n_tiles, st) : launch_walk<64>(a, pl.waves, n_tiles, st);
    if (rc != DG_OK) return rc;
    const int n_slots = pl.waves * pl.n_split;
    if (n_slots > 1) {
        const int mcap = dg::list_cap(topk);
        hipLaunchKernelGGL(node_topk_merge_kernel, dim3((unsigned)dg::ceil_div(n_queries, kMergeWaves)),
                           dim3(64 * kMergeWaves), kMergeWaves * mcap * 8, st, a.lists, n_slots, n_queries, topk, mcap,
                           out_score, out_col, out_count);
        return dg::launch_status();
    }
    return DG_OK;
}

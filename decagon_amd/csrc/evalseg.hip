// Evaluation of ALL relations of one edge type in one pass: the sampled pairs of every relation
// scored by one launch, and AUROC / AUPRC / AP@k of every relation by three.
//
// Replaces (paths relative to the reference root):
//   the loop of get_accuracy_scores over every relation          main.py:38-80 and its final loop
//   DecagonAccuracyEvaluator.evaluateAll / _evaluateRelation      main/AccuracyEvaluators/Tensorflow/
//                                                                 DecagonAccuracyEvaluator.py:57-120
// which here was one dg_decoder_score_f32 pair and one dg_rank_metrics_ex_f32 per relation.
//
// Both halves run over SEGMENTS of packed arrays (segment s = [ptr[s], ptr[s+1]), ptr on the
// device) through the virtual-tile map of segmap.h, so nothing is read back to size a grid and
// the calls can be captured in a graph.
//
// Scorer: one wave per 32-pair tile of one segment runs dg::score_tile (decoder_tile.h, the tile
// of dg_decoder_score_f32) with the segment's G_k, l_k.  score_tile's result for a pair depends
// neither on its slot in the tile nor on its neighbours (an MFMA row is independent of the other
// rows, and the reduce-scatter tree has the same shape for every slot), so a segment's scores
// equal dg_decoder_score_f32's on that segment alone, bit for bit.
//
// Metrics: keys of all logits in one launch (dg::score_key); then one workgroup per (segment,
// block of 256 positives), one positive per thread: the segment's positive keys, then its
// negative keys, pass through LDS in tiles of kStage keys, every lane reading the same address
// (a broadcast: no bank conflict), and each thread keeps its positive's six integer counts in
// registers — no block reduction, no atomics (eval.hip's count kernel spends a workgroup and six
// block reductions per positive).  The counts are exact integers in rank_counts_kernel's record
// layout, and one workgroup per segment sums them with dg::rank_reduce_block, so every row
// equals dg_rank_metrics_ex_f32 on that segment alone, bit for bit.
#include "common.h"
#include "decoder_tile.h"
#include "rank_metrics.h"
#include "rel_operands.h"
#include "segmap.h"

namespace {

using dg::DecTab;

struct SegScoreArgs {
    DecTab t;  // (G, l: relation 0's, as in ops)
    dg::RelOps ops;
    const int32_t* row_idx;
    const int32_t* col_idx;
    const int32_t* seg_ptr;
    const int32_t* seg_rel;
    float* out;
    int32_t n_rows, n_cols, n_seg, n_pairs, n_tiles;
};

// Pairs whose index lies outside the tables, and segments whose relation lies outside [0, n_rel),
// score NaN and read nothing out of range.
__global__ __launch_bounds__(256) void decoder_score_seg_kernel(const SegScoreArgs a) {
    const int lane = threadIdx.x & 63;
    const int vt = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (vt >= a.n_tiles) return;
    int s, local;
    if (!dg::seg_tile_find(a.seg_ptr, a.n_seg, 32, vt, s, local)) return;
    s = __builtin_amdgcn_readfirstlane(s);
    int beg, end;
    if (!dg::seg_bounds(a.seg_ptr, a.n_pairs, s, beg, end)) return;
    const int p0 = beg + local * 32;
    if (p0 >= end) return;
    int k;
    const bool rel_ok = dg::seg_relation(a.seg_rel, a.ops.n_rel, s, k);
    if (!rel_ok) k = 0;
    DecTab t = a.t;
    t.G = dg::rel_G(a.ops, k);
    t.l = dg::rel_l(a.ops, k);

    const int i = lane & 31;
    const int h = lane >> 5;
    const int p = p0 + i;
    const bool in_seg = p < end;
    int r = in_seg ? a.row_idx[p] : 0, c = in_seg ? a.col_idx[p] : 0;
    const bool ok = rel_ok && r >= 0 && r < a.n_rows && c >= 0 && c < a.n_cols;
    if (!ok) r = c = 0;
    float part[16];
    dg::score_tile(t, r, c, in_seg && ok, part);
    // lane 2q holds score q of its half; the pair it belongs to is named by lane `slot`
    const int q = i >> 1;
    const int slot = dg::acc_row(q, h);
    const int slot_ok = __shfl((int)ok, slot);
    if ((i & 1) == 0) {
        const int pp = p0 + slot;
        if (pp < end) a.out[pp] = slot_ok ? part[0] : __builtin_nanf("");
    }
}

constexpr int kStage = 256;  // keys per LDS stage: one per thread (2 KiB — occupancy stays wave-limited)

// key[i] of logit i of pos ++ neg
__global__ __launch_bounds__(256) void score_key_seg_kernel(const float* pos, int n_pos, const float* neg, int n_neg,
                                                            int mode, double* key) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)n_pos + n_neg) return;
    key[i] = dg::score_key(i < n_pos ? pos[i] : neg[i - n_pos], mode);
}

struct SegRankArgs {
    const double* kp;  // keys of the positives, by segment
    const double* kn;
    const int32_t* pos_ptr;
    const int32_t* neg_ptr;
    int* counts;       // [n_pos_total][8]
    double* out;       // [n_seg][3]
    int32_t n_pos, n_neg, n_seg, n_tiles, k;
};

// [beg, end) of segment s clamped into [0, total]
__device__ __forceinline__ void seg_range(const int32_t* ptr, int s, int total, int& beg, int& end) {
    beg = ptr[s];
    end = ptr[s + 1];
    if (beg < 0) beg = 0;
    if (end > total) end = total;
    if (end < beg) end = beg;
}

__global__ __launch_bounds__(256) void rank_counts_seg_kernel(const SegRankArgs a) {
    __shared__ double stage[kStage];
    int s, local;
    if (!dg::seg_tile_find(a.pos_ptr, a.n_seg, 256, (int)blockIdx.x, s, local)) return;
    int pb, pe, nb, ne;
    seg_range(a.pos_ptr, s, a.n_pos, pb, pe);
    seg_range(a.neg_ptr, s, a.n_neg, nb, ne);
    const int tid = threadIdx.x;
    const int mine = local * 256 + tid;  // this thread's positive, counted from the segment's first
    const bool active = pb + mine < pe;
    const double sc = active ? a.kp[pb + mine] : 0.0;
    int lt_neg = 0, eq_neg = 0, ge_pos = 0, gt_pos = 0, eq_before = 0, gt_neg = 0;
#pragma unroll 1
    for (int j0 = pb; j0 < pe; j0 += kStage) {
        const int n = pe - j0 < kStage ? pe - j0 : kStage;
        __syncthreads();  // the previous stage has been read
        if (tid < n) stage[tid] = a.kp[j0 + tid];
        __syncthreads();
        const int before = pb + mine - j0;  // staged keys [0, before) precede this positive
#pragma unroll 4
        for (int t = 0; t < n; ++t) {
            const double v = stage[t];
            ge_pos += v >= sc;
            gt_pos += v > sc;
            eq_before += (v == sc) && (t < before);
        }
    }
#pragma unroll 1
    for (int j0 = nb; j0 < ne; j0 += kStage) {
        const int n = ne - j0 < kStage ? ne - j0 : kStage;
        __syncthreads();
        if (tid < n) stage[tid] = a.kn[j0 + tid];
        __syncthreads();
#pragma unroll 4
        for (int t = 0; t < n; ++t) {
            const double v = stage[t];
            lt_neg += v < sc;
            eq_neg += v == sc;
            gt_neg += v > sc;
        }
    }
    if (active) dg::rank_record(a.counts + (int64_t)(pb + mine) * 8, lt_neg, eq_neg, ge_pos, gt_pos, eq_before, gt_neg);
}

__global__ __launch_bounds__(256) void rank_reduce_seg_kernel(const SegRankArgs a) {
    __shared__ double red[3][256];
    const int s = blockIdx.x;
    int pb, pe, nb, ne;
    seg_range(a.pos_ptr, s, a.n_pos, pb, pe);
    seg_range(a.neg_ptr, s, a.n_neg, nb, ne);
    dg::rank_reduce_block(a.counts + (int64_t)pb * 8, pe - pb, ne - nb, a.k, a.out + (int64_t)s * 3, red);
}

}  // namespace

extern "C" int32_t dg_seg_tile_lookup(const int32_t* seg_ptr, int32_t n_seg, int32_t tile, int32_t vt,
                                      int32_t* seg, int32_t* local) {
    if (!seg_ptr || n_seg < 1 || tile < 1 || !seg || !local) return DG_EINVAL;
    if (vt < 0 || vt >= dg::seg_tile_grid(seg_ptr[n_seg], n_seg, tile)) return DG_EINVAL;
    int s, t;
    const bool live = dg::seg_tile_find(seg_ptr, n_seg, tile, vt, s, t);
    *seg = s;
    *local = t;
    return live ? 1 : 0;
}

extern "C" int dg_decoder_score_seg_f32(const float* row_table, int64_t ld_row, int32_t n_rows,
                                        const float* col_table, int64_t ld_col, int32_t n_cols,
                                        const int32_t* row_idx, const int32_t* col_idx, const int32_t* seg_ptr,
                                        const int32_t* seg_rel, int32_t n_seg, int32_t n_pairs, const float* G,
                                        int64_t g_stride, const float* l, int64_t l_stride, int32_t n_rel,
                                        int32_t d, float* out, void* stream) {
    if (n_seg <= 0 || n_pairs < 0 || d <= 0 || (d % 32) || d > 256) return DG_EINVAL;
    if (!row_table || !col_table || !seg_ptr || !G) return DG_EINVAL;
    if (n_pairs > 0 && (!row_idx || !col_idx || !out)) return DG_EINVAL;
    if (n_rows < 1 || n_cols < 1 || ld_row < d || ld_col < d) return DG_EINVAL;
    SegScoreArgs a{};
    if (dg::rel_ops(G, g_stride, l, l_stride, n_rel, d, seg_rel != nullptr, n_seg, a.ops) != DG_OK) return DG_EINVAL;
    if ((int64_t)n_pairs + 32LL * n_seg >= (1ll << 31)) return DG_EINVAL;  // 32-bit pair offsets
    if (n_pairs == 0) return DG_OK;
    a.t = DecTab{row_table, col_table, G, l, ld_row, ld_col, d,
                 dg::aligned16(row_table) && (ld_row & 3) == 0 && (!l || dg::aligned16(l))};
    a.row_idx = row_idx;
    a.col_idx = col_idx;
    a.seg_ptr = seg_ptr;
    a.seg_rel = seg_rel;
    a.out = out;
    a.n_rows = n_rows;
    a.n_cols = n_cols;
    a.n_seg = n_seg;
    a.n_pairs = n_pairs;
    a.n_tiles = (int32_t)dg::seg_tile_grid(n_pairs, n_seg, 32);
    hipLaunchKernelGGL(decoder_score_seg_kernel, dim3(dg::ceil_div(a.n_tiles, 4)), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), a);
    return dg::launch_status();
}

extern "C" int64_t dg_rank_metrics_seg_workspace(int32_t n_pos_total, int32_t n_neg_total, int32_t n_seg) {
    if (n_pos_total < 0 || n_neg_total < 0 || n_seg < 0) return 0;
    return 32LL * n_pos_total + 8LL * ((int64_t)n_pos_total + n_neg_total) + 16;
}

extern "C" int dg_rank_metrics_seg_f32(const float* pos, const int32_t* pos_ptr, int32_t n_pos_total,
                                       const float* neg, const int32_t* neg_ptr, int32_t n_neg_total,
                                       int32_t n_seg, int32_t k, int32_t mode, double* out, void* workspace,
                                       int64_t workspace_bytes, void* stream) {
    if (n_seg <= 0 || n_pos_total < 0 || n_neg_total < 0 || k < 1 || !out || !workspace) return DG_EINVAL;
    if (!pos_ptr || !neg_ptr) return DG_EINVAL;
    if (mode != DG_RANK_LOGIT && mode != DG_RANK_SIGMOID64 && mode != DG_RANK_SIGMOID32) return DG_EINVAL;
    if (workspace_bytes < dg_rank_metrics_seg_workspace(n_pos_total, n_neg_total, n_seg)) return DG_EINVAL;
    if ((n_pos_total > 0 && !pos) || (n_neg_total > 0 && !neg)) return DG_EINVAL;
    if ((int64_t)n_pos_total + n_neg_total + 256LL * n_seg >= (1ll << 31)) return DG_EINVAL;  // 32-bit offsets
    if (!dg::aligned16(workspace)) return DG_EALIGN;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    SegRankArgs a{};
    double* keys = static_cast<double*>(workspace);
    a.kp = keys;
    a.kn = keys + n_pos_total;
    a.counts = reinterpret_cast<int*>(keys + (int64_t)n_pos_total + n_neg_total + 1);
    a.pos_ptr = pos_ptr;
    a.neg_ptr = neg_ptr;
    a.out = out;
    a.n_pos = n_pos_total;
    a.n_neg = n_neg_total;
    a.n_seg = n_seg;
    a.n_tiles = (int32_t)dg::seg_tile_grid(n_pos_total, n_seg, 256);
    a.k = k;
    const int n_all = n_pos_total + n_neg_total;
    if (n_all > 0)
        hipLaunchKernelGGL(score_key_seg_kernel, dim3(dg::ceil_div(n_all, 256)), dim3(256), 0, st, pos, n_pos_total,
                           neg, n_neg_total, mode, keys);
    if (n_pos_total > 0)
        hipLaunchKernelGGL(rank_counts_seg_kernel, dim3(a.n_tiles), dim3(256), 0, st, a);
    hipLaunchKernelGGL(rank_reduce_seg_kernel, dim3(n_seg), dim3(256), 0, st, a);
    return dg::launch_status();
}

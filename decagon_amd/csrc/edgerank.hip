// Filtered rank of held-out edges: for every query (r, c) of a relation k, where column c stands
// among the permitted columns c' of row r under
//   s_k[r, c'] = (E_i[r] ∘ l_k)ᵀ · G_k · (l_k ∘ E_j[c'])
// — the rank behind mean reciprocal rank and Hits@k — without ever forming an N_i×N_j matrix.
//
// Replaces (paths relative to the reference root):
//   session.run(predictions) of one relation, a dense mask of the known edges and a count on the
//   host, once per relation                            main/Predictor/NpPredictor.py:293-313
//
// Form.  One workgroup (4 waves) per 32-query tile of one segment (segmap.h) and per column
// split.  It forms A = ((U ∘ l)·G) ∘ l of its 32 query rows once on v_mfma_f32_32x32x2_f32 into LDS
// (rank_walk.h's A block, the one topk.hip and nodetopk.hip form, so that a query's score has the
// bits dg_decoder_topk_f32 returns for the pair); wave 0 gets the 32 true scores as the diagonal of
// one more tile whose B operand is the gathered rows E_j[c_q].  The waves then take rank_walk.h's
// walk over the split's column tiles: contiguous runs, in blocks of 16 tiles whose row masks of
// countable columns (inside the table, not excluded, not c, not r under NO_SELF) are built first.
// What this file adds to the walk is the count: a mask's popcount is the tile's share of `cand`,
// and it gates the comparison of every accumulator element with its row's true score and column.
// The comparisons are counted with ballots, so a wave's 32 rank counts live in scalar registers;
// waves are combined with integer LDS adds and splits with integer global adds — sums commute,
// there is no float atomic.
#include "common.h"
#include "decagon_hip_ext.h"
#include "rank_walk.h"

namespace {

using dg::f32x16;
using dg::kBlock;
using dg::load_half_row;

constexpr int kWaves = 4;         // waves per workgroup: column runs per split
constexpr int kWaveMinTiles = 2;  // column tiles a wave keeps at least when the columns are split

struct EdgeRankArgs {
    const float* row_table;
    const float* col_table;
    dg::RelOps ops;
    const int32_t* row_idx;
    const int32_t* col_idx;
    const int32_t* seg_ptr;
    const int32_t* seg_rel;
    const int32_t* ex_rowptr;
    const int32_t* ex_col;
    int32_t* out_rank;
    float* out_score;
    int32_t* out_cand;
    int64_t ld_row, ld_col;
    int32_t n_rows, n_cols, n_seg, n_queries, n_split, flags;
};

// d = 32 fits the 128 registers of 4 workgroups a CU without a spill (3 otherwise); d = 64 does
// not, and stays at 2.
template <int D>
__global__ __launch_bounds__(256, D == 32 ? 4 : 2) void edge_rank_kernel(const EdgeRankArgs a) {
    constexpr int H = D / 2;
    constexpr int LDA = dg::a_ld(D);
    __shared__ __attribute__((aligned(16))) float As[32 * LDA];
    __shared__ __attribute__((aligned(16))) uint32_t s_mask[kWaves][kBlock][32];  // a wave's row masks of one block of tiles
    __shared__ float s_ts[32];  // true score of query row i
    __shared__ int s_tc[32];    // true column
    __shared__ int s_rank[32], s_cand[32];

    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int i = lane & 31, h = lane >> 5;
    const int split = blockIdx.y;
    dg::QueryTile qt;
    if (!dg::query_tile(a.seg_ptr, a.seg_rel, a.n_seg, a.n_queries, a.ops.n_rel, (int)blockIdx.x, i, qt)) return;
    const int p = qt.p;
    const bool in_seg = qt.in_seg;
    const float nan = __builtin_nanf("");
    if (qt.dead) {  // the whole segment: rank 0, cand 0, NaN
        if (split == 0 && threadIdx.x < 32 && in_seg) {
            if (a.n_split == 1) {  // (split outputs were zeroed by the call)
                a.out_rank[p] = 0;
                if (a.out_cand) a.out_cand[p] = 0;
            }
            if (a.out_score) a.out_score[p] = nan;
        }
        return;
    }
    const int k = qt.k;
    const float* G = dg::rel_G(a.ops, k);
    const float* l = dg::rel_l(a.ops, k);

    int r = in_seg ? a.row_idx[p] : 0, c = in_seg ? a.col_idx[p] : 0;
    const bool ok = in_seg && r >= 0 && r < a.n_rows && c >= 0 && c < a.n_cols;
    if (!ok) r = c = 0;

    // this wave's run of column tiles inside the split's, this lane's exclusion cursor at the
    // run's first tile and the first tile's rows — in flight behind the A stripe and the true scores
    int n_ct, t0, t1;
    dg::tile_run(a.n_cols, split * kWaves + w, a.n_split * kWaves, n_ct, t0, t1);
    int pc = 0, pe = 0;
    if (a.ex_rowptr && ok) dg::excl_cursor(a.ex_rowptr, a.ex_col, (int64_t)k * a.n_rows + r, t0, pc, pe);
    float b[H];
    dg::load_col_tile<H>(a.col_table, a.ld_col, a.n_cols, n_ct, t0 < t1 ? t0 : n_ct, i, h, b);

    // A of the 32 query rows, 32 columns per wave
    if (w < D / 32) {
        float u[H];
        load_half_row<H>(a.row_table + (int64_t)r * a.ld_row + H * h, ok, u);
        dg::a_block<D>(u, G, l, w, i, h, As);
    }
    if (threadIdx.x < 32) {
        s_tc[i] = c;
        s_rank[i] = 0;
        s_cand[i] = 0;
    }
    __syncthreads();

    float af[H];
    load_half_row<H>(As + i * LDA + H * h, true, af);

    if (w == 0) {  // the true scores: the diagonal of A · (gathered rows E_j[c_q])ᵀ
        float bt[H];
        load_half_row<H>(a.col_table + (int64_t)c * a.ld_col + H * h, ok, bt);
        const f32x16 acc = dg::tile_scores<H>(af, bt);
#pragma unroll
        for (int q = 0; q < 16; ++q)
            if (dg::acc_row(q, h) == i) s_ts[i] = acc[q];
    }
    __syncthreads();

    float ts[16];  // of the 16 tile rows this lane's accumulator registers hold
    int tc[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        ts[q] = s_ts[dg::acc_row(q, h)];
        tc[q] = s_tc[dg::acc_row(q, h)];
    }

    const bool no_self = (a.flags & DG_EDGE_RANK_NO_SELF) != 0;
    int cand = 0;        // countable columns of query row i in this wave's run
    int rk[2][16] = {};  // wave-uniform: candidates before the true column, per tile row acc_row(q, half)
    uint32_t* mask = &s_mask[w][0][0];
    float bn[H];
#pragma unroll 1
    for (int tb = t0; tb < t1; tb += kBlock) {  // the run in blocks of kBlock tiles: masks first, then the walk
        const int nt = t1 - tb < kBlock ? t1 - tb : kBlock;
        dg::wave_lds_sync();  // the previous block's masks have been read
        if (h == 0)
            dg::build_masks(mask, i, tb, nt, a.n_cols, a.ex_col, pc, pe, [&](int ct, uint32_t m) {
                if ((c >> 5) == ct) m &= ~(1u << (c & 31));             // not c
                if (no_self && (r >> 5) == ct) m &= ~(1u << (r & 31));  // not r under NO_SELF
                return m;
            });
        dg::wave_lds_sync();
#pragma unroll 1
        for (int t = 0; t < nt; ++t) {
            const int ct = tb + t;
            // next tile's rows in flight behind this tile's MFMAs
            dg::load_col_tile<H>(a.col_table, a.ld_col, a.n_cols, n_ct, ct + 1 < t1 ? ct + 1 : n_ct, i, h, bn);
            const f32x16 acc = dg::tile_scores<H>(af, b);
            cand += __popc(mask[t * 32 + i]);
            uint32_t mr[16];
            dg::row_masks(mask + t * 32, h, mr);
            const int col = (int)((uint32_t)ct * 32u + (uint32_t)i);
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const float sc = acc[q];  // (−0 == +0 in fp32; no short circuit: straight-line code)
                const bool before = (sc > ts[q]) | ((sc == ts[q]) & (col < tc[q]));
                const uint64_t mb = __ballot(before & (((mr[q] >> i) & 1u) != 0));
                rk[0][q] += __popc((uint32_t)mb);
                rk[1][q] += __popc((uint32_t)(mb >> 32));
            }
#pragma unroll
            for (int u = 0; u < H; ++u) b[u] = bn[u];
        }
    }

    int mine = 0;  // lane i: the wave's count of query row i
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        if (dg::acc_row(q, 0) == i) mine = rk[0][q];
        if (dg::acc_row(q, 1) == i) mine = rk[1][q];
    }
    if (h == 0) {
        atomicAdd(&s_rank[i], mine);
        atomicAdd(&s_cand[i], cand);
    }
    __syncthreads();
    if (threadIdx.x < 32 && in_seg) {
        const int first = split == 0 ? 1 : 0;  // the true column itself: rank 1, one candidate
        if (a.n_split == 1) {
            a.out_rank[p] = ok ? 1 + s_rank[i] : 0;
            if (a.out_cand) a.out_cand[p] = ok ? 1 + s_cand[i] : 0;
        } else if (ok) {
            atomicAdd(a.out_rank + p, first + s_rank[i]);
            if (a.out_cand) atomicAdd(a.out_cand + p, first + s_cand[i]);
        }
        if (split == 0 && a.out_score) {
            float v = s_ts[i];
            if (__float_as_uint(v) == 0x80000000u) v = 0.f;  // −0 is returned as +0
            a.out_score[p] = ok ? v : nan;
        }
    }
}

}  // namespace

extern "C" int dg_decoder_edge_rank_f32(const float* row_table, int64_t ld_row, int32_t n_rows,
                                        const float* col_table, int64_t ld_col, int32_t n_cols,
                                        const int32_t* row_idx, const int32_t* col_idx, const int32_t* seg_ptr,
                                        const int32_t* seg_rel, int32_t n_seg, int32_t n_queries, const float* G,
                                        int64_t g_stride, const float* l, int64_t l_stride, int32_t n_rel,
                                        int32_t d, const int32_t* excl_rowptr, const int32_t* excl_col,
                                        int32_t flags, int32_t* out_rank, float* out_score, int32_t* out_cand,
                                        void* stream) {
    if (n_queries > 0 && (!col_idx || !out_rank)) return DG_EINVAL;
    EdgeRankArgs a{};
    const int rc = dg::check_rank_call(row_table, ld_row, n_rows, col_table, ld_col, n_cols, row_idx, seg_ptr, seg_rel,
                                       n_seg, n_queries, G, g_stride, l, l_stride, n_rel, d, excl_rowptr, excl_col,
                                       flags, DG_EDGE_RANK_NO_SELF, DG_EDGE_RANK_NO_SPLIT, a.ops);
    if (rc != DG_OK) return rc;
    if (n_queries == 0) return DG_OK;

    a.row_table = row_table;
    a.col_table = col_table;
    a.row_idx = row_idx;
    a.col_idx = col_idx;
    a.seg_ptr = seg_ptr;
    a.seg_rel = seg_rel;
    a.ex_rowptr = excl_rowptr;
    a.ex_col = excl_col;
    a.out_rank = out_rank;
    a.out_score = out_score;
    a.out_cand = out_cand;
    a.ld_row = ld_row;
    a.ld_col = ld_col;
    a.n_rows = n_rows;
    a.n_cols = n_cols;
    a.n_seg = n_seg;
    a.n_queries = n_queries;
    a.flags = flags;
    const int64_t n_tiles = dg::seg_tile_grid(n_queries, n_seg, 32);
    a.n_split = dg::column_splits(n_tiles, dg::ceil_div(n_cols, 32), kWaves, kWaveMinTiles,
                                  !(flags & DG_EDGE_RANK_NO_SPLIT));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (a.n_split > 1) {  // the splits add their counts onto zeroes
        hipError_t e = hipMemsetAsync(out_rank, 0, sizeof(int32_t) * (size_t)n_queries, st);
        if (e == hipSuccess && out_cand) e = hipMemsetAsync(out_cand, 0, sizeof(int32_t) * (size_t)n_queries, st);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return static_cast<int>(e);
        }
    }
    const dim3 grid((unsigned)n_tiles, (unsigned)a.n_split);
    if (d == 32)
        hipLaunchKernelGGL(edge_rank_kernel<32>, grid, dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL(edge_rank_kernel<64>, grid, dim3(256), 0, st, a);
    return dg::launch_status();
}

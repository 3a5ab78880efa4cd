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
// split.  It forms A = ((U ∘ l)·G) ∘ l of its 32 query rows once on v_mfma_f32_32x32x2_f32 into LDS,
// exactly as topk.hip forms a stripe's; wave 0 gets the 32 true scores as the diagonal of one more
// tile whose B operand is the gathered rows E_j[c_q].  The column tiles of the split are dealt to
// the waves in contiguous runs (each lane's cursor into its query's sorted exclusion row then
// starts at one lower bound and never skips another wave's columns).  A wave takes its run in
// blocks of 16 tiles.  First the lane that owns query row i builds the row's 32-bit masks of
// countable columns (inside the table, not excluded, not c, not r under NO_SELF) of the whole block
// in LDS, fetching the sorted exclusion row 8 entries per round trip — walking it one dependent
// load per entry beside the tiles, as topk.hip does, cost more than the MFMAs.  Then
// it walks the tiles, the next tile's rows in flight behind the current MFMAs: a mask's popcount is
// the tile's share of `cand`, and it gates the comparison of every accumulator element with its
// row's true score and column.  The comparisons are counted with ballots, so a wave's 32 rank
// counts live in scalar registers; waves are combined with integer LDS adds and splits with
// integer global adds — sums commute, there is no float atomic.
//
// topk.hip's two short routines (the half-row load and the A stripe) are restated here: that
// file's generated code is measured and pinned by exact tests, and this one must form A with the
// same arithmetic so that a query's score has the bits dg_decoder_topk_f32 returns for the pair.
#include "common.h"
#include "decagon_hip_ext.h"
#include "rel_operands.h"
#include "segmap.h"
#include "topk_list.h"

namespace {

using dg::f32x16;

constexpr int kWaves = 4;          // waves per workgroup: column runs per split
constexpr int kSplitGrid = 1024;   // workgroups a call wants before it stops splitting (4 per CU)
constexpr int kSplitMinTiles = 8;  // column tiles a split keeps at least (2 per wave)
constexpr int kBlock = 16;         // column tiles whose row masks a wave builds at once (2 KiB of LDS a wave)
constexpr int kBatch = 8;          // exclusion entries a lane fetches per round trip

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

// MFMA s of a 32×32 tile takes k = H·h + s from lane half h, as in topk.hip.  d = 32 fits the 128
// registers of 4 workgroups a CU without a spill (3 otherwise); d = 64 does not, and stays at 2.
template <int D>
__global__ __launch_bounds__(256, D == 32 ? 4 : 2) void edge_rank_kernel(const EdgeRankArgs a) {
    constexpr int H = D / 2;
    constexpr int LDA = D + 4;  // padded: 16-byte rows that do not all start on one bank
    __shared__ __attribute__((aligned(16))) float As[32 * LDA];
    __shared__ __attribute__((aligned(16))) uint32_t s_mask[kWaves][kBlock][32];  // a wave's row masks of one block of tiles
    __shared__ float s_ts[32];  // true score of query row i
    __shared__ int s_tc[32];    // true column
    __shared__ int s_rank[32], s_cand[32];

    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int i = lane & 31, h = lane >> 5;
    const int split = blockIdx.y;
    int s, local;
    if (!dg::seg_tile_find(a.seg_ptr, a.n_seg, 32, (int)blockIdx.x, s, local)) return;
    s = __builtin_amdgcn_readfirstlane(s);
    int beg, end;
    if (!dg::seg_bounds(a.seg_ptr, a.n_queries, s, beg, end)) return;
    const int p0 = beg + local * 32;
    if (p0 >= end) return;
    const int p = p0 + i;
    const bool in_seg = p < end;
    const float nan = __builtin_nanf("");
    int k;
    if (!dg::seg_relation(a.seg_rel, a.ops.n_rel, s, k)) {  // the whole segment: rank 0, cand 0, NaN
        if (split == 0 && threadIdx.x < 32 && in_seg) {
            if (a.n_split == 1) {  // (split outputs were zeroed by the call)
                a.out_rank[p] = 0;
                if (a.out_cand) a.out_cand[p] = 0;
            }
            if (a.out_score) a.out_score[p] = nan;
        }
        return;
    }
    const float* G = dg::rel_G(a.ops, k);
    const float* l = dg::rel_l(a.ops, k);

    int r = in_seg ? a.row_idx[p] : 0, c = in_seg ? a.col_idx[p] : 0;
    const bool ok = in_seg && r >= 0 && r < a.n_rows && c >= 0 && c < a.n_cols;
    if (!ok) r = c = 0;

    // this wave's contiguous run of column tiles inside the split's
    const int n_ct = (int)(((int64_t)a.n_cols + 31) >> 5);
    const int slot = split * kWaves + w, n_slots = a.n_split * kWaves;
    const int t0 = (int)((int64_t)n_ct * slot / n_slots), t1 = (int)((int64_t)n_ct * (slot + 1) / n_slots);

    // this lane's cursor into the exclusion row of query row i (columns ascending), at the run's
    // first tile; and the first tile's rows — both in flight behind the A stripe and the true scores
    int pc = 0, pe = 0;
    if (a.ex_rowptr && ok) {
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
    auto load_b = [&](int t, float(&x)[H]) {
        const uint32_t col = (uint32_t)t * 32u + (uint32_t)i;
        const bool in = t < n_ct && col < (uint32_t)a.n_cols;
        load_half_row<H>(a.col_table + (int64_t)(in ? col : 0u) * a.ld_col + H * h, in, x);
    };
    float b[H], bn[H];
    load_b(t0 < t1 ? t0 : n_ct, b);

    // A = ((U ∘ l)·G) ∘ l of the 32 query rows, 32 columns per wave (topk.hip's stripe, one block)
    if (w < D / 32) {
        const int nb = w;
        float u[H];
        load_half_row<H>(a.row_table + (int64_t)r * a.ld_row + H * h, ok, u);
        f32x16 acc = {};
#pragma unroll
        for (int t = 0; t < H; ++t) {
            const int kk = H * h + t;
            const float av = l ? u[t] * l[kk] : u[t];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, G[kk * D + nb * 32 + i], acc, 0, 0, 0);
        }
        const float lj = l ? l[nb * 32 + i] : 1.0f;
#pragma unroll
        for (int q = 0; q < 16; ++q) As[dg::acc_row(q, h) * LDA + nb * 32 + i] = acc[q] * lj;
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
        f32x16 acc = {};
#pragma unroll
        for (int t = 0; t < H; ++t) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af[t], bt[t], acc, 0, 0, 0);
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
#pragma unroll 1
    for (int tb = t0; tb < t1; tb += kBlock) {  // the run in blocks of kBlock tiles: masks first, then the walk
        const int nt = t1 - tb < kBlock ? t1 - tb : kBlock;
        dg::wave_lds_sync();  // the previous block's masks have been read
        if (h == 0) {
            // row i's countable columns of every tile of the block, before the exclusion ...
#pragma unroll 1
            for (int t = 0; t < nt; ++t) {
                const int ct = tb + t;
                const uint32_t left = (uint32_t)a.n_cols - (uint32_t)ct * 32u;  // ≥ 1: columns from the tile's first on
                uint32_t m = left >= 32u ? ~0u : (1u << left) - 1u;
                if ((c >> 5) == ct) m &= ~(1u << (c & 31));
                if (no_self && (r >> 5) == ct) m &= ~(1u << (r & 31));
                s_mask[w][t][i] = m;
            }
            // ... and without the excluded ones: kBatch entries of the sorted row per round trip,
            // until one lies past the block
            bool more = pc < pe;
            while (more) {
                int e[kBatch];
#pragma unroll
                for (int j = 0; j < kBatch; ++j) e[j] = a.ex_col[pc + j < pe ? pc + j : pe - 1];
                int used = 0;
#pragma unroll
                for (int j = 0; j < kBatch; ++j) {
                    const int t = (e[j] >> 5) - tb;
                    const bool live = pc + j < pe && t < nt;
                    if (live && t >= 0) atomicAnd(&s_mask[w][t][i], ~(1u << (e[j] & 31)));
                    used += live;
                }
                pc += used;
                more = used == kBatch && pc < pe;
            }
        }
        dg::wave_lds_sync();
#pragma unroll 1
        for (int t = 0; t < nt; ++t) {
            const int ct = tb + t;
            load_b(ct + 1 < t1 ? ct + 1 : n_ct, bn);  // next tile's rows in flight behind this tile's MFMAs
            f32x16 acc = {};
#pragma unroll
            for (int u = 0; u < H; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af[u], b[u], acc, 0, 0, 0);
            cand += __popc(s_mask[w][t][i]);
            uint32_t mr[16];  // mr[q]: the mask of tile row acc_row(q, h) = (q & 3) + 8·(q >> 2) + 4·h
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const uint4 v = *reinterpret_cast<const uint4*>(&s_mask[w][t][8 * g + 4 * h]);
                mr[4 * g] = v.x;
                mr[4 * g + 1] = v.y;
                mr[4 * g + 2] = v.z;
                mr[4 * g + 3] = v.w;
            }
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
    if (n_seg <= 0 || n_queries < 0 || (d != 32 && d != 64)) return DG_EINVAL;
    if (!row_table || !col_table || !seg_ptr || !G) return DG_EINVAL;
    if (n_queries > 0 && (!row_idx || !col_idx || !out_rank)) return DG_EINVAL;
    if (n_rows < 1 || n_cols < 1 || ld_row < d || ld_col < d) return DG_EINVAL;
    EdgeRankArgs a{};
    if (dg::rel_ops(G, g_stride, l, l_stride, n_rel, d, seg_rel != nullptr, n_seg, a.ops) != DG_OK) return DG_EINVAL;
    if ((excl_rowptr == nullptr) != (excl_col == nullptr)) return DG_EINVAL;
    if (excl_rowptr && !seg_rel && n_seg > n_rel) return DG_EINVAL;  // segment s reads exclusion relation s
    if (flags & ~(DG_EDGE_RANK_NO_SELF | DG_EDGE_RANK_NO_SPLIT)) return DG_EINVAL;
    if ((flags & DG_EDGE_RANK_NO_SELF) && n_rows != n_cols) return DG_EINVAL;
    if ((int64_t)n_queries + 32LL * n_seg >= (1ll << 31)) return DG_EINVAL;  // 32-bit query offsets
    if (!dg::aligned16(row_table) || !dg::aligned16(col_table) || (ld_row & 3) || (ld_col & 3)) return DG_EALIGN;
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
    const int n_ct = dg::ceil_div(n_cols, 32);
    int64_t n_split = 1;
    if (!(flags & DG_EDGE_RANK_NO_SPLIT) && n_tiles < kSplitGrid) {
        n_split = (kSplitGrid + n_tiles - 1) / n_tiles;
        const int64_t most = n_ct / kSplitMinTiles;
        if (n_split > most) n_split = most;
        if (n_split < 1) n_split = 1;
    }
    a.n_split = (int32_t)n_split;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (n_split > 1) {  // the splits add their counts onto zeroes
        hipError_t e = hipMemsetAsync(out_rank, 0, sizeof(int32_t) * (size_t)n_queries, st);
        if (e == hipSuccess && out_cand) e = hipMemsetAsync(out_cand, 0, sizeof(int32_t) * (size_t)n_queries, st);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return static_cast<int>(e);
        }
    }
    const dim3 grid((unsigned)n_tiles, (unsigned)n_split);
    if (d == 32)
        hipLaunchKernelGGL(edge_rank_kernel<32>, grid, dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL(edge_rank_kernel<64>, grid, dim3(256), 0, st, a);
    return dg::launch_status();
}

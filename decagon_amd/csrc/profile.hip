// The profile of node pairs: for given pairs (r, c), the score of EVERY relation of one edge type,
//   out[p, s] = (E_i[r_p] ∘ l_k)ᵀ · G_k · (l_k ∘ E_j[c_p]),   k = rel_idx[s],
// and the best columns of every row of such a matrix (a pair's likeliest relations).
//
// Replaces (paths relative to the reference root):
//   NpPredictor(relationId)._predictEdges: E·D·R·D·Eᵀ of ONE relation, then the wanted entries
//                                          main/Predictor/NpPredictor.py:293-313
//   the loop of that over relations in _write_as_parquet, and the per-relation
//   session.run(predictions) of DecagonAccuracyEvaluator._computePredictions
// which here was dg_decoder_score_seg_f32 over K segments that each repeat the same pairs.
//
// Scorer.  One wave owns one 32-pair tile and a chunk of C ≤ 32 consecutive slots.  It gathers the
// tile's U and V rows once (and, where G is shared, its G fragments once) and keeps them in
// registers while it walks its slots; per slot it loads l_k (and G_k when G is per relation),
// scales, runs the MFMA chain and reduces.  The arithmetic of a score is dg::score_tile's
// (decoder_tile.h), operation for operation: av = u·l as one fp32 product, the
// v_mfma_f32_32x32x2_f32 chain in score_tile's k order (k = 16h + s in one block at d = 32; the
// n-block / k-block loops with k = k0 + 2s + h at d = 64), part = fmaf(acc·l_j, v, part), then
// dg::reduce_scatter32, the tree score_tile itself calls.  Only the loads are hoisted.  An MFMA row
// is independent of the other rows and the tree has one shape for every slot, so every out[p, s]
// equals dg_decoder_score_f32 on that pair with G_k, l_k bit for bit, for any pair order and tail.
// The 32 × C scores pass through the wave's own LDS slice and leave as contiguous pieces of the
// rows of `out` (128 B at C = 32) instead of 4-byte stores at stride ld_out.
//
// Row top-k.  One wave per row reads the row once, coalesced, through the list of topk_list.h
// (append above the threshold, sort when full, truncate) under the keys of dg_decoder_topk_f32
// with the column as the index: the unique top-k of the row whatever the tiling.
// dg_row_topk_excl_f32 selects among the columns a per-row ascending list does not name (a pair's
// known relations — what the reference drops on the host after _predictEdges per relation id): a
// sibling kernel merges the list into the same single pass, row_topk_kernel itself is untouched.
#include "common.h"
#include "decoder_tile.h"
#include "rel_operands.h"
#include "segmap.h"
#include "topk_list.h"

namespace {

using dg::f32x16;

constexpr int kSlotMax = 32;        // slots per wave at most: one LDS slice, one 128-byte row piece
constexpr int kSlotMin = 4;         // … and at least (a 16-byte row piece), when the grid is small
constexpr int kWavesWanted = 2048;  // 256 CUs × 4 SIMDs × 2 waves: below it the slot chunk is halved
constexpr int kLdTile = kSlotMax + 1;  // padded LDS row: the 32 pairs of one slot fall on 32 banks

// The slot chunk C of a launch: the largest of 32, 16, 8, 4 whose grid of ⌈P/32⌉ × ⌈n_sel/C⌉ waves
// still fills the chip, so that a few pairs against many relations do not run on a few SIMDs.
inline int slot_chunk(int64_t n_pairs, int64_t n_sel) {
    const int64_t tiles = (n_pairs + 31) / 32;
    int c = kSlotMax;
    while (c > kSlotMin && tiles * ((n_sel + c - 1) / c) < kWavesWanted) c >>= 1;
    return c;
}

struct CrossArgs {
    const float* row_table;
    const float* col_table;
    dg::RelOps ops;
    const int32_t* row_idx;
    const int32_t* col_idx;
    const int32_t* rel_idx;
    float* out;
    int64_t ld_row, ld_col, ld_out;
    int32_t n_rows, n_cols, n_pairs, n_sel, chunk, n_chunks, n_waves, l_vec4;
};

// The B fragments of one d×d G for every (n-block, k-block) of score_tile's loops:
// b[(nb·KB + kb)·16 + s] = G[k][32·nb + i], k = 16h + s at d = 32 and 32·kb + 2s + h at d = 64.
template <int D>
__device__ __forceinline__ void load_g(const float* G, int i, int h, float (&b)[D * D / 64]) {
    constexpr int NB = D / 32;
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int kb = 0; kb < NB; ++kb)
#pragma unroll
            for (int s = 0; s < 16; ++s) {
                const int k = D == 32 ? 16 * h + s : 32 * kb + 2 * s + h;
                b[(nb * NB + kb) * 16 + s] = G[k * D + 32 * nb + i];
            }
}

// l_k at this lane's k values, in the order of the lane's U elements, and at its columns.
template <int D>
__device__ __forceinline__ void load_l(const float* l, bool vec4, int i, int h, float (&w)[D / 2],
                                       float (&lj)[D / 32]) {
#pragma unroll
    for (int nb = 0; nb < D / 32; ++nb) lj[nb] = l[32 * nb + i];
    if (D == 32 && vec4) {
        const float4* l4 = reinterpret_cast<const float4*>(l + 16 * h);
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) dg::put4(w + 4 * s4, l4[s4]);
    } else {
#pragma unroll
        for (int q = 0; q < D / 2; ++q) w[q] = l[D == 32 ? 16 * h + q : 2 * q + h];
    }
}

template <int D, bool kPerG, bool kHasL>
__global__ __launch_bounds__(256) void score_cross_kernel(const CrossArgs a) {
    constexpr int NB = D / 32;  // n-blocks = k-blocks
    constexpr int H = D / 2;    // U elements a lane holds
    __shared__ float tile[4][32][kLdTile];

    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int gw = blockIdx.x * 4 + w;
    if (gw >= a.n_waves) return;  // (no workgroup barrier below: the waves are independent)
    // chunks of one pair tile are neighbours: they gather the same rows
    const int pt = gw / a.n_chunks;
    const int s0 = (gw - pt * a.n_chunks) * a.chunk;
    const int cnt = min(a.chunk, a.n_sel - s0);
    const int p0 = pt * 32;
    const int i = lane & 31;
    const int h = lane >> 5;

    const int p = p0 + i;
    const bool in_tile = p < a.n_pairs;
    int r = in_tile ? a.row_idx[p] : 0, c = in_tile ? a.col_idx[p] : 0;
    const bool ok = r >= 0 && r < a.n_rows && c >= 0 && c < a.n_cols;
    if (!ok) r = c = 0;  // (scored on row 0, stored as NaN)

    // the tile's operands, once: U in the lane order of the A operand, V in the order of the
    // accumulator's rows
    float u[H], v[NB][16];
    const float* up = a.row_table + (int64_t)r * a.ld_row;
    if (D == 32) {
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) dg::put4(u + 4 * s4, *reinterpret_cast<const float4*>(up + 16 * h + 4 * s4));
    } else {
#pragma unroll
        for (int q = 0; q < H; ++q) u[q] = up[2 * q + h];
    }
#pragma unroll
    for (int rr = 0; rr < 16; ++rr) {
        const int prow = dg::acc_row(rr, h);
        const float* vp = a.col_table + (int64_t)__shfl(c, prow) * a.ld_col + i;  // lane prow names pair prow
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) v[nb][rr] = vp[32 * nb];
    }
    float b[D * D / 64];
    if (!kPerG) load_g<D>(a.ops.G, i, h, b);

    // lane 2q holds score q of its half; the pair it belongs to is named by lane `slot`
    const int q = i >> 1;
    const int slot = dg::acc_row(q, h);
    const bool slot_ok = __shfl((int)ok, slot) != 0;

#pragma unroll 1
    for (int j = 0; j < cnt; ++j) {
        int k;
        const bool rel_ok = dg::seg_relation(a.rel_idx, a.ops.n_rel, s0 + j, k);
        if (!rel_ok) k = 0;
        float wl[H], lj[NB];
        if (kHasL) load_l<D>(dg::rel_l(a.ops, k), a.l_vec4 != 0, i, h, wl, lj);
        if (kPerG) load_g<D>(dg::rel_G(a.ops, k), i, h, b);
        float av[H];
#pragma unroll
        for (int x = 0; x < H; ++x) av[x] = kHasL ? u[x] * wl[x] : u[x];
        float part[16];
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) part[rr] = 0.f;
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            f32x16 acc = {};
#pragma unroll
            for (int kb = 0; kb < NB; ++kb)
#pragma unroll
                for (int s = 0; s < 16; ++s)
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[kb * 16 + s], b[(nb * NB + kb) * 16 + s], acc, 0, 0,
                                                               0);
            const float ljn = kHasL ? lj[nb] : 1.0f;
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) part[rr] = fmaf(acc[rr] * ljn, v[nb][rr], part[rr]);
        }
        const float sc = dg::reduce_scatter32(part);
        if ((i & 1) == 0) tile[w][slot][j] = (slot_ok && rel_ok) ? sc : __builtin_nanf("");
    }
    dg::wave_lds_sync();
    // rows of `out`: lane half h writes pair 2t + h, lane i its slot i — cnt contiguous floats
#pragma unroll 4
    for (int t = 0; t < 16; ++t) {
        const int pr = 2 * t + h;
        if (p0 + pr < a.n_pairs && i < cnt) a.out[(int64_t)(p0 + pr) * a.ld_out + s0 + i] = tile[w][pr][i];
    }
}

template <int D, bool kPerG>
void launch_cross_l(const CrossArgs& a, hipStream_t st) {
    const dim3 grid((unsigned)dg::ceil_div(a.n_waves, 4)), block(256);
    if (a.ops.l)
        hipLaunchKernelGGL((score_cross_kernel<D, kPerG, true>), grid, block, 0, st, a);
    else
        hipLaunchKernelGGL((score_cross_kernel<D, kPerG, false>), grid, block, 0, st, a);
}

template <int D>
void launch_cross(const CrossArgs& a, hipStream_t st) {
    if (a.ops.g_stride)
        launch_cross_l<D, true>(a, st);
    else
        launch_cross_l<D, false>(a, st);
}

struct RowTopkArgs {
    const float* x;
    float* out_val;
    int32_t* out_idx;
    int32_t* out_count;
    int64_t ld;
    int32_t n_cols, topk, cap;
};

__global__ __launch_bounds__(64) void row_topk_kernel(const RowTopkArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char row_topk_smem[];
    const int lane = threadIdx.x;
    const int64_t row = blockIdx.x;
    const float* x = a.x + row * a.ld;
    dg::WaveTopK tk;
    tk.init(reinterpret_cast<uint64_t*>(row_topk_smem), a.cap, a.topk, lane);
#pragma unroll 1
    for (int c0 = 0; c0 < a.n_cols; c0 += dg::kWave) {
        const int c = c0 + lane;
        const bool ok = c < a.n_cols;
        tk.push(dg::make_key(ok ? x[c] : 0.f, (uint32_t)c), ok);
    }
    tk.compact();
    for (int t = lane; t < a.topk; t += dg::kWave) {
        const uint64_t key = tk.buf[t];
        const int64_t o = row * a.topk + t;
        const bool live = t < tk.n;
        a.out_val[o] = live ? dg::key_score(key) : -__builtin_inff();
        a.out_idx[o] = live ? (int32_t)~(uint32_t)key : -1;
    }
    if (lane == 0) a.out_count[row] = tk.n;
}

struct RowTopkExclArgs {
    RowTopkArgs t;
    const int32_t* excl_ptr;
    const int32_t* excl_slot;
    int32_t excl_nnz;
};

// row_topk_kernel over the columns that the row's ascending list excl_slot[e0, e1) does not name.
// Columns and list both ascend, so the wave merges them: the lanes hold the next 64 entries of the
// list in registers (one coalesced load per 64 entries), the entries that fall into the 64-column
// block at c0 tag position entry − c0 of a 64-entry LDS strip behind the list's buffer with the
// block's number, and lane i pushes its column only when strip[i] does not carry that number.
// The cursor then passes the entries below c0 + 64.  The tag makes a strip entry of an earlier
// block stale by itself, so the strip is cleared once.  Every index is formed from clamped,
// wave-uniform bounds: cur ≤ win + 64 and cur ≤ e1 ≤ excl_nnz hold whatever the list contains, and
// the strip is written only at entry − c0 ∈ [0, 64).
__global__ __launch_bounds__(64) void row_topk_excl_kernel(const RowTopkExclArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char row_topk_excl_smem[];
    const int lane = threadIdx.x;
    const int64_t row = blockIdx.x;
    const float* x = a.t.x + row * a.t.ld;
    dg::WaveTopK tk;
    tk.init(reinterpret_cast<uint64_t*>(row_topk_excl_smem), a.t.cap, a.t.topk, lane);
    int32_t* strip = reinterpret_cast<int32_t*>(row_topk_excl_smem + (size_t)a.t.cap * 8);
    strip[lane] = 0;  // (block numbers start at 1)
    dg::wave_lds_sync();

    int cur = __builtin_amdgcn_readfirstlane(a.excl_ptr[row]);
    int e1 = __builtin_amdgcn_readfirstlane(a.excl_ptr[row + 1]);
    cur = min(max(cur, 0), a.excl_nnz);
    e1 = min(max(e1, cur), a.excl_nnz);  // a non-increasing pair: an empty list
    int win = cur;                       // lane i holds entry win + i, where the list has one
    int32_t ent = lane < e1 - win ? a.excl_slot[(int64_t)win + lane] : 0;
#pragma unroll 1
    for (int c0 = 0; c0 < a.t.n_cols; c0 += dg::kWave) {
        const int c = c0 + lane;
        const bool ok = c < a.t.n_cols;
        const int tag = (c0 >> 6) + 1;
        bool keep = ok;
        if (cur < e1) {  // (wave-uniform)
            const int64_t c_end = (int64_t)c0 + dg::kWave;
            for (;;) {
                const bool below = lane >= cur - win && lane < e1 - win && (int64_t)ent < c_end;
                if (below && ent >= c0) strip[ent - c0] = tag;
                cur += __popcll(__ballot(below));
                if (cur - win < dg::kWave || cur >= e1) break;
                win = cur;  // every held entry lies below the block's end: the next 64
                ent = lane < e1 - win ? a.excl_slot[(int64_t)win + lane] : 0;
            }
            dg::wave_lds_sync();
            keep = ok && strip[lane] != tag;
        }
        tk.push(dg::make_key(ok ? x[c] : 0.f, (uint32_t)c), keep);
    }
    tk.compact();
    for (int t = lane; t < a.t.topk; t += dg::kWave) {
        const uint64_t key = tk.buf[t];
        const int64_t o = row * a.t.topk + t;
        const bool live = t < tk.n;
        a.t.out_val[o] = live ? dg::key_score(key) : -__builtin_inff();
        a.t.out_idx[o] = live ? (int32_t)~(uint32_t)key : -1;
    }
    if (lane == 0) a.t.out_count[row] = tk.n;
}

// The argument checks of both row selections, and the launch arguments when there is work.
int row_topk_args(const float* x, int64_t ld, int32_t n_rows, int32_t n_cols, int32_t topk, float* out_val,
                  int32_t* out_idx, int32_t* out_count, RowTopkArgs& a) {
    if (n_rows < 0 || n_cols < 1 || topk < 1 || topk > DG_TOPK_MAX_K || ld < n_cols) return DG_EINVAL;
    if (n_rows > 0 && (!x || !out_val || !out_idx || !out_count)) return DG_EINVAL;
    a.x = x;
    a.out_val = out_val;
    a.out_idx = out_idx;
    a.out_count = out_count;
    a.ld = ld;
    a.n_cols = n_cols;
    a.topk = topk;
    a.cap = dg::list_cap(topk);
    return DG_OK;
}

}  // namespace

extern "C" int32_t dg_decoder_score_cross_chunk(int32_t n_pairs, int32_t n_sel) {
    if (n_pairs < 0 || n_sel < 1) return 0;
    return slot_chunk(n_pairs, n_sel);
}

extern "C" int dg_decoder_score_cross_f32(const float* row_table, int64_t ld_row, int32_t n_rows,
                                          const float* col_table, int64_t ld_col, int32_t n_cols,
                                          const int32_t* row_idx, const int32_t* col_idx, int32_t n_pairs,
                                          const float* G, int64_t g_stride, const float* l, int64_t l_stride,
                                          const int32_t* rel_idx, int32_t n_sel, int32_t n_rel, int32_t d,
                                          float* out, int64_t ld_out, void* stream) {
    if (!row_table || !col_table || !G) return DG_EINVAL;
    if (n_pairs < 0 || n_sel < 1 || n_rel < 1 || n_rows < 1 || n_cols < 1) return DG_EINVAL;
    if (n_pairs > 0 && (!row_idx || !col_idx || !out)) return DG_EINVAL;
    if (d != 32 && d != 64) return DG_EINVAL;
    if (ld_row < d || ld_col < d || ld_out < n_sel) return DG_EINVAL;
    CrossArgs a{};
    if (dg::rel_ops(G, g_stride, l, l_stride, n_rel, d, rel_idx != nullptr, n_sel, a.ops) != DG_OK) return DG_EINVAL;
    if ((int64_t)n_pairs * ld_out >= DG_CROSS_MAX_OUT || n_pairs > INT32_MAX - 64) return DG_EINVAL;  // 32-bit pair offsets
    if (!dg::aligned16(row_table) || !dg::aligned16(col_table) || (ld_row & 3) || (ld_col & 3)) return DG_EALIGN;
    if (n_pairs == 0) return DG_OK;

    a.row_table = row_table;
    a.col_table = col_table;
    a.row_idx = row_idx;
    a.col_idx = col_idx;
    a.rel_idx = rel_idx;
    a.out = out;
    a.ld_row = ld_row;
    a.ld_col = ld_col;
    a.ld_out = ld_out;
    a.n_rows = n_rows;
    a.n_cols = n_cols;
    a.n_pairs = n_pairs;
    a.n_sel = n_sel;
    a.chunk = slot_chunk(n_pairs, n_sel);
    a.n_chunks = dg::ceil_div(n_sel, a.chunk);
    a.n_waves = dg::ceil_div(n_pairs, 32) * a.n_chunks;  // < 2^29 under DG_CROSS_MAX_OUT
    a.l_vec4 = l && dg::aligned16(l);                   // (l_stride is 0 or d: every l_k is aligned with l)
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (d == 32)
        launch_cross<32>(a, st);
    else
        launch_cross<64>(a, st);
    return dg::launch_status();
}

extern "C" int64_t dg_row_topk_workspace(int32_t n_rows, int32_t n_cols, int32_t topk) {
    (void)n_rows, (void)n_cols, (void)topk;
    return 0;  // the lists live in LDS
}

extern "C" int dg_row_topk_f32(const float* x, int64_t ld, int32_t n_rows, int32_t n_cols, int32_t topk,
                               float* out_val, int32_t* out_idx, int32_t* out_count, void* workspace,
                               int64_t workspace_bytes, void* stream) {
    (void)workspace, (void)workspace_bytes;
    RowTopkArgs a{};
    if (row_topk_args(x, ld, n_rows, n_cols, topk, out_val, out_idx, out_count, a) != DG_OK) return DG_EINVAL;
    if (n_rows == 0) return DG_OK;
    hipLaunchKernelGGL(row_topk_kernel, dim3((unsigned)n_rows), dim3(64), a.cap * 8,
                       reinterpret_cast<hipStream_t>(stream), a);
    return dg::launch_status();
}

extern "C" int dg_row_topk_excl_f32(const float* x, int64_t ld, int32_t n_rows, int32_t n_cols, int32_t topk,
                                    const int32_t* excl_ptr, const int32_t* excl_slot, int32_t excl_nnz,
                                    float* out_val, int32_t* out_idx, int32_t* out_count, void* stream) {
    RowTopkExclArgs a{};
    if (row_topk_args(x, ld, n_rows, n_cols, topk, out_val, out_idx, out_count, a.t) != DG_OK) return DG_EINVAL;
    if ((excl_ptr == nullptr) != (excl_slot == nullptr) || excl_nnz < 0) return DG_EINVAL;
    if (n_rows == 0) return DG_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (!excl_ptr || excl_nnz == 0) {  // nothing can be excluded: the unmasked kernel, the same bytes
        hipLaunchKernelGGL(row_topk_kernel, dim3((unsigned)n_rows), dim3(64), a.t.cap * 8, st, a.t);
        return dg::launch_status();
    }
    a.excl_ptr = excl_ptr;
    a.excl_slot = excl_slot;
    a.excl_nnz = excl_nnz;
    hipLaunchKernelGGL(row_topk_excl_kernel, dim3((unsigned)n_rows), dim3(64), a.t.cap * 8 + dg::kWave * 4, st, a);
    return dg::launch_status();
}

// The decoder backward of the cost (hinge or sigmoid cross-entropy: loss_policy.h, whose a_p, b_p
// are used below) for EVERY relation's batch of one edge type in one pass, and the row reduction
// that turns per-pair gradient rows into the embeddings' gradient.
//
// Replaces (paths relative to the reference root):
//   one tf.train.AdamOptimizer.minimize step per (relation, batch)   decagon/deep/optimizer.py:108-114,
//                                                                   decagon/deep/minibatch.py:278-313
// whose decoder half here was dg_decoder_grad_f32 + two dg_scatter_rows_f32 per relation
// (train.hip).  The gradient of a sum of costs is the sum of the gradients, so one step can take a
// batch of every relation; what depends on the relation is only this file's work.
//
// Pairs are packed by SEGMENT (segment s = [seg_ptr[s], seg_ptr[s+1]), relation seg_rel[s]) with
// the conventions of dg_decoder_score_seg_f32 (evalseg.hip) and dealt to waves in 32-pair tiles
// by the virtual-tile map of segmap.h: no prefix sum, nothing read on the host.
//
//   pairs kernel   one wave per tile: (a_p, b_p), then on the exact-fp32 MFMA (v_mfma_f32_32x32x2_f32)
//                    mv[p]        = m_p · L·G·L·v_p                = ((V∘l)·Gᵀ)∘l
//                    grad_cols[p] = L·Gᵀ·L·(b_p·un_p − a_p·u_p)    = ((D∘l)·G)∘l
//                  G_k's fragments are loaded once per wave and serve the tile's 32 pairs.  Hinge:
//                  m_p = a_p = b_p, the mask, so −mv[p] / +mv[p] are the two rows' gradients.  Xent:
//                  m_p = 1 (mv stays one row per pair) and coef[p] = −a_p, coef[n_pairs + p] = +b_p
//                  are stored beside it: the row reduction's `sign` carries the weights.
//   dM kernel      one wave per (segment, 32×32 tile of dM): dM_s = Σ_p (b_p·un_p − a_p·u_p)·v_pᵀ
//                  over the segment's pairs in order (the contraction index of the MFMA chain).
//   vars kernel    dG / dG_diag / dl of every segment's relation from dM_s; and, for a shared G,
//   shared-G sum   dG = Σ_s L_k·dM_s·L_k over 16 contiguous slices of the segment list, each in
//                  segment order, the slices' sums added in slice order.
//
// dg_segment_rows_sum_f32: out[r] += Σ_q sign[q]·src[item[q]] over a node-major occurrence list —
// one workgroup per output row, the list split over the waves in fixed chunks and the waves'
// sums combined in a fixed tree.  No float atomics anywhere: results are bitwise reproducible.
#include "common.h"
#include "loss_policy.h"
#include "rel_operands.h"
#include "segmap.h"

namespace {

using dg::f32x16;

struct GradSegArgs {
    const float* row_table;
    const float* col_table;
    const int32_t* rows;
    const int32_t* cols;
    const int32_t* negs;
    const int32_t* seg_ptr;
    const int32_t* seg_rel;
    const float* pos;
    const float* neg;
    dg::RelOps ops;
    float* mv;
    float* grad_cols;
    float* coef;  // [2·n_pairs] (policies with kCoef)
    float* dM;    // [n_seg][d][d]
    float* dG;
    float* dl;
    float* dG_diag;
    int64_t ld_row, ld_col;
    int32_t n_rows, n_cols, n_seg, n_pairs, n_tiles;
    float param;  // the cost's parameter: margin (hinge), neg_weight (xent)
    int32_t pad;
};

// Pair p's indices and the cost's coefficients (hinge: the mask, inside the tables and
// neg − (pos − margin) > 0; a pair outside the tables has none).  A pair that is not live gets
// index 0 everywhere (a row that exists: loads stay unconditional).
template <class Loss>
__device__ __forceinline__ typename Loss::Coef pair_meta(const GradSegArgs& a, int p, bool in_seg, int& r, int& c,
                                                         int& rn) {
    r = in_seg ? a.rows[p] : 0;
    c = in_seg ? a.cols[p] : 0;
    rn = in_seg ? a.negs[p] : 0;
    const bool ok = in_seg && r >= 0 && r < a.n_rows && rn >= 0 && rn < a.n_rows && c >= 0 && c < a.n_cols;
    const typename Loss::Coef cf =
        in_seg ? Loss::coef(a.pos[p], a.neg[p], a.param, ok) : Loss::coef(0.f, 0.f, 0.f, false);
    if (!Loss::live(cf)) r = c = rn = 0;
    return cf;
}

// One wave per 32-pair tile.  MFMA step j of a k-chunk takes k = (kD/2)·h + j from lane half h
// (the contraction order is free), so a lane's A operands are kD/2 contiguous floats of its
// pair's rows (float4 loads) and its Gᵀ fragment kD/2 contiguous floats of one row of G.
template <int kD, class Loss>
__global__ __launch_bounds__(256) void grad_seg_pairs_kernel(const GradSegArgs a) {
    constexpr int kH = kD / 2;
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
    const float* G = dg::rel_G(a.ops, k);
    const float* l = dg::rel_l(a.ops, k);

    const int i = lane & 31;
    const int h = lane >> 5;
    int r, c, rn;
    const typename Loss::Coef cf = pair_meta<Loss>(a, p0 + i, rel_ok && p0 + i < end, r, c, rn);
    const bool act = Loss::live(cf);
    if constexpr (Loss::kCoef) {
        if (h == 0 && p0 + i < end) {
            a.coef[p0 + i] = -Loss::a(cf);
            a.coef[(int64_t)a.n_pairs + p0 + i] = Loss::b(cf);
        }
    }
    const float4* u4 = reinterpret_cast<const float4*>(a.row_table + (int64_t)r * a.ld_row + kH * h);
    const float4* un4 = reinterpret_cast<const float4*>(a.row_table + (int64_t)rn * a.ld_row + kH * h);
    const float4* v4 = reinterpret_cast<const float4*>(a.col_table + (int64_t)c * a.ld_col + kH * h);
    float xv[kH], xd[kH];
#pragma unroll
    for (int j4 = 0; j4 < kH / 4; ++j4) {
        const float4 uu = u4[j4], nn = un4[j4], vv = v4[j4];
        float4 ll = make_float4(1.f, 1.f, 1.f, 1.f);
        if (l) ll = *reinterpret_cast<const float4*>(l + kH * h + 4 * j4);
        xv[4 * j4] = act ? vv.x * ll.x : 0.f;
        xv[4 * j4 + 1] = act ? vv.y * ll.y : 0.f;
        xv[4 * j4 + 2] = act ? vv.z * ll.z : 0.f;
        xv[4 * j4 + 3] = act ? vv.w * ll.w : 0.f;
        xd[4 * j4] = act ? Loss::diff(cf, nn.x, uu.x) * ll.x : 0.f;
        xd[4 * j4 + 1] = act ? Loss::diff(cf, nn.y, uu.y) * ll.y : 0.f;
        xd[4 * j4 + 2] = act ? Loss::diff(cf, nn.z, uu.z) * ll.z : 0.f;
        xd[4 * j4 + 3] = act ? Loss::diff(cf, nn.w, uu.w) * ll.w : 0.f;
    }
#pragma unroll 1
    for (int n0 = 0; n0 < kD; n0 += 32) {
        // B[k][n] of the two products at column n = n0 + i: Gᵀ (= G[n][k]) and G (= G[k][n])
        float bt[kH], bg[kH];
        const float4* gt4 = reinterpret_cast<const float4*>(G + (int64_t)(n0 + i) * kD + kH * h);
#pragma unroll
        for (int j4 = 0; j4 < kH / 4; ++j4)
            dg::put4(bt + 4 * j4, gt4[j4]);
#pragma unroll
        for (int j = 0; j < kH; ++j) bg[j] = G[(int64_t)(kH * h + j) * kD + n0 + i];
        f32x16 accv = {}, accd = {};
#pragma unroll
        for (int j = 0; j < kH; ++j) {
            accv = __builtin_amdgcn_mfma_f32_32x32x2f32(xv[j], bt[j], accv, 0, 0, 0);
            accd = __builtin_amdgcn_mfma_f32_32x32x2f32(xd[j], bg[j], accd, 0, 0, 0);
        }
        const float ln = l ? l[n0 + i] : 1.0f;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int pp = p0 + dg::acc_row(q, h);
            if (pp < end) {
                a.mv[(int64_t)pp * kD + n0 + i] = accv[q] * ln;
                a.grad_cols[(int64_t)pp * kD + n0 + i] = accd[q] * ln;
            }
        }
    }
}

// One wave per (segment, 32×32 tile (ta, tb) of dM): the segment's pairs in chunks of 32, MFMA
// step s2 of a chunk taking pair 2·s2 + h from lane half h — pairs in order.  Lane j < 32 (both
// halves) reads chunk pair j's indices and mask once; the steps fetch them by shuffle.
template <int kD, class Loss>
__global__ __launch_bounds__(256) void grad_seg_dm_kernel(const GradSegArgs a) {
    constexpr int kT = kD / 32;
    const int lane = threadIdx.x & 63;
    const int i = lane & 31, h = lane >> 5;
    const int wid = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (wid >= a.n_seg * kT * kT) return;
    const int s = wid / (kT * kT);
    const int t = wid - s * kT * kT;
    const int ta = t / kT, tb = t - ta * kT;
    int beg, end, k;
    const bool live = dg::seg_bounds(a.seg_ptr, a.n_pairs, s, beg, end);
    const bool rel_ok = dg::seg_relation(a.seg_rel, a.ops.n_rel, s, k);
    f32x16 acc = {};
    if (live && rel_ok) {
#pragma unroll 1
        for (int c0 = beg; c0 < end; c0 += 32) {
            int r, c, rn;
            const typename Loss::Coef cf = pair_meta<Loss>(a, c0 + i, c0 + i < end, r, c, rn);
            float un[16], uu[16], vv[16];
            typename Loss::Coef on[16];
#pragma unroll
            for (int s2 = 0; s2 < 16; ++s2) {
                const int src = 2 * s2 + h;
                const int rr = __shfl(r, src), cc = __shfl(c, src), nn = __shfl(rn, src);
                on[s2] = Loss::shfl(cf, src);
                uu[s2] = a.row_table[(int64_t)rr * a.ld_row + ta * 32 + i];
                un[s2] = a.row_table[(int64_t)nn * a.ld_row + ta * 32 + i];
                vv[s2] = a.col_table[(int64_t)cc * a.ld_col + tb * 32 + i];
            }
#pragma unroll
            for (int s2 = 0; s2 < 16; ++s2) {
                const bool lv = Loss::live(on[s2]);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(lv ? Loss::diff(on[s2], un[s2], uu[s2]) : 0.f,
                                                           lv ? vv[s2] : 0.f, acc, 0, 0, 0);
            }
        }
    }
    float* out = a.dM + (int64_t)s * kD * kD;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int row = ta * 32 + dg::acc_row(q, h);
        out[(int64_t)row * kD + tb * 32 + i] = acc[q];
    }
}

// The per-relation outputs of segment s's relation k, eb blocks of 256 elements per segment:
// dG[k] = L_k·dM_s·L_k (per-relation G; eb = ⌈d²/256⌉), and in the segment's first block dG_diag[k]
// and dl[k] by dg_decoder_grad_f32's formulas (eb = 1 when only those are asked for).  Segments
// whose relation is out of range are skipped.
__global__ __launch_bounds__(256) void grad_seg_vars_kernel(const GradSegArgs a, int d, int eb) {
    const int dd = d * d;
    const int s = blockIdx.x / eb;
    const int e = (blockIdx.x - s * eb) * 256 + threadIdx.x;
    int k;
    if (!dg::seg_relation(a.seg_rel, a.ops.n_rel, s, k)) return;
    const float* dM = a.dM + (int64_t)s * dd;
    const float* l = dg::rel_l(a.ops, k);
    if (a.dG && a.ops.g_stride != 0 && e < dd) {
        const int ra = e / d, cb = e - ra * d;
        a.dG[(int64_t)k * dd + e] = l ? l[ra] * dM[e] * l[cb] : dM[e];
    }
    if (e < d) {  // (the segment's first block)
        if (a.dl) {
            const float* G = dg::rel_G(a.ops, k);
            float sum = 0.f;
#pragma unroll 16
            for (int c = 0; c < d; ++c) sum = fmaf(dM[(int64_t)e * d + c] * G[(int64_t)e * d + c], l[c], sum);
#pragma unroll 16
            for (int c = 0; c < d; ++c) sum = fmaf(dM[(int64_t)c * d + e] * G[(int64_t)c * d + e], l[c], sum);
            a.dl[(int64_t)k * d + e] = sum;
        }
        if (a.dG_diag) {
            const float le = l ? l[e] : 1.0f;
            a.dG_diag[(int64_t)k * d + e] = le * dM[(int64_t)e * d + e] * le;
        }
    }
}

constexpr int kSumSlices = 16;  // slices of the segment list one workgroup of the shared-G sum adds side by side
constexpr int kSumBatch = 8;    // segments of a slice whose loads are in flight together

// A shared G's dG = Σ_s L_k·dM_s·L_k in a fixed order: a workgroup owns 64 elements of dG and cuts
// the segment list into kSumSlices contiguous slices, one per wave; a wave adds its slice's
// segments in order, and the slices' sums are added in slice order.  Segments whose relation is
// out of range add nothing.
__global__ __launch_bounds__(64 * kSumSlices) void grad_seg_shared_dg_kernel(const GradSegArgs a, int d) {
    __shared__ float part[kSumSlices][64];
    const int el = threadIdx.x & 63;
    const int j = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int dd = d * d;
    const int e = blockIdx.x * 64 + el;  // (d*d is a multiple of 64)
    const int ra = e / d, cb = e - ra * d;
    const int per = (a.n_seg + kSumSlices - 1) / kSumSlices;
    const int s0 = j * per;
    const int s1 = s0 + per < a.n_seg ? s0 + per : a.n_seg;
    float sum = 0.f;
#pragma unroll 1
    for (int sb = s0; sb < s1; sb += kSumBatch) {
        float m[kSumBatch], la[kSumBatch], lb[kSumBatch];
        bool ok[kSumBatch];
#pragma unroll
        for (int u = 0; u < kSumBatch; ++u) {
            const int s = sb + u < s1 ? sb + u : s0;  // (clamped: the loads stay unconditional)
            const int k = a.seg_rel ? a.seg_rel[s] : s;
            ok[u] = sb + u < s1 && k >= 0 && k < a.ops.n_rel;
            const int kc = ok[u] ? k : 0;
            m[u] = a.dM[(int64_t)s * dd + e];
            const float* l = dg::rel_l(a.ops, kc);
            la[u] = l ? l[ra] : 1.0f;
            lb[u] = l ? l[cb] : 1.0f;
        }
#pragma unroll
        for (int u = 0; u < kSumBatch; ++u) sum += ok[u] ? la[u] * m[u] * lb[u] : 0.f;
    }
    part[j][el] = sum;
    __syncthreads();
    if (j == 0) {
        float t = part[0][el];
#pragma unroll
        for (int q = 1; q < kSumSlices; ++q) t += part[q][el];
        a.dG[e] = t;
    }
}

// ---------------------------------------------------------------- segmented row sums
constexpr int kRowWaves = 4;   // waves of the workgroup that owns an output row
constexpr int kRowChunk = 32;  // consecutive list items one wave adds before it skips to its next chunk
constexpr int kRowBatch = 8;   // items of a chunk (per lane group) whose loads are in flight together

struct RowSumArgs {
    const int32_t* node_ptr;
    const int32_t* item;
    const float* sign;
    const float* src;
    float* out;
    int64_t ld_out;
    int32_t n_items, n_src_rows, d, pad;
};

// One workgroup per output row r.  Its list [node_ptr[r], node_ptr[r+1]) is cut into chunks of
// kRowChunk items; wave w adds chunks w, w + kRowWaves, ... in order into one running sum, and
// the row's sum is (w0 + w1) + (w2 + w3).  kLP lanes hold a row of src (columns li + kLP·t); with
// kLP = 32 the wave's two lane groups take the chunk's even and odd items and are added at the
// end.  Items outside [0, n_src_rows) add nothing and read nothing out of range.
template <int kLP, int kT>
__global__ __launch_bounds__(64 * kRowWaves) void segment_rows_sum_kernel(const RowSumArgs a) {
    constexpr int kSub = 64 / kLP;
    __shared__ float red[kRowWaves][kLP * kT];
    const int r = blockIdx.x;
    int beg = a.node_ptr[r], end = a.node_ptr[r + 1];
    if (beg < 0) beg = 0;
    if (end > a.n_items) end = a.n_items;
    if (end <= beg) return;  // (block-uniform: before any barrier)
    const int lane = threadIdx.x & 63;
    const int w = threadIdx.x >> 6;
    const int li = lane % kLP, g = lane / kLP;
    const int nch = (end - beg + kRowChunk - 1) / kRowChunk;
    float acc[kT];
#pragma unroll
    for (int t = 0; t < kT; ++t) acc[t] = 0.f;
#pragma unroll 1
    for (int ch = w; ch < nch; ch += kRowWaves) {
        const int q0 = beg + ch * kRowChunk;
        const int qe = q0 + kRowChunk < end ? q0 + kRowChunk : end;
#pragma unroll 1
        for (int j0 = 0; j0 < kRowChunk / kSub; j0 += kRowBatch) {
            if (q0 + kSub * j0 >= qe) break;  // wave-uniform
            int it[kRowBatch];
            float sg[kRowBatch];
#pragma unroll
            for (int j = 0; j < kRowBatch; ++j) {
                const int q = q0 + kSub * (j0 + j) + g;
                const bool in = q < qe;
                it[j] = in ? a.item[q] : -1;
                sg[j] = in && a.sign ? a.sign[q] : 1.0f;
                if (it[j] < 0 || it[j] >= a.n_src_rows) {
                    it[j] = 0;
                    sg[j] = 0.f;
                }
            }
            float x[kRowBatch][kT];
#pragma unroll
            for (int j = 0; j < kRowBatch; ++j)
#pragma unroll
                for (int t = 0; t < kT; ++t) {
                    const int col = li + kLP * t;
                    x[j][t] = col < a.d ? a.src[(int64_t)it[j] * a.d + col] : 0.f;
                }
#pragma unroll
            for (int j = 0; j < kRowBatch; ++j)
#pragma unroll
                for (int t = 0; t < kT; ++t) acc[t] += sg[j] != 0.f ? sg[j] * x[j][t] : 0.f;
        }
    }
    if (kSub == 2) acc[0] += __shfl_xor(acc[0], 32);  // (kLP = 32 comes with kT = 1)
    if (g == 0) {
#pragma unroll
        for (int t = 0; t < kT; ++t) red[w][li + kLP * t] = acc[t];
    }
    __syncthreads();
    const int col = threadIdx.x;
    if (col < a.d && col < kLP * kT)
        a.out[(int64_t)r * a.ld_out + col] += (red[0][col] + red[1][col]) + (red[2][col] + red[3][col]);
}

}  // namespace

extern "C" int64_t dg_decoder_grad_seg_workspace(int32_t n_seg, int32_t d) {
    if (n_seg < 1 || (d != 32 && d != 64)) return 0;
    return 4LL * n_seg * d * d;
}

// dg_decoder_grad_seg_f32 / dg_decoder_grad_seg_xent_f32: the same launches, the pair and dM kernels
// of the cost (coef: the xent form's output, NULL for the hinge).
template <class Loss>
static int grad_seg_launch(const float* row_table, int64_t ld_row, int32_t n_rows, const float* col_table,
                           int64_t ld_col, int32_t n_cols, const int32_t* rows, const int32_t* cols,
                           const int32_t* neg_rows, const int32_t* seg_ptr, const int32_t* seg_rel, int32_t n_seg,
                           int32_t n_pairs, const float* pos, const float* neg, float param, const float* G,
                           int64_t g_stride, const float* l, int64_t l_stride, int32_t n_rel, int32_t d, float* mv,
                           float* grad_cols, float* coef, float* dG, float* dl, float* dG_diag, void* workspace,
                           int64_t workspace_bytes, void* stream) {
    if (n_seg <= 0 || n_pairs < 0 || (d != 32 && d != 64)) return DG_EINVAL;
    if (!row_table || !col_table || !seg_ptr || !G) return DG_EINVAL;
    if (n_pairs > 0 && (!rows || !cols || !neg_rows || !pos || !neg || !mv || !grad_cols)) return DG_EINVAL;
    if (Loss::kCoef && n_pairs > 0 && !coef) return DG_EINVAL;
    if (n_rows < 1 || n_cols < 1 || ld_row < d || ld_col < d) return DG_EINVAL;
    GradSegArgs a{};
    if (dg::rel_ops(G, g_stride, l, l_stride, n_rel, d, seg_rel != nullptr, n_seg, a.ops) != DG_OK) return DG_EINVAL;
    if (dl && (!l || l_stride != d)) return DG_EINVAL;  // dl[k] is the gradient of a per-relation l_k
    if (dG_diag && g_stride == 0) return DG_EINVAL;     // a per-relation output of a shared G
    const bool vars = dG || dl || dG_diag;
    if (vars && (!workspace || workspace_bytes < dg_decoder_grad_seg_workspace(n_seg, d))) return DG_EINVAL;
    if ((int64_t)n_pairs + 32LL * n_seg >= (1ll << 31)) return DG_EINVAL;  // 32-bit pair offsets
    if ((int64_t)n_seg * (d * d / 256) >= (1ll << 31)) return DG_EINVAL;  // the per-segment grids
    if (!dg::aligned16(row_table) || !dg::aligned16(col_table) || (ld_row & 3) || (ld_col & 3) ||
        !dg::aligned16(G) || (l && !dg::aligned16(l)) || (vars && !dg::aligned16(workspace)))
        return DG_EALIGN;
    if (n_pairs == 0) return DG_OK;
    a.row_table = row_table;
    a.col_table = col_table;
    a.rows = rows;
    a.cols = cols;
    a.negs = neg_rows;
    a.seg_ptr = seg_ptr;
    a.seg_rel = seg_rel;
    a.pos = pos;
    a.neg = neg;
    a.mv = mv;
    a.grad_cols = grad_cols;
    a.coef = coef;
    a.dM = static_cast<float*>(workspace);
    a.dG = dG;
    a.dl = dl;
    a.dG_diag = dG_diag;
    a.ld_row = ld_row;
    a.ld_col = ld_col;
    a.n_rows = n_rows;
    a.n_cols = n_cols;
    a.n_seg = n_seg;
    a.n_pairs = n_pairs;
    a.n_tiles = (int32_t)dg::seg_tile_grid(n_pairs, n_seg, 32);
    a.param = param;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid(dg::ceil_div(a.n_tiles, 4)), block(256);
    if (d == 32)
        hipLaunchKernelGGL((grad_seg_pairs_kernel<32, Loss>), grid, block, 0, st, a);
    else
        hipLaunchKernelGGL((grad_seg_pairs_kernel<64, Loss>), grid, block, 0, st, a);
    if (!vars) return dg::launch_status();
    const int tiles = d / 32;
    const dim3 dgrid(dg::ceil_div((int64_t)n_seg * tiles * tiles, 4));
    if (d == 32)
        hipLaunchKernelGGL((grad_seg_dm_kernel<32, Loss>), dgrid, block, 0, st, a);
    else
        hipLaunchKernelGGL((grad_seg_dm_kernel<64, Loss>), dgrid, block, 0, st, a);
    const bool per_rel_dG = dG && g_stride != 0;
    if (per_rel_dG || dl || dG_diag) {
        const int eb = per_rel_dG ? dg::ceil_div((int64_t)d * d, 256) : 1;
        hipLaunchKernelGGL(grad_seg_vars_kernel, dim3((unsigned)((int64_t)n_seg * eb)), block, 0, st, a, d, eb);
    }
    if (dG && g_stride == 0)
        hipLaunchKernelGGL(grad_seg_shared_dg_kernel, dim3(d * d / 64), dim3(64 * kSumSlices), 0, st, a, d);
    return dg::launch_status();
}

extern "C" int dg_decoder_grad_seg_f32(const float* row_table, int64_t ld_row, int32_t n_rows,
                                       const float* col_table, int64_t ld_col, int32_t n_cols,
                                       const int32_t* rows, const int32_t* cols, const int32_t* neg_rows,
                                       const int32_t* seg_ptr, const int32_t* seg_rel, int32_t n_seg,
                                       int32_t n_pairs, const float* pos, const float* neg, float margin,
                                       const float* G, int64_t g_stride, const float* l, int64_t l_stride,
                                       int32_t n_rel, int32_t d, float* mv, float* grad_cols, float* dG, float* dl,
                                       float* dG_diag, void* workspace, int64_t workspace_bytes, void* stream) {
    return grad_seg_launch<dg::HingeLoss>(row_table, ld_row, n_rows, col_table, ld_col, n_cols, rows, cols, neg_rows,
                                          seg_ptr, seg_rel, n_seg, n_pairs, pos, neg, margin, G, g_stride, l, l_stride,
                                          n_rel, d, mv, grad_cols, nullptr, dG, dl, dG_diag, workspace,
                                          workspace_bytes, stream);
}

extern "C" int dg_decoder_grad_seg_xent_f32(const float* row_table, int64_t ld_row, int32_t n_rows,
                                            const float* col_table, int64_t ld_col, int32_t n_cols,
                                            const int32_t* rows, const int32_t* cols, const int32_t* neg_rows,
                                            const int32_t* seg_ptr, const int32_t* seg_rel, int32_t n_seg,
                                            int32_t n_pairs, const float* pos, const float* neg, float neg_weight,
                                            const float* G, int64_t g_stride, const float* l, int64_t l_stride,
                                            int32_t n_rel, int32_t d, float* mv, float* grad_cols, float* coef,
                                            float* dG, float* dl, float* dG_diag, void* workspace,
                                            int64_t workspace_bytes, void* stream) {
    return grad_seg_launch<dg::XentLoss>(row_table, ld_row, n_rows, col_table, ld_col, n_cols, rows, cols, neg_rows,
                                         seg_ptr, seg_rel, n_seg, n_pairs, pos, neg, neg_weight, G, g_stride, l,
                                         l_stride, n_rel, d, mv, grad_cols, coef, dG, dl, dG_diag, workspace,
                                         workspace_bytes, stream);
}

extern "C" int32_t dg_segment_rows_sum_chunk(void) { return kRowChunk; }

extern "C" int32_t dg_segment_rows_sum_waves(void) { return kRowWaves; }

extern "C" int dg_segment_rows_sum_f32(const int32_t* node_ptr, const int32_t* item, const float* sign,
                                       int32_t n_items, const float* src, int32_t n_src_rows, int32_t d, float* out,
                                       int64_t ld_out, int32_t n_out_rows, void* stream) {
    if (n_items < 0 || n_src_rows < 0 || d < 1 || d > 256 || ld_out < d || n_out_rows < 0) return DG_EINVAL;
    if (n_items == 0 || n_out_rows == 0) return DG_OK;
    if (!node_ptr || !item || !src || !out || n_src_rows < 1) return DG_EINVAL;
    RowSumArgs a{node_ptr, item, sign, src, out, ld_out, n_items, n_src_rows, d, 0};
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid(n_out_rows), block(64 * kRowWaves);
    if (d <= 32)
        hipLaunchKernelGGL((segment_rows_sum_kernel<32, 1>), grid, block, 0, st, a);
    else if (d <= 64)
        hipLaunchKernelGGL((segment_rows_sum_kernel<64, 1>), grid, block, 0, st, a);
    else if (d <= 128)
        hipLaunchKernelGGL((segment_rows_sum_kernel<64, 2>), grid, block, 0, st, a);
    else
        hipLaunchKernelGGL((segment_rows_sum_kernel<64, 4>), grid, block, 0, st, a);
    return dg::launch_status();
}

// Fused top-k candidate ranking over all relations of one edge type (i, j): for every relation
// k the `topk` highest-scoring permitted pairs (r, c) of
//   s_k[r, c] = (E_i[r] ∘ l_k)ᵀ · G_k · (l_k ∘ E_j[c])
// without ever forming an N_i×N_j matrix.
//
// Replaces (paths relative to the reference root):
//   session.run(predictionsTensor) + sigmoid + np.take + argsort()[::-1][:numToUnmask]
//                                          main/ActiveLearner/GreedyActiveLearner.py:66-96
//   E·D·R·D·Eᵀ of one relation before sampling         main/Predictor/NpPredictor.py:293-313
//
// Form.  Launch 1: one workgroup (4 waves) per (relation, stripe of 128 rows).  It forms the
// stripe's A = ((E_i ∘ l)·G) ∘ l (128×d) once on v_mfma_f32_32x32x2_f32 into LDS; wave w then keeps
// the A fragments of its 32-row block in registers and walks all 32-column tiles (one 32×32
// score tile = d/2 MFMAs, exact fp32).  Each wave keeps its OWN candidate list in
// LDS (no workgroup barrier in the walk): scores above the wave's threshold are compacted into
// the list (ballot + prefix); when the list is full it is sorted (bitonic, descending),
// truncated to topk, and the threshold becomes its last key.  Launch 2: one wave per relation
// runs the same list over the ⌈N_i/32⌉ wave lists of the relation and decodes the result.
//
// Ordering.  A candidate is one 64-bit key, (monotone map of the score's bits) << 32 | ~(r·N_j + c):
// unsigned comparison orders by higher score, then smaller linear index (−0 is made +0 first).
// Keys are unique, and a key is only ever dropped when topk larger keys of the same relation
// exist, so the result is the unique top-k of the relation whatever the tiling, the grid or
// the order in which waves run.
//
// The half-row load, the A block and the tile product are rank_walk.h's, shared with edgerank.hip
// and nodetopk.hip (a pair's score has the same bits from all three).  The walk itself is this
// file's own: one dependent exclusion load per entry beside each tile and one list per wave — the
// later kernels left it for rank_walk.h's masks.
#include "common.h"
#include "rank_walk.h"

namespace {

using dg::f32x16;
using dg::load_half_row;

constexpr int kStripe = 128;  // rows per workgroup: one 32-row block per wave
constexpr int kWaves = 4;    // waves per workgroup = candidate lists per stripe

using dg::key_score;
using dg::list_cap;
using dg::make_key;
using dg::WaveTopK;

struct TopkArgs {
    const float* row_table;
    const float* col_table;
    const float* G;  // dg::RelOps's fields, in the order this kernel was measured with
    const float* l;
    const int32_t* ex_rowptr;
    const int32_t* ex_col;
    uint64_t* lists;
    int64_t ld_row, ld_col, g_stride, l_stride;
    int32_t n_rows, n_cols, n_stripes, topk, cap, flags;
};

template <int D>
__global__ __launch_bounds__(256) void topk_stripe_kernel(TopkArgs a) {
    constexpr int H = D / 2;
    constexpr int LDA = dg::a_ld(D);
    extern __shared__ __attribute__((aligned(16))) unsigned char topk_smem[];
    float* As = reinterpret_cast<float*>(topk_smem);  // [kStripe][LDA]
    uint64_t* bufs = reinterpret_cast<uint64_t*>(topk_smem + kStripe * LDA * sizeof(float));

    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int i = lane & 31, h = lane >> 5;
    const int rel = blockIdx.x / a.n_stripes;
    const int r0 = (blockIdx.x - rel * a.n_stripes) * kStripe;
    const float* G = a.G + (int64_t)rel * a.g_stride;
    const float* l = a.l ? a.l + (int64_t)rel * a.l_stride : nullptr;

    // A = ((U ∘ l)·G) ∘ l: wave w forms its own 32 rows, 32 columns at a time
    const int rb = w;
    {
        const int row = r0 + rb * 32 + i;
        const bool ok = row < a.n_rows;
        float u[H];
        load_half_row<H>(a.row_table + (int64_t)(ok ? row : 0) * a.ld_row + H * h, ok, u);
#pragma unroll
        for (int nb = 0; nb < D / 32; ++nb) dg::a_block<D>(u, G, l, nb, i, h, As + rb * 32 * LDA);
    }
    __syncthreads();

    float af[H];
    load_half_row<H>(As + (rb * 32 + i) * LDA + H * h, true, af);

    WaveTopK tk;
    tk.init(bufs + w * a.cap, a.cap, a.topk, lane);

    // this lane's cursor into the exclusion row of row 32·rb + i (columns ascending)
    const int myrow = r0 + rb * 32 + i;
    int p = 0, pe = 0;
    if (a.ex_rowptr && myrow < a.n_rows) {
        const int64_t q = (int64_t)rel * a.n_rows + myrow;
        p = a.ex_rowptr[q];
        pe = a.ex_rowptr[q + 1];
    }
    const bool upper = (a.flags & DG_TOPK_UPPER) != 0, no_diag = (a.flags & DG_TOPK_NO_DIAG) != 0;
    const int n_ct = (a.n_cols + 31) / 32;
    int ct = 0;
    if (upper) {  // tiles whose last column is ≤ the block's first row hold no r < c
        ct = (r0 + rb * 32 + 1) / 32;
        if (ct > n_ct) ct = n_ct;
    }

    auto load_b = [&](int t, float(&x)[H]) {
        const int c = t * 32 + i;
        const bool ok = c < a.n_cols;
        load_half_row<H>(a.col_table + (int64_t)(ok ? c : 0) * a.ld_col + H * h, ok, x);
    };
    float b[H], bn[H];
    load_b(ct, b);
#pragma unroll 1
    for (; ct < n_ct; ++ct) {
        load_b(ct + 1, bn);  // next tile's rows in flight behind this tile's MFMAs
        const f32x16 acc = dg::tile_scores<H>(af, b);
        const int c0 = ct * 32, c = c0 + i;
        uint32_t ex = 0;  // excluded columns of row myrow inside this tile
        while (p < pe) {
            const int ec = a.ex_col[p];
            if (ec >= c0 + 32) break;
            if (ec >= c0) ex |= 1u << (ec - c0);
            ++p;
        }
        const bool cok = c < a.n_cols;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int rl = dg::acc_row(r, h);
            const int row = r0 + rb * 32 + rl;
            const uint32_t exr = (uint32_t)__shfl((int)ex, rl);  // lane rl holds row rl's mask
            bool ok = cok && row < a.n_rows && !((exr >> i) & 1u);
            if (upper) ok = ok && row < c;
            if (no_diag) ok = ok && row != c;
            tk.push(make_key(acc[r], (uint32_t)row * (uint32_t)a.n_cols + (uint32_t)c), ok);
        }
#pragma unroll
        for (int s = 0; s < H; ++s) b[s] = bn[s];
    }
    tk.compact();
    uint64_t* out = a.lists + ((int64_t)blockIdx.x * kWaves + w) * a.topk;
    for (int t = lane; t < a.topk; t += dg::kWave) out[t] = tk.buf[t];
}

// One wave per relation: the top-k of the relation's n_lists descending lists, decoded.
__global__ __launch_bounds__(64) void topk_merge_kernel(const uint64_t* lists, int n_lists, int topk, int cap,
                                                        int n_cols, float* out_score, int32_t* out_row,
                                                        int32_t* out_col, int32_t* out_count) {
    extern __shared__ __attribute__((aligned(16))) unsigned char topk_smem[];
    const int lane = threadIdx.x, rel = blockIdx.x;
    WaveTopK tk;
    tk.init(reinterpret_cast<uint64_t*>(topk_smem), cap, topk, lane);
#pragma unroll 1
    for (int L = 0; L < n_lists; ++L) {
        const uint64_t* src = lists + ((int64_t)rel * n_lists + L) * topk;
#pragma unroll 1
        for (int t0 = 0; t0 < topk; t0 += dg::kWave) {
            const int t = t0 + lane;
            const uint64_t key = t < topk ? src[t] : 0;
            const bool ok = key > tk.thr;             // (padding is 0)
            if (__ballot(ok) == 0) break;             // descending: nothing further can enter
            tk.push(key, ok);
        }
    }
    tk.compact();
    for (int t = lane; t < topk; t += dg::kWave) {
        const uint64_t key = tk.buf[t];
        const int64_t o = (int64_t)rel * topk + t;
        if (t < tk.n) {
            const uint32_t lin = ~(uint32_t)key;
            const uint32_t row = lin / (uint32_t)n_cols;
            out_score[o] = key_score(key);
            out_row[o] = (int32_t)row;
            out_col[o] = (int32_t)(lin - row * (uint32_t)n_cols);
        } else {
            out_score[o] = -__builtin_inff();
            out_row[o] = -1;
            out_col[o] = -1;
        }
    }
    if (lane == 0) out_count[rel] = tk.n;
}

template <int D>
int launch_stripes(const TopkArgs& a, int n_rel, hipStream_t st) {
    static std::atomic<uint64_t> optin{0};
    const int a_bytes = kStripe * (D + 4) * (int)sizeof(float);
    const int bytes = a_bytes + kWaves * a.cap * 8;
    if (bytes > 65536)
        dg::lds_optin(reinterpret_cast<const void*>(&topk_stripe_kernel<D>), a_bytes + kWaves * list_cap(DG_TOPK_MAX_K) * 8,
                      optin);
    hipLaunchKernelGGL(topk_stripe_kernel<D>, dim3((unsigned)(n_rel * a.n_stripes)), dim3(256), bytes, st, a);
    return dg::launch_status();
}

}  // namespace

extern "C" int64_t dg_decoder_topk_workspace(int32_t n_rel, int32_t n_rows, int32_t n_cols, int32_t topk) {
    if (n_rel < 1 || n_rows < 1 || n_cols < 1 || topk < 1 || topk > DG_TOPK_MAX_K) return 0;
    return (int64_t)n_rel * dg::ceil_div(n_rows, kStripe) * kWaves * topk * 8;
}

extern "C" int dg_decoder_topk_f32(const float* row_table, int64_t ld_row, int32_t n_rows, const float* col_table,
                                   int64_t ld_col, int32_t n_cols, const float* G, int64_t g_stride,
                                   const float* l, int64_t l_stride, int32_t n_rel, int32_t d, int32_t topk,
                                   const int32_t* excl_rowptr, const int32_t* excl_col, int32_t flags,
                                   float* out_score, int32_t* out_row, int32_t* out_col, int32_t* out_count,
                                   void* workspace, int64_t workspace_bytes, void* stream) {
    if (!row_table || !col_table || !G || !out_score || !out_row || !out_col || !out_count || !workspace)
        return DG_EINVAL;
    if (d != 32 && d != 64) return DG_EINVAL;
    if (topk < 1 || topk > DG_TOPK_MAX_K || n_rel < 1 || n_rows < 1 || n_cols < 1) return DG_EINVAL;
    if (ld_row < d || ld_col < d) return DG_EINVAL;
    if ((uint64_t)n_rows * (uint64_t)n_cols >= (1ull << 32)) return DG_EINVAL;  // 32-bit linear index
    if ((int64_t)n_rel * dg::ceil_div(n_rows, kStripe) >= (1ll << 31)) return DG_EINVAL;
    dg::RelOps ops;
    if (dg::rel_ops(G, g_stride, l, l_stride, n_rel, d, false, n_rel, ops) != DG_OK) return DG_EINVAL;
    if ((excl_rowptr == nullptr) != (excl_col == nullptr)) return DG_EINVAL;
    if (flags & ~(DG_TOPK_UPPER | DG_TOPK_NO_DIAG)) return DG_EINVAL;
    if ((flags & DG_TOPK_UPPER) && n_rows != n_cols) return DG_EINVAL;
    if (workspace_bytes < dg_decoder_topk_workspace(n_rel, n_rows, n_cols, topk)) return DG_EINVAL;
    if (!dg::aligned16(row_table) || !dg::aligned16(col_table) || (ld_row & 3) || (ld_col & 3) ||
        !dg::aligned16(workspace))
        return DG_EALIGN;

    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    TopkArgs a;
    a.row_table = row_table;
    a.col_table = col_table;
    a.G = ops.G;
    a.l = ops.l;
    a.ex_rowptr = excl_rowptr;
    a.ex_col = excl_col;
    a.lists = static_cast<uint64_t*>(workspace);
    a.ld_row = ld_row;
    a.ld_col = ld_col;
    a.g_stride = ops.g_stride;
    a.l_stride = ops.l_stride;
    a.n_rows = n_rows;
    a.n_cols = n_cols;
    a.n_stripes = dg::ceil_div(n_rows, kStripe);
    a.topk = topk;
    a.cap = list_cap(topk);
    a.flags = flags;
    const int rc = d == 32 ? launch_stripes<32>(a, n_rel, st) : launch_stripes<64>(a, n_rel, st);
    if (rc != DG_OK) return rc;
    hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)n_rel), dim3(64), a.cap * 8, st, a.lists,
                       a.n_stripes * kWaves, topk, a.cap, n_cols, out_score, out_row, out_col, out_count);
    return dg::launch_status();
}

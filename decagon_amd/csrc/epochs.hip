// One step's batches of every relation of an edge type, gathered from the device-resident training
// edges in the epoch's shuffled order (dg_epoch_batch_i32), in the layout the segmented kernels take.
//
// Replaces (paths relative to the reference root):
//   EdgeMinibatchIterator.shuffle: np.random.permutation of every relation's training edges
//                                  decagon/deep/minibatch.py:315-322
//   EdgeMinibatchIterator.next_minibatch_feed_dict: the batch [start : start + batch_size] of ONE
//     relation, the relation leaving the epoch when fewer than a batch remains (and the iterator of
//     edge types (0,0), (0,1), (1,0) wrapping round instead)   decagon/deep/minibatch.py:278-313
// which the package left to its callers: 1,932 numpy index arrays packed and uploaded per step.
//
// No shuffled copy exists.  Pair c of segment s (relation k = seg_rel[s], n_k edges, nb_k = ⌊n_k/B⌋
// batches an epoch) is edge perm(n_k, epoch_key(seed, epoch, first_slot + k), tb·B + c) of the
// relation (permute.h), tb = t mod nb_k where the relation wraps and t otherwise: a handful of integer
// hashes and one 8-byte gather of the interleaved (row, col) pair per output pair.  One thread per
// output pair; where B is a multiple of 64 a wave lies inside one segment and everything but the
// permutation and the gather is scalar.  A segment without a batch (nb_k = 0, t >= nb_k without
// wrapping, k outside [0, n_rel), or an edge_ptr entry outside the edge list) reads no edge and gets
// the row `bad_row` — the row table's length, which the segmented kernels treat as "contributes
// nothing" — and column 0.
#include "common.h"
#include "permute.h"

namespace {

struct EpochArgs {
    const int2* edges;
    const int64_t* edge_ptr;
    const int32_t* seg_rel;
    const uint32_t* wrap_mask;
    int32_t* rows;
    int32_t* cols;
    int64_t n_edges;
    uint64_t seed;
    uint32_t epoch, first_slot;
    int32_t n_rel, batch, t, bad_row, total;
};

template <bool kUniform>
__global__ __launch_bounds__(256) void epoch_batch_kernel(const EpochArgs a) {
    int idx, s, c;
    if (kUniform) {  // batch % 64 == 0: the wave's 64 pairs are of one segment
        const int lane = threadIdx.x & 63;
        const int w0 = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 256 + (threadIdx.x & ~63u)));
        if (w0 >= a.total) return;  // (total is a multiple of 64 here: whole waves leave)
        s = w0 / a.batch;
        c = w0 - s * a.batch + lane;
        idx = w0 + lane;
    } else {
        idx = blockIdx.x * 256 + threadIdx.x;
        if (idx >= a.total) return;
        s = idx / a.batch;
        c = idx - s * a.batch;
    }
    const int k = a.seg_rel[s];
    bool ok = k >= 0 && k < a.n_rel;
    int64_t e0 = 0;
    uint32_t n = 0;
    if (ok) {
        e0 = a.edge_ptr[k];
        const int64_t e1 = a.edge_ptr[k + 1], nk = e1 - e0;
        ok = e0 >= 0 && e1 <= a.n_edges && nk >= a.batch && nk < (1ll << 31);
        n = static_cast<uint32_t>(nk);
    }
    uint32_t tb = static_cast<uint32_t>(a.t);
    if (ok) {
        const uint32_t nb = n / static_cast<uint32_t>(a.batch);  // >= 1
        const bool wrap = a.wrap_mask && ((a.wrap_mask[k >> 5] >> (k & 31)) & 1u);
        if (wrap)
            tb %= nb;
        else
            ok = tb < nb;
    }
    int r = a.bad_row, cc = 0;
    if (ok) {
        const uint32_t key = dg::epoch_key(a.seed, a.epoch, a.first_slot + static_cast<uint32_t>(k));
        // tb < nb: tb·B + c < n < 2^31
        const uint32_t q = dg::perm(n, key, tb * static_cast<uint32_t>(a.batch) + static_cast<uint32_t>(c));
        const int2 e = a.edges[e0 + q];  // q < n = e1 − e0 and e1 <= n_edges
        r = e.x;
        cc = e.y;
    }
    a.rows[idx] = r;
    a.cols[idx] = cc;
}

inline bool aligned(const void* p, uintptr_t b) { return (reinterpret_cast<uintptr_t>(p) & (b - 1)) == 0; }

}  // namespace

extern "C" uint32_t dg_epoch_key_host(uint64_t seed, uint32_t epoch, uint32_t slot) {
    return dg::epoch_key(seed, epoch, slot);
}

extern "C" int dg_epoch_perm_host(int32_t n, uint32_t key, const int32_t* x, int32_t* out, int64_t count) {
    if (n < 1 || count < 0) return DG_EINVAL;
    if (count > 0 && (!x || !out)) return DG_EINVAL;
    for (int64_t i = 0; i < count; ++i) {
        if (x[i] < 0 || x[i] >= n) return DG_EINVAL;
        out[i] = static_cast<int32_t>(dg::perm(static_cast<uint32_t>(n), key, static_cast<uint32_t>(x[i])));
    }
    return DG_OK;
}

extern "C" int dg_epoch_batch_i32(const int32_t* edges, int64_t n_edges, const int64_t* edge_ptr, int32_t n_rel,
                                  const int32_t* seg_rel, int32_t n_seg, const uint32_t* wrap_mask, int32_t batch,
                                  int32_t t, uint32_t epoch, uint64_t seed, int32_t first_slot, int32_t bad_row,
                                  int32_t* rows, int32_t* cols, void* stream) {
    if (!edge_ptr || n_rel < 1 || n_edges < 0 || (n_edges > 0 && !edges)) return DG_EINVAL;
    if (batch <= 0 || n_seg < 0 || t < 0 || first_slot < 0) return DG_EINVAL;
    if (n_seg > 0 && (!seg_rel || !rows || !cols)) return DG_EINVAL;
    if ((int64_t)n_seg * batch > INT32_MAX - 256) return DG_EINVAL;  // 32-bit pair offsets
    if (!aligned(edges, 8) || !aligned(edge_ptr, 8) || !aligned(seg_rel, 4) || !aligned(wrap_mask, 4) ||
        !aligned(rows, 4) || !aligned(cols, 4))
        return DG_EALIGN;
    if (n_seg == 0) return DG_OK;

    EpochArgs a{};
    a.edges = reinterpret_cast<const int2*>(edges);
    a.edge_ptr = edge_ptr;
    a.seg_rel = seg_rel;
    a.wrap_mask = wrap_mask;
    a.rows = rows;
    a.cols = cols;
    a.n_edges = n_edges;
    a.seed = seed;
    a.epoch = epoch;
    a.first_slot = static_cast<uint32_t>(first_slot);
    a.n_rel = n_rel;
    a.batch = batch;
    a.t = t;
    a.bad_row = bad_row;
    a.total = n_seg * batch;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)dg::ceil_div(a.total, 256)), block(256);
    if (batch % dg::kWave == 0)
        hipLaunchKernelGGL(epoch_batch_kernel<true>, grid, block, 0, st, a);
    else
        hipLaunchKernelGGL(epoch_batch_kernel<false>, grid, block, 0, st, a);
    return dg::launch_status();
}

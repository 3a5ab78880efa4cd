/*
 * decagon_hip.h — C ABI of libdecagon_hip.so, the MI355X (gfx950) kernels behind the
 * Decagon multi-relational GCN forward and its edge decoders.
 *
 * The reference (jrectorb/decagon, TF 1.8) has no FFI: its "boundary" is a set of TF ops
 * called from the decagon/deep modules.  Every entry point below replaces one or a fused run of
 * those ops; the replaced call sites are cited per function (paths relative to the
 * reference root).  The Python layer in decagon_amd/ binds these with ctypes
 * (decagon_amd/_lib.py); INTEGRATION.md shows the binding.
 *
 * Conventions (all entry points):
 *   - every pointer argument is a caller-owned DEVICE pointer unless documented as host;
 *     the library never allocates or frees caller memory; the only state it keeps between
 *     calls is, per kernel that opts into more than 64 KB of dynamic LDS, the set of devices
 *     on which that (idempotent) hipFuncSetAttribute has been applied — thread-safe;
 *   - launches are asynchronous on `stream` (a hipStream_t passed as void*; NULL = the
 *     null stream) and are safe to capture into a hipGraph;
 *   - the return value is DG_OK (0), a negative DG_E* code for an argument error detected
 *     on the host before any launch, or a positive hipError_t from the launch.
 *   - float arithmetic is IEEE fp32 (no fast-math); sums are in a fixed order, so results
 *     are bitwise reproducible run to run (no float atomics anywhere).
 */
#ifndef DECAGON_HIP_H
#define DECAGON_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DG_OK 0
#define DG_EINVAL (-1)     /* bad size / null pointer / unsupported shape            */
#define DG_EALIGN (-2)     /* a dense operand is not 16-byte aligned row by row      */
#define DG_ETOOMANY (-3)   /* more groups than DG_MAX_GROUPS in one launch           */

#define DG_MAX_GROUPS 8

/* ABI version (39); bumped whenever a struct layout or a signature changes or an entry point is added
 * (36: DG_PEER_STATE_WORDS grew; 39: dg_decoder_topk_f32).  Added since 39 without a bump, purely
 * additive: dg_decoder_score_seg_f32, dg_rank_metrics_seg_workspace, dg_rank_metrics_seg_f32 and
 * the host helper dg_seg_tile_lookup (evaluation of all relations of an edge type in one pass);
 * dg_decoder_grad_seg_workspace, dg_decoder_grad_seg_f32, dg_segment_rows_sum_f32 and the host
 * helpers dg_segment_rows_sum_chunk / dg_segment_rows_sum_waves (the decoder backward of every
 * relation's batch of an edge type in one pass); dg_epoch_batch_i32 and the host helpers
 * dg_epoch_perm_host / dg_epoch_key_host (a step's batches of every relation from device-resident
 * edges in the epoch's shuffled order). */
int32_t dg_abi_version(void);

/* --------------------------------------------------------------------------------------
 * Relation-group SpMM (T3 + T4 of SURVEY §2.2) over a chunk-merged CSR.
 *
 * A group's relations A_k (k < K, all n_rows x n_cols) are split into chunks of consecutive
 * relations; for chunk c and row r the nonzeros of every relation in the chunk are stored
 * contiguously, [rowptr[c*n_rows + r], rowptr[c*n_rows + r + 1]), each with a virtual
 * column vcol = k*n_cols + col — the row of the relation-stacked dense operand
 * X = [X_0; X_1; ...] (row v at x + v*x_ld) that it multiplies.  Then
 *
 *     out[c][r][:] = sum_{p in range(c, r)} val[p] * X[vcol[p]][:]
 *                  = sum_{k in chunk c} (A_k · X_k)[r][:]
 *
 * With one chunk this is the add_n of layers.py:92/116.  The layout is built once at upload
 * (decagon_amd/sparse.py: merge_chunks).
 * Replaces: tf.sparse_tensor_dense_matmul(adj_mats[edge_type][k], x)  layers.py:90, :114
 *           tf.sparse_tensor_dense_matmul(x, weights_k) (sparse features) layers.py:89
 *           tf.add_n(outputs)                                         layers.py:92, :116
 * Requirements: d % 4 == 0, 4 <= d <= 256, x and x_ld 16-byte aligned (x_ld % 4 == 0),
 * x_rows * x_ld < 2^31 (gathers use 32-bit offsets), 0 <= vcol < x_rows.
 * -------------------------------------------------------------------------------------- */
typedef struct dg_rel_group {
    const int32_t* rowptr;      /* device, [n_chunks*n_rows + 1]                          */
    const int32_t* vcol;        /* device, [nnz] virtual columns (rows of X)              */
    const float* val;           /* device, [nnz].  vcol/val may be NULL when nnz == 0.    */
    const float* x;             /* device, relation-stacked dense operand                 */
    float* out;                 /* device, [n_chunks][n_rows][d] (unused in fused mode)   */
    int64_t x_ld;               /* elements between consecutive rows of X                 */
    int32_t n_rows;
    int32_t n_chunks;
    int32_t x_rows;             /* rows of X addressable (bound on vcol); per chunk when  */
                                /* DG_GROUP_SHARED_PATTERN is set                         */
    int32_t flags;              /* 0, or DG_GROUP_SHARED_PATTERN [| DG_GROUP_DROPOUT]      */
                                /* (dg_spmm_groups_f32 only), or DG_GROUP_DENSE_ROWS       */
                                /* (dg_gcn_fused_f32 only)                                */
    uint32_t drop_tag;          /* DG_GROUP_DROPOUT: mask stream of the group             */
    float drop_keep;            /* DG_GROUP_DROPOUT: keep probability in (0, 1]           */
    int32_t drop_stride;        /* DG_GROUP_DROPOUT: mask elements per chunk (the nnz of  */
                                /* the pattern)                                           */
    const uint64_t* drop_state; /* DG_GROUP_DROPOUT: device {seed, step}, else NULL       */
    const int32_t* drop_index;  /* DG_GROUP_DROPOUT: device [nnz] mask element of each    */
                                /* nonzero, or NULL (its position)                        */
} dg_rel_group;

/* Every chunk c uses the same CSR pattern (rowptr[0..n_rows], vcol, val) over its own slab of
 * X: rows [c*x_rows, (c+1)*x_rows).  The relation-batched X_j·W_k of sparse features
 * (layers.py:89, one X_j for every relation k) and its backward X_jᵀ·G_k, without K copies
 * of the pattern. */
#define DG_GROUP_SHARED_PATTERN 1

/* With DG_GROUP_SHARED_PATTERN: chunk c multiplies nonzero p's value by the dropout scale of
 * mask element c*drop_stride + (drop_index ? drop_index[p] : p) of stream drop_tag (dropout.h:
 * kept with probability drop_keep, scaled by 1/drop_keep) — dropout_sparse on the features
 * of every relation (layers.py:23-31, :88), each relation its own draw, the backward X_jᵀ·G_k
 * (drop_index: the transposed pattern's nonzeros mapped to the forward's) on the same masks. */
#define DG_GROUP_DROPOUT 2

/* dg_gcn_fused_f32 only: the group has no adjacency — row r of its sum IS row r of X
 * (x[r * x_ld ..], x_rows >= n_rows; rowptr / vcol / val unused, may be NULL), or with
 * n_chunks = S > 1 (S <= DG_PEER_MAX) the sum of S slots of such rows, slot c at
 * x + c*x_rows*x_ld, added in slot order (fp32, deterministic).  The sharded forward finishes
 * its all-reduced pre-normalisation sums S_ij this way (layers.py:92-93 after the cross-rank
 * Σ_k), without an identity CSR's two dependent loads; with the peer exchange the slots are
 * the ranks' partial sums, so the all-reduce's addition happens here. */
#define DG_GROUP_DENSE_ROWS 4

int dg_spmm_groups_f32(const dg_rel_group* groups /* HOST array */, int32_t n_groups,
                       int32_t d, void* stream);

/* The same partial-mode product (out[c][r][:] = Σ val·X[vcol][:]) for groups whose whole
 * dense operand is small — x_rows <= 1137 rows (it is staged in LDS, 144 B per row per
 * 32-column slice): the backward's Âᵀ·dS_ij, where every relation of the group reads the
 * same dS_ij (decagon_amd/train.py).  out must be 16-byte aligned; other requirements as
 * dg_spmm_groups_f32.  Replaces the gradient of tf.sparse_tensor_dense_matmul w.r.t. its
 * dense operand (layers.py:90, :114). */
int dg_spmm_groups_lds_f32(const dg_rel_group* groups /* HOST array */, int32_t n_groups, int32_t d,
                           void* stream);

/* Single relation, plain CSR: Y[r][:] = sum_p val[p] * X[col[p]][:] + beta * Y[r][:]
 * (Y dense, ld = ldy; fmaf(beta, Y, sum) per element).  beta == 0 writes Y without reading it
 * (no NaN carried over from uninitialised memory); beta == 1 accumulates one relation's product
 * into a running sum — tf.add_n over the per-relation products (layers.py:92, :116) done one
 * relation at a time.  Replaces one tf.sparse_tensor_dense_matmul (layers.py:90, :114).  ldy
 * must equal d; beta must be finite (ABI 37: beta added). */
int dg_spmm_csr_f32(const int32_t* rowptr, const int32_t* col, const float* val,
                    int32_t n_rows, int32_t n_cols, const float* x, int64_t ldx, float* y,
                    int64_t ldy, int32_t d, float beta, void* stream);

/* Row-wise L2 normalisation, stand-alone (ABI 37):
 *     y[r] = x[r] * rsqrt(max(sum_c x[r][c]^2, 1e-12))          (tf.nn.l2_normalize(x, dim=1))
 * then relu if flags == DG_EPI_RELU (model.py:75).  x, y: [n_rows][d], contiguous, 16-byte
 * aligned; y == x is allowed (each row is read whole before it is written).  Replaces
 * layers.py:93 / :117 when the sum was formed elsewhere (dg_spmm_csr_f32 with beta = 1); the
 * layer kernels fuse the same arithmetic into their epilogues (dg_gcn_epilogue_f32 with one
 * group of one chunk runs it: bitwise the same rows). */
int dg_rownorm_l2_f32(const float* x, float* y, int32_t n_rows, int32_t d, int32_t flags, void* stream);

/* --------------------------------------------------------------------------------------
 * Fused GCN layer (T3 + T4 + T5 + T6, optionally T7 of the next layer, in one launch) for
 * node types whose groups each fit one chunk: for every target t (a node type i), r < n_rows,
 *
 *     out_t[r] = act( sum_{g in [g_begin, g_begin+g_count)} l2norm( sum_k A_g,k[r]·X_g,k ) )
 *
 * act = relu if flags & DG_EPI_RELU.  Every group must have n_chunks == 1; `out` is ignored.
 * One workgroup per output row, `waves_per_group` waves per group sharing the row's nonzeros
 * (g_count * waves_per_group <= 16).
 * Projection epilogue: for each dg_proj p with p.target == t,
 *     p.out[rel(kk)][r][c] = sum_k out_t[r][k] * p.w[rel(kk)][k][c]   kk < p.n_rels, c < d_out
 * (rel(kk) = p.rel_map[kk] or kk; p.w is a [K][d][d_out] stack, p.out [K][n_rows][d_out])
 * — the next layer's H_j·W_k (layers.py:113) for the rows just produced.
 * Replaces the per-relation SpMM + add_n + l2_normalize of layers.py:85-94 / 109-118 and the
 * sum over edge types (+ relu) of model.py:74-75 / 85-88.
 * -------------------------------------------------------------------------------------- */
typedef struct dg_fused_target {
    float* out;                 /* device, [n_rows][d] */
    int32_t n_rows;
    int32_t g_begin;
    int32_t g_count;
    int32_t flags;              /* 0 or DG_EPI_RELU */
} dg_fused_target;

typedef struct dg_proj {
    const float* w;             /* device, [K][d][d_out] weight stack        */
    const int32_t* rel_map;     /* device, [n_rels] or NULL                  */
    float* out;                 /* device, [K][n_rows of target][d_out]      */
    int32_t n_rels;
    int32_t target;             /* index into the targets array              */
    int32_t d_out;
    int32_t reserved;
} dg_proj;

int dg_gcn_fused_f32(const dg_rel_group* groups /* HOST */, int32_t n_groups,
                     const dg_fused_target* targets /* HOST */, int32_t n_targets,
                     const dg_proj* projs /* HOST, may be NULL */, int32_t n_projs,
                     int32_t waves_per_group, int32_t d, void* stream);

/* --------------------------------------------------------------------------------------
 * Relation-segment SpMM (partial mode; one wave per (row, relation)), optionally with the
 * next layer's projection reassociated into it — the sharded config-S form (one relation set
 * per GPU, every node type row-split), where a rank's short row block would leave
 * most CUs idle at one workgroup per row.  Over dg_rel_group's chunk-merged CSR with `chunk`
 * relations per chunk (relation k = c*chunk + t), for every chunk c and row r:
 *
 *   w == NULL:  out[c][r][:]  = sum_{t} sum_{p in seg(c,r,t)} val[p] * X[vcol[p]][:]
 *   w != NULL:  out[c][r][:]  = sum_{t} ( sum_{p in seg(c,r,t)} val[p] * H[vcol[p] - s*n_cols][:] ) · W[s]
 *               (s = slab[k] or k; H = x, [n_cols][x_ld]; W a [K][64][32] stack)
 *
 * The second form is layer 2 as sum_k (A_k·H1_j)·W2_k instead of sum_k A_k·(H1_j·W2_k)
 * (layers.py:113-114): the shared H1_j is gathered and only this rank's rows are projected.
 * seg[(c*n_rows + r)*chunk + t] is the first nonzero of relation t of chunk c in row r inside
 * [rowptr[c*n_rows + r], rowptr[c*n_rows + r + 1]); a segment ends where the next one starts
 * (the last one at the range's end).  Relations run in t order within a range (merge_chunks).
 * Requirements: 1 <= chunk <= 16, (n_chunks - 1)*chunk < n_rels <= n_chunks*chunk;
 * w == NULL: d_in == d_out in {32, 64}; w != NULL (every group): d_in == 64, d_out == 32;
 * x, out, w and x_ld 16-byte aligned; x_rows * x_ld < 2^31 with 0 <= vcol < x_rows.
 * Replaces: tf.sparse_tensor_dense_matmul + tf.add_n (layers.py:90-92, :114-116) over a
 * chunk's relations, and tf.matmul(x, weights_k) (layers.py:113).
 * -------------------------------------------------------------------------------------- */
typedef struct dg_seg_group {
    const int32_t* rowptr;      /* device, [n_chunks*n_rows + 1]                          */
    const int32_t* seg;         /* device, [n_chunks*n_rows*chunk] segment starts         */
    const int32_t* vcol;        /* device, [nnz]                                          */
    const float* val;           /* device, [nnz]                                          */
    const int32_t* slab;        /* device, [n_rels] slab of local relation k, or NULL     */
    const float* x;             /* device: stacked X (w == NULL) or H [n_cols][x_ld]      */
    const float* w;             /* device, [K][64][32] weight stack, or NULL              */
    float* out;                 /* device, [n_chunks][n_rows][d_out]                      */
    int64_t x_ld;
    int32_t n_rows;
    int32_t n_cols;
    int32_t n_chunks;
    int32_t chunk;
    int32_t n_rels;
    int32_t x_rows;             /* bound on vcol (K*n_cols for the stacked forms)         */
} dg_seg_group;

int dg_spmm_seg_f32(const dg_seg_group* groups /* HOST array */, int32_t n_groups, int32_t d_in,
                    int32_t d_out, void* stream);

/* The fused form: a whole layer for the target node types, every output row finished in one
 * workgroup.  Groups are chunk-merged as for dg_spmm_seg_f32 (any n_chunks; n_rels >= 1).
 * For every target t (dg_fused_target: out [n_rows][d_out], groups [g_begin, g_begin + g_count),
 * flags 0 or DG_EPI_RELU; groups[i].out unused) and row r < n_rows:
 *
 *   out_t[r] = act( sum_g l2norm( sum_{t < n_rels_g} seg-sum_g(r, t) ) )
 *
 * with seg-sum as dg_spmm_seg_f32's over relation t = c*chunk + t' of the group (projected by
 * W[slab] when the groups carry w), at most 16 relations a target row in total.  One
 * workgroup per row, one wave per (group, relation); relations and groups summed in order.
 * With w this is layer 2 (layers.py:109-118) reassociated, Σ_k (Â_k·H1_j)·W2_k, so layer 1
 * needs no projection of its rows.  Replaces layers.py:85-94 / 109-118 and model.py:74-75,
 * 85-88 for such node types. */
int dg_gcn_fused_seg_f32(const dg_seg_group* groups /* HOST */, int32_t n_groups,
                         const dg_fused_target* targets /* HOST */, int32_t n_targets, int32_t d_in,
                         int32_t d_out, void* stream);

/* The wave-table form of dg_gcn_fused_seg_f32 (round 5): the same launch — workgroups, waves and
 * arithmetic — with everything a wave needs before its gathers precomputed on the host
 * (decagon_amd/wavetable.py; kernels.PreparedFusedTab uploads it) instead of found at run time from the
 * group and target arguments.  Wave w of workgroup b (slot i = b * nw_stride + w) reads desc[i]
 * and the first batch of its pairs (vcol, fp32 value bits: int32 pairs) in one round trip: the
 * first batch is compact, the S = slot_pairs pairs at pairs[S i .. S i + S - 1]; a wave with
 * more than S pairs continues in ovf[desc[i].ovf ..] in batches of 64.  Every shape uses the DPP
 * hand-out order of the seg form (both layers since round 6): with G = 256 / (4 d_in) pairs
 * handed out at once (4 at d_in 64, 8 at d_in 32), pair m < S of the wave sits at slot entry
 * (m % G) * S/G + m / G, and pair j of a later batch at entry (64/G) * (j % G) + j / G.
 * A wave with cnt 0 gathers nothing.  The wave whose desc.orow != NULL finishes that output row
 * alone after the workgroup's barrier: wr holds the row's group count, its relu bit and its row
 * slot (DG_TAB_WR_*), gwaves the (wave count - 1) of group u in bits 4u .. 4u + 3, first_wave the
 * row slot's first wave; it adds each group's waves in order, L2-normalises the group sums, adds
 * them in order, applies relu and stores the row.  The rows are bitwise dg_gcn_fused_seg_f32's only
 * for a table with one wave per relation; a table that deals a group's pairs over several waves
 * (PreparedFusedTab's balance) re-associates the group's fp32 sum.
 *
 * Which entry point reads which field beyond x, w, orow, cnt, x_ld and ovf (all of them), and
 * what the auxiliary words (aux_lo, aux_hi: the low and high half of one 64-bit value, or two
 * 32-bit values) hold; the builder writes nothing else:
 *
 *   entry point                 role                        wr, gwaves, first_wave  aux_lo, aux_hi
 *   dg_gcn_fused_tab_f32        -                           finishing wave          -
 *   dg_gcn_fused_tab_peer_f32   -                           finishing wave          finishing wave: the row's byte
 *                                                                                   offset in its target, the
 *                                                                                   target's bytes
 *   dg_gcn_fused_tab_post_f32   DG_TAB_ROLE_PROJ_BIT and    finishing wave          projecting wave: the address of
 *                               the PROJ_SLOTS mask                                 row slot 0's P row
 *   dg_gcn_fused_tab_dec_f32    DG_TAB_ROLE_DEC_BIT         finishing wave          flagged finishing wave: the
 *                                                                                   address of the row's Q row
 *   dg_spmm_seg_tab_f32         the SEG_WAVES field         -                       -
 *
 * Every finishing wave of a fused table carries the peer form's two values unless a projection
 * job or a decoder row of the same wave needs the words (neither form has an exchange).
 * Shapes: d_in = d_out = 64; d_in = 64, d_out = 32 with W slabs (desc.w: the aggregate times the
 * relation's slab, so such a wave holds pairs of one relation); d_in = d_out = 32 (no exchange
 * form).  Replaces layers.py:85-94 / 109-118 and model.py:74-75, 85-88 as dg_gcn_fused_seg_f32
 * does. */
typedef struct dg_tab_desc {
    const float* x;       /* device: gather base (vcol * x_ld floats from here)             */
    const float* w;       /* device: the wave's W slab [64][32] (d_out 32, or a projection   */
                          /* job of dg_gcn_fused_tab_post_f32), or NULL                      */
    float* orow;          /* device: the output row this wave finishes and writes, or NULL  */
    int32_t cnt;          /* pairs of the wave (0: none)                                     */
    int32_t x_ld;         /* floats                                                          */
    int32_t ovf;          /* first entry of the later batches in ovf                         */
    uint32_t role;        /* DG_TAB_ROLE_* below                                             */
    uint32_t wr;          /* finishing wave: DG_TAB_WR_* below                               */
    int32_t aux_lo;       /* the auxiliary value (table above), low half or first value      */
    int32_t aux_hi;       /* high half or second value                                       */
    int32_t gwaves;       /* finishing wave: the groups' wave counts, DG_TAB_GWAVES_BITS each */
    int32_t first_wave;   /* finishing wave: the first wave of its row slot                  */
    int32_t reserved;     /* 0                                                               */
} dg_tab_desc;            /* 64 bytes                                                        */

/* dg_tab_desc.role */
#define DG_TAB_ROLE_PROJ_BIT 30         /* the wave holds a projection job (..._tab_post_f32)   */
#define DG_TAB_ROLE_PROJ_SLOTS_SHIFT 24 /* the job's row slots: a mask of                       */
#define DG_TAB_ROLE_PROJ_SLOTS_BITS 4   /* DG_TAB_MAX_ROW_SLOTS bits                            */
#define DG_TAB_ROLE_DEC_BIT 29          /* the finishing wave also stores its Q row (..._dec_f32) */
#define DG_TAB_ROLE_SEG_WAVES_SHIFT 8   /* dg_spmm_seg_tab_f32: the waves the first wave of a    */
#define DG_TAB_ROLE_SEG_WAVES_BITS 8    /* (chunk, row) sums, itself included                    */
/* dg_tab_desc.wr */
#define DG_TAB_WR_GROUPS_BITS 8         /* bits 0-7: the row's groups                           */
#define DG_TAB_WR_RELU_BIT 8            /* relu the finished row                                */
#define DG_TAB_WR_SLOT_SHIFT 16         /* bits 16 and up: the row slot                         */
/* dg_tab_desc.gwaves: (wave count - 1) of group u in bits 4u .. 4u + 3 */
#define DG_TAB_GWAVES_BITS 4
#define DG_TAB_MAX_ROW_SLOTS 4          /* rows a workgroup finishes, at most                   */

typedef struct dg_wave_table {
    const int32_t* pairs; /* device, [n_blocks * nw_stride * slot_pairs][2], 16-byte aligned */
    const int32_t* ovf;   /* device, [..][2], or NULL                                        */
    const dg_tab_desc* desc; /* device, [n_blocks * nw_stride], 64-byte aligned             */
    int32_t n_blocks;
    int32_t nw;           /* waves per workgroup, 1..16                                      */
    int32_t nw_stride;    /* 8 if nw <= 8, else 16                                           */
    int32_t slot_pairs;   /* S: pairs of a wave's first batch, 16 / 32 / 48 / 64 (ABI 37;     */
                          /* 0 means 64), laid out as described above                         */
} dg_wave_table;

int dg_gcn_fused_tab_f32(const dg_wave_table* table /* HOST */, int32_t d_in, int32_t d_out, void* stream);

/* dg_gcn_fused_tab_f32 for a d_in = d_out = 64 table that also carries projection jobs: layer 1
 * makes layer 2's operands P_k = H1_j·W2_k (layers.py:113, the reference's own order: matmul,
 * then the sparse product) in the workgroup that finishes the H1 row.  The finishing wave also
 * leaves its row (after relu, as stored) in LDS; after one more barrier every wave whose
 * desc.role has DG_TAB_ROLE_PROJ_BIT set multiplies the row of each row slot s in its PROJ_SLOTS mask
 * by the [64][32] slab at desc.w and stores the 32 floats at A + 128 s bytes, A the 16-byte
 * aligned address in aux_lo (low half) and aux_hi (high half): row slot 0's P row (the rows of a
 * workgroup are consecutive).  A wave may hold a gather job, a projection job, both or neither; a
 * job names only row slots whose finishing wave exists in the same workgroup.  The H1 rows are
 * bitwise dg_gcn_fused_tab_f32's of the same table.  The table itself cannot say that it carries
 * jobs, hence the separate entry point; arguments are checked as dg_gcn_fused_tab_f32's, and
 * only d_in = d_out = 64 is accepted. */
int dg_gcn_fused_tab_post_f32(const dg_wave_table* table /* HOST */, int32_t d_in, int32_t d_out, void* stream);

/* dg_gcn_fused_tab_f32 for a d_in = d_out = 32 table (layer 2 over pre-projected operands) that
 * also makes the DEDICOM decoder's row operands: the finishing wave of a row whose desc.role has
 * DG_TAB_ROLE_DEC_BIT set stores, after the row itself, Q[r] = l ∘ ((row ∘ l)·G) — 32 floats at the
 * 16-byte aligned address in aux_lo (low half) and aux_hi (high half) — so that a score is the dot
 * product Q[r]·E[c] (dg_decoder_hinge_rows_f32).  G is [32][32] row-major, l [32] or NULL (all
 * ones), both device, 16-byte aligned (DG_EALIGN otherwise).  The summation order is fixed: Q is
 * bitwise reproducible, and the rows are bitwise dg_gcn_fused_tab_f32's of the same table.  Other
 * shapes, or G == NULL, give DG_EINVAL. */
int dg_gcn_fused_tab_dec_f32(const dg_wave_table* table /* HOST */, int32_t d_in, int32_t d_out, const float* G,
                             const float* l, void* stream);

/* dg_gcn_fused_tab_f32 with the peer-store exchange (config S at N = 2 with --exchange peer):
 * every finished row also goes to every peer's copy of its target — desc.aux_lo = the row's
 * byte offset in its target, desc.aux_hi = the target's bytes, the target inside the exchange
 * region — and the launch ends with the exchange, as dg_gcn_fused_seg_peer_f32.  xchg as
 * dg_peer_allgather; at least one workgroup. */
struct dg_peer_xchg;
int dg_gcn_fused_tab_peer_f32(const dg_wave_table* table /* HOST */, int32_t d_in, int32_t d_out,
                              const struct dg_peer_xchg* xchg /* HOST */, void* stream);

/* The wave-table form of dg_spmm_seg_f32 (partial mode; config S's N-GPU layers): the same
 * workgroups (in that entry point's XCD-contiguous item order), waves and chunk partials, bit
 * for bit, from a host-built table with the layout above.  A wave whose desc.orow != NULL is
 * the first wave of its (chunk, row): after the barrier it adds the waves of desc.role's
 * SEG_WAVES field from itself on, in order, and stores the partial row there.  Shapes as above. */
int dg_spmm_seg_tab_f32(const dg_wave_table* table /* HOST */, int32_t d_in, int32_t d_out, void* stream);

/* --------------------------------------------------------------------------------------
 * LDS-staged relation SpMM for groups of many relations over a narrow column space
 * (polypharmacy drug x drug: 1,928 relations of 645 x 645).  For output chunk c (out_chunk
 * consecutive relations):
 *
 *     out[c][r][:] = sum_{k in chunk c} sum_{p in row r of A_k} val[p] * X[slab(k)*n_cols + col[p]][:]
 *
 * Layout (built on the host by decagon_amd/sparse.py: staged_layout): per relation, a long
 * row becomes a group of <= 8 equal-length segments (virtual rows; padding pairs read one
 * of sixteen zero columns n_cols .. n_cols + 15, value 0), at most 1024 virtual rows (16 waves of 64 lanes) sorted by length
 * with each group inside one wave; wave w's pairs form a dense block [rlw_w][64] (rlw_w a
 * multiple of 4; holes are padding pairs), lane j's pair at diagonal m at woff_w + 64 m + j:
 *   pairs      [n_pairs][2] int32: (column, fp32 value bits), relations and waves back to
 *              back; 16-byte aligned
 *   jm, jmoff  relation k's tables at jm[jmoff[k] .. jmoff[k+1]): [n_waves, largest group,
 *              0, 0], woff[16], rlw[16] (0 past n_waves), vinfo[64 n_waves] = row |
 *              segment << 10 | (group size - 1) << 13 | length << 16 (row 1023: padding
 *              lane); jm ends with 1024 spare ints (jm_len >= jmoff[n_rels] + 1024)
 * One workgroup of 1024 threads per (c, 16-float column slice); thread i owns sorted virtual
 * row i and streams its pairs from global memory (one coalesced load per wave and diagonal);
 * the slab slice is in LDS and every nonzero gathers from it; the segments of a row are
 * summed in segment order.  Requirements: n_rows < 1023; n_cols <= 1024; out_chunk <= 64;
 * d % 4 == 0; x, x_ld 16-byte aligned.
 * Replaces layers.py:90-92 / :114-116 for such groups.
 * -------------------------------------------------------------------------------------- */
typedef struct dg_staged_group {
    const int32_t* pairs;       /* device, [n_pairs][2]                                  */
    const int32_t* jm;          /* device                                                */
    const int32_t* jmoff;       /* device, [n_rels + 1]                                  */
    const int32_t* slab;        /* device, [n_rels] slab of relation k, or NULL (= k)    */
    const float* x;             /* device, relation-stacked dense operand                */
    float* out;                 /* device, [ceil(n_rels/out_chunk)][n_rows][d]           */
    int64_t x_ld;
    int32_t n_rows;
    int32_t n_cols;
    int32_t n_rels;
    int32_t out_chunk;          /* relations summed into one output chunk (<= 64)        */
    int32_t x_rows;             /* rows of x addressable                                 */
    int32_t jm_len;             /* ints in jm, including the 1024 spare                  */
    /* Variable output chunks (or NULL: chunk c = relations [c·out_chunk, (c+1)·out_chunk)):
     * HOST [n_chunks + 1], chunk c = relations [chunk_start[c], chunk_start[c+1]); starts at 0,
     * ends at n_rels (<= 65535), 1..64 relations a chunk, n_chunks <= DG_STAGED_MAX_CHUNKS.
     * out is then [n_chunks][n_rows][d].  Copied into the launch's arguments. */
    const int32_t* chunk_start;
    int32_t n_chunks;
    int32_t pad;
} dg_staged_group;
#define DG_STAGED_MAX_CHUNKS 128

int dg_spmm_staged_f32(const dg_staged_group* groups /* HOST */, int32_t n_groups, int32_t d,
                       void* stream);

/* The same SpMM with each relation's dense operand made in the workgroup instead of read:
 *     X_k = H · W[slab(k)]        (H [n_cols][64] row-major, leading dimension h_ld; W [K][64][d])
 * — layer 2's projection H1_j · W2_k (layers.py:113) fused into its SpMM (layers.py:114): the
 * slab slice comes from the fp32 MFMA (exact fp32 products, k summed in a fixed order) into
 * LDS, so the [K][n_cols][d] operand is never written to or read from HBM.  groups[i].x /
 * x_ld / x_rows are ignored.  Requirements as dg_spmm_staged_f32, plus din == 64, h and h_ld
 * 16-byte aligned.  Replaces layers.py:113-116 for such groups. */
typedef struct dg_staged_proj {
    const float* h;             /* device, [n_cols][h_ld]                                 */
    const float* w;             /* device, [K][din][d]                                     */
    int64_t h_ld;
    int32_t din;                /* 64                                                      */
    int32_t pad;
} dg_staged_proj;

int dg_spmm_staged_proj_f32(const dg_staged_group* groups /* HOST */, const dg_staged_proj* projs /* HOST */,
                            int32_t n_groups, int32_t d, void* stream);


/* Host-only layout helper: one relation's pair block of the staged layout.  Its lanes
 * (virtual rows; n_lanes = 64 x waves) are given as a CSR over lanes (HOST arrays: lrowptr
 * [n_lanes + 1], lcol / lval the lanes' nonzeros in any order), rlw[wave] the wave's diagonals
 * (>= its longest lane).  Fills pairs [sum rlw x 64][2] (wave w's block after the blocks of
 * waves < w; lane j's pair at diagonal m at 64 m + j: (column, fp32 value bits); holes
 * (n_cols + z, 0) with z < 16).  The diagonal of each nonzero and the zero column of each
 * hole are chosen so that the lanes of each ds_read_b128 lane group read different bank
 * slots at every diagonal where the relation allows (a fixed order: the row sums change only
 * by rounding, deterministically). */
int dg_staged_block(const int32_t* lrowptr, const int32_t* lcol, const float* lval, int32_t n_lanes,
                    const int32_t* rlw, int32_t n_cols, int32_t* pairs);

/* --------------------------------------------------------------------------------------
 * GCN epilogue (T4 tail + T5 + T6):  for one node type i with groups g = (i, j_1..j_m),
 *
 *     s_g[r]   = sum_{c < n_chunks_g} partial_g[c][r][:]              (chunk order)
 *     y_g[r]   = s_g[r] * rsqrt(max(sum(s_g[r]^2), 1e-12))            if DG_EPI_L2NORM
 *     out[r]   = act( sum_g y_g[r] )                                  (group order)
 *
 * act = relu if DG_EPI_RELU.  With DG_EPI_CHUNK_RELU each chunk partial is passed through
 * relu before the chunk sum (a layer built with act=relu and chunk = 1 applies the
 * activation per relation before add_n, layers.py:91).  With one group and no flags this is
 * the plain chunk reduce used before the cross-GPU all-reduce.
 * Replaces: tf.nn.l2_normalize(outputs, dim=1)   layers.py:93, :117
 *           tf.nn.relu(tf.add_n(hid1))           model.py:75
 *           tf.add_n(embeds)                     model.py:88
 * -------------------------------------------------------------------------------------- */
#define DG_EPI_L2NORM 1
#define DG_EPI_RELU 2
#define DG_EPI_CHUNK_RELU 4

typedef struct dg_epi_group {
    const float* partial;       /* device, [n_chunks][n_rows][d] */
    float* sum_out;             /* device, [n_rows][d]: the group's pre-normalisation sum
                                   S_ij (what the backward of l2_normalize needs), or NULL */
    int32_t n_chunks;
    int32_t group_flags;        /* 0, or DG_EPI_PUSH (dg_gcn_epilogue_peer_f32 only): sum_out also
                                 * stored into every peer's copy — the rank's slot of the peer
                                 * all-reduce of the sums (ABI 34) */
} dg_epi_group;

int dg_gcn_epilogue_f32(const dg_epi_group* groups /* HOST array */, int32_t n_groups,
                        float* out, int32_t n_rows, int32_t d, int32_t flags, void* stream);

/* Several node types' epilogues in one launch (every target's rows finish side by side; the
 * groups of all targets together at most DG_MAX_GROUPS).  Same flags for all targets. */
#define DG_EPI_MAX_TARGETS 8
typedef struct dg_epi_target {
    const dg_epi_group* groups; /* HOST array of n_groups                                   */
    int32_t n_groups;
    int32_t reserved0;
    float* out;                 /* device, [n_rows][d], 16-byte aligned                     */
    int32_t n_rows;
    int32_t target_flags;       /* 0, or DG_EPI_PUSH (dg_gcn_epilogue_peer_f32 only)        */
    int32_t reserved[2];
} dg_epi_target;

int dg_gcn_epilogue_multi_f32(const dg_epi_target* targets /* HOST array */, int32_t n_targets,
                              int32_t d, int32_t flags, void* stream);

/* The row-table form (round 5): the same rows, sums and order — bitwise the multi form's rows —
 * from a host-built descriptor per output row (decagon_amd/kernels.py: PreparedEpilogueTab), so
 * a wave issues every group's partial loads at once.  Row i of the table: rows[i].out + off is
 * the output row (its target's output base in .out); group g < (info & 7) <= 4 has
 * (n_chunks >> 8g) & 0xff chunk partials at part[g] + c * plane; info bit 8: with xchg, the row
 * also goes to every peer's copy of .out (bytes = the target's output size).  No group sums
 * (dg_epi_group.sum_out).  d = 32 or 64; rows 64-byte aligned; xchg as dg_gcn_epilogue_peer_f32
 * (the launch then ends with the exchange), or NULL. */
typedef struct dg_epi_row_desc {
    float* out;
    const float* part[4];
    int32_t off;
    int32_t plane;
    uint32_t n_chunks;
    uint32_t info;
    int32_t bytes;
    int32_t pad;
} dg_epi_row_desc;        /* 64 bytes */

struct dg_peer_xchg;
int dg_gcn_epilogue_tab_f32(const dg_epi_row_desc* rows, int32_t n_rows, int32_t d, int32_t flags,
                            const struct dg_peer_xchg* xchg /* HOST, or NULL */, void* stream);

/* --------------------------------------------------------------------------------------
 * Peer-store exchange over xGMI: the all-gather of the row-split blocks of the sharded
 * forward (decagon_amd/sharding.py; one per layer, made necessary by the normalisation of
 * the full per-(i,j) sum, layers.py:92-93), without RCCL.
 *
 * Every rank holds the row-split outputs of a layer in ONE exchange region of the same layout
 * on every rank (its own rows block `rank`); each rank maps every peer's region (IPC) and
 * stores its finished rows straight into them, write-through at system scope.  The launch's
 * last workgroup then stores the slot's epoch into word [slot][rank] of every peer's flag
 * block (uncached memory) and waits — bounded by timeout_ticks of the 100 MHz s_memrealtime
 * clock — until every rank's epoch for the slot has arrived in its own block; the kernels
 * that read the gathered rows start after that launch ends.  A wait that times out sets the
 * error word state[DG_PEER_ERROR_WORD] (0x10000 | slot << 8 | source rank) and returns; once
 * it is set, every later wait returns at once (the host checks the word and raises).
 * state: this rank's device words (DG_PEER_STATE_WORDS), zeroed once: per slot {arrivals, epoch},
 * then the error word; from DG_PEER_SUB_BASE, 8 arrival sub-counters per slot, DG_PEER_SUB_STRIDE
 * words apart (launches of >= 128 workgroups count their arrivals in two levels).
 * A slot's launches must all use the same grid (the arrival count), and every rank must run
 * the same sequence of exchanges per slot.
 * Replaces: the RCCL/NCCL all-gather of the sharded step (the reference has no parallelism).
 * -------------------------------------------------------------------------------------- */
#define DG_PEER_MAX 8
#define DG_PEER_SLOTS 8
#define DG_PEER_SUB_BASE 64
#define DG_PEER_SUB_STRIDE 16
#define DG_PEER_STATE_WORDS (DG_PEER_SUB_BASE + DG_PEER_SLOTS * 8 * DG_PEER_SUB_STRIDE)
#define DG_PEER_ERROR_WORD (2 * DG_PEER_SLOTS)
/* Wait records (round 6), in the state words between the error word and the sub-counters.
 * The wait that times out writes, before the error word: DIAG+0 its slot, +1 the epoch it
 * expected, +2..+9 the flag word it last read from each source, +10/+11 the s_memrealtime tick
 * its wait started (low / high word), +12/+13 the tick it gave up, +14/+15 the tick this rank
 * raised its own flags.  Every wait that completes after more than DG_PEER_SLOW_TICKS adds 1 to
 * +16 and max-updates +17 with its ticks (a completed wait costs one compare otherwise).  A
 * host that finds the error word reads these and, with dg_peer_read, the flag words as they
 * stand now: a late source's flag that has since reached the expected epoch was late (a host or
 * scheduling skew longer than the bound); one still short of it was never raised. */
#define DG_PEER_DIAG_BASE 24
#define DG_PEER_DIAG_WORDS 18
#define DG_PEER_SLOW_TICKS 10000 /* 100 µs */
#define DG_IPC_HANDLE_BYTES 64
#define DG_EPI_PUSH 1           /* dg_epi_target.target_flags: push this target's rows          */

typedef struct dg_peer_xchg {
    int64_t delta[DG_PEER_MAX];   /* bytes from this rank's exchange region to rank p's region as
                                     mapped in this process (delta[rank] = 0; 16-byte multiples) */
    uint32_t* flags[DG_PEER_MAX]; /* rank p's flag block [DG_PEER_SLOTS][DG_PEER_MAX], mapped here */
    uint32_t* state;              /* device, DG_PEER_STATE_WORDS words of THIS rank, zeroed once  */
    int64_t timeout_ticks;        /* > 0: s_memrealtime ticks (100 MHz) a wait may spin           */
    int32_t rank, world;          /* 1 <= world <= DG_PEER_MAX                                    */
    int32_t slot;                 /* < DG_PEER_SLOTS                                              */
    int32_t loopback;             /* 1: one-GPU rehearsal — every "peer" region is local scratch, */
                                  /* flags[p] all this rank's block, and the last workgroup raises */
                                  /* word [slot][p] for every p itself                             */
} dg_peer_xchg;

/* Device memory for the exchange: kind 0 = hipMalloc-like (coarse-grained), 1 = fine-grained,
 * 2 = uncached (the flag blocks).  Zero-filled.  These two are the library's only allocating
 * entry points; the memory is the caller's to free with dg_peer_free. */
int dg_peer_alloc(int64_t bytes, int32_t kind, void** ptr /* HOST out */);
int dg_peer_free(void* ptr);
/* IPC: the handle (DG_IPC_HANDLE_BYTES, host) of the allocation holding ptr and ptr's byte
 * offset in it; open / close a peer process's handle in this process. */
int dg_ipc_get_handle(void* ptr, void* handle /* HOST out */, int64_t* offset /* HOST out */);
int dg_ipc_open(const void* handle /* HOST */, void** ptr /* HOST out */);
int dg_ipc_close(void* ptr);
/* Synchronous copy of `bytes` of device memory (a flag block) to the host: the timeout record's
 * "flag words now" read (decagon_amd/peer.py PeerExchange.diagnostics). */
int dg_peer_read(const void* device, void* host /* HOST out */, int64_t bytes);

/* Stand-alone exchange: push bytes [offsets[s], offsets[s] + sizes[s]) of this rank's region
 * (its blocks) into every peer's region at the same offsets, then raise / wait as above. */
int dg_peer_allgather(const dg_peer_xchg* xchg /* HOST */, const void* region, const int64_t* offsets /* HOST */,
                      const int64_t* sizes /* HOST */, int32_t n_seg, void* stream);

/* dg_gcn_epilogue_multi_f32 that also pushes the rows of every target with DG_EPI_PUSH (its
 * `out` inside the exchange region) to every peer and ends with the exchange: the finishing
 * launch of a row-split layer and its all-gather in one kernel. */
int dg_gcn_epilogue_peer_f32(const dg_epi_target* targets /* HOST array */, int32_t n_targets, int32_t d,
                             int32_t flags, const dg_peer_xchg* xchg /* HOST */, void* stream);

/* dg_gcn_fused_seg_f32 whose every target's `out` lies in the exchange region: the rows are
 * also pushed to every peer and the launch ends with the exchange (config S at N = 2: a
 * layer and its all-gather in one kernel). */
int dg_gcn_fused_seg_peer_f32(const dg_seg_group* groups /* HOST */, int32_t n_groups,
                              const dg_fused_target* targets /* HOST */, int32_t n_targets, int32_t d_in,
                              int32_t d_out, const dg_peer_xchg* xchg /* HOST */, void* stream);

/* --------------------------------------------------------------------------------------
 * Batched strided fp32 GEMM on the f32-input MFMA (v_mfma_f32_32x32x2_f32, exact fp32):
 *
 *   C_b[m][n] = sc[n] * sum_k (sa[k] * A_b[m][k]) * B_b[k][n]        b < batch
 *
 * Element (m,k) of A_b is A[b*a_bs + m*a_sm + k*a_sk]; likewise B (k,n) and C (m,n).
 * sa / sc are optional (NULL = ones).  If b_map is non-NULL, batch b reads B at
 * b + b_map[b]*b_bs and writes C at c + b_map[b]*c_bs (a rank's relation shard of a
 * relation-indexed stack).  No alignment requirement.
 * Replaces: tf.matmul(x, weights_k)                          layers.py:113 (batched over k)
 *           tf.matmul chain row·L·G·L·colᵀ (predict)         optimizer.py:87-106
 * -------------------------------------------------------------------------------------- */
typedef struct dg_gemm_desc {
    const float* a;
    const float* b;
    float* c;
    const float* sa;            /* [K] or NULL */
    const float* sc;            /* [N] or NULL */
    const int32_t* b_map;       /* [batch] or NULL */
    int64_t a_bs, a_sm, a_sk;
    int64_t b_bs, b_sk, b_sn;
    int64_t c_bs, c_sm, c_sn;
    int32_t m, n, k, batch;
    int32_t reduce;             /* 0, or R > 0: batch-reduce mode (below; b_map maps B and the mask) */
    uint32_t drop_tag;          /* batch-reduce with dropout: mask stream tag */
    const uint64_t* drop_state; /* NULL, or the device dropout state {seed, step} (below) */
    float drop_keep;            /* keep probability when drop_state != NULL */
    int32_t reserved;
} dg_gemm_desc;

int dg_gemm_f32(const dg_gemm_desc* descs /* HOST array */, int32_t n_desc, void* stream);
/* n_desc <= DG_MAX_GROUPS independent GEMMs in one launch (e.g. every (i,j) group's
 * layer-2 projection).
 * Batch-reduce mode (reduce = R > 0): the batches are summed in runs of R consecutive
 * batches (in batch order) and run q's sum is written at c + q*c_bs, q < ceil(batch / R):
 *     C_q = Σ_{b in [qR, min(qR+R, batch))} A_b·B_b
 * — the backward's Σ_k dP_k·W_kᵀ (gradient of the per-relation projections, layers.py:113)
 * as partial sums that dg_gcn_epilogue_f32 (no flags) adds up.  With drop_state != NULL each
 * batch product is first multiplied element-wise by its dropout mask (mask element
 * (b·m + row)·n + col of stream drop_tag, scaled by 1/keep, as dg_dropout_elems_f32 draws it):
 *     C_q = Σ_b M_b∘(A_b·B_b)   — the gradient through tf.nn.dropout (layers.py:112).
 * With b_map in batch-reduce mode, batch b reads B at b_map[b] and takes the mask of batch
 * b_map[b] (a rank's relation shard: local batch b is global relation b_map[b]); A and the run
 * index are not mapped. */

/* Batched Aᵀ·B over a long reduction (the weight gradient H_jᵀ·dP_k, backward of
 * layers.py:113):  C_b[m][n] = Σ_{r < rows} A[b*a_bs + r*lda + m] · B[b*b_bs + r*ldb + n],  C
 * contiguous [batch][M][N].  M, N multiples of 32 with (M/32)(N/32) <= 4.  With n_split > 1
 * the rows are cut into n_split ranges whose partials ([n_split][batch][M][N], caller's
 * 16-byte aligned `partial`) are then summed in range order. */
int dg_gemm_tn_f32(const float* a, int64_t lda, int64_t a_bs, const float* b, int64_t ldb, int64_t b_bs,
                   float* c, int32_t rows, int32_t M, int32_t N, int32_t batch, int32_t n_split,
                   float* partial, void* stream);

/* --------------------------------------------------------------------------------------
 * Edge decoder scores (T8 + T9):  for pair p,
 *     u = row_table[row_idx[p]],  v = col_table[col_idx[p]]       (rows of length d)
 *     out[p] = sum_j ( sum_k u[k] l[k] G[k][j] ) l[j] v[j]         (= uᵀ·L·G·L·v)
 * G is dense d×d row-major; l is the diagonal of L (NULL = identity).  This is the diagonal
 * of the reference's B×B product, computed without forming it.
 * Replaces: batch_predict + tf.diag_part   optimizer.py:51-57, :63-85
 * Requirements: d % 32 == 0, d <= 256.
 * -------------------------------------------------------------------------------------- */
int dg_decoder_score_f32(const float* row_table, int64_t ld_row, const float* col_table,
                         int64_t ld_col, const int32_t* row_idx, const int32_t* col_idx,
                         int32_t n_pairs, const float* G, const float* l, int32_t d,
                         float* out, void* stream);

/* bf16 DEDICOM scores (BASELINE config 5): for pair p of relation k = rel_idx[p] (rel_idx
 * NULL: k = 0), u = row_table[row_idx[p]], v = col_table[col_idx[p]] (bf16 rows),
 *     out[p] = sum_n ( sum_i bf16(u_i * l_k[i]) * G[i][n] ) * l_k[n] * v_n     (fp32 accumulation)
 * G: bf16 d×d row-major (DEDICOM's global R); l_table: bf16 [n_rel][d] diagonals D_k (NULL =
 * identity).  Pairs may mix relations.  d ∈ {64, 128, 256}; tables 16-byte aligned rows.
 * Replaces batch_predict (optimizer.py:63-85) for DEDICOM relations (model.py:130-134). */
int dg_decoder_score_bf16(const uint16_t* row_table, int64_t ld_row, const uint16_t* col_table,
                          int64_t ld_col, const int32_t* row_idx, const int32_t* col_idx,
                          const int32_t* rel_idx, int32_t n_pairs, const uint16_t* G,
                          const uint16_t* l_table, int32_t d, float* out, void* stream);

/* The same scores for config 5's layout: pairs p < n_half and p + n_half (a positive and its
 * negative, optimizer.py:37-57 — the negative replaces the row) share the column and the
 * relation, so col_idx / rel_idx are read for the first half only (row_idx, out hold 2*n_half
 * entries).  The shared side is contracted once: T = G·bf16(l_k ∘ v) on the bf16 MFMA (fp32
 * accumulation), then out[p] = sum_i u_p[i] l_k[i] T[i] and out[p + n_half] = sum_i u_n[i] l_k[i] T[i]
 * in fp32 — half the MFMA work of scoring the two pairs apart.  The bf16 operand rounding sits
 * on l_k∘v instead of u∘l_k, so the scores agree with dg_decoder_score_bf16 to bf16 operand
 * rounding.  G must be 16-byte aligned.  n_row_table / n_col_table: the tables' row counts
 * (every index must be below them); tables whose byte offsets exceed 31 bits take the 64-bit
 * addressed kernel (ABI 34). */
int dg_decoder_score_bf16_paired(const uint16_t* row_table, int64_t ld_row, int64_t n_row_table,
                                 const uint16_t* col_table, int64_t ld_col, int64_t n_col_table,
                                 const int32_t* row_idx, const int32_t* col_idx,
                                 const int32_t* rel_idx, int32_t n_half, const uint16_t* G,
                                 const uint16_t* l_table, int32_t d, float* out, void* stream);

/* Config 5's whole step in one launch: every relation slot's positive batch, its sampled
 * negatives and the hinge loss.  For local slot s < n_slots (relation slot0 + s) and i < batch,
 * p = s*batch + i:
 *     neg_rows[p]            = draw slot0*batch + p of slot (slot0+s)'s alias table
 *                              (alias_table + (slot0+s)*alias_stride entries; stride 0: one
 *                              shared table) — exactly dg_unigram_sample_slots' draws;
 *     out[p]                 = score(pos_rows[p], pos_cols[p]),
 *     out[n_slots*batch + p] = score(neg_rows[p], pos_cols[p])     (dg_decoder_score_bf16_paired,
 *                              D_k = l_table[slot0 + s]);
 *     loss[0]                = sum_p relu(out[nh + p] - (out[p] - margin))   (per-workgroup sums
 *                              in a fixed order, added in block order: deterministic).
 * workspace: DG_HINGE_WS_BYTES bytes, 16-byte aligned, first word zero before the first call
 * (left zero).  d == 256; G, tables and l_table 16-byte aligned.  Replaces optimizer.py:38-47
 * (fixed_unigram_candidate_sampler over the relation's degrees), :51-57 / :63-85 (batch_predict,
 * G = R, L = D_k: model.py:130-134) and :116-120 (_hinge_loss).  n_row_table / n_col_table:
 * the tables' row counts (range <= n_row_table), as for dg_decoder_score_bf16_paired.
 * The scores are dg_decoder_score_bf16_paired's bit for bit when batch % 32 == 0 and both tables
 * lie within 31-bit byte offsets (both calls run the 16x16x32 kernel), or when a table exceeds
 * them (both run the 64-bit addressed 32x32x16 kernel).  With batch % 32 != 0 on small tables this
 * call runs the 32x32x16 kernel (tiles may straddle slots; the last may be ragged) and the paired
 * call the 16x16x32 one: the same bf16 operands, another fp32 accumulation order — equal where
 * the sums are exact, else within fp32 accumulation rounding (tests/test_gpu_bf16_paths.py). */
int dg_slot_score_hinge_bf16(const uint16_t* row_table, int64_t ld_row, int64_t n_row_table,
                             const uint16_t* col_table, int64_t ld_col, int64_t n_col_table,
                             const int32_t* pos_rows, const int32_t* pos_cols,
                             const uint32_t* alias_table, int32_t range, int64_t alias_stride,
                             int32_t slot0, int32_t n_slots, int32_t batch, uint64_t seed,
                             const uint16_t* G, const uint16_t* l_table, int32_t d, float margin,
                             float* out, int32_t* neg_rows, float* loss, void* workspace, void* stream);

/* Fused decoder step (T8 + T9 + T11 + T12 in one launch):
 *   neg_row[b] = neg_rows[b] if neg_rows != NULL, else draw (offset + b) of the alias
 *                sampler — the same draws as dg_unigram_sample — written to neg_rows_out[b]
 *                if non-NULL;
 *   pos[b] = score(rows[b], cols[b]);  neg[b] = score(neg_row[b], cols[b])   (as above)
 *   loss[0] = sum_b relu(neg[b] - (pos[b] - margin))   (fixed block order)
 * workspace: device, 16-byte aligned, 16 + 4*ceil(n/32) bytes, all zero before the first
 * call (the kernel leaves it so).  n >= 1.  The partial sums of the 32-pair blocks meet in one
 * returning 64-bit integer atomic per block (fixed point, each partial rounded to the nearest
 * 2^-32: the loss is within 255·2^-33 ≈ 3e-8 absolute of the sum of the fp32 partials; integer
 * adds are order-free, so bitwise reproducible) when there are at most 255 blocks, else
 * through a ticket and block-order reads (the fp32 partials in block order).
 * Replaces optimizer.py:37-57 (sampler, gathers, pos/neg scores) + :116-120 (hinge). */
int dg_decoder_hinge_f32(const float* row_table, int64_t ld_row, const float* col_table,
                         int64_t ld_col, const int32_t* rows, const int32_t* cols,
                         const int32_t* neg_rows, const uint32_t* alias_table, int32_t range,
                         uint64_t seed, uint64_t offset, int32_t n, const float* G,
                         const float* l, int32_t d, float margin, float* pos, float* neg,
                         int32_t* neg_rows_out, float* loss, void* workspace, void* stream);

/* dg_decoder_hinge_f32 over row operands (d = 32): Q[r] = l ∘ ((row_table[r] ∘ l)·G), [.., ld_q],
 * as dg_gcn_fused_tab_dec_f32 stores them, takes the place of row_table, G and l, and
 * score(r, c) = Q[r]·col_table[c].  Draws, outputs, the loss' hand-off and its reproducibility
 * are dg_decoder_hinge_f32's, over blocks of DG_DEC_ROWS_PAIRS pairs: workspace is 16-byte
 * aligned, 16 + 4*ceil(n/8) bytes, all zero before the first call.  Q and col_table are 16-byte
 * aligned, ld_q and ld_col multiples of 4 (DG_EALIGN otherwise); d must be 32, n >= 1.  The scores
 * are those of G and l at the time Q was made. */
#ifndef DG_DEC_ROWS_PAIRS
#define DG_DEC_ROWS_PAIRS 16
#endif
int dg_decoder_hinge_rows_f32(const float* Q, int64_t ld_q, const float* col_table, int64_t ld_col,
                              const int32_t* rows, const int32_t* cols, const int32_t* neg_rows,
                              const uint32_t* alias_table, int32_t range, uint64_t seed, uint64_t offset,
                              int32_t n, int32_t d, float margin, float* pos, float* neg,
                              int32_t* neg_rows_out, float* loss, void* workspace, void* stream);

/* Hinge loss (T12):  loss[0] = sum_p relu(neg[p] - pos[p] + margin).
 * Replaces DecagonOptimizer._hinge_loss  optimizer.py:116-120.  Single workgroup,
 * fixed summation order. */
int dg_hinge_loss_f32(const float* pos, const float* neg, int32_t n, float margin,
                      float* loss, void* stream);

/* The same hinge sum over many pairs (config 5: every slot's batch, 10^6 pairs) on up to
 * DG_HINGE_WS_BLOCKS workgroups, partials added in block order (deterministic for a given n).
 * workspace: device, 16-byte aligned, DG_HINGE_WS_BYTES bytes, its first word zero before the
 * first call (the kernel leaves it zero again).  optimizer.py:116-120. */
#define DG_HINGE_WS_BLOCKS 256
#define DG_HINGE_WS_BYTES (16 + 4 * DG_HINGE_WS_BLOCKS)
int dg_hinge_loss_ws_f32(const float* pos, const float* neg, int32_t n, float margin, float* loss,
                         void* workspace, void* stream);

/* Cross-entropy loss:  loss[0] = sum_p softplus(-pos[p]) + w * sum_p softplus(neg[p])
 * (sigmoid_cross_entropy_with_logits with labels 1 / 0).  optimizer.py:122-127. */
int dg_xent_loss_f32(const float* pos, const float* neg, int32_t n, float neg_weight,
                     float* loss, void* stream);

/* The same cross-entropy sum over many pairs (an all-relation step: 10^6 pairs) on up to
 * DG_HINGE_WS_BLOCKS workgroups, with dg_hinge_loss_ws_f32's workspace contract (the same
 * DG_HINGE_WS_BYTES buffer serves both: first word zero before the first call, zero again after
 * every call) and its order: block b sums its contiguous chunk, the partials are added in block
 * order (deterministic for a given n).  One fp32 term per pair,
 *     max(x,0) - x + log1p(exp(-|x|))  at x = pos[p]   plus   w * (max(y,0) + log1p(exp(-|y|)))  at y = neg[p]
 * with log1p(e) formed in single precision as log(1 + e) plus the first-order correction for the
 * rounding of 1 + e.  Finite for every finite score.  optimizer.py:122-127. */
int dg_xent_loss_ws_f32(const float* pos, const float* neg, int32_t n, float neg_weight, float* loss,
                        void* workspace, void* stream);

/* --------------------------------------------------------------------------------------
 * Training step (backward of the hinge cost + TF Adam), optimizer.py:108-114.
 * -------------------------------------------------------------------------------------- */
/* Decoder gradient for the n positive pairs (rows[p], cols[p]) and negatives (neg_rows[p],
 * cols[p]) whose scores pos / neg the forward produced (dg_decoder_hinge_f32): with
 * a_p = [neg[p] - (pos[p] - margin) > 0] and M = L·G·L (L = diag(l), NULL = I),
 *     grad_rows[p] = -a_p·M·v_p,  grad_rows[n + p] = a_p·M·v_p,  grad_cols[p] = a_p·Mᵀ·(un_p - u_p)
 *     dM = Σ_p a_p·(un_p - u_p)·v_pᵀ;   dG = L·dM·L   (if dG != NULL)
 *     dl[a] = Σ_b dM[a][b]G[a][b]l[b] + Σ_c dM[c][a]G[c][a]l[c]   (if dl != NULL; needs l)
 *     dG_diag[a] = dG[a][a]                                      (if dG_diag != NULL)
 * grad_rows is [2n][d], grad_cols [n][d] (dense rows; dg_scatter_rows_f32 adds them into the
 * embedding gradients).  workspace: 16-byte aligned, dg_decoder_grad_workspace(n, d) bytes.
 * d % 32 == 0, d <= 256.  Replaces the gradient of optimizer.py:51-57, :63-85, :116-120. */
int64_t dg_decoder_grad_workspace(int32_t n, int32_t d);
int dg_decoder_grad_f32(const float* row_table, int64_t ld_row, const float* col_table,
                        int64_t ld_col, const int32_t* rows, const int32_t* cols,
                        const int32_t* neg_rows, int32_t n, const float* pos, const float* neg,
                        const float* G, const float* l, int32_t d, float margin,
                        float* grad_rows, float* grad_cols, float* dG, float* dl, float* dG_diag,
                        void* workspace, int64_t workspace_bytes, void* stream);

/* The same backward for the sigmoid cross-entropy cost (optimizer.py:122-127)
 *     cost = Σ_p softplus(-pos[p]) + w·Σ_p softplus(neg[p]),   w = neg_weight
 * whose gradient w.r.t. pos[p] is -a_p and w.r.t. neg[p] +b_p with a_p = σ(-pos[p]),
 * b_p = w·σ(neg[p]) (σ(-pos) computed directly in fp32, overflow-safe: 1 - σ(pos) would cancel):
 *     grad_rows[p] = -a_p·M·v_p,  grad_rows[n + p] = +b_p·M·v_p,  grad_cols[p] = Mᵀ·(b_p·un_p - a_p·u_p)
 *     dM = Σ_p (b_p·un_p - a_p·u_p)·v_pᵀ;   dG, dl, dG_diag from dM as above.
 * The hinge is the special case a_p = b_p = [neg[p] - (pos[p] - margin) > 0].  Arguments, outputs,
 * workspace and limits are dg_decoder_grad_f32's, with neg_weight in place of margin. */
int dg_decoder_grad_xent_f32(const float* row_table, int64_t ld_row, const float* col_table,
                             int64_t ld_col, const int32_t* rows, const int32_t* cols,
                             const int32_t* neg_rows, int32_t n, const float* pos, const float* neg,
                             const float* G, const float* l, int32_t d, float neg_weight,
                             float* grad_rows, float* grad_cols, float* dG, float* dl, float* dG_diag,
                             void* workspace, int64_t workspace_bytes, void* stream);

/* out[idx[q]][:] += Σ_{q' : idx[q'] = idx[q]} src[q'][:]  (occurrences summed in q' order,
 * each distinct row written once).  The gradient of tf.gather (optimizer.py:66-76).
 * d <= 256; indices outside [0, n_out_rows) update nothing (device-side guard: the
 * indices may be sampled on the device, where the host cannot check them). */
int dg_scatter_rows_f32(const int32_t* idx, int32_t n, const float* src, int32_t d, float* out,
                        int64_t ld_out, int32_t n_out_rows, void* stream);

/* Backward of y_g = l2_normalize(s_g) for every group g of one node type (layers.py:93,
 * :117; model.py:75): dy' = dy ∘ [mask > 0] (mask = the relu output, or NULL), then
 *     ds_g = dy'·inv − s_g·inv³·(s_g·dy')·[Σs_g² >= 1e-12],   inv = rsqrt(max(Σs_g², 1e-12))
 * (tf.maximum passes its gradient to Σs² where Σs² >= ε).  All rows [n_rows][d], 16-byte
 * aligned; d % 4 == 0, d <= 256. */
typedef struct dg_l2g_group {
    const float* s;             /* [n_rows][d] the pre-normalisation sum (forward) */
    float* ds;                  /* [n_rows][d] its gradient (output) */
} dg_l2g_group;

int dg_l2norm_grad_f32(const dg_l2g_group* groups /* HOST array */, int32_t n_groups,
                       const float* dy, const float* mask, int32_t n_rows, int32_t d,
                       void* stream);

/* TF 1.8 ApplyAdam (use_nesterov = false) on up to DG_MAX_ADAM_SEGS segments in one launch:
 *     m += (g − m)(1 − β1);  v += (g² − v)(1 − β2);  param −= alpha·m / (sqrt(v) + ε)
 * alpha = lr·sqrt(1 − β2^t)/(1 − β1^t): read from state[2] when `state` (device, float[3] =
 * {β1^t, β2^t, alpha}) is non-NULL — graph-capturable, advanced on the device by
 * dg_adam_advance after the update, as TF's _finish advances its beta-power variables —
 * else the `alpha` argument.  grad NULL = a zero gradient (TF updates every variable each
 * step).  16-byte aligned.  Initial state: {β1, β2, lr·sqrt(1 − β2)/(1 − β1)}. */
#define DG_MAX_ADAM_SEGS 32

typedef struct dg_adam_seg {
    float* param;
    const float* grad;          /* or NULL */
    float* m;
    float* v;
    int64_t n;
} dg_adam_seg;

int dg_adam_f32(const dg_adam_seg* segs /* HOST array */, int32_t n_segs, float alpha, float beta1,
                float beta2, float eps, const float* state, void* stream);
int dg_adam_advance(float* state, float lr, float beta1, float beta2, void* stream);

/* --------------------------------------------------------------------------------------
 * Dropout (training path): dropout_sparse (layers.py:23-31, :88) and tf.nn.dropout (:112).
 * state: device uint64 {seed, step}.  Element idx of stream `tag` is kept iff
 *   lowbias32(key ^ idx) >> 8 < (uint32)(keep·2^24),
 *   key = lowbias32(lowbias32(seed_lo ^ tag·0x9E3779B9) ^ (seed_hi + step·0x85EBCA6B)),
 *   lowbias32(x): x ^= x>>16; x *= 0x7feb352d; x ^= x>>15; x *= 0x846ca68b; x ^= x>>16,
 * and a kept element is scaled by 1/keep (TF's distribution; its RNG stream is not
 * reproducible).  dg_dropout_advance increments step (a new draw per training step, on the
 * device: graph-capturable).
 * -------------------------------------------------------------------------------------- */
/* out[r][:] = in[r][:] · s(r)  (row masks: identity features' dropout_sparse, one relation's
 * rows at a time in the relation-stacked W1; in place allowed).  n_rows·d < 2^32. */
int dg_dropout_rows_f32(const float* in, float* out, int64_t n_rows, int32_t d, const uint64_t* state,
                        uint32_t tag, float keep, void* stream);
/* out[k][r][f] = src[r][f] · s(k·n_rows·d + r·d + f)  for k < K: tf.nn.dropout of H_j drawn
 * independently for each of the K relations.  K·n_rows·d < 2^32. */
int dg_dropout_elems_f32(const float* src, float* out, int32_t K, int32_t n_rows, int32_t d,
                         const uint64_t* state, uint32_t tag, float keep, void* stream);
/* Relation-mapped forms for a rank's relation shard (sharding.py): local slab b is global
 * relation rel_map[b] and draws THAT relation's mask bits (the bits the unmapped forms draw
 * for it).  Rows: slab b is rows_per_slab rows; flags bit 1 / bit 2 address `in` / `out` at
 * slab rel_map[b] (else b).  Elems: out[b] = src ∘ M_{rel_map[b]} (out local, contiguous). */
int dg_dropout_rows_map_f32(const float* in, float* out, const int32_t* rel_map, int32_t n_map,
                            int64_t rows_per_slab, int32_t d, int32_t flags, const uint64_t* state,
                            uint32_t tag, float keep, void* stream);
int dg_dropout_elems_map_f32(const float* src, float* out, const int32_t* rel_map, int32_t K,
                             int32_t n_rows, int32_t d, const uint64_t* state, uint32_t tag, float keep,
                             void* stream);
int dg_dropout_advance(uint64_t* state, void* stream);

/* --------------------------------------------------------------------------------------
 * Evaluation: AUROC, AUPRC and AP@k of n_pos positive vs n_neg negative edge
 * scores, exactly as roc_auc_score (ties count ½), average_precision_score and
 * rank_metrics.apk(actual = positives, predicted = all sorted by score, stable, descending)
 * compute them in get_accuracy_scores (main.py:38-80): out[0..2] = {auroc, auprc, apk}
 * (double).  Integer pair counts per positive, no sort; workspace 16-byte aligned,
 * dg_rank_metrics_workspace(n_pos) bytes.
 * -------------------------------------------------------------------------------------- */
int64_t dg_rank_metrics_workspace(int32_t n_pos);
int dg_rank_metrics_f32(const float* pos, int32_t n_pos, const float* neg, int32_t n_neg, int32_t k,
                        double* out, void* workspace, int64_t workspace_bytes, void* stream);

/* The same metrics of the scores the reference actually ranks: mode DG_RANK_SIGMOID64 =
 * main.py:51-52,60,70,81 under numpy 1.14 (requirements.txt:14) — float32 exp of TF's float32
 * logit (correctly rounded, as glibc expf), float64 `1. / (1 + e)`, np.nan_to_num — so logits
 * above ≈36.7 / below ≈-88.7 tie at 1.0 / 0.0; DG_RANK_SIGMOID32 = MathUtils.sigmoid on the
 * float32 decoder output (DecagonAccuracyEvaluator.py:123, all float32); DG_RANK_LOGIT = the
 * logits (as dg_rank_metrics_f32).  pos / neg are the LOGITS.  Workspace 16-byte aligned,
 * dg_rank_metrics_ex_workspace(n_pos, n_neg) bytes. */
#define DG_RANK_LOGIT 0
#define DG_RANK_SIGMOID64 1
#define DG_RANK_SIGMOID32 2
int64_t dg_rank_metrics_ex_workspace(int32_t n_pos, int32_t n_neg);
int dg_rank_metrics_ex_f32(const float* pos, int32_t n_pos, const float* neg, int32_t n_neg, int32_t k,
                           int32_t mode, double* out, void* workspace, int64_t workspace_bytes, void* stream);

/* --------------------------------------------------------------------------------------
 * Per-relation operands: what (G, g_stride, l, l_stride, n_rel) and a relation map mean to the
 * entry points that take every relation of one edge type in one pass (dg_decoder_topk_f32,
 * dg_decoder_score_seg_f32, dg_decoder_score_cross_f32, dg_decoder_grad_seg_f32).
 *   G_k = G + k*g_stride, row-major d x d: g_stride 0 (one G shared by every relation: DEDICOM's
 *         R) or d*d (per relation: Bilinear);
 *   l_k = l + k*l_stride: l_stride 0 (shared) or d (per relation); l NULL = identity, and then
 *         l_stride is ignored.  Any other stride is DG_EINVAL.
 * A SLOT of a call (a segment, a selected column, a relation of the grid) is relation k = map[s]
 * (the call's seg_rel / rel_idx, device int32, never read on the host), or k = s where the map is
 * NULL or the call has none.  With a map, n_rel >= 1 bounds its values: a slot whose relation lies
 * outside [0, n_rel) reads no operand and scores NaN (the backward skips it).  Without a map every
 * slot is in range, and a per-relation operand needs slots <= n_rel (DG_EINVAL otherwise); where
 * no operand is per relation, any relation index serves.
 * -------------------------------------------------------------------------------------- */

/* --------------------------------------------------------------------------------------
 * Top-k candidate ranking (ABI 39): for every relation k < n_rel of one edge type, the `topk`
 * highest-scoring permitted pairs (r, c), r < n_rows, c < n_cols, of
 *
 *     s_k[r, c] = (row_table[r] ∘ l_k)ᵀ · G_k · (l_k ∘ col_table[c])          (fp32, MFMA)
 *
 * without forming any n_rows x n_cols matrix.
 * Replaces: session.run(predictionsTensor) → sigmoid → np.take(candidates) → argsort()[::-1][:n]
 *           main/ActiveLearner/GreedyActiveLearner.py:66-96; the E·D·R·D·Eᵀ matrix of
 *           main/Predictor/NpPredictor.py:293-313.
 *
 * Operands: row_table / col_table: row r at table + r*ld (ld >= d, ld % 4 == 0, 16-byte aligned);
 * G_k, l_k: "Per-relation operands" above (no map: the grid's relation k is relation k).
 * d is 32 or 64; 1 <= topk <= DG_TOPK_MAX_K; n_rows * n_cols < 2^32.
 *
 * Permitted: (r, c) is not in relation k's exclusion set; with DG_TOPK_UPPER only r < c (needs
 * n_rows == n_cols); with DG_TOPK_NO_DIAG not r == c.  The exclusion sets are a relation-stacked
 * CSR (as StackedCSR, without values): relation k's row r excludes the columns
 * excl_col[excl_rowptr[k*n_rows + r] .. excl_rowptr[k*n_rows + r + 1]), which MUST be ascending
 * and unique within the row (the kernel walks them once beside its column tiles; unsorted
 * columns give a wrong selection, never an out-of-range access).  Rows may be empty, a relation
 * may exclude everything; excl_rowptr == excl_col == NULL excludes nothing (one of them NULL
 * alone is an error).
 *
 * Ordering (total, so the result is unique and independent of tiling, grid and scheduling):
 * higher fp32 score first; equal scores by smaller linear index r*n_cols + c first; −0 compares
 * (and is returned) as +0.  Non-finite scores are ordered by their bit pattern (sign-magnitude
 * order of the float's bits: +NaN above +inf, −NaN below −inf) with no further promise.
 *
 * Outputs: out_score float [n_rel x topk], out_row / out_col int32 [n_rel x topk], descending in
 * that ordering; out_count int32 [n_rel] = min(topk, permitted pairs); slots past out_count[k]
 * hold −inf and −1.  Workspace: dg_decoder_topk_workspace(n_rel, n_rows, n_cols, topk) bytes
 * (0 for arguments out of range), 16-byte aligned: topk 8-byte keys per 32 rows and relation —
 * it grows with n_rows, never with n_rows * n_cols.
 * -------------------------------------------------------------------------------------- */
#define DG_TOPK_MAX_K 1024
#define DG_TOPK_UPPER 1
#define DG_TOPK_NO_DIAG 2
int64_t dg_decoder_topk_workspace(int32_t n_rel, int32_t n_rows, int32_t n_cols, int32_t topk);
int dg_decoder_topk_f32(const float* row_table, int64_t ld_row, int32_t n_rows, const float* col_table,
                        int64_t ld_col, int32_t n_cols, const float* G, int64_t g_stride, const float* l,
                        int64_t l_stride, int32_t n_rel, int32_t d, int32_t topk,
                        const int32_t* excl_rowptr, const int32_t* excl_col, int32_t flags,
                        float* out_score, int32_t* out_row, int32_t* out_col, int32_t* out_count,
                        void* workspace, int64_t workspace_bytes, void* stream);

/* --------------------------------------------------------------------------------------
 * Evaluation of all relations of one edge type in one pass (additive to ABI 39).
 * Replaces the loop of get_accuracy_scores over every relation (main.py:38-80 and its final loop)
 * and DecagonAccuracyEvaluator.evaluateAll (DecagonAccuracyEvaluator.py:57-91), which through
 * dg_decoder_score_f32 + dg_rank_metrics_ex_f32 cost one set of launches and a host round trip
 * per relation.
 *
 * Both entry points work on SEGMENTS of packed device arrays: segment s is elements
 * [ptr[s], ptr[s+1]) with ptr int32 [n_seg + 1] ON THE DEVICE, ascending, ptr[0] = 0 and
 * ptr[n_seg] = the total.  Neither reads ptr on the host: the calls are asynchronous and can be
 * captured in a graph.  Segments may be empty.
 *
 * dg_decoder_score_seg_f32: for pair p of segment s with k = seg_rel[s] (seg_rel NULL: k = s),
 *
 *     out[p] = (row_table[row_idx[p]] ∘ l_k)ᵀ · G_k · (l_k ∘ col_table[col_idx[p]])
 *
 * with G_k, l_k, n_rel as "Per-relation operands" above (the slots are the segments) and d as
 * dg_decoder_score_f32 (d % 32 == 0, d <= 256).  n_pairs + 32*n_seg < 2^31.  One wave scores one 32-pair tile of one segment
 * with the tile routine of dg_decoder_score_f32, so a segment's scores equal that entry point's
 * on the segment's pairs with G_k, l_k bit for bit.  A pair whose index lies outside
 * [0, n_rows) x [0, n_cols), and every pair of a segment whose relation lies outside [0, n_rel),
 * scores NaN (nothing out of range is read).
 *
 * dg_rank_metrics_seg_f32: out[s][0..2] = {AUROC, AUPRC, AP@k} (double) of segment s's positive
 * logits pos[pos_ptr[s] .. pos_ptr[s+1]) against its negative logits neg[neg_ptr[s] ..
 * neg_ptr[s+1]), ranked under `mode` (DG_RANK_*) — bit for bit what dg_rank_metrics_ex_f32 returns
 * for that segment alone, including its conventions for an empty class (no positives: NaN, NaN,
 * 0.0; no negatives: AUROC NaN).  Workspace 16-byte aligned, dg_rank_metrics_seg_workspace(...)
 * bytes (linear in the totals; 0 for negative arguments).
 * n_pos_total + n_neg_total + 256*n_seg < 2^31.
 *
 * dg_seg_tile_lookup (HOST arrays; no device): the map both launches use to deal tiles of `tile`
 * elements to segments without a prefix sum — segment s owns the virtual tiles starting at
 * seg_ptr[s]/tile + s, the grid is seg_ptr[n_seg]/tile + n_seg.  For virtual tile vt it stores
 * the segment and the tile's index inside it and returns 1, or 0 when that slot lies past the
 * segment's end (the wave exits); DG_EINVAL for vt outside the grid or bad arguments.
 * -------------------------------------------------------------------------------------- */
int dg_decoder_score_seg_f32(const float* row_table, int64_t ld_row, int32_t n_rows, const float* col_table,
                             int64_t ld_col, int32_t n_cols, const int32_t* row_idx, const int32_t* col_idx,
                             const int32_t* seg_ptr, const int32_t* seg_rel, int32_t n_seg, int32_t n_pairs,
                             const float* G, int64_t g_stride, const float* l, int64_t l_stride, int32_t n_rel,
                             int32_t d, float* out, void* stream);
int64_t dg_rank_metrics_seg_workspace(int32_t n_pos_total, int32_t n_neg_total, int32_t n_seg);
int dg_rank_metrics_seg_f32(const float* pos, const int32_t* pos_ptr, int32_t n_pos_total, const float* neg,
                            const int32_t* neg_ptr, int32_t n_neg_total, int32_t n_seg, int32_t k, int32_t mode,
                            double* out, void* workspace, int64_t workspace_bytes, void* stream);
int32_t dg_seg_tile_lookup(const int32_t* seg_ptr, int32_t n_seg, int32_t tile, int32_t vt, int32_t* /* HOST out */ seg,
                           int32_t* /* HOST out */ local);

/* --------------------------------------------------------------------------------------
 * The profile of node pairs: every relation of one edge type scored for given pairs, and the
 * best relations of every pair (additive to ABI 39).
 * Replaces NpPredictor(relationId)._predictEdges (main/Predictor/NpPredictor.py:293-313: the
 * E·D·R·D·Eᵀ matrix of ONE relation, then the wanted entries) looped over relations, and the
 * per-relation session.run(predictions) of DecagonAccuracyEvaluator._computePredictions.
 *
 * dg_decoder_score_cross_f32: for pair p < n_pairs and slot s < n_sel with k = rel_idx[s]
 * (rel_idx device int32 [n_sel]; NULL: k = s),
 *
 *     out[p*ld_out + s] = (row_table[row_idx[p]] ∘ l_k)ᵀ · G_k · (l_k ∘ col_table[col_idx[p]])
 *
 * with G_k, l_k, n_rel as "Per-relation operands" above (the slots are the n_sel columns) and d
 * 32 or 64.  rel_idx may repeat relations, in any order.  ld_out >= n_sel; columns
 * [n_sel, ld_out) of a row are not written.  Every out[p, s] equals, bit for bit, what
 * dg_decoder_score_f32 returns for that pair with G_k, l_k, whatever the pair's place in the
 * call.  A pair whose index lies outside [0, n_rows) x [0, n_cols) gets a whole row of NaN, a
 * slot whose relation lies outside [0, n_rel) a whole column of NaN; nothing out of range is
 * read.  Asynchronous on `stream`; allocates nothing and reads nothing on the host (graph
 * capture).  n_pairs == 0 succeeds without a launch.
 * Rejected on the host, before any HIP call: DG_EINVAL for a NULL table, G, or (n_pairs > 0)
 * index or out; n_sel < 1, n_rel < 1, n_pairs < 0, empty tables; d not 32 or 64; ld_row or
 * ld_col < d; ld_out < n_sel; a stride other than the two allowed; rel_idx NULL with a
 * per-relation operand and n_sel > n_rel; n_pairs * ld_out >= DG_CROSS_MAX_OUT (2^38 elements:
 * it keeps the grid of ⌈n_pairs/32⌉·⌈n_sel/C⌉ waves 32-bit; the offsets into out are 64-bit) or
 * n_pairs > 2^31 − 65 (32-bit pair offsets).
 * DG_EALIGN for row_table or col_table not 16-byte aligned or ld_row / ld_col not a multiple of
 * 4 (the rules of dg_decoder_topk_f32; G and l need no alignment).
 *
 * dg_decoder_score_cross_chunk: the slot chunk C that call uses for (n_pairs, n_sel) — one wave
 * scores one 32-pair tile against C consecutive slots; C is 32, halved down to 4 while the grid
 * would leave SIMDs idle (0 for n_pairs < 0 or n_sel < 1).  Host only; for tests and tools.
 *
 * dg_row_topk_f32: for every row r < n_rows of x (row r at x + r*ld, ld >= n_cols) the `topk`
 * highest entries among columns [0, n_cols), descending, in the total order of
 * dg_decoder_topk_f32 with the column as the index: higher fp32 value first, equal values by
 * smaller column, −0 compares and is returned as +0, non-finite values by bit pattern with no
 * further promise.  out_val float / out_idx int32 [n_rows x topk], out_count int32 [n_rows] =
 * min(topk, n_cols); slots past the count hold −inf / −1.  1 <= topk <= DG_TOPK_MAX_K,
 * 1 <= n_cols < 2^31.  One wave per row keeps the list in LDS: no workspace is needed —
 * dg_row_topk_workspace returns 0 and a NULL workspace is accepted.  Asynchronous; n_rows == 0
 * succeeds without a launch.
 *
 * dg_row_topk_excl_f32: dg_row_topk_f32 over the columns of row r that are NOT named by
 * excl_slot[excl_ptr[r] : excl_ptr[r+1]] — a pair's known relations, which the reference drops on
 * the host after NpPredictor._predictEdges per relation id.  excl_ptr is device int32
 * [n_rows + 1], excl_slot device int32 [excl_nnz], each row's entries ascending and unique.
 * Order, −0 handling and −inf / −1 past the count are those of dg_row_topk_f32; out_count[r] is
 * the number of slots written, min(topk, permitted columns of row r), 0 when every column is
 * excluded.  One wave per row merges the list into its single pass over the row (the list is read
 * once, coalesced; the running top-k stays in LDS): no workspace.  A row's range is clamped to
 * [0, excl_nnz) and a non-increasing excl_ptr pair is an empty list; an entry outside
 * [0, n_cols) excludes nothing; an unsorted list leaves unspecified which of its entries apply;
 * no input makes the kernel read or write out of range.  Both pointers NULL (or excl_nnz == 0)
 * mean no exclusion, the bytes of dg_row_topk_f32; exactly one NULL, or excl_nnz < 0, is
 * DG_EINVAL (the rule of dg_decoder_topk_f32), as is everything dg_row_topk_f32 rejects.
 * Asynchronous, allocates nothing, reads nothing on the host (graph capture).
 * -------------------------------------------------------------------------------------- */
#define DG_CROSS_MAX_OUT (1ll << 38)
int dg_decoder_score_cross_f32(const float* row_table, int64_t ld_row, int32_t n_rows,
                               const float* col_table, int64_t ld_col, int32_t n_cols,
                               const int32_t* row_idx, const int32_t* col_idx, int32_t n_pairs,
                               const float* G, int64_t g_stride, const float* l, int64_t l_stride,
                               const int32_t* rel_idx, int32_t n_sel, int32_t n_rel, int32_t d,
                               float* out, int64_t ld_out, void* stream);
int32_t dg_decoder_score_cross_chunk(int32_t n_pairs, int32_t n_sel);
int64_t dg_row_topk_workspace(int32_t n_rows, int32_t n_cols, int32_t topk);
int dg_row_topk_f32(const float* x, int64_t ld, int32_t n_rows, int32_t n_cols, int32_t topk,
                    float* out_val, int32_t* out_idx, int32_t* out_count, void* workspace,
                    int64_t workspace_bytes, void* stream);
int dg_row_topk_excl_f32(const float* x, int64_t ld, int32_t n_rows, int32_t n_cols, int32_t topk,
                         const int32_t* excl_ptr, const int32_t* excl_slot, int32_t excl_nnz,
                         float* out_val, int32_t* out_idx, int32_t* out_count, void* stream);

/* --------------------------------------------------------------------------------------
 * The decoder backward of the hinge cost for every relation's batch of one edge type in one pass
 * (additive to ABI 39).
 * Replaces one tf.train.AdamOptimizer.minimize step per (relation, batch) (optimizer.py:108-114,
 * minibatch.py:278-313) where only the decoder's gradient depends on the relation: the gradient
 * of the summed cost Σ_k cost_k is the sum of the gradients, so one GCN backward and one Adam
 * update serve a batch of every relation.
 *
 * dg_decoder_grad_seg_f32: dg_decoder_grad_f32 over packed SEGMENTS with the conventions of
 * dg_decoder_score_seg_f32: segment s is pairs [seg_ptr[s], seg_ptr[s+1]) (seg_ptr int32
 * [n_seg + 1] on the device, never read on the host; segments may be empty) and belongs to
 * relation k = seg_rel[s] (seg_rel NULL: k = s), with G_k, l_k, n_rel as "Per-relation operands"
 * above.  The relations in
 * seg_rel must be DISTINCT (two segments of one relation would both write its outputs).
 * d is 32 or 64 (the per-segment dM buffer is n_seg*d*d floats).  With M_k = L_k·G_k·L_k, u / un
 * / v the rows row_table[rows[p]] / row_table[neg_rows[p]] / col_table[cols[p]], and
 * a_p = [neg[p] − (pos[p] − margin) > 0]:
 *
 *     mv[p]        = a_p · M_k·v_p                  float [n_pairs x d]
 *     grad_cols[p] = a_p · M_kᵀ·(un_p − u_p)        float [n_pairs x d]
 *     dM_s         = Σ_{p in s} a_p·(un_p − u_p)·v_pᵀ, pairs in order (workspace)
 *
 * mv is stored ONCE per pair: the gradient of the positive row u_p is −mv[p] and that of the
 * negative row un_p is +mv[p]; the row reduction (dg_segment_rows_sum_f32) applies the signs.
 * A pair with an index outside [0, n_rows) x [0, n_cols), and every pair of a segment whose
 * relation lies outside [0, n_rel), gets zero rows and contributes nothing to dM (nothing out of
 * range is read).  Rows of pairs outside every segment are not written.
 * From dM a second, small launch writes the variables' gradients, each optional (NULL skips it):
 *     dG       g_stride == 0: float [d x d] = Σ_s L_k·dM_s·L_k (DEDICOM's R), in a fixed order: the
 *              segment list in 16 contiguous slices, each added in segment order, then the slices'
 *              sums in slice order (one more launch);
 *              g_stride != 0: dG[k] = L_k·dM_s·L_k, float [n_rel x d x d] (Bilinear)
 *     dG_diag  dG_diag[k][a] = (L_k·dM_s·L_k)[a][a], float [n_rel x d]; needs g_stride != 0 (DistMult)
 *     dl       dl[k][a] = Σ_b dM_s[a][b]·G_k[a][b]·l_k[b] + Σ_c dM_s[c][a]·G_k[c][a]·l_k[c],
 *              float [n_rel x d]; needs l with l_stride == d (DEDICOM's D_k)
 * Per-relation outputs of relations absent from seg_rel are left untouched (the caller zeroes
 * the buffers); an empty segment's relation gets zeros.  Workspace: 16-byte aligned,
 * dg_decoder_grad_seg_workspace(n_seg, d) bytes (0 for bad arguments), needed only when a
 * variable output is requested.  Asynchronous; n_pairs == 0 succeeds without a launch.
 * Rejected on the host before any HIP call: DG_EINVAL for d not 32 or 64, n_seg < 1, n_pairs < 0,
 * a NULL table, seg_ptr or G, (n_pairs > 0) a NULL index, score or gradient array, empty tables,
 * ld_row / ld_col < d, a stride other than the two allowed, seg_rel NULL with a per-relation
 * operand and n_seg > n_rel, dl without a per-relation l, dG_diag with g_stride == 0, a missing or
 * short workspace, n_pairs + 32*n_seg >= 2^31; DG_EALIGN for row_table, col_table, G, l or the
 * workspace not 16-byte aligned, or ld_row / ld_col not a multiple of 4.
 *
 * dg_decoder_grad_seg_xent_f32: the same pass for the sigmoid cross-entropy cost (see
 * dg_decoder_grad_xent_f32: a_p = σ(-pos[p]), b_p = neg_weight·σ(neg[p])), with neg_weight in place
 * of margin and one more output:
 *     coef       float [2*n_pairs]: coef[p] = -a_p, coef[n_pairs + p] = +b_p
 *     mv[p]      = M_k·v_p, unweighted (one row per pair, as for the hinge; a zero row where both
 *                coefficients are zero): the gradient of the
 *                positive row is coef[p]·mv[p], of the negative row coef[n_pairs + p]·mv[p] — the
 *                weights go through dg_segment_rows_sum_f32's `sign` array
 *     grad_cols[p] = M_kᵀ·(b_p·un_p - a_p·u_p),   dM_s = Σ_p (b_p·un_p - a_p·u_p)·v_pᵀ
 * and dG, dG_diag, dl from dM_s as above.  A pair with an index outside the tables, and every pair
 * of a segment whose relation is out of range, has both coefficients 0, zero rows, and contributes
 * nothing.  Same limits, workspace and error codes; coef NULL with n_pairs > 0 is DG_EINVAL.
 *
 * dg_segment_rows_sum_f32: for every output row r < n_out_rows (row r at out + r*ld_out,
 * ld_out >= d, 1 <= d <= 256)
 *
 *     out[r][:] += Σ_q sign[q] · src[item[q]][:],  q in [node_ptr[r], node_ptr[r+1]) in q order
 *
 * over a node-major occurrence list the caller builds once per batch (a stable sort of the index
 * array): node_ptr int32 [n_out_rows + 1] ascending within [0, n_items], item int32 [n_items]
 * rows of src (float [n_src_rows x d]), sign float [n_items] or NULL (all +1).  Items outside
 * [0, n_src_rows) add nothing.  One workgroup of dg_segment_rows_sum_waves() waves owns a row:
 * the list is cut into chunks of dg_segment_rows_sum_chunk() items, wave w adds chunks w,
 * w + waves, ... in order, and the waves' sums are combined in a fixed tree — the result does not
 * depend on scheduling, and a row with thousands of occurrences does not serialise on one wave.
 * It replaces dg_scatter_rows_f32 (which scans the whole index array per pair) where n is large.
 * The two helpers are host only, for tests and tools.
 * -------------------------------------------------------------------------------------- */
int64_t dg_decoder_grad_seg_workspace(int32_t n_seg, int32_t d);
int dg_decoder_grad_seg_f32(const float* row_table, int64_t ld_row, int32_t n_rows, const float* col_table,
                            int64_t ld_col, int32_t n_cols, const int32_t* rows, const int32_t* cols,
                            const int32_t* neg_rows, const int32_t* seg_ptr, const int32_t* seg_rel,
                            int32_t n_seg, int32_t n_pairs, const float* pos, const float* neg, float margin,
                            const float* G, int64_t g_stride, const float* l, int64_t l_stride, int32_t n_rel,
                            int32_t d, float* mv, float* grad_cols, float* dG, float* dl, float* dG_diag,
                            void* workspace, int64_t workspace_bytes, void* stream);
int dg_decoder_grad_seg_xent_f32(const float* row_table, int64_t ld_row, int32_t n_rows, const float* col_table,
                                 int64_t ld_col, int32_t n_cols, const int32_t* rows, const int32_t* cols,
                                 const int32_t* neg_rows, const int32_t* seg_ptr, const int32_t* seg_rel,
                                 int32_t n_seg, int32_t n_pairs, const float* pos, const float* neg,
                                 float neg_weight, const float* G, int64_t g_stride, const float* l,
                                 int64_t l_stride, int32_t n_rel, int32_t d, float* mv, float* grad_cols,
                                 float* coef, float* dG, float* dl, float* dG_diag, void* workspace,
                                 int64_t workspace_bytes, void* stream);
int dg_segment_rows_sum_f32(const int32_t* node_ptr, const int32_t* item, const float* sign, int32_t n_items,
                            const float* src, int32_t n_src_rows, int32_t d, float* out, int64_t ld_out,
                            int32_t n_out_rows, void* stream);
int32_t dg_segment_rows_sum_chunk(void);
int32_t dg_segment_rows_sum_waves(void);

/* --------------------------------------------------------------------------------------
 * Unigram negative sampler (T11):  out[i] ~ Categorical(p), p_c ∝ degree_c^0.75, draw
 * (offset + i) of a counter-based hash stream, through a Walker alias table of `range`
 * entries {acceptance probability as float bits, alias index} (uint32 pairs, built once on
 * the host: decagon_amd/sampling.py).
 * Replaces tf.nn.fixed_unigram_candidate_sampler(distortion=0.75, unique=False)
 * optimizer.py:40-47 (distribution only — TF's RNG stream is not reproducible).
 * -------------------------------------------------------------------------------------- */
int dg_unigram_sample(const uint32_t* alias_table, int32_t range, int32_t n, uint64_t seed,
                      uint64_t offset, int32_t* out, void* stream);

/* The same draws with one table per relation slot (optimizer.py:38-47 samples relation k's
 * negatives from ITS degrees, degrees[i][k]): draw i < n is draw slot0*batch + i of the table
 * of slot slot0 + i / batch, at alias_table + (slot0 + i / batch) * alias_stride entries
 * (alias_stride 0: one shared table, = dg_unigram_sample with offset slot0*batch). */
int dg_unigram_sample_slots(const uint32_t* alias_table, int32_t range, int64_t alias_stride,
                            int32_t slot0, int32_t batch, int32_t n, uint64_t seed, int32_t* out,
                            void* stream);

/* --------------------------------------------------------------------------------------
 * One step's batches of every relation of an edge type, from device-resident training edges in
 * the epoch's shuffled order (csrc/epochs.hip, csrc/permute.h; additive to ABI 39).
 * Replaces EdgeMinibatchIterator.shuffle and .next_minibatch_feed_dict's batch slicing
 * (decagon/deep/minibatch.py:278-322).
 *
 * edges: the edge type's training edges, relation-major, interleaved (row, col) int32 pairs
 * [n_edges x 2], 8-byte aligned; edge_ptr int64 [n_rel + 1]: relation k's edges are
 * [edge_ptr[k], edge_ptr[k+1]), n_k of them (< 2^31); seg_rel int32 [n_seg]; wrap_mask: bit
 * (k & 31) of word k >> 5 set when relation k wraps round, or NULL (none does).  For segment s,
 * k = seg_rel[s], nb = n_k / batch (rounded down), tb = t mod nb if k wraps, else t, and c in
 * [0, batch):
 *
 *     (rows, cols)[s*batch + c] = edges[edge_ptr[k] + perm(n_k, key, tb*batch + c)],
 *     key = epoch_key(seed, epoch, first_slot + k)                       (permute.h)
 *
 * A segment without a batch — nb == 0, tb >= nb without wrapping, k outside [0, n_rel), or an
 * edge_ptr entry outside [0, n_edges] — reads no edge: its rows are `bad_row` (pass the row
 * table's length: the segmented kernels skip such pairs) and its columns 0.  Exactly
 * n_seg*batch entries of rows and of cols are written.  Asynchronous; n_seg == 0 succeeds
 * without a launch.  Rejected on the host before any HIP call: DG_EINVAL for a NULL edge_ptr,
 * (n_edges > 0) NULL edges, (n_seg > 0) NULL seg_rel, rows or cols, n_rel < 1, n_edges < 0,
 * batch <= 0, n_seg < 0, t < 0, first_slot < 0, n_seg*batch > 2^31 - 257; DG_EALIGN for
 * edges or edge_ptr not 8-byte aligned, or seg_rel, wrap_mask, rows or cols not 4-byte aligned.
 *
 * dg_epoch_perm_host / dg_epoch_key_host: permute.h's perm (out[i] = perm(n, key, x[i]);
 * DG_EINVAL for n < 1, count < 0, a NULL array or an x[i] outside [0, n)) and epoch_key on the
 * host, for tests of the numpy restatement (decagon_amd/epochs.py).
 * -------------------------------------------------------------------------------------- */
int dg_epoch_batch_i32(const int32_t* edges, int64_t n_edges, const int64_t* edge_ptr, int32_t n_rel,
                       const int32_t* seg_rel, int32_t n_seg, const uint32_t* wrap_mask, int32_t batch,
                       int32_t t, uint32_t epoch, uint64_t seed, int32_t first_slot, int32_t bad_row,
                       int32_t* rows, int32_t* cols, void* stream);
int dg_epoch_perm_host(int32_t n, uint32_t key, const int32_t* x, int32_t* out, int64_t count);
uint32_t dg_epoch_key_host(uint64_t seed, uint32_t epoch, uint32_t slot);

#ifdef __cplusplus
}
#endif

#endif /* DECAGON_HIP_H */

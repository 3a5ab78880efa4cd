/*
 * decagon_hip_ext2.h — entry points of libdecagon_hip.so added after decagon_hip_ext.h.
 *
 * decagon_hip.h is frozen at ABI 39 and decagon_hip_ext.h at the filtered edge rank: existing
 * bindings were generated from them.  What the library gains afterwards is declared here, purely
 * additive: dg_abi_version() stays 39, and a binding of the earlier headers keeps working
 * unchanged.  The conventions of decagon_hip.h hold for every entry point below (device pointers
 * unless marked host, asynchronous launches on `stream`, DG_OK / negative DG_E* / positive
 * hipError_t, IEEE fp32 in a fixed order, no float atomics), the constants and structs of both
 * earlier headers are in scope, and the header is written in the same C subset:
 * decagon_amd/abi.py parses it with the same parser into a table of its own.
 */
#ifndef DECAGON_HIP_EXT2_H
#define DECAGON_HIP_EXT2_H

#include "decagon_hip_ext.h"

#ifdef __cplusplus
extern "C" {
#endif

/* --------------------------------------------------------------------------------------
 * A node's best partners per relation (additive to ABI 39): for query q = row node r of segment
 * s with relation k = seg_rel[s] (seg_rel NULL: k = s), the `topk` best PERMITTED columns c' of
 *
 *     s_k[r, c'] = (row_table[r] ∘ l_k)ᵀ · G_k · (l_k ∘ col_table[c'])          (fp32, MFMA)
 *
 * without forming any n_rows x n_cols matrix, or a chunk of one — "given drug u and side effect
 * k, which drugs are u's likeliest partners outside the known ones?".
 * Replaces: session.run(predictions) of one relation, a dense mask of the known edges and a sort
 *           of each wanted row on the host, once per relation: the E·D·R·D·Eᵀ matrix of
 *           main/Predictor/NpPredictor.py:293-313 (_predictEdges).
 *
 * Operands and queries: as dg_decoder_edge_rank_f32, without col_idx — row_table / col_table (row
 * r at table + r*ld, ld >= d, ld % 4 == 0, 16-byte aligned; G and l need no alignment); d is 32 or
 * 64; G_k, l_k, n_rel: "Per-relation operands" of decagon_hip.h (the slots are the segments);
 * segment s is queries [seg_ptr[s], seg_ptr[s+1]) with seg_ptr int32 [n_seg + 1] ON THE DEVICE,
 * ascending from 0 to n_queries, never read on the host; segments may be empty.
 * n_queries + 32*n_seg < 2^31.
 *
 * Permitted columns of q: c' in [0, n_cols) that is not in relation k's exclusion row of r,
 * excl_col[excl_rowptr[k*n_rows + r] .. excl_rowptr[k*n_rows + r + 1]) — the relation-stacked CSR
 * of dg_decoder_topk_f32 over the relation ids [0, n_rel), ascending and unique within a row
 * (unsorted columns may give a wrong list, never an out-of-range access); rows may be empty, a row
 * may exclude everything; excl_rowptr == excl_col == NULL excludes nothing, one of them NULL alone
 * is DG_EINVAL, and without a map the exclusion needs n_seg <= n_rel.  With DG_NODE_TOPK_NO_SELF
 * c' == r is dropped as well (needs n_rows == n_cols).
 *
 * Order: that of dg_decoder_topk_f32 with the column as the index — higher fp32 score first,
 * equal scores by smaller column, −0 as +0 (non-finite scores: no promise).  Keys are unique, so
 * the result is the unique top-k of the row whatever the tiling, the grid or the order in which
 * waves run.  A score has the bits dg_decoder_topk_f32 and dg_decoder_edge_rank_f32 give for the
 * pair (the same tile arithmetic).
 *
 * Outputs: out_score float32 [n_queries, topk], descending; out_col int32 [n_queries, topk];
 * out_count int32 [n_queries] = min(topk, permitted columns); slots past the count hold −inf / −1,
 * and −0 is returned as +0.  A query whose node lies outside [0, n_rows), and every query of a
 * segment whose relation lies outside [0, n_rel), gets count 0 and −inf / −1 (nothing out of range
 * is read for it).  A query's outputs depend on the query alone — not on its place in the call,
 * on the other queries, on the tiling or on the grid: two calls give identical bytes.
 *
 * topk in [1, DG_NODE_TOPK_MAX_K].  One workgroup takes one 32-query tile of one segment (the tile
 * map of dg_seg_tile_lookup); a tile's columns are dealt over the workgroup's waves and, where the
 * call has few query tiles, over several workgroups; their partial lists go to `workspace`
 * (16-byte aligned, at least dg_decoder_node_topk_workspace(n_queries, n_seg, n_cols, topk) bytes;
 * that may be 0, and then `workspace` may be NULL) and a second launch merges them.
 * DG_NODE_TOPK_NO_SPLIT keeps every tile's columns in one workgroup (the measured alternative,
 * DESIGN.md §21; identical results).
 *
 * Asynchronous on `stream`; allocates nothing and reads nothing on the host, so the call can be
 * captured in a graph.  n_queries == 0 succeeds without a launch.  DG_EINVAL / DG_EALIGN before
 * any HIP call for everything dg_decoder_edge_rank_f32 rejects in these arguments (with
 * n_queries > 0 a NULL row_idx, out_score, out_col or out_count), a topk out of range, a short or
 * missing workspace, an unknown flag, DG_NODE_TOPK_NO_SELF with n_rows != n_cols; DG_EALIGN for a
 * misaligned table or workspace or ld % 4 != 0.
 * -------------------------------------------------------------------------------------- */
#define DG_NODE_TOPK_MAX_K 128
#define DG_NODE_TOPK_NO_SELF 1
#define DG_NODE_TOPK_NO_SPLIT 2
int64_t dg_decoder_node_topk_workspace(int32_t n_queries, int32_t n_seg, int32_t n_cols, int32_t topk);
int dg_decoder_node_topk_f32(const float* row_table, int64_t ld_row, int32_t n_rows,
                             const float* col_table, int64_t ld_col, int32_t n_cols,
                             const int32_t* row_idx,
                             const int32_t* seg_ptr, const int32_t* seg_rel, int32_t n_seg, int32_t n_queries,
                             const float* G, int64_t g_stride, const float* l, int64_t l_stride,
                             int32_t n_rel, int32_t d, int32_t topk,
                             const int32_t* excl_rowptr, const int32_t* excl_col, int32_t flags,
                             float* out_score, int32_t* out_col, int32_t* out_count,
                             void* workspace, int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DECAGON_HIP_EXT2_H */

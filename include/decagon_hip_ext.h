/*
 * decagon_hip_ext.h — entry points of libdecagon_hip.so added after the 78 of ABI 39.
 *
 * decagon_hip.h is frozen at ABI 39: its 78 prototypes and 15 structs are what existing bindings
 * were generated from.  What the library gains afterwards is declared here, purely additive:
 * dg_abi_version() stays 39, and a binding of decagon_hip.h alone keeps working unchanged.  The
 * conventions of decagon_hip.h hold for every entry point below (device pointers unless marked
 * host, asynchronous launches on `stream`, DG_OK / negative DG_E* / positive hipError_t, IEEE fp32
 * in a fixed order, no float atomics), its constants and structs are in scope, and the header is
 * written in the same C subset: decagon_amd/abi.py parses it with the same parser
 * into a table of its own.
 */
#ifndef DECAGON_HIP_EXT_H
#define DECAGON_HIP_EXT_H

#include "decagon_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* --------------------------------------------------------------------------------------
 * Filtered rank of held-out edges (additive to ABI 39): for query q = (r, c) of segment s with
 * relation k = seg_rel[s] (seg_rel NULL: k = s), where the column c stands among the CANDIDATE
 * columns c' of row r under
 *
 *     s_k[r, c'] = (row_table[r] ∘ l_k)ᵀ · G_k · (l_k ∘ col_table[c'])          (fp32, MFMA)
 *
 * without forming any n_rows x n_cols matrix — the filtered rank of link prediction (mean
 * reciprocal rank, Hits@k).
 * Replaces: session.run(predictions) of one relation, a dense mask of the known edges and a count
 *           on the host, once per relation: the E·D·R·D·Eᵀ matrix of
 *           main/Predictor/NpPredictor.py:293-313 (_predictEdges).
 *
 * Operands: row_table / col_table as dg_decoder_topk_f32 (row r at table + r*ld, ld >= d,
 * ld % 4 == 0, 16-byte aligned; G and l need no alignment); d is 32 or 64; G_k, l_k, n_rel:
 * "Per-relation operands" of decagon_hip.h (the slots are the segments).  Queries are packed by
 * segment as dg_decoder_score_seg_f32 packs pairs: segment s is queries [seg_ptr[s], seg_ptr[s+1])
 * with seg_ptr int32 [n_seg + 1] ON THE DEVICE, ascending from 0 to n_queries, never read on the
 * host; segments may be empty.  n_queries + 32*n_seg < 2^31.
 *
 * Candidates of q: the columns c' in [0, n_cols) that are permitted, plus c itself, which is
 * always a candidate.  c' is permitted when it is not in relation k's exclusion row of r,
 * excl_col[excl_rowptr[k*n_rows + r] .. excl_rowptr[k*n_rows + r + 1]) — the relation-stacked CSR
 * of dg_decoder_topk_f32 over the relation ids [0, n_rel), ascending and unique within a row
 * (unsorted columns give a wrong count, never an out-of-range access); rows may be empty, a row
 * may exclude everything; excl_rowptr == excl_col == NULL excludes nothing, one of them NULL
 * alone is DG_EINVAL, and without a map the exclusion needs n_seg <= n_rel.  With
 * DG_EDGE_RANK_NO_SELF a candidate c' == r is dropped as well (needs n_rows == n_cols).
 *
 * Outputs, per query: out_rank[q] = 1 + the number of candidates c' != c that come before c in
 * the order of dg_decoder_topk_f32 with the column as the index — higher fp32 score first, equal
 * scores by smaller column, −0 as +0 (non-finite scores: no promise); out_score[q] = the fp32
 * score of (r, c) that was compared (−0 is returned as +0), computed with the candidates' own
 * tile arithmetic, so equal operands give equal bits; out_cand[q] = the number of candidates, c
 * included: 1 <= rank <= cand.  A query whose index lies outside [0, n_rows) x [0, n_cols), and
 * every query of a segment whose relation lies outside [0, n_rel), gets rank 0, cand 0 and score
 * NaN (nothing out of range is read).  out_score and out_cand may be NULL.
 *
 * A query's three outputs depend on the query alone — not on its place in the call, on the other
 * queries, on the tiling or on the grid: two calls give identical bytes.  One workgroup takes one
 * 32-query tile of one segment (the tile map of dg_seg_tile_lookup); where the call has few
 * query tiles, the column range of a tile is also dealt over several workgroups, whose integer
 * counts are added with integer atomics onto outputs the call zeroes first (sums commute: the
 * result is the same).  DG_EDGE_RANK_NO_SPLIT keeps every tile's columns in one workgroup (the
 * measured alternative; identical results).
 *
 * Asynchronous on `stream`; allocates nothing and reads nothing on the host, so the call can be
 * captured in a graph.  n_queries == 0 succeeds without a launch.  DG_EINVAL / DG_EALIGN before
 * any HIP call for everything dg_decoder_score_seg_f32 and dg_decoder_topk_f32 reject in these
 * arguments: a NULL table, seg_ptr or G; with n_queries > 0 a NULL row_idx, col_idx or out_rank;
 * n_seg < 1, n_queries < 0, n_rows < 1, n_cols < 1, ld < d, d not 32 or 64, a bad operand stride
 * or slot count, an unknown flag, DG_EDGE_RANK_NO_SELF with n_rows != n_cols, the 2^31 bound;
 * DG_EALIGN for a misaligned table or ld % 4 != 0.
 * -------------------------------------------------------------------------------------- */
#define DG_EDGE_RANK_NO_SELF 1
#define DG_EDGE_RANK_NO_SPLIT 2
int dg_decoder_edge_rank_f32(const float* row_table, int64_t ld_row, int32_t n_rows,
                             const float* col_table, int64_t ld_col, int32_t n_cols,
                             const int32_t* row_idx, const int32_t* col_idx,
                             const int32_t* seg_ptr, const int32_t* seg_rel, int32_t n_seg, int32_t n_queries,
                             const float* G, int64_t g_stride, const float* l, int64_t l_stride,
                             int32_t n_rel, int32_t d,
                             const int32_t* excl_rowptr, const int32_t* excl_col, int32_t flags,
                             int32_t* out_rank, float* out_score, int32_t* out_cand, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DECAGON_HIP_EXT_H */

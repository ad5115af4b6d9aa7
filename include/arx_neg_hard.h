/* arx_neg_hard.h -- pair losses: the hardest of C drawn negatives, drawn, scored and picked per batch row in one launch
 * (dynamic negative sampling).  Included by arx.h (include that); bound by NEG_HARD_PROTOTYPES in arx/_lib.py.  The
 * conventions are arx.h's: the function returns 0 or a negative ARX_E* code with the message through arx_last_error,
 * validates every argument before its first HIP call, and launches on `stream`. */
#ifndef ARX_NEG_HARD_H_
#define ARX_NEG_HARD_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* Build-defined (the reference's negative draw is a commented-out host loop that never looks at the model).
 * arx_neg_draw_hardest: for every batch row r of B, draw C candidate columns, score each against the row's user and
 * return the one the model scores highest.  No atomics, no workspace, graph-capturable, bit-reproducible: the result
 * depends on the arguments only, never on the grid.
 *
 * CANDIDATES.  2 <= C <= 64.  Candidate j is exactly the column arx_neg_draw_uniform (cum == ex_cum == NULL) or
 * arx_neg_draw_weighted (both set; NULL together, else ARX_EINVAL) gives row r at counter + j: the key is
 * (seed, *step_dev + counter + j, r), mix32 / multiply-high 32 for the uniform rule, mix64 / multiply-high 64 for the
 * weighted one, the same rank-select and the same binary searches; users, n_users, ex_ptr, ex_cols, ex_cum, cum, V and
 * step_dev (NULL: 0) are those calls' arguments.  The candidates are drawn independently: duplicates are legal.  A row
 * is VOID when the plain draw is void (no eligible column, or no eligible weight) and when its user has no table row
 * (below).  A candidate the plain draw reports as -1 although the row is not void (a list that is not sorted and
 * unique) is kept as column -1, scores -inf, and gives item -1 if it is picked.
 *
 * SCORES.  s_j = U[U_row(r)] . P[P_row(c_j)] + pbias[P_row(c_j)] in arx_slate_scores' arithmetic, bit for bit: the
 * ORDER OF THE ADDS of arx_slate.h (a group of L lanes, L the smallest power of two >= d / 4, owns one (row, candidate)
 * pair; one multiply and three fused multiply-adds per lane, xor-shuffle fold 1, 2, 4, ... L / 2, the bias last; pbias
 * may be NULL: no bias).  U_row(r) = umap ? umap[users[r]] : users[r] names a row of U [n_urows, ldu]; umap holds n_umap
 * entries.  P_row(c) = col2row ? col2row[c] : c names a row of P [n_prows, ldp]; col2row holds V entries.  A user id
 * outside [0, n_umap) is not looked up and a row outside [0, n_urows) is not read: the batch row is void.  A candidate
 * whose P_row is outside [0, n_prows) is not read and scores -inf (the map lives on the device, so the host cannot
 * reject it; it is what arx_slate_scores does with such an id).
 *
 * PICK.  v_j = isnan(s_j) ? -inf : s_j; the pick is the smallest j that maximises v_j.  A NaN never beats a number,
 * ties go to the earlier candidate, an all-NaN or all -inf row picks candidate 0.
 *
 * OUTPUTS.  neg_items[r] = col2item ? col2item[c_pick] : c_pick, -1 for a void row.  lookup_items (nullable): the same
 * ids with col2item[0] (or 0) in place of -1, as in the two plain draws.  Nullable diagnostics: out_pick [B]: j, -1
 * for a void row; out_cand [B, ldc]: the C columns, -1 across a void row; out_score [B, lds]: the bits of s_j (NOT
 * v_j: a NaN stays), -inf across a void row.  ldc, lds >= C.
 *
 * ENVELOPE.  d % 4 == 0 and 4 <= d <= 256, else ARX_EUNSUPPORTED (the widths arx_slate_scores serves).  Everything
 * else that is malformed is ARX_EINVAL: ldu, ldp multiples of 4 and >= d; U and P 16-byte aligned; 0 < V < 2^31;
 * 0 <= n_urows, n_prows < 2^31; B, n_users, n_umap >= 0; users, ex_ptr, ex_cols, U, P, neg_items not NULL.  B == 0
 * is legal and launches nothing.  Outputs are untouched on an error. */
int arx_neg_draw_hardest(const int32_t* users, int64_t B, int64_t n_users, const int32_t* ex_ptr,
                         const int32_t* ex_cols, const int64_t* ex_cum, const int64_t* cum, int64_t V,
                         const int32_t* col2item, uint64_t seed, const uint64_t* step_dev, uint64_t counter, int C,
                         const float* U, int64_t ldu, int64_t n_urows, const int32_t* umap, int64_t n_umap,
                         const float* P, int64_t ldp, int64_t n_prows, const float* pbias, const int32_t* col2row,
                         int d, int32_t* neg_items, int32_t* lookup_items, int32_t* out_pick, int32_t* out_cand,
                         int64_t ldc, float* out_score, int64_t lds, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ARX_NEG_HARD_H_ */

/* arx_tags.h -- recommend within item tags: the two entry points of the per-request any/all eligibility filter of the
 * full-vocabulary top-k.  Included by arx.h (include that); bound by TAGS_PROTOTYPES in arx/_lib.py.  The conventions
 * are arx.h's: every function returns 0 or a negative ARX_E* code with the message through arx_last_error, validates
 * its arguments before its first HIP call, and launches on `stream`. */
#ifndef ARX_TAGS_H_
#define ARX_TAGS_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* Recommend within item tags (opt-in; every call of arx.h is unchanged).  Every absolute logit column c carries one
 * 32-bit TAG WORD col_tags[c] (32 independent bits, their meaning the caller's; int32 bit patterns), every row r of a
 * recommend batch two words want_any[r % want_rows] and want_all[r % want_rows] (the modulo convention of row_keys /
 * key_rows of arx.h).  Column c is ELIGIBLE for row r iff
 *     (any == 0 || (tags & any) != 0)  &&  (tags & all) == all
 * -- a zero word is no constraint, (0, 0) makes every column eligible.  An ineligible column never appears in a
 * result; the others keep tf.nn.top_k's order; a row with fewer than k eligible columns ends in (-inf, -1)
 * (arx_topk_mark_empty).  The filter composes with the exclusion lists: a column must pass both.
 * arx_topk_tags_fill: logits[r * ld + (c - col0)] = -inf for every ineligible c in [col0, col0 + ncols), r < M --
 * the twin of arx_topk_exclude_fill (col_tags is indexed by the ABSOLUTE column; strided views; ncols == 0 is legal;
 * col0 + ncols < 2^31).
 * arx_gemm_nt_topk_filter_tags: arx_gemm_nt_topk_filter_excl (same arguments, same outputs, the same lse_part bits:
 * the normaliser stays over ALL the columns) whose candidates also skip the ineligible columns.  col_tags points at
 * the launch's FIRST column, like col_bias.  The exclusion lists are optional: row_keys, ex_ptr and ex_cols NULL
 * together means none.  lse_part is optional.  A tag too rare to give k eligible columns in the first chunk leaves
 * thr = -inf: the segments may overflow and the caller takes the chunked path, as for any overflow.
 * col_base >= 0, col_base + N < 2^31, want_rows > 0. */
int arx_topk_tags_fill(float* logits, int64_t ld, int64_t M, int32_t col0, int64_t ncols, const int32_t* col_tags,
                       const int32_t* want_any, const int32_t* want_all, int64_t want_rows, void* stream);
int arx_gemm_nt_topk_filter_tags(const float* A, int64_t lda, int64_t M, const float* Bm, int64_t ldb, int64_t N,
                                 int64_t K, const float* col_bias, const float* thr, int64_t ldthr, int32_t col_base,
                                 float* cand_v, int32_t* cand_i, int64_t ldcand, int capp, int* overflow, float* lse_part,
                                 int64_t ldl, const int32_t* row_keys, int64_t key_rows, const int32_t* ex_ptr,
                                 const int32_t* ex_cols, const int32_t* col_tags, const int32_t* want_any,
                                 const int32_t* want_all, int64_t want_rows, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ARX_TAGS_H_ */

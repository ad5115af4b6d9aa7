/* arx_topk_bf16.h -- recommend(scan_dtype='bf16'): the full-vocabulary top-k whose FILTER scan multiplies on the bf16
 * matrix pipe while every value and every decision the caller sees stays f32.  Included by arx.h (include that); bound by
 * TOPK_BF16_PROTOTYPES in arx/_lib.py.  The conventions are arx.h's: every function returns 0 or a negative ARX_E*
 * code with the message through arx_last_error, validates its arguments before its first HIP call, and launches on
 * `stream`. */
#ifndef ARX_TOPK_BF16_H_
#define ARX_TOPK_BF16_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* Build-defined (opt-in; every call of arx.h is unchanged).  The streaming top-k needs the scorer GEMM over the tail
 * of the vocabulary only as a filter: a logit leaves the kernel when it may beat its row's threshold, the k-th best of
 * an exactly scored first chunk.  The three calls below run that filter on bf16 roundings of both operands, widen its
 * test by a PROVEN bound of the rounding error so that it errs to one side only, and re-score what passed in f32:
 *     v~   = (bf16(U[r]) . bf16(P[c]), accumulated in f32) + bias[c]
 *     pass   iff   fmaf(rowm[r], coln[c], v~) > thr[r]         rowm[r] = coeff * |U[r]|_2,  coln[c] = |P[c]|_2
 * both norms rounded UP.  With coeff >= arx.topk.bf16_margin_coeff(K) (DESIGN.md section 4 item 20 has the proof and
 * the input domain: finite values well inside f32's range) every column whose f32 score -- arx_slate_scores'
 * arithmetic -- beats thr[r] passes.  The kernel compares against the float two steps BELOW thr[r]: that pays for
 * the roundings of the bias add and of the fmaf itself.  A NaN never passes.
 *
 * arx_rows_bf16_norm: one pass over N rows of P [N, K] f32 (row stride ldp).  img[n * ldi + j] = the round-to-nearest-
 * even bf16 of P[n, j] (a NaN becomes the quiet NaN 0x7fc0), norms[n] = sqrt(sum_j P[n, j]^2) * (1 + 2^-20): >= the
 * exact norm, within 2^-18 of it relatively.  ORDER OF THE ADDS: a group of L lanes (the smallest power of two >= K / 8)
 * owns a row, lane i squares and adds elements 8i .. 8i + 7 in that order (one multiply, seven fused multiply-adds),
 * the group folds by xor shuffles 1, 2, 4, ... L / 2.  K % 8 == 0, 8 <= K <= 512 (else ARX_EUNSUPPORTED); ldp % 4 == 0,
 * ldi % 8 == 0, ldp, ldi >= K, P and img 16-byte aligned.  N == 0 is legal.
 *
 * arx_gemm_nt_topk_filter_bf16: arx_gemm_nt_topk_filter_tags' decomposition, arguments and outputs (128 rows per
 * workgroup, the column ranges of arx_gemm_nt_topk_parts, candidate segments in ascending column order, *overflow) with
 * Bimg [N, K] bf16 (row stride ldbi) and coln [N] from arx_rows_bf16_norm in place of the f32 pool, and the test above.
 * cand_v receives v~ (NOT a score: arx_cand_rescore overwrites it), cand_i the absolute column col_base + c.  col_bias,
 * the exclusion lists (row_keys, ex_ptr, ex_cols: NULL together) and the tag arrays (col_tags, want_any, want_all:
 * NULL together; col_tags points at the launch's first column) are optional run-time operands; an ineligible column
 * takes no position.  K in {32, 64, 128} (else ARX_EUNSUPPORTED); A and Bimg 16-byte aligned, lda % 4 == 0,
 * ldbi % 8 == 0, lda, ldbi >= K; coeff finite and >= 0; col_base >= 0, col_base + N < 2^31.
 *
 * arx_cand_rescore: every OCCUPIED slot of the candidate rows (cand_v[r * ldcand + j] != -inf; j < ncand) gets
 * cand_v = U[r] . P[cand_i] + pbias[cand_i] in arx_slate_scores' arithmetic, bit for bit (the same order of the adds:
 * arx_slate.h); an empty slot is skipped, its cand_i is not read as a column.  P is the WHOLE pool (cand_i holds
 * absolute columns, 0 <= cand_i < V for an occupied slot: anything else is written as -inf).  d % 4 == 0,
 * 4 <= d <= 256 (else ARX_EUNSUPPORTED), ldu, ldp multiples of 4 and >= d, U and P 16-byte aligned, ldcand >= ncand,
 * B * ncand < 2^31.  B == 0 or ncand == 0 is legal. */
int arx_rows_bf16_norm(const float* P, int64_t ldp, int64_t N, int64_t K, uint16_t* img, int64_t ldi, float* norms,
                       void* stream);
int arx_gemm_nt_topk_filter_bf16(const float* A, int64_t lda, int64_t M, const uint16_t* Bimg, int64_t ldbi,
                                 const float* coln, int64_t N, int64_t K, float coeff, const float* col_bias,
                                 const float* thr, int64_t ldthr, int32_t col_base, float* cand_v, int32_t* cand_i,
                                 int64_t ldcand, int capp, int* overflow, const int32_t* row_keys, int64_t key_rows,
                                 const int32_t* ex_ptr, const int32_t* ex_cols, const int32_t* col_tags,
                                 const int32_t* want_any, const int32_t* want_all, int64_t want_rows, void* stream);
int arx_cand_rescore(const float* U, int64_t ldu, int64_t B, const float* P, int64_t ldp, const float* pbias, int64_t V,
                     int d, float* cand_v, const int32_t* cand_i, int64_t ldcand, int64_t ncand, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ARX_TOPK_BF16_H_ */

/* arx_sample_logp.h -- recommend(sample_temperature=, return_logprob=True): the log-probability of every draw of the
 * sampled recommend of arx_sample.h -- k distinct columns per row drawn from softmax(score / tau) over the WHOLE
 * vocabulary, one after the other without replacement (the Plackett-Luce law) -- the propensity a logged exploration
 * sample needs for off-policy evaluation.  The mass is taken in a pass of its own AFTER the picks are known: one more
 * scan of the scorer GEMM that sums, per row, what is LEFT (never "total minus picked"), then one finishing kernel.
 * Included by arx.h (include that); bound by SAMPLE_LOGP_PROTOTYPES in arx/_lib.py.  The conventions are arx.h's:
 * every function returns 0 or a negative ARX_E* code with the message through arx_last_error, validates its arguments
 * before its first HIP call, and launches on `stream`.  A call with nothing to do (B == 0) returns 0 and launches
 * nothing.  No atomics; tau and the picks are read from device memory, so a captured plan replays with new values. */
#ifndef ARX_SAMPLE_LOGP_H_
#define ARX_SAMPLE_LOGP_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* Build-defined (the reference ranks by score only).
 * THE RULE.  For request row r take as given the scores s[c] = latent_r . pool_c + bias_c (the bits of the project's
 * scorer GEMM), tau = tau[r % tau_rows] (finite and >= 0: arx.topk.sample_params) and the picks pi_0 .. pi_{k-1} the
 * sampled recommend returned, in SELECTION order; an entry -1 is past the last eligible column.
 *   ELIGIBLE  column c is eligible iff it is not in the row's exclusion list (row_keys / ex_ptr / ex_cols: the
 *             convention of arx_gemm_nt_topk_filter_excl), it passes the tag test of arx_tags.h where tags are given,
 *             and s[c] > -inf.  NaN and +inf are outside the contract, as for lse_part.
 *   REST      the eligible columns that are not among the row's picks.
 *   LOGP      logp[r][t] = a_{pi_t} - log sum over j in REST u {pi_t, .., pi_last} of exp(a_j), a = s / tau: the
 *             log-probability of pick t given the picks before it.  0 for every pick of a tau == 0 row (the list is
 *             certain) and for every -1 column.  The row sum is the log-propensity of the returned ordered list.
 * HOW LOGP IS FORMED (as arx_slate_sample.h): a mass is a pair (m, S), m the largest SCORE in it and
 * S = sum exp((s_j - m) / tau) >= 1; the empty mass is (-FLT_MAX, 0).  Two pairs join as
 * (max, S_hi + S_lo * exp((m_lo - m_hi) / tau)).  Only score DIFFERENCES meet tau and every mass is a sum of what is
 * left.  logp_t = (s_t - m_t) / tau - log S_t, (m_t, S_t) REST's mass joined with the picks t .. last, built from the
 * back.  The order of the joins depends on k and the number of parts P only: a row's outputs depend on that row's
 * inputs, k and P, not on B, the leading dimensions or the grid.
 * THE PICKS' SCORES.  The mass pass has to recognise a pick's column to leave it out; it writes that column's score
 * into pick_score[r][slot] there.  logp is formed from THESE scores, not from the stripped keys
 * (arx_topk_gumbel_strip is only within 2^-23 (|key| + |score|) of the score, an error a small tau magnifies), and
 * with return_logprob the returned `values` are these exact scores: values[r][t] carries the bits of the project's
 * scorer GEMM at (r, pi_t), -inf beside an index -1.  A selected column of score -inf (a row with fewer than k finite
 * scores and no filters, where the plain sampled call keeps the column's index) is not ELIGIBLE: the nodes mark it -1
 * (arx_topk_mark_empty) before this pass, the one place where the ids of the two calls may differ.  The finishing
 * kernel holds the same line on its own: a pick whose score came out as -inf is treated as a -1 column (logp 0).
 *
 * arx_sample_logp_sort: the row's picks sorted by column for the two mass kernels -- pk_cols[r * ldp + j] ascending
 * (as unsigned: the -1 entries last), pk_slot[r * ldp + j] the selection slot t of that column, j < k.  One wave per
 * row, an LDS rank sort; 1 <= k <= 1024, ldi >= k, ldp >= k.
 * arx_gemm_nt_rest_mass, the streaming form: one scan of A . Bm^T + col_bias over all N columns of the launch with no
 * logits in memory.  Per row and column range p < arx_gemm_nt_topk_parts(M, N) it writes REST's pair
 * (m_part[row * ldl + p], s_part[row * ldl + p]), and pick_score[row * ldps + slot] for every pick whose column the
 * launch covers (col_base <= column < col_base + N).  col_bias may be NULL; the exclusion lists (row_keys, ex_ptr,
 * ex_cols) and the tag arrays (col_tags, already offset to this launch's columns like col_bias; want_any, want_all)
 * are each optional as a group: all NULL = none.  K in {32, 64, 128}, 16-byte aligned operands (lda, ldb multiples of
 * 4), col_base >= 0, col_base + N < 2^31, tau_rows > 0, ldl >= parts, ldps >= k: otherwise ARX_EINVAL, a K the
 * kernel does not take ARX_EUNSUPPORTED.
 * arx_rest_mass_chunk, the materialised form: logits [B, ncols] (leading dimension ld) hold the scores of the
 * ABSOLUTE columns [col0, col0 + ncols) with -inf at every ineligible column (arx_topk_exclude_fill /
 * arx_topk_tags_fill ran).  One workgroup per row (a grid-stride loop over the rows, a capped grid) folds the chunk's
 * columns into the row's running REST pair (m_run[r], s_run[r]) -- first != 0: the pair starts empty -- skipping -inf
 * and the row's picks, and writes pick_score for the picks it meets.  ncols == 0 is a no-op (with first != 0 the
 * pairs are still reset).  col0 >= 0, col0 + ncols < 2^31.
 * arx_sample_logp_finish: one wave per row joins the P parts (m_part[r * ldl + p], s_part[..]) in part order (P = 1,
 * ldl = 1 for the running pairs of arx_rest_mass_chunk), runs the backward join over the picks in selection order with
 * the scores of pick_score, and stores logp[r * ldo + t], t < k.  values (nullable): values[r * ldv + t] =
 * pick_score[r * ldps + t], -inf where indices[r * ldi + t] < 0.  1 <= k <= 1024, P >= 1, ldl >= P. */
int arx_sample_logp_sort(const int32_t* indices, int64_t ldi, int64_t B, int k, int32_t* pk_cols, int32_t* pk_slot,
                         int64_t ldp, void* stream);
int arx_gemm_nt_rest_mass(const float* A, int64_t lda, int64_t M, const float* Bm, int64_t ldb, int64_t N, int64_t K,
                          const float* col_bias, int32_t col_base, const float* tau, int64_t tau_rows,
                          const int32_t* row_keys, int64_t key_rows, const int32_t* ex_ptr, const int32_t* ex_cols,
                          const int32_t* col_tags, const int32_t* want_any, const int32_t* want_all, int64_t want_rows,
                          const int32_t* pk_cols, const int32_t* pk_slot, int64_t ldp, int k, float* m_part,
                          float* s_part, int64_t ldl, float* pick_score, int64_t ldps, void* stream);
int arx_rest_mass_chunk(const float* logits, int64_t ld, int64_t B, int32_t col0, int64_t ncols, const float* tau,
                        int64_t tau_rows, const int32_t* pk_cols, const int32_t* pk_slot, int64_t ldp, int k, int first,
                        float* m_run, float* s_run, float* pick_score, int64_t ldps, void* stream);
int arx_sample_logp_finish(const int32_t* indices, int64_t ldi, const float* pick_score, int64_t ldps,
                           const float* m_part, const float* s_part, int64_t ldl, int P, const float* tau,
                           int64_t tau_rows, int64_t B, int k, float* logp, int64_t ldo, float* values, int64_t ldv,
                           void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ARX_SAMPLE_LOGP_H_ */

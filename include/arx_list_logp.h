/* arx_list_logp.h -- list_logprob: the log-probability of a GIVEN ordered list under the sampling policy of
 * arx_sample.h / arx_sample_logp.h -- the numerator of an importance weight pi_target(logged list) / pi_logging(logged
 * list), where arx_sample_logp.h gives the denominator at serving time.  A list that was logged elsewhere may hold
 * entries the policy could never draw (an item seen since, an item outside today's tags, a repeat, an id past the
 * vocabulary): two kernels around the UNCHANGED mass pass and finish of arx_sample_logp.h turn such a list into one
 * those kernels accept, say why each entry was rejected, and mark the impossible entries.
 * Included by arx.h (include that); bound by LIST_LOGP_PROTOTYPES in arx/_lib.py.  The conventions are arx.h's: every
 * function returns 0 or a negative ARX_E* code with the message through arx_last_error, validates its arguments before
 * its first HIP call, and launches on `stream`.  A call with nothing to do (B == 0) returns 0 and launches nothing.
 * No atomics; the lists, the filters and the scores are read from device memory, so a captured plan replays with new
 * values. */
#ifndef ARX_LIST_LOGP_H_
#define ARX_LIST_LOGP_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* The reason codes of an entry (int32, part of the ABI).  Where several apply, the lowest wins. */
#define ARX_LIST_OK 0        /* drawable */
#define ARX_LIST_EMPTY 1     /* the entry is -1 */
#define ARX_LIST_RANGE 2     /* any other negative value, or >= V */
#define ARX_LIST_EXCLUDED 3  /* the column is in the row's exclusion list */
#define ARX_LIST_TAGS 4      /* the column fails the tag test */
#define ARX_LIST_REPEAT 5    /* the column passed 2-4 and an earlier slot of the row holds it (the lowest slot stays OK) */
#define ARX_LIST_NOSCORE 6   /* the column passed all of that and its score is -inf */

/* Build-defined (the reference ranks by score only).  The terms are those of arx_sample_logp.h.
 * THE RULE.  For request row r take as given the scores s[c] of the project's scorer GEMM, tau = tau[r % tau_rows] > 0
 * (tau == 0 is refused on the host: a deterministic policy has no propensities), the row's ELIGIBLE set exactly as
 * arx_sample_logp.h defines it (exclusion list, tag test, s > -inf) and a list L[r][0 .. k-1] of logit indices, -1 an
 * empty slot.
 *   DRAWABLE  entry t is drawable iff 0 <= L[t] < V, L[t] is ELIGIBLE, and no DRAWABLE entry before it holds the same
 *             column.  Every other entry carries one of the codes 1-6 above.
 *   ABSENT    a non-drawable entry is absent for every other entry of the row: it is no pick, and where it was
 *             ineligible it was never in any mass.  (The alternative -- one impossible entry poisons the whole row's
 *             entries -- would lose what the other entries say; the ROW SUM is -inf either way.)
 *   REST      the ELIGIBLE columns that are not DRAWABLE entries of the row.
 *   LOGP      logp[r][t] of a DRAWABLE entry = a_t - log sum over REST u {drawable entries t .. last} of exp(a),
 *             a = s / tau, formed from (max, sum) pairs with the joins of arx_sample_logp.h, unchanged; 0 at EMPTY;
 *             -inf at the codes 2-6.  The row sum is the log-probability that the policy returns exactly this ordered
 *             list as its first k draws, -inf if it cannot.
 *   VALUES    values[r][t] carries the bits of the scorer GEMM at a DRAWABLE entry, -inf elsewhere.
 * THE CALL SEQUENCE: arx_list_logp_prepare; the mass pass of arx_sample_logp.h on `clean` with the (pk_cols, pk_slot)
 * prepare wrote (arx_gemm_nt_rest_mass, or arx_rest_mass_chunk per chunk) -- after prepare its contract holds: the
 * picks are distinct, in range, not excluded and pass the tags --; arx_sample_logp_finish on `clean`, which treats a
 * pick whose score came out -inf as an empty slot; arx_list_logp_stamp.  A list the policy drew itself passes
 * prepare unchanged (clean == list, the sorted picks are those of arx_sample_logp_sort), so its logp and values are
 * bit-identical to those reported with the draw.
 *
 * arx_list_logp_prepare: one wave per row (a grid-stride loop over the rows, a capped grid).  lists [B, k] int32 with
 * leading dimension ldl; V the vocabulary, 0 < V < 2^31; 1 <= k <= 1024.  The exclusion group (row_keys, key_rows,
 * ex_ptr, ex_cols: the convention of arx_gemm_nt_topk_filter_excl, the row's columns ascending, a key < 0: none) and
 * the tag group (col_tags [V] by absolute column, want_any, want_all, want_rows: arx_tags.h) are each optional as a
 * group: all NULL = none; with a group key_rows / want_rows > 0.  Outputs, each [B, k]: clean (ldc) -- the column where
 * the code is 0 so far, else -1; why (ldw) -- the codes 0-5; pk_cols / pk_slot (ldp) -- bit-identical to what
 * arx_sample_logp_sort writes for `clean`.  Range and tag tests are per entry, the exclusion test is a binary search
 * in the row's list; the survivors are held in LDS, one sweep over the earlier slots finds the repeats among them, and
 * the rank sort of arx_sample_logp_sort by (column as unsigned, slot) over the cleaned row writes the sorted picks.
 * arx_list_logp_stamp: one thread per entry, after arx_sample_logp_finish.  A clean entry >= 0 whose pick_score is
 * -inf gets why = 6; every entry of code >= 2 gets logp = -inf and (values nullable) value = -inf.  Nothing else is
 * written; pick_score is read only where clean >= 0.  ldc, ldps, ldw, ldo (and ldv with values) >= k. */
int arx_list_logp_prepare(const int32_t* lists, int64_t ldl, int64_t B, int k, int64_t V, const int32_t* row_keys,
                          int64_t key_rows, const int32_t* ex_ptr, const int32_t* ex_cols, const int32_t* col_tags,
                          const int32_t* want_any, const int32_t* want_all, int64_t want_rows, int32_t* clean,
                          int64_t ldc, int32_t* why, int64_t ldw, int32_t* pk_cols, int32_t* pk_slot, int64_t ldp,
                          void* stream);
int arx_list_logp_stamp(const int32_t* clean, int64_t ldc, const float* pick_score, int64_t ldps, int64_t B, int k,
                        int32_t* why, int64_t ldw, float* logp, int64_t ldo, float* values, int64_t ldv, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ARX_LIST_LOGP_H_ */

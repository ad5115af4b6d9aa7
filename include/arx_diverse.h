/* arx_diverse.h -- score_items(diversify=): a greedy MMR (maximal marginal relevance) re-rank of a scored per-row
 * candidate slate, optionally with a cap on how many picks one group (category / brand / seller) may take.  Included by
 * arx.h (include that); bound by DIVERSE_PROTOTYPES in arx/_lib.py.  The conventions are arx.h's: every function
 * returns 0 or a negative ARX_E* code with the message through arx_last_error, validates its arguments before its first
 * HIP call, and launches on `stream`.  A call with nothing to do (B == 0) returns 0 and launches nothing. */
#ifndef ARX_DIVERSE_H_
#define ARX_DIVERSE_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* Build-defined (the reference ranks by score only).
 * arx_slate_mmr: for request row r, with cand = cand[r * ldc + j], s = scores[r * lds + j] (as arx_slate_scores wrote
 * them), lambda = lam[r] in [0, 1] and, where groups is given, g[j] = groups[cand[j]] and m = max(1, max_per_group[r]):
 *   LIVE      slot j is live iff 0 <= cand[j] < V and s[j] is finite.  No pool row is read for any other slot.
 *   REL       smin / smax the smallest / largest live score; rel[j] = (s[j] - smin) / (smax - smin) where smax > smin,
 *             1 for every live slot otherwise (float32, a correctly rounded division).
 *   COS       cos(i, j) = sum_c x_i[c] * x_j[c] over the UNIT rows x = P[cand] * inv, inv = 1.0f / sqrtf(sum of
 *             squares) (0 for a zero row): the sum and the inverse are arx_rows_inv_norm's, bit for bit.  No bias.
 *   SELECT    for t = 0 .. k - 1: among the live, unselected slots whose group is not full (a slot with g < 0, or any
 *             slot when groups is NULL, is never full; a group is full once m selected slots carry it) take the one
 *             with the largest obj[j] = lambda * rel[j] - (1 - lambda) * pen[j]; ties go to the higher s[j], then to
 *             the lower slot.  ids[r * ldi + t] = cand[j*], values[r * ldv + t] = s[j*] (the score, not obj),
 *             pos[r * ldq + t] = j*; then pen[j] = max(pen[j], cos(j, j*)) for every j.  pen starts at 0, so a negative
 *             cosine never rewards a candidate.  When no slot qualifies the rest of the row is (-1, -inf, -1).
 * The same item in two slots is two candidates with cosine 1 between them.  Hence: the first pick is the best-scored
 * eligible slot, and lambda = 1 without groups gives the order of arx_topk over the scores (score desc, slot asc) bit
 * for bit -- the tie-break on s before the slot holds that even where the division maps two scores to one rel.
 * lam [B], groups [V] and max_per_group [B] are read from device memory by the kernel: one captured launch serves every
 * lambda and cap.  lam[r] outside [0, 1] or NaN is the caller's to refuse.
 * ORDER OF THE ADDS of a cosine: four partial sums, one per element index mod 4, each a chain of fused multiply-adds
 * over c = 0, 4, 8, ... in that order, then (p0 + p1) + (p2 + p3).  That depends on d ONLY: a row's outputs depend on
 * that row's inputs only, not on B, the leading dimensions or the grid.
 * d % 4 == 0, d >= 4, ldp a multiple of 4 and >= d, P 16-byte aligned, ldc, lds >= C, ldi, ldv, ldq >= k, 1 <= k <= C,
 * B >= 0, 0 <= V < 2^31, groups and max_per_group both NULL or both given (else ARX_EINVAL); a (C, d) that
 * arx_slate_mmr_supported refuses gives ARX_EUNSUPPORTED with the rule in the message.  Outputs are untouched on an
 * error.  One workgroup per row keeps the row's C unit rows in LDS for all k steps: no atomics, no global scratch, no
 * workspace.
 * arx_slate_mmr_supported: 1 iff d % 4 == 0, 4 <= d <= 128, 1 <= C <= 512 and C * d <= 32768 (the C rows, their padding
 * and the per-row state fit the 160 KiB of LDS one workgroup may declare), else 0.  A pure host predicate: no HIP
 * call, no error message. */
int arx_slate_mmr_supported(int64_t C, int d);
int arx_slate_mmr(const float* P, int64_t ldp, int64_t V, int d, const int32_t* cand, int64_t ldc, const float* scores,
                  int64_t lds, int64_t B, int64_t C, const float* lam, const int32_t* groups,
                  const int32_t* max_per_group, int k, int32_t* ids, int64_t ldi, float* values, int64_t ldv,
                  int32_t* pos, int64_t ldq, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ARX_DIVERSE_H_ */

/* arx_slate_sample.h -- score_items(sample_temperature=): k distinct items of a scored per-row candidate slate drawn
 * with probability proportional to exp(score / tau), one after the other without replacement (the Plackett-Luce law),
 * together with the log-probability of every draw -- the propensity a logged sample needs for off-policy evaluation.
 * The draw is the top-k of the KEYS score + tau * G of arx_sample.h over the slate (Gumbel-top-k).  Included by arx.h
 * (include that); bound by SLATE_SAMPLE_PROTOTYPES in arx/_lib.py.  The conventions are arx.h's: every function returns
 * 0 or a negative ARX_E* code with the message through arx_last_error, validates its arguments before its first HIP
 * call, and launches on `stream`.  A call with nothing to do (B == 0) returns 0 and launches nothing. */
#ifndef ARX_SLATE_SAMPLE_H_
#define ARX_SLATE_SAMPLE_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* Build-defined (the reference ranks by score only).
 * arx_slate_sample: for request row r, with cand[j] = cand[r * ldc + j], s[j] = scores[r * lds + j] (as
 * arx_slate_scores wrote them), tau = tau[r % tau_rows] (finite and >= 0: the caller's duty, arx.topk.sample_params)
 * and the noise row r % tau_rows of arx_sample.h (seed = seed_words[0] | seed_words[1] << 32):
 *   LIVE      slot j is live iff cand[j] >= 0 and s[j] is finite (-inf marks an empty slot or an item switched off by
 *             its bias; NaN and +inf are not live either).
 *   DISTINCT  a live slot whose id equals that of a lower-numbered live slot of the row does not compete and adds no
 *             weight: the law is over the row's distinct items.  The call relies on slots of one row that carry the
 *             same id also carrying the same score bits (arx_slate_scores guarantees it): they then carry the same key
 *             and meet in one run of the sorted order.  The COMPETITORS are the live slots that are left.
 *   KEY       key[j] = fmaf(tau, g(r % tau_rows, (uint32) cand[j]), s[j]), g of csrc/gumbel.h (gumbel_row, gumbel_bits,
 *             gumbel_of_bits) and nothing else: the noise is a function of the ITEM, so a slate draw is the restriction
 *             of the sampled recommend's draw to the slate and does not depend on the order of the slate.  tau == 0:
 *             key == s bit for bit.
 *   SELECT    the competitors by (key desc, slot asc), keys compared as arx_topk compares values (-0 below +0); the
 *             first k in that order are output, pick t at column t: ids[r * ldi + t] = cand[j_t],
 *             values[r * ldv + t] = s[j_t] (the score itself, the bits of the slate's entry -- no key is stripped),
 *             pos[r * ldq + t] = j_t; past the last competitor (-1, -inf, -1).
 *   LOGP      (logp may be NULL: nothing is computed)  logp[r * ldl + t] = a_t - log sum over the competitors j not
 *             picked before t of exp(a_j), a_j = s[j] / tau: the log-probability of pick t given the picks before it;
 *             the row sum is the log-propensity of the returned ordered list.  0 for every pick of a tau == 0 row (the
 *             list is certain) and for every column past the last competitor.
 * HOW LOGP IS FORMED: the remaining mass of a pick is carried as a pair (m, S), m the largest SCORE among what is left
 * and S = sum exp((s[j] - m) / tau) >= 1, so logp = (s_t - m) / tau - logf(S).  Only score DIFFERENCES are divided by
 * tau and every mass is re-centred on its own maximum: finite for every real pick and every finite tau > 0, however
 * small.  Every S is a sum of the weights of what is left (a suffix scan over the sorted order: two pairs join as
 * (max, S_hi + S_lo * expf((m_lo - m_hi) / tau))), never "total minus picked".  The order of the joins depends on C
 * only: a row's outputs depend on that row's inputs only, not on B, the leading dimensions or the grid.
 * tau [tau_rows], seed_words [2] and the slate are read from device memory by the kernel: one captured launch serves
 * every temperature and seed.
 * NULL cand, scores, tau, seed_words, ids, values or pos, B < 0, C < 0, k outside [1, C], ldc or lds < C, ldi, ldv or
 * ldq < k, ldl < k with logp given, tau_rows <= 0: ARX_EINVAL; a C that arx_slate_sample_supported refuses:
 * ARX_EUNSUPPORTED with the rule in the message.  Outputs are untouched on an error.  One workgroup per row keeps the
 * row's sort words in LDS: no atomics, no global scratch, no workspace.
 * arx_slate_sample_supported: 1 iff 1 <= C <= 1024 (arx_topk's limit on k, and what a 256-thread workgroup sorts in
 * four words per thread), else 0.  A pure host predicate: no HIP call, no error message. */
int arx_slate_sample_supported(int64_t C);
int arx_slate_sample(const int32_t* cand, int64_t ldc, const float* scores, int64_t lds, int64_t B, int64_t C,
                     const float* tau, int64_t tau_rows, const int32_t* seed_words, int k, int32_t* ids, int64_t ldi,
                     float* values, int64_t ldv, int32_t* pos, int64_t ldq, float* logp, int64_t ldl, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ARX_SLATE_SAMPLE_H_ */

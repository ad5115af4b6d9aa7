/* arx_slate.h -- score_items: score a per-row candidate slate against the item pool, and the shard merge of the
 * row-sharded form.  Included by arx.h (include that); bound by SLATE_PROTOTYPES in arx/_lib.py.  The conventions are
 * arx.h's: every function returns 0 or a negative ARX_E* code with the message through arx_last_error, validates its
 * arguments before its first HIP call, and launches on `stream`.  A call with nothing to do (B == 0 or C == 0) returns
 * 0 and launches nothing. */
#ifndef ARX_SLATE_H_
#define ARX_SLATE_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* Build-defined (the reference scores one pool for the whole batch or the full vocabulary, never a list per row).
 * arx_slate_scores: row r of U [B, d] against the C pool rows its slate names.  With c = cand[r * ldc + j]:
 *     0 <= c < V:  scores[r * lds + j] = sum_i U[r, i] * P[c, i] + pbias[c]      (pbias may be NULL: no bias)
 *     otherwise:   scores[r * lds + j] = -inf, and no pool row is read
 * -- otherwise covers -1 (an empty slot), every other negative id, ARX_KEY_NONE (what arx_shard_route gives for an item
 * of another shard) and anything >= V.  A gather and a dot: [B, C, d] is never materialised.
 * d % 4 == 0 and ldu, ldp multiples of 4 and >= d, U and P 16-byte aligned, ldc, lds >= C, B * C < 2^31, V < 2^31
 * (else ARX_EINVAL); 4 <= d <= 256 (else ARX_EUNSUPPORTED, the envelope of arx_pair_loss_fwdbwd).  Outputs are
 * untouched on an error.  No atomics.
 * ORDER OF THE ADDS: a group of L lanes (L the smallest power of two >= d / 4) owns one (row, slot) pair; lane i
 * multiplies elements 4i .. 4i + 3 and adds them in that order (one multiply, three fused multiply-adds), the group
 * folds by xor shuffles 1, 2, 4, ... L / 2, and the bias is added last.  That order depends on d ONLY -- not on the
 * slot, C, B, the leading dimensions or the grid -- so the same item in two slots of a row, or the same slate
 * permuted or padded, gives equal bit patterns.
 * arx_slate_merge_shards: parts [W][B][C] contiguous, block s the scores shard s computed (as all_to_all delivers
 * them); out[r * ldo + j] = max over s of parts[s][r][j].  Exactly one shard owns a live slot and every other shard
 * wrote -inf, so the max is that shard's bits, unchanged (a NaN of the owner stays a NaN).  1 <= W <= 64, ldo >= C,
 * B * C < 2^31. */
int arx_slate_scores(const float* U, int64_t ldu, int64_t B, const float* P, int64_t ldp, const float* pbias, int64_t V,
                     int d, const int32_t* cand, int64_t ldc, int64_t C, float* scores, int64_t lds, void* stream);
int arx_slate_merge_shards(const float* parts, int64_t B, int64_t C, int W, float* out, int64_t ldo, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ARX_SLATE_H_ */

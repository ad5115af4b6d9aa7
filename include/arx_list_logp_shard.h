/* arx_list_logp_shard.h -- list_logprob (arx_list_logp.h) on the ROW-SHARDED models (arx.dist: ShardedHMF, ShardedW2V,
 * ShardedHetView), whose item table is striped over W ranks: global item id = local column * W + shard.  The rule, the
 * reason codes and the terms are arx_list_logp.h's, over the user's eligible vocabulary ACROSS the shards; the mass pass
 * and arx_sample_logp_finish_shards (arx_sample_shard.h) and arx_list_logp_stamp run unchanged.  What is new is the part
 * that takes a list the policy did not draw itself when eligibility is decided on another rank: the exclusion lists and
 * the tag words live with the item's owner, as LOCAL columns.
 * Included by arx.h (include that); bound by LIST_LOGP_SHARD_PROTOTYPES in arx/_lib.py.  The conventions are arx.h's:
 * every function returns 0 or a negative ARX_E* code with the message through arx_last_error, validates its arguments
 * before its first HIP call, and launches on `stream`.  B == 0: returns 0 and launches nothing.  No atomics.
 *
 * THE CALL SEQUENCE.  Every shard s, over ALL B request rows (the lists gathered to every rank):
 * arx_list_logp_prepare_shard, then the mass pass of arx_sample_logp.h over the shard's rows with the (pk_cols, pk_slot)
 * it wrote; the REST parts, the pick scores and the codes cross to the rows' owners; there
 * arx_list_logp_merge_shards, arx_sample_logp_finish_shards on the merged `clean`, arx_list_logp_stamp with the
 * finish's values as the score it tests (NOSCORE, and -inf at the codes 2-6).
 *
 * arx_list_logp_prepare_shard: arx_list_logp_prepare by (W, s) -- ONE kernel body; arx_list_logp_prepare is this at
 * (1, 0), bit for bit.  lists [B, k] hold GLOBAL ids.  Per entry v:
 *   v == -1                          code 1 (EMPTY), no pick      } the same on every shard; the owner's merge
 *   any other v outside [0, V_global) code 2 (RANGE), no pick     } decides these two from the list alone
 *   v % W != s                       NOT MINE: no pick, code 0
 *   otherwise                        the LOCAL column v / W goes through the binary search in the row's exclusion list
 *                                    (local columns, the convention of arx_list_logp_prepare) -> 3, then the tag test on
 *                                    col_tags[v / W] (this shard's words) -> 4, then the repeat sweep -> 5.
 * Two copies of an id have one owner, so the owner alone decides REPEAT (a first copy whose score turns out -inf still
 * makes the next a REPEAT: the sweep runs before any score is known).  Outputs, each [B, k]: clean (ldc) -- the LOCAL
 * column of an owned entry of code 0, else -1; why (ldw) -- the codes above; pk_cols / pk_slot (ldp) -- bit-identical to
 * arx_picks_to_shard(W, s) + arx_sample_logp_sort over the merged global clean list.  col_tags needs one word per row of
 * the shard (ceil((V_global - s) / W)).  W >= 1, 0 <= s < W, 0 < V_global < 2^31, 1 <= k <= 1024; one wave per row, a
 * grid-stride loop over the rows under a capped grid.
 *
 * arx_list_logp_merge_shards: one thread per entry of the owner's lists [B, k] (B: the owner's rows; GLOBAL ids).
 * -1 -> why 1; any other v outside [0, V_global) -> why 2; otherwise why = codes[(v % W) * slab + r * ldcode + j], the
 * verdict of the entry's owner shard (codes: W shard-major slabs [B, k] of what prepare_shard wrote for these rows; a
 * view into a packed exchange buffer is fine).  clean[r][j] = v where why is 0, else -1: what the finish reads as the
 * picks.  1 <= W <= 64; ldl, ldcode, ldc, ldw >= k; slab >= 0. */
#ifndef ARX_LIST_LOGP_SHARD_H_
#define ARX_LIST_LOGP_SHARD_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

int arx_list_logp_prepare_shard(const int32_t* lists, int64_t ldl, int64_t B, int k, int64_t V_global, int W, int s,
                                const int32_t* row_keys, int64_t key_rows, const int32_t* ex_ptr,
                                const int32_t* ex_cols, const int32_t* col_tags, const int32_t* want_any,
                                const int32_t* want_all, int64_t want_rows, int32_t* clean, int64_t ldc, int32_t* why,
                                int64_t ldw, int32_t* pk_cols, int32_t* pk_slot, int64_t ldp, void* stream);
int arx_list_logp_merge_shards(const int32_t* lists, int64_t ldl, int64_t B, int k, int64_t V_global,
                               const int32_t* codes, int64_t ldcode, int64_t slab, int W, int32_t* clean, int64_t ldc,
                               int32_t* why, int64_t ldw, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ARX_LIST_LOGP_SHARD_H_ */

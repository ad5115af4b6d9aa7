/* arx_sample_shard.h -- the sampled recommend of arx_sample.h and its propensities (arx_sample_logp.h) on the
 * ROW-SHARDED models (arx.dist: ShardedHMF, ShardedW2V, ShardedHetView), whose item table is striped over W ranks:
 * global item id = local column * W + shard.  Included by arx.h (include that); bound by SAMPLE_SHARD_PROTOTYPES in
 * arx/_lib.py.  The conventions are arx.h's: every function returns 0 or a negative ARX_E* code with the message
 * through arx_last_error, validates its arguments before its first HIP call, and launches on `stream`.  No atomics.
 *
 * THE KEYED NOISE.  g(seed, noise row, noise column) is the hash of arx_sample.h, unchanged; only what is fed to it
 * changes.  The three *_keyed functions are the three functions of arx_sample.h with (col_mul, col_add, noise_rows):
 *   noise column = (absolute column) * col_mul + col_add      col_mul >= 1, 0 <= col_add < col_mul; the largest noise
 *                  column of the call's columns must be < 2^31 (checked before the first HIP call where the columns
 *                  are arguments -- add, filter; strip reads them from device memory: the caller's duty)
 *   noise row of batch row r = noise_rows[r % tau_rows], int32 [tau_rows] on the device; NULL: r % tau_rows
 *   a row whose noise row is negative (a padding row, key -1) is a tau == 0 row: add and the filter leave its logits
 *   as its keys, strip leaves its values alone (-inf beside an index -1, as for every row).
 * ONE kernel body per operation: the functions of arx_sample.h are these at (1, 0, NULL), bit for bit (in the fused
 * filter the column map is a compile-time mode of the one GEMM body, off at (1, 0, NULL)).  Shard s of W
 * passes (W, s, the rows' GLOBAL user ids): a draw is then a function of (seed, user, global item) and of the scores
 * alone -- not of W, the batch, or the row's position in it.  Stripping MERGED lists of global ids: (1, 0, user ids).
 *
 * arx_picks_to_shard: the picks of merged lists as columns of one shard: cols[r * ldc + j] = id / W where
 * id = ids[r * ldi + j] >= 0 and id % W == s, else -1 -- what arx_sample_logp_sort and the mass pass of that shard take.
 * B >= 0 (0: no launch), k >= 1, ldi >= k, ldc >= k, W >= 1, 0 <= s < W.
 *
 * arx_sample_logp_finish_shards: arx_sample_logp_finish over W shard-major slabs.  Shard w's REST parts of row r are
 * (m_part, s_part)[w * slab_l + r * ldl + p], p < P (a shard with fewer parts pads with the empty mass (-FLT_MAX, 0)),
 * its pick scores pick_score[w * slab_ps + r * ldps + t] (-inf where the shard does not own pick t).  The parts join in
 * (shard, part) order; the score of pick t is read from slab indices[t] % W (indices: GLOBAL ids in selection order);
 * then the backward join and logp of arx_sample_logp.h.  A row's outputs depend on that row's inputs, k, W and P only.
 * One wave per row.  values (nullable) gets the exact pick scores, -inf beside an index -1.  1 <= W <= 64,
 * 1 <= k <= 1024, P >= 1, ldl >= P, slab strides >= 0; W == 1 equals arx_sample_logp_finish bit for bit. */
#ifndef ARX_SAMPLE_SHARD_H_
#define ARX_SAMPLE_SHARD_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

int arx_topk_gumbel_add_keyed(float* logits, int64_t ld, int64_t M, int32_t col0, int64_t ncols, const float* tau,
                              int64_t tau_rows, const int32_t* seed_words, int32_t col_mul, int32_t col_add,
                              const int32_t* noise_rows, void* stream);
int arx_topk_gumbel_strip_keyed(float* values, int64_t ldv, const int32_t* indices, int64_t ldi, int64_t B, int k,
                                const float* tau, int64_t tau_rows, const int32_t* seed_words, int32_t col_mul,
                                int32_t col_add, const int32_t* noise_rows, void* stream);
int arx_gemm_nt_topk_filter_sample_keyed(const float* A, int64_t lda, int64_t M, const float* Bm, int64_t ldb,
                                         int64_t N, int64_t K, const float* col_bias, const float* thr, int64_t ldthr,
                                         int32_t col_base, float* cand_v, int32_t* cand_i, int64_t ldcand, int capp,
                                         int* overflow, float* lse_part, int64_t ldl, const int32_t* row_keys,
                                         int64_t key_rows, const int32_t* ex_ptr, const int32_t* ex_cols,
                                         const int32_t* col_tags, const int32_t* want_any, const int32_t* want_all,
                                         int64_t want_rows, const float* tau, int64_t tau_rows,
                                         const int32_t* seed_words, int32_t col_mul, int32_t col_add,
                                         const int32_t* noise_rows, void* stream);
int arx_picks_to_shard(const int32_t* ids, int64_t ldi, int64_t B, int k, int W, int s, int32_t* cols, int64_t ldc,
                       void* stream);
int arx_sample_logp_finish_shards(const int32_t* indices, int64_t ldi, const float* pick_score, int64_t ldps,
                                  int64_t slab_ps, const float* m_part, const float* s_part, int64_t ldl,
                                  int64_t slab_l, int W, int P, const float* tau, int64_t tau_rows, int64_t B, int k,
                                  float* logp, int64_t ldo, float* values, int64_t ldv, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ARX_SAMPLE_SHARD_H_ */

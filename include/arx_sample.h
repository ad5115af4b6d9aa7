/* arx_sample.h -- the sampled recommend: k distinct items per row drawn with probability proportional to
 * exp(score / tau), sequentially without replacement (the Plackett-Luce law), as the top-k of the KEYS
 * score + tau * G with independent standard Gumbel noise G per (row, column) (Gumbel-top-k).  Included by arx.h
 * (include that); bound by SAMPLE_PROTOTYPES in arx/_lib.py.  The conventions are arx.h's: every function returns 0 or
 * a negative ARX_E* code with the message through arx_last_error, validates its arguments before its first HIP call,
 * and launches on `stream`. */
#ifndef ARX_SAMPLE_H_
#define ARX_SAMPLE_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* The noise (csrc/gumbel.h, the one definition) is a pure function of (seed, row, col), so the dense, the chunked and
 * the fused path draw the same sample and a request re-run after a candidate overflow returns the same items.  All
 * integer arithmetic is unsigned and wrapping; seed = seed_words[0] (low) | seed_words[1] << 32, two int32 words ON THE
 * DEVICE (a captured plan replays with a new seed); col is the ABSOLUTE logit column; row r of a batch reads
 * tau[r % tau_rows] and its noise row is r % tau_rows (the modulo convention of want_rows of arx_tags.h: row
 * pos * B + i of SeqModel's [L * B, V] logits is sequence i).
 *   per row:    z = seed * 0x9E3779B97F4A7C15 + (row + 1) * 0xD1B54A32D192ED03                         (u64)
 *               z = (z ^ z >> 30) * 0xbf58476d1ce4e5b9;  z = (z ^ z >> 27) * 0x94d049bb133111eb;  z ^= z >> 31
 *               b0 = (u32) z, b1 = (u32)(z >> 32)
 *   per column: x = col + b0;  x ^= x >> 16;  x *= 0x7feb352d;  x ^= x >> 15;  x ^= b1;  x *= 0x846ca68b;  x ^= x >> 16
 *               m = x >> 9;  u = ((float) m + 0.5f) * 2^-23  (exact; never 0 or 1);  g = -logf(-logf(u))
 *   key = fmaf(tau, g, v)   g in [-2.8116, 16.6356]: tau == 0 gives key == v bit for bit, v == -inf stays -inf.
 * tau must be finite and >= 0 (the caller's duty: arx.topk.sample_params).
 * arx_topk_gumbel_add: logits[r * ld + c] = fmaf(tau, g(r % tau_rows, col0 + c), logits[r * ld + c]) in place for
 * c < ncols, r < M; a row of tau == 0 is not touched.  M == 0 or ncols == 0 is a no-op; col0 >= 0,
 * col0 + ncols < 2^31; strided views.
 * arx_topk_gumbel_strip: after the select, the winners' keys back into the model's scores:
 * values[r * ldv + j] = fmaf(-tau, g(r % tau_rows, indices[r * ldi + j]), values[r * ldv + j]), -inf where the index
 * is < 0.  Exact for tau == 0; otherwise within 2^-23 (|key| + |score|) of the score (one rounding at the key, one at
 * the difference; the product inside fmaf is exact).
 * arx_gemm_nt_topk_filter_sample: arx_gemm_nt_topk_filter_tags whose survivor test, stored cand_v and thr are all
 * KEYS (the noise column is col_base + column); lse_part stays over the raw logits.  The exclusion lists (row_keys,
 * ex_ptr, ex_cols) and the tag arrays (col_tags, want_any, want_all) are each optional as a group: all NULL = none.
 * tau_rows > 0. */
int arx_topk_gumbel_add(float* logits, int64_t ld, int64_t M, int32_t col0, int64_t ncols, const float* tau,
                        int64_t tau_rows, const int32_t* seed_words, void* stream);
int arx_topk_gumbel_strip(float* values, int64_t ldv, const int32_t* indices, int64_t ldi, int64_t B, int k,
                          const float* tau, int64_t tau_rows, const int32_t* seed_words, void* stream);
int arx_gemm_nt_topk_filter_sample(const float* A, int64_t lda, int64_t M, const float* Bm, int64_t ldb, int64_t N,
                                   int64_t K, const float* col_bias, const float* thr, int64_t ldthr, int32_t col_base,
                                   float* cand_v, int32_t* cand_i, int64_t ldcand, int capp, int* overflow,
                                   float* lse_part, int64_t ldl, const int32_t* row_keys, int64_t key_rows,
                                   const int32_t* ex_ptr, const int32_t* ex_cols, const int32_t* col_tags,
                                   const int32_t* want_any, const int32_t* want_all, int64_t want_rows, const float* tau,
                                   int64_t tau_rows, const int32_t* seed_words, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ARX_SAMPLE_H_ */

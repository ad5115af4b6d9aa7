/* arx_explain.h -- explain_items: the score of a (row, item) pair taken apart into the contributions of the item's
 * output features and of the single tokens of its bags.  Included by arx.h (include that); bound by EXPLAIN_PROTOTYPES
 * in arx/_lib.py.  The conventions are arx.h's: the function returns 0 or a negative ARX_E* code with the message
 * through arx_last_error, validates every argument before its first HIP call, and launches on `stream`. */
#ifndef ARX_EXPLAIN_H_
#define ARX_EXPLAIN_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define ARX_EXPLAIN_CAT 0        /* kind[f]: a one-hot feature, row cat_map[f][c] (cat_map[f] NULL: row c) of E[f] */
#define ARX_EXPLAIN_MULHOT 1     /* kind[f]: a bag, rows vals[f][starts[f][c] .. + lens[f][c]) of E[f] */
#define ARX_EXPLAIN_MAX_FEATS 8
#define ARX_EXPLAIN_MAX_TOP 16

/* Build-defined (the reference never takes a score apart).
 * arx_explain_slate: an item's latent is the mean over its F output features of an id row or a bag mean, so the score
 * of row r of U [B, d] for the item c = cand[r * ldc + j] is an exact sum of parts:
 *     score(r, c) = 1/F * sum_f s_f(r, c)
 *     cat feature f:     s_f = u_r . E_f[m_f(c)] + b_f[m_f(c)]
 *     mulhot feature f:  s_f = 1/len_f(c) * sum_t ( u_r . E_f[v_{f,c,t}] + b_f[v_{f,c,t}] )
 * One launch, no workspace, no atomics, graph-capturable.  [B, C, len, d] is never materialised.
 *
 * INPUTS.  U [B, d], row stride ldu.  cand [B, C] int32 logit columns, row stride ldc; a column < 0 or >= V is an EMPTY
 * slot (what arx_slate_scores calls one) and nothing is read for it.  F feature descriptors, 1 <= F <= 8, as HOST
 * arrays of F entries each: kind[f] (ARX_EXPLAIN_CAT / ARX_EXPLAIN_MULHOT), the table E[f] with row stride lde[f], its
 * bias fbias[f] (the array or an entry may be NULL: no bias, b_f = 0), and cat_map[f] (NULL: the identity) or vals[f],
 * starts[f], lens[f].  Every map is indexed by logit column and holds V entries; the arrays of the kind a feature is
 * not are not looked at.  The maps live on the device: the rows they name are read unchecked, as in the gather
 * kernels.  A bag of length 0 is outside the contract (the preprocessing never writes one).
 *
 * OUTPUTS, each nullable; tok_val, tok_id and tok_feat are NULL together, and must be NULL when T == 0.
 *     feat    [B, C, F] f32 at feat[r * ldf + j * F + f]:  1/F * s_f, bias included; ldf >= C * F
 *     bias    [B, C]    f32 at bias[r * ldb + j]:          1/F * sum_f of the bias part of s_f alone; ldb >= C
 *     tok_val / tok_id / tok_feat [B, C, T] at [r * ldt + j * T + t], 0 <= T <= 16, ldt >= C * T: the T largest token
 *         contributions 1/(F * len) * (u . E_f[v] + b_f[v]) over all bag positions of all mulhot features of the item,
 *         by (value desc, feature index asc, bag position asc).  Every bag position is an entry of its own: a token
 *         that stands twice in a bag appears twice.  tok_id is the row of E_f, tok_feat is f.  (-inf, -1, -1) past the
 *         last entry.  A NaN contribution never enters.
 * An empty slot gives feat = 0, bias = 0 and (-inf, -1, -1) in all T places.
 *
 * ORDER OF THE ADDS.  A group of L lanes (L the smallest power of two >= d / 4) owns one (row, slot) pair.  Every
 * u . E_f[row] is arx_slate_scores' dot: lane i multiplies elements 4i .. 4i + 3 and adds them in that order (one
 * multiply, three fused multiply-adds), the group folds by xor shuffles 1, 2, 4, ... L / 2.  Then, in float32:
 *     cat:     feat = (dot + b) * invF,                                   invF = 1.0f / (float)F
 *     mulhot:  x_t = dot_t + b_t;  the contribution of position t is x_t * coef,   coef = 1.0f / ((float)F * (float)len)
 *              feat = (((x_0 + x_1) + x_2) + ...) * coef     -- a running sum in bag order, starting from x_0
 *     bias  = sum over f in index order, starting from 0, of b * invF (cat) or (((b_0 + b_1) + ...) * coef) (mulhot)
 * That order depends on d, F and the item's bags ONLY -- not on the slot, C, B, the leading dimensions or the grid:
 * a (row, item) pair yields the same bits wherever it stands in a slate and whatever B and C are.
 * THE GRID IS NOT CAPPED: one group per (row, slot) pair, ceil(B * C / (64 / L)) waves in blocks of four, no loop
 * over pairs (B * C < 2^31 keeps the block count below 2^29).
 *
 * ENVELOPE.  d % 4 == 0 and 4 <= d <= 256, else ARX_EUNSUPPORTED (the widths arx_slate_scores serves).  Everything else
 * that is malformed is ARX_EINVAL: F outside [1, 8]; T outside [0, 16]; a kind that is neither; ldu, lde[f] multiples
 * of 4 and >= d; U and every E[f] 16-byte aligned; a NULL U, cand, kind, E, lde or E[f]; a mulhot feature without
 * vals / starts / lens; tok_* partly NULL, or set while T == 0 (all three NULL is legal for any T: the top T is then
 * not formed); ldc < C, ldf < C * F, ldb < C, ldt < C * T; B, C < 0; V outside [0, 2^31); B * C >= 2^31.  B == 0 or
 * C == 0 is legal and launches nothing.  Outputs are untouched on an error. */
int arx_explain_slate(const float* U, int64_t ldu, int64_t B, int d, const int32_t* cand, int64_t ldc, int64_t C,
                      int64_t V, int F, const int* kind, const float* const* E, const int64_t* lde,
                      const float* const* fbias, const int32_t* const* cat_map, const int32_t* const* vals,
                      const int32_t* const* starts, const int32_t* const* lens, int T, float* feat, int64_t ldf,
                      float* bias, int64_t ldb, float* tok_val, int32_t* tok_id, int32_t* tok_feat, int64_t ldt,
                      void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ARX_EXPLAIN_H_ */

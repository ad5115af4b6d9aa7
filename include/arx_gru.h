/* arx_gru.h -- GRU sequence encoder: SeqModel(cell='gru').  Included by arx.h (include that); bound by GRU_PROTOTYPES
 * in arx/_lib.py.  The conventions are arx.h's: a function returns 0 or a negative ARX_E* code with the message through
 * arx_last_error, validates every argument before its first HIP call, and launches on `stream`. */
#ifndef ARX_GRU_H_
#define ARX_GRU_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* Build-defined (the reference has the LSTM cell only).  tf.contrib.rnn.GRUCell(h) of TF 1.0 under static_rnn over L
 * steps from the zero state -- the reset gate is applied BEFORE the candidate's product (not cuDNN's form):
 *     [r | u] = sigmoid([x_t, h_{t-1}] . Wg + bg)       Wg [din + h, 2h], bg [2h]; columns: r first, then u
 *     c       = tanh([x_t, r * h_{t-1}] . Wc + bc)      Wc [din + h, h],  bc [h]
 *     h_t     = u * h_{t-1} + (1 - u) * c
 * x: [L, B, din] time-major.  hs: [L, B, h] outputs; gates: [L, B, 3h] post-activation (r, u, c) and
 * rh: [L, B, h] = r * h_{t-1} (the A operand of the caller's dWc product) are saved for backward.
 *
 * Three kernel pairs, chosen by (din, h) alone and the same way forward and backward: din == h == 64 weights held in
 * registers; h in {64, 128} with din % 4 == 0 weights streamed as MFMA operands (both: 16 batch rows per workgroup;
 * rows >= B of a tail tile are read as zeros and never written); anything else one workgroup per batch row.
 * ARX_EINVAL ahead of any launch: a NULL pointer, din <= 0, h <= 0, L < 0, B < 0, or dynamic LDS past 160 KB
 * (streamed: 4 * 16 * (2 * (din + 2) + 3 * (h + 2)) bytes; per-row: 4 * (din + 4h) forward, 4 * 5h backward).
 * L == 0 or B == 0 is legal, launches nothing and writes nothing. */
int arx_gru_fwd(const float* x, const float* Wg, const float* bg, const float* Wc, const float* bc, int64_t L,
                int64_t B, int din, int h, float* hs, float* gates, float* rh, void* stream);
/* dhs: [L, B, h] upstream gradient of every output.  Produces the pre-activation gradients of the whole unrolled
 * cell (BPTT through h), as two plain arrays so that the caller's GEMMs never read a column slice:
 *     du = dh * (h_prev - c)      dc = dh * (1 - u)        dzc = dc * (1 - c^2)
 *     q  = dzc . Wc[din:]^T       dr = q * h_prev
 *     dzr = dr * r * (1 - r)      dzu = du * u * (1 - u)
 *     dh_prev = dh * u + q * r + [dzr | dzu] . Wg[din:]^T
 * dzg: [L, B, 2h] (dzr, dzu); dzc: [L, B, h].  dx, dWg, dbg, dWc, dbc are then GEMMs / column sums the caller
 * issues (arx_gemm_f32: dx = dzg . Wg[:din]^T + dzc . Wc[:din]^T; dWg = [x | h_prev]^T . dzg; dWc = [x | rh]^T . dzc). */
int arx_gru_bwd(const float* Wg, const float* Wc, const float* hs, const float* gates, const float* dhs, int64_t L,
                int64_t B, int din, int h, float* dzg, float* dzc, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ARX_GRU_H_ */

// gemm_nt.hip -- the scorer GEMM  logits[M,N] = U[M,K] . I[N,K]^T + b[N]  for K = d <= 128
// (embed_attribute.py:171,188-193: tf.matmul(user, item_pool, transpose_b=True) + bias).
//
// K is the embedding width (32..128), so a generic K-loop kernel spends most of its time
// in prologue / epilogue: at M=16384, N=1024, K=128 the tiled kernel in gemm.hip reaches
// 59 TF (37% of the fp32 MFMA peak).  Here the whole K extent of the A operand lives in
// REGISTERS for the lifetime of a workgroup:
//   * a workgroup owns 128 rows of U (4 waves x 32 rows) and a range of item-pool tiles;
//   * each lane keeps its row's K/2 values in K/8 float4 registers, laid out so that one
//     16-byte LDS read of the B operand feeds four v_mfma_f32_32x32x2_f32 (the k index a
//     lane supplies is arbitrary as long as A and B agree: lane l holds k = 8s + 4*(l/32) + j
//     for MFMA j of step s);
//   * pool tiles (64 items x K) stream into a double-buffered LDS image by LDS-DMA
//     (global_load_lds_dwordx4: no staging registers, no ds_write pass, and -- unlike
//     register-staged loads, which hipcc drained with s_waitcnt vmcnt(0) AHEAD of the MFMA
//     block because the accumulators wanted the same registers -- the copy of tile t+1
//     stays in flight while tile t is multiplied);
//   * the DMA writes lane-linear (wave base + 16 B x lane), so the image is unpadded and
//     bank conflicts are avoided by an XOR swizzle applied to the SOURCE chunk index and
//     again on the ds_read_b128 side: 16 B chunk c of pool row r lives at slot c ^ swz(r);
//   * 64 KB of LDS and ~200 VGPRs => two workgroups per CU.
#include "common.h"
#include "gumbel.h"
#include "rest_mass.h"

namespace arx {

typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

constexpr int kNtBM = 128;   // rows per workgroup
constexpr int kNtBN = 64;    // pool rows (output columns) per tile

template <int KT>
__device__ __forceinline__ int nt_swz(int r) {
  // chunks per row: 32 (K=128), 16 (K=64): 16 consecutive rows must hit 16 distinct 16-B
  // slots of the 256-B bank row; 8 (K=32): rows are 128 B, pairs of rows share a bank row.
  return (KT >= 64) ? (r & 15) : ((r >> 1) & 7);
}

// FILTER (round 5, the recommend path: hmf_model.py:154 tf.nn.top_k over the FULL vocabulary): no C.  A logit leaves
// the kernel only if it beats its row's threshold thr[row] (the k-th best of the columns scored so far): it is appended
// to the row's candidate segment of this workgroup's column range, cand[row][part * capp ..), in ascending column
// order -- a wave owns its 32 rows, keeps their 16 + 16 counters in registers and places a tile's survivors by ballot
// + prefix count, so the lists are deterministic, need no atomics, and POSITION order is COLUMN order (what
// arx_topk_chunk's tie rule needs).  A full segment raises *overflow (the caller falls back to the chunked path).
// lse_part (nullable): also the log-sum-exp of the row's logits over the workgroup's column range, lse_part[row * ldl +
// part] -- the softmax normaliser of seqModel.py:514-517 top_k(softmax(logits)) without the logits: every lane keeps a
// running (max, sum exp(v - max)) per row over ITS columns, the 32 lanes of a row meet once at the end.
struct NtFilter {
  const float* thr; int64_t ldthr;
  float* cand_v; int32_t* cand_i; int64_t ldcand;
  int capp; int32_t col_base;
  int* overflow;
  float* lse_part; int64_t ldl;
  // the evaluation losses of a sampled-loss model over the FULL vocabulary (hmf_model.py:130,144, seqModel.py:510)
  // without the logits: relu_part[row * ldl + part] = sum over the range of relu(v - tsc[row] + 1) (WMRB, :605-618);
  // thr == nullptr: no candidate lists at all (arx_gemm_nt_eval_parts)
  const float* tsc; float* relu_part;
  // kNtExcl (the recommend path with each user's seen items left out): row r's excluded ABSOLUTE columns are
  // ex_cols[ex_ptr[key] .. ex_ptr[key + 1]), sorted ascending, key = row_keys[r % key_rows] (< 0: nothing excluded)
  const int32_t* row_keys; int64_t key_rows;
  const int32_t* ex_ptr; const int32_t* ex_cols;
  // kNtRank (with kNtRelu: warp_eval, embed_attribute.py:620-639 [margin_rank, true_rank]): tsc[row] is t itself, the
  // margin term is relu((v - t) + 1) and cnt_part[row * ldl + part] = #columns of the range with v > t; the row's own
  // target column tcol[row] (a column of this launch, anything else: none) counts as (1, 0)
  // kNtSelf (with kNtCos: the item-to-item scan) reads tcol too: the row's own ABSOLUTE column col_base + col (anything
  // outside the launch's columns: none), dropped before it takes a position in the row's list
  const int32_t* tcol; int32_t* cnt_part;
  // kNtTags (the recommend path within item tags): column c of this launch carries the 32 tag bits col_tags[c], row r
  // the two words want_any / want_all [r % want_rows]; c is eligible for r iff
  // (any == 0 || (tags & any) != 0) && (tags & all) == all -- a zero word is no constraint
  const int32_t* col_tags; const int32_t* want_any; const int32_t* want_all; int64_t want_rows;
  // kNtGumbel (the sampled recommend, gumbel.h): row r competes with the KEYS fmaf(tau, g, v), tau = tau[r % tau_rows],
  // g the noise of (seed_words, noise row, noise column); thr and cand_v are keys, lse_part stays over v.  The noise
  // row is noise_rows[r % tau_rows] (nullptr: r % tau_rows; negative: the row competes as a tau == 0 row), the noise
  // column col * noise_mul + noise_add (unsigned, wrapping), noise_add = col_base * col_mul + col_add formed on the host
  // and added to the row word b0 in the prologue (kNtKeyed, arx_sample_shard.h); without that bit the plain convention
  // of arx_sample.h: noise row r % tau_rows, noise column col_base + col
  const float* tau; int64_t tau_rows; const int32_t* seed_words;
  const int32_t* noise_rows; uint32_t noise_mul, noise_add;
  // kNtRest (the mass pass of the sampled recommend's propensities, arx_sample_logp.h): row r's picks sorted by
  // ABSOLUTE column, pk_cols[r * ldp + j] with the selection slot pk_slot[r * ldp + j] beside it, j < pk_k (-1 entries
  // last); per column range REST's pair (m_part, s_part)[row * ldl + part], and pick_score[row * ldps + slot] = the
  // score of a pick's column.  Reads tau, the exclusion lists and the tag arrays above (each group nullable)
  const int32_t* pk_cols; const int32_t* pk_slot; int64_t ldp; int pk_k;
  float* m_part; float* s_part; float* pick_score; int64_t ldps;
};

// MODE (FILTER kernels): bit 0 candidate lists (thr), bit 1 lse_part, bit 2 relu_part, bit 3 exclusion lists (with
// bit 0 only), bit 4 rank counts (with bit 2 only) -- a template parameter, not a run-time switch: every feature is 32
// registers of per-row state and the plain kernel already holds 246.  bit 5 cosine (with bit 0 alone, or bit 0 and
// bit 6): v = acc * col_scale[col], the scale travelling where the bias does; bit 6 the row's self column (with bit 5);
// bit 7 item tags (with bit 0, optionally bits 1 and 3): the eligibility test of NtFilter::col_tags on a survivor -- the
// column's tag word is loaded from global memory THERE, not carried per lane beside the bias: two more registers per
// lane for every tile would not fit under the 256 the two workgroups per CU leave (the plain filter holds 246)
// bit 8 Gumbel keys (with bit 0, optionally bits 1, 3 and 7): every logit's hash and a logarithm-free upper bound of
// its key (gumbel_upper) are computed; the two accurate logarithms only where a lane of the wave may pass.  The row's
// (tau, b0, b1, thr) come from LDS per logit (one 16-byte read, two addresses per wave): 48 more registers would not
// fit, and the 16 of the thresholds are given back
constexpr int kNtTopk = 1, kNtLse = 2, kNtRelu = 4, kNtExcl = 8, kNtRank = 16, kNtCos = 32, kNtSelf = 64, kNtTags = 128;
constexpr int kNtGumbel = 256;
// bit 10 (with bit 8) the keyed noise of arx_sample_shard.h: the noise row comes from NtFilter::noise_rows and the noise
// column is col * noise_mul + noise_add.  A mode bit like every other feature of this body, not a run-time operand of
// the plain Gumbel instances: with the multiply in them the K = 128 instance of bits 0 + 8 went from 200 to 248 bytes of
// scratch per lane and the un-keyed sampled scan from 18.8 to 20.2 ms (4096 x 1 M x 128) -- with
// the bit off the instances are the ones they were, instruction for instruction
constexpr int kNtKeyed = 1024;
// bit 9 (alone) REST's mass per column range, an eval-style scan without candidate lists: the 32 registers of the lse
// mode hold each row's (m, S) at ITS temperature, the column's tag word travels beside the bias (no lists: there are
// registers for it), and the two sorted lists a row leaves out -- its exclusion list and its picks -- are walked by
// cursors: lane (list = lane / 32, row = lane % 32) of a wave keeps the next listed column of its row in a register,
// and only a tile that holds one for some row of the wave takes the compare path (rows' next columns by ds_bpermute)
constexpr int kNtRest = 512;

template <int KT, int MODE = 0>
__global__ __launch_bounds__(256, 2) void k_gemm_nt_areg(
    int64_t M, int64_t N, const float* __restrict__ A, int64_t lda, const float* __restrict__ B,
    int64_t ldb, float alpha, float* __restrict__ C, int64_t ldc,
    const float* __restrict__ col_bias, int tiles_per_block, int nsplit, NtFilter flt) {
  constexpr bool FILTER = MODE != 0;
  constexpr bool want_topk = (MODE & kNtTopk) != 0, want_lse = (MODE & kNtLse) != 0, want_relu = (MODE & kNtRelu) != 0;
  constexpr bool want_excl = (MODE & kNtExcl) != 0, want_rank = (MODE & kNtRank) != 0;
  static_assert(!want_excl || want_topk, "the exclusion lists filter candidates");
  static_assert(!want_rank || (want_relu && !want_topk && !want_lse), "the rank counts ride on the margin sums");
  constexpr bool want_cos = (MODE & kNtCos) != 0, want_self = (MODE & kNtSelf) != 0;
  static_assert(!want_cos || (want_topk && !want_lse && !want_relu && !want_excl), "the cosine scale serves the lists");
  static_assert(!want_self || want_cos, "the self column belongs to the item-to-item scan");
  constexpr bool want_tags = (MODE & kNtTags) != 0;
  static_assert(!want_tags || (want_topk && !want_relu && !want_cos), "the item tags filter the recommend candidates");
  constexpr bool want_gumbel = (MODE & kNtGumbel) != 0;
  static_assert(!want_gumbel || (want_topk && !want_relu && !want_cos), "the Gumbel keys rank the recommend candidates");
  constexpr bool want_keyed = (MODE & kNtKeyed) != 0;
  static_assert(!want_keyed || want_gumbel, "the keyed noise belongs to the Gumbel keys");
  constexpr bool want_rest = (MODE & kNtRest) != 0;
  static_assert(!want_rest || MODE == kNtRest, "the mass pass is a scan of its own");
  constexpr int NS = KT / 8;                  // steps of 4 MFMAs
  constexpr int CPR = KT / 4;                 // 16-B chunks per pool row
  constexpr int NLB = kNtBN * CPR / 256;      // DMA pieces per thread per tile
  static_assert(NLB >= 1, "tile too small");
  // two separate arrays (not sB[2][..]): the compiler must see that the DMA destination and
  // the buffer being read never alias, or it drains the DMA (vmcnt(0)) before the first ds_read
  __shared__ __attribute__((aligned(1024))) float sB0[kNtBN * KT];
  __shared__ __attribute__((aligned(1024))) float sB1[kNtBN * KT];

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l31 = lane & 31, lhi = lane >> 5;
  // XCD-aware order: the nsplit blocks that share one A panel get consecutive ids on one XCD
  int bid = blockIdx.x;
  {
    const int nblk = gridDim.x;
    const int q = nblk / 8, r = nblk % 8, xcd = bid % 8, loc = bid / 8;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc;
  }
  const int panel = bid / nsplit, part = bid % nsplit;
  const int64_t m0 = (int64_t)panel * kNtBM;
  const int64_t tiles_n = ceil_div(N, (int64_t)kNtBN);
  const int64_t t_beg = (int64_t)part * tiles_per_block;
  const int64_t t_end = min(tiles_n, t_beg + tiles_per_block);
  if (t_beg >= t_end) return;

  // LDS-DMA of one pool tile: piece f = threadIdx.x + 256 i lands at chunk f of the image;
  // it fetches chunk (f % CPR) ^ swz(row) of pool row n0 + f / CPR (rows past N clamped:
  // their columns are never stored).
  auto dma_b = [&](int64_t t, float* img) {
    const int64_t n0 = t * kNtBN;
#pragma unroll
    for (int i = 0; i < NLB; ++i) {
      const int f = threadIdx.x + i * 256;
      const int r = f / CPR, slot = f % CPR;
      const int c = slot ^ nt_swz<KT>(r);
      const int64_t gr = min(n0 + r, N - 1);
      const float* src = B + gr * ldb + c * 4;
      float* dst = img + (f - lane) * 4;           // wave-uniform base; HW adds 16 B x lane
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                       (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
    }
  };

  dma_b(t_beg, sB0);

  // ---- A operand: this lane's row, k = 8s + 4*lhi + {0..3} ----
  float4 a[NS];
  {
    const int64_t row = m0 + wave * 32 + l31;
    const bool ok = row < M;
    const float* ap = A + (ok ? row : 0) * lda + 4 * lhi;
#pragma unroll
    for (int s = 0; s < NS; ++s) a[s] = *reinterpret_cast<const float4*>(ap + 8 * s);
    if (!ok) {
#pragma unroll
      for (int s = 0; s < NS; ++s) a[s] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
  // FILTER: thresholds and list lengths of the lane's 16 rows (row = rbase + (e & 3) + 8 (e >> 2))
  // per-row CONSTANTS (thresholds, target scores) and the list lengths live in LDS -- read four rows at a time per
  // tile, the lengths only when a tile has a survivor; only the running sums are registers (the plain kernel holds
  // 246 VGPRs: with everything in registers the top-k form spilled 476 bytes per lane)
  __shared__ float s_th[want_topk ? kNtBM : 1];
  __shared__ float s_tq[want_relu ? kNtBM : 1];
  __shared__ int s_cnt[want_topk ? kNtBM : 1];
  // kNtExcl: [beg, end) of each row's exclusion list (1 KB; read only by a lane whose logit beat the threshold)
  __shared__ int s_xb[want_excl ? kNtBM : 1], s_xe[want_excl ? kNtBM : 1];
  // kNtTags: each row's two request words (1 KB; read only by a lane whose logit beat the threshold)
  __shared__ uint32_t s_wa[want_tags ? kNtBM : 1], s_wl[want_tags ? kNtBM : 1];
  // kNtGumbel: each row's (tau, b0, b1, thr) (2 KB; read per logit, 16 bytes at two addresses per wave -- the
  // threshold too: th[] below then holds no registers in this mode)
  __shared__ uint4 s_gm[want_gumbel ? kNtBM : 1];
  // kNtRank: the rows' target columns (read per tile by one lane per row, per logit only in a tile that holds one)
  // kNtSelf: the rows' own columns, absolute (read only by a lane whose logit beat the threshold)
  __shared__ int s_tc[(want_rank || want_self) ? kNtBM : 1];
  // kNtRest: each row's tau (> 0: rm_tau), its finite reciprocal and its two request words (2 KB; read four rows at a
  // time per tile)
  __shared__ __attribute__((aligned(16))) float s_rt[want_rest ? kNtBM : 1];
  __shared__ __attribute__((aligned(16))) float s_ri[want_rest ? kNtBM : 1];
  __shared__ __attribute__((aligned(16))) uint32_t s_ra[want_rest ? kNtBM : 1];
  __shared__ __attribute__((aligned(16))) uint32_t s_rl[want_rest ? kNtBM : 1];
  // kNtRest: the masses of the lane's 16 rows; the cursor of the lane's own (list, row): [r_cur, r_end) of r_lp
  // narrowed to this workgroup's columns, r_nxt the next listed column (none: 0xffffffff), r_slot its pick slot
  float rm_m[want_rest ? 16 : 1], rm_s[want_rest ? 16 : 1];
  int r_cur = 0, r_end = 0, r_slot = 0;
  uint32_t r_nxt = 0xffffffffu;
  const int32_t* r_lp = nullptr;
  const int32_t* r_ls = nullptr;
  float lm[want_lse ? 16 : 1], ls[want_lse ? 16 : 1], rsum[want_relu ? 16 : 1];
  // kNtRank: ONE register per count -- a row's count is the popcount of its half of a ballot (wave-uniform), kept by
  // the lane l31 == e of the half (16 counters spilled at K=128: the margin mode already holds 236 VGPRs).  The margin
  // is kept as #active + sum over the active columns of (v - t): summing the terms relu((v - t) + 1) themselves, ~1
  // each where the scores sit close together (an untrained model), a lane's running sum outgrows their fractions
  // (measured: 1e-4 relative at 100 M columns); acnt counts the active columns exactly
  int rcnt = 0, acnt = 0;
  bool ovf = false;
  if (FILTER) {
    if (threadIdx.x < kNtBM) {
      const int64_t row = m0 + threadIdx.x;
      if (want_topk) {
        s_th[threadIdx.x] = row < M ? flt.thr[row * flt.ldthr] : __builtin_inff();
        s_cnt[threadIdx.x] = 0;
      }
      if (want_self) s_tc[threadIdx.x] = row < M ? flt.tcol[row] : -1;
      if (want_relu && !want_rank) s_tq[threadIdx.x] = row < M ? flt.tsc[row] - 1.f : 0.f;
      if (want_rank) {
        s_tq[threadIdx.x] = row < M ? flt.tsc[row] : 0.f;
        s_tc[threadIdx.x] = row < M ? flt.tcol[row] : -1;
      }
      if (want_excl) {
        int xb = 0, xe = 0;
        if (row < M) {
          const int32_t key = flt.row_keys[row % flt.key_rows];
          if (key >= 0) {
            // narrowed to this workgroup's columns [c_lo, c_hi) once here: the survivor searches get shorter
            const int32_t c_lo = flt.col_base + (int32_t)(t_beg * kNtBN);
            const int32_t c_hi = flt.col_base + (int32_t)min(t_end * kNtBN, N);
            int lo = flt.ex_ptr[key], hi = flt.ex_ptr[key + 1];
            xe = hi;
            while (lo < hi) {
              const int mid = (lo + hi) >> 1;
              if (flt.ex_cols[mid] < c_lo) lo = mid + 1;
              else hi = mid;
            }
            xb = lo;
            hi = xe;
            while (lo < hi) {
              const int mid = (lo + hi) >> 1;
              if (flt.ex_cols[mid] < c_hi) lo = mid + 1;
              else hi = mid;
            }
            xe = lo;
          }
        }
        s_xb[threadIdx.x] = xb;
        s_xe[threadIdx.x] = xe;
      }
      if (want_tags) {
        const int64_t wr = row < M ? row % flt.want_rows : 0;
        s_wa[threadIdx.x] = row < M ? (uint32_t)flt.want_any[wr] : 0u;
        s_wl[threadIdx.x] = row < M ? (uint32_t)flt.want_all[wr] : 0u;
      }
      if (want_gumbel && !want_keyed) {
        const int64_t nr = row < M ? row % flt.tau_rows : 0;
        const GumbelRow gr = gumbel_row(flt.seed_words, nr);
        s_gm[threadIdx.x] = make_uint4(__float_as_uint(row < M ? flt.tau[nr] : 0.f), gr.b0, gr.b1,
                                       __float_as_uint(row < M ? flt.thr[row * flt.ldthr] : __builtin_inff()));
      }
      if (want_keyed) {
        // the row words are formed once here; noise_add rides in b0: the column's hash starts with
        // noise column + b0 = col * noise_mul + (noise_add + b0)
        const int64_t tr = row < M ? row % flt.tau_rows : 0;
        const int64_t nr = flt.noise_rows ? (int64_t)flt.noise_rows[tr] : tr;
        const GumbelRow gr = gumbel_row(flt.seed_words, nr);
        s_gm[threadIdx.x] = make_uint4(__float_as_uint(row < M && nr >= 0 ? flt.tau[tr] : 0.f), gr.b0 + flt.noise_add,
                                       gr.b1, __float_as_uint(row < M ? flt.thr[row * flt.ldthr] : __builtin_inff()));
      }
      if (want_rest) {
        const float t = rm_tau(row < M ? flt.tau[row % flt.tau_rows] : 1.f);
        s_rt[threadIdx.x] = t;
        s_ri[threadIdx.x] = rm_itau(t);
        const bool tg = row < M && flt.col_tags != nullptr;
        s_ra[threadIdx.x] = tg ? (uint32_t)flt.want_any[row % flt.want_rows] : 0u;
        s_rl[threadIdx.x] = tg ? (uint32_t)flt.want_all[row % flt.want_rows] : 0u;
      }
    }
    if (want_rest) {
      // lane (lhi, l31): list lhi (0 the exclusion list, 1 the picks) of row wave * 32 + l31, narrowed to this
      // workgroup's columns [c_lo, c_hi) once; columns compare as unsigned (the picks' -1 entries sort last)
      const int64_t row = m0 + wave * 32 + l31;
      const uint32_t c_lo = (uint32_t)flt.col_base + (uint32_t)(t_beg * kNtBN);
      const uint32_t c_hi = (uint32_t)flt.col_base + (uint32_t)min(t_end * kNtBN, N);
      int lo = 0, hi = 0;
      if (row < M) {
        if (lhi) {
          r_lp = flt.pk_cols + row * flt.ldp;
          r_ls = flt.pk_slot + row * flt.ldp;
          hi = flt.pk_k;
        } else if (flt.row_keys) {
          const int32_t key = flt.row_keys[row % flt.key_rows];
          if (key >= 0) {
            r_lp = flt.ex_cols;
            lo = flt.ex_ptr[key];
            hi = flt.ex_ptr[key + 1];
          }
        }
      }
      const int top = hi;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((uint32_t)r_lp[mid] < c_lo) lo = mid + 1;
        else hi = mid;
      }
      r_cur = lo;
      hi = top;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((uint32_t)r_lp[mid] < c_hi) lo = mid + 1;
        else hi = mid;
      }
      r_end = lo;
      if (r_cur < r_end) {
        r_nxt = (uint32_t)r_lp[r_cur];
        if (lhi) r_slot = r_ls[r_cur];
      }
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        rm_m[e] = -__FLT_MAX__;
        rm_s[e] = 0.f;
      }
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      if (want_lse) {
        // the empty state is (-FLT_MAX, 0), not (-inf, 0): a -inf logit (an item switched off by its bias) met in that
        // state gives dd = -inf (ex = 0: it adds nothing) where -inf - -inf would be NaN for good; the first finite
        // logit gives dd = +huge as before, and a range of nothing but -inf ends as -FLT_MAX + log(0) = -inf
        lm[e] = -__FLT_MAX__;
        ls[e] = 0.f;
      }
      if (want_relu) rsum[e] = 0.f;
    }
  }
  // bias of the first tile (later ones are fetched one tile ahead, behind the DMA issue)
  float bias0 = 0.f, bias1 = 0.f;
  if (col_bias) {
    const int64_t c0 = min(t_beg * kNtBN + l31, N - 1), c1 = min(t_beg * kNtBN + 32 + l31, N - 1);
    bias0 = col_bias[c0];
    bias1 = col_bias[c1];
  }
  // kNtRest: the tag words of the tile's two columns, fetched like the bias (0 without tags: every row's words are 0)
  uint32_t tg0 = 0u, tg1 = 0u;
  if (want_rest && flt.col_tags) {
    tg0 = (uint32_t)flt.col_tags[min(t_beg * kNtBN + l31, N - 1)];
    tg1 = (uint32_t)flt.col_tags[min(t_beg * kNtBN + 32 + l31, N - 1)];
  }
  __syncthreads();

  // read-side swizzle: chunk 2s + lhi of pool row (l31 [+32]); swz(l31) == swz(l31 + 32)
  const int sw = nt_swz<KT>(l31);
  auto tile = [&](int64_t t, const float* cur_img, float* nxt_img) {
    float nb0 = 0.f, nb1 = 0.f;
    uint32_t ng0 = 0u, ng1 = 0u;
    if (t + 1 < t_end) {
      if (col_bias) {
        const int64_t c0 = min((t + 1) * kNtBN + l31, N - 1);
        const int64_t c1 = min((t + 1) * kNtBN + 32 + l31, N - 1);
        nb0 = col_bias[c0];
        nb1 = col_bias[c1];
      }
      if (want_rest && flt.col_tags) {
        ng0 = (uint32_t)flt.col_tags[min((t + 1) * kNtBN + l31, N - 1)];
        ng1 = (uint32_t)flt.col_tags[min((t + 1) * kNtBN + 32 + l31, N - 1)];
      }
      dma_b(t + 1, nxt_img);
    }
    f32x16 acc0, acc1;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      acc0[e] = 0.f;
      acc1[e] = 0.f;
    }
    const float* b0p = cur_img + l31 * KT;
    const float* b1p = b0p + 32 * KT;
    // operands of step s+1 are fetched from LDS before the 8 MFMAs of step s issue (an LDS
    // round trip is ~128 cycles; issued right in front of their use they stalled ~20% of the
    // wave's cycles in s_waitcnt lgkmcnt -- PMC SQ_WAIT_ANY)
    float4 b0 = *reinterpret_cast<const float4*>(b0p + ((lhi ^ sw) * 4));
    float4 b1 = *reinterpret_cast<const float4*>(b1p + ((lhi ^ sw) * 4));
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      float4 n0 = b0, n1 = b1;
      if (s + 1 < NS) {
        const int off = ((2 * (s + 1) + lhi) ^ sw) * 4;
        n0 = *reinterpret_cast<const float4*>(b0p + off);
        n1 = *reinterpret_cast<const float4*>(b1p + off);
      }
      __builtin_amdgcn_sched_barrier(0);      // keep the fetch ahead of this step's MFMAs (hipcc sinks it otherwise)
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s].x, b0.x, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s].x, b1.x, acc1, 0, 0, 0);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s].y, b0.y, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s].y, b1.y, acc1, 0, 0, 0);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s].z, b0.z, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s].z, b1.z, acc1, 0, 0, 0);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s].w, b0.w, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s].w, b1.w, acc1, 0, 0, 0);
      b0 = n0;
      b1 = n1;
    }
    // epilogue.  C/D map of the 32x32 MFMA: col = lane&31, row = (e&3) + 8*(e>>2) + 4*(lane>>5)
    const int64_t n0 = t * kNtBN;
    const int64_t rbase = m0 + wave * 32 + 4 * lhi;
    if (want_rest) {
      const int rl0 = wave * 32 + 4 * lhi;
      const uint32_t ct = (uint32_t)flt.col_base + (uint32_t)n0;    // the tile's first ABSOLUTE column
      const uint32_t c0 = ct + (uint32_t)l31, c1 = c0 + 32u;
      // bit 16 j + e: logit (j, e) is a listed column of its row -- it adds no mass.  One trip per listed column a row
      // has in this tile (almost always none, else one): the rows' next columns come from their cursor lanes, the
      // matching lane writes a pick's score, and every cursor that pointed into the tile steps forward
      uint32_t skip = 0u;
      while (__ballot(r_nxt < ct + (uint32_t)kNtBN) != 0ull) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int src = 4 * lhi + (e & 3) + 8 * (e >> 2);         // the logit's row within the wave
          const uint32_t nx = (uint32_t)__shfl((int)r_nxt, src, 64), np = (uint32_t)__shfl((int)r_nxt, src + 32, 64);
          const bool p0 = np == c0, p1 = np == c1;
          if (nx == c0 || p0) skip |= 1u << e;
          if (nx == c1 || p1) skip |= 1u << (16 + e);
          if (__ballot(p0 || p1) != 0ull) {
            const int slot = __shfl(r_slot, src + 32, 64);
            if (p0 || p1) {
              const float v = alpha * (p0 ? acc0[e] : acc1[e]) + (p0 ? bias0 : bias1);
              flt.pick_score[(rbase + (e & 3) + 8 * (e >> 2)) * flt.ldps + slot] = v;
            }
          }
        }
        if (r_nxt < ct + (uint32_t)kNtBN) {
          ++r_cur;
          r_nxt = 0xffffffffu;
          if (r_cur < r_end) {
            r_nxt = (uint32_t)r_lp[r_cur];
            if (lhi) r_slot = r_ls[r_cur];
          }
        }
      }
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const float4 it4 = *reinterpret_cast<const float4*>(&s_ri[rl0 + 8 * g4]);
        const uint4 wa4 = *reinterpret_cast<const uint4*>(&s_ra[rl0 + 8 * g4]);
        const uint4 wl4 = *reinterpret_cast<const uint4*>(&s_rl[rl0 + 8 * g4]);
        const float it[4] = {it4.x, it4.y, it4.z, it4.w};
        const uint32_t wa[4] = {wa4.x, wa4.y, wa4.z, wa4.w}, wl[4] = {wl4.x, wl4.y, wl4.z, wl4.w};
#pragma unroll
        for (int e2 = 0; e2 < 4; ++e2) {
          const int e = 4 * g4 + e2;
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            const int64_t col = n0 + j * 32 + l31;
            const uint32_t tg = (j == 0) ? tg0 : tg1;
            const float v = alpha * (j == 0 ? acc0[e] : acc1[e]) + ((j == 0) ? bias0 : bias1);
            const bool ok = col < N && ((skip >> (16 * j + e)) & 1u) == 0u && (wa[e2] == 0u || (tg & wa[e2]) != 0u) &&
                            (tg & wl[e2]) == wl[e2];
            rm_add(rm_m[e], rm_s[e], ok ? v : -__builtin_inff(), it[e2]);
          }
        }
      }
    } else if (FILTER) {
      const int rl0 = wave * 32 + 4 * lhi;                          // the lane's rows: rl0 + (e & 3) + 8 (e >> 2)
      float th[want_topk ? 16 : 1], tq[want_relu ? 16 : 1];
      // kNtRank: does a row of this wave have its target column in this tile?  (wave-uniform; rarely true)
      bool tc_hit = false;
      if (want_rank) {
        const int tc = s_tc[wave * 32 + l31];
        tc_hit = __ballot(tc >= n0 && tc < n0 + kNtBN) != 0ull;
      }
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        if (want_topk) {
          const float4 t4 = *reinterpret_cast<const float4*>(&s_th[rl0 + 8 * g4]);
          th[4 * g4] = t4.x; th[4 * g4 + 1] = t4.y; th[4 * g4 + 2] = t4.z; th[4 * g4 + 3] = t4.w;
        }
        if (want_relu) {
          const float4 t4 = *reinterpret_cast<const float4*>(&s_tq[rl0 + 8 * g4]);
          tq[4 * g4] = t4.x; tq[4 * g4 + 1] = t4.y; tq[4 * g4 + 2] = t4.z; tq[4 * g4 + 3] = t4.w;
        }
      }
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int64_t col = n0 + j * 32 + l31;
        const float bias = (j == 0) ? bias0 : bias1;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          // kNtCos: `bias` is the column's 1 / norm; + 0.f turns a product -0 (a zero column under a negative dot)
          // into +0, so a cosine 0 has ONE bit pattern and ties on it break by column like any other
          const float v = want_cos ? (j == 0 ? acc0[e] : acc1[e]) * bias + 0.f
                                   : alpha * (j == 0 ? acc0[e] : acc1[e]) + bias;
          if (want_rank) {
            float dz = v - tq[e];
            bool act = dz + 1.f > 0.f, gt = v > tq[e];
            if (tc_hit && col == s_tc[rl0 + (e & 3) + 8 * (e >> 2)]) {   // the target itself: (1, 0)
              dz = 0.f;
              act = true;
              gt = false;
            }
            act = act && col < N;
            if (act) rsum[e] += dz;
            const unsigned long long m = __ballot(gt && col < N), ma = __ballot(act);
            const int c = __popc(lhi ? (uint32_t)(m >> 32) : (uint32_t)m);
            const int ca = __popc(lhi ? (uint32_t)(ma >> 32) : (uint32_t)ma);
            if (l31 == e) {
              rcnt += c;
              acnt += ca;
            }
            continue;
          }
          if (want_relu && col < N) rsum[e] += fmaxf(v - tq[e], 0.f);
          if (want_lse && col < N) {                                // online (max, sum): ONE exp per logit
            const float dd = v - lm[e];
            const float ex = __expf(-fabsf(dd));                    // (first logit: dd ~ FLT_MAX, ex = 0: ls = 0 * 0 + 1)
            ls[e] = dd > 0.f ? ls[e] * ex + 1.f : ls[e] + ex;
            lm[e] = fmaxf(lm[e], v);
          }
          if (!want_topk) continue;
          bool pred = col < N && v > th[e];
          const int rl = rl0 + (e & 3) + 8 * (e >> 2);
          float key = v;
          if (want_gumbel) {
            // g <= gumbel_upper and fmaf is monotone in g (tau >= 0): a logit whose bound fails cannot pass, and the
            // logarithms run only in a wave where some lane's bound passes (tau == 0: key == v bit for bit)
            const uint4 gm = s_gm[rl];
            const float tau = __uint_as_float(gm.x);
            const uint32_t x = want_keyed ? gumbel_bits(gm.y, gm.z, (uint32_t)col * flt.noise_mul)
                                          : gumbel_bits(gm.y, gm.z, (uint32_t)flt.col_base + (uint32_t)col);
            const float thk = __uint_as_float(gm.w);
            pred = col < N && fmaf(tau, gumbel_upper(x), v) > thk;
            if (__ballot(pred) == 0ull) continue;
            if (pred) {
              key = fmaf(tau, gumbel_of_bits(x), v);
              pred = key > thk;
            }
          }
          // the row's own column (a survivor: rare) leaves BEFORE the ballot, as an excluded one does
          if (want_self && pred && flt.col_base + (int32_t)col == s_tc[rl]) pred = false;
          if (want_tags && pred) {
            // a survivor (rare): its column's tag word comes from global memory here, BEFORE the ballot, so an
            // ineligible column takes no position; a row of two zero words loads nothing
            const uint32_t wa = s_wa[rl], wl = s_wl[rl];
            if ((wa | wl) != 0u) {
              const uint32_t tg = (uint32_t)flt.col_tags[col];
              if ((wa != 0u && (tg & wa) == 0u) || (tg & wl) != wl) pred = false;
            }
          }
          if (want_excl && pred) {
            // a survivor (rare): lower_bound of its absolute column in the row's list, BEFORE the ballot, so an
            // excluded column takes no position and the placement stays deterministic
            const int32_t c = flt.col_base + (int32_t)col;
            const int xe = s_xe[rl];
            int lo = s_xb[rl], hi = xe;
            while (lo < hi) {
              const int mid = (lo + hi) >> 1;
              if (flt.ex_cols[mid] < c) lo = mid + 1;
              else hi = mid;
            }
            if (lo < xe && flt.ex_cols[lo] == c) pred = false;
          }
          const unsigned long long m = __ballot(pred);
          if (m == 0ull) continue;                                  // (the common case by far)
          const uint32_t mh = lhi ? (uint32_t)(m >> 32) : (uint32_t)m;
          // (the wave owns its rows: no other writer.  volatile: lane l31 == 0 stores the new length, the other lanes of
          // the half read it in the next (j, e) iteration -- a plain access would let the compiler carry a lane's
          // earlier load across a store that lane did not execute; advisor, round 5)
          const int c0 = *const_cast<volatile int*>(&s_cnt[rl]);
          const int pos = c0 + __popc(mh & ((1u << l31) - 1u));
          if (pred) {
            if (pos < flt.capp) {
              const int64_t at = (rbase + (e & 3) + 8 * (e >> 2)) * flt.ldcand + (int64_t)part * flt.capp + pos;
              flt.cand_v[at] = key;
              flt.cand_i[at] = flt.col_base + (int32_t)col;
            } else {
              ovf = true;
            }
          }
          if (l31 == 0 && mh) *const_cast<volatile int*>(&s_cnt[rl]) = c0 + __popc(mh);
        }
      }
    } else
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int64_t col = n0 + j * 32 + l31;
      if (col < N) {
        const float bias = (j == 0) ? bias0 : bias1;
        float* cp = C + rbase * ldc + col;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int ro = (e & 3) + 8 * (e >> 2);
          if (rbase + ro < M)
            __builtin_nontemporal_store(alpha * (j == 0 ? acc0[e] : acc1[e]) + bias, cp + (int64_t)ro * ldc);
        }
      }
    }
    bias0 = nb0;
    bias1 = nb1;
    if (want_rest) {
      tg0 = ng0;
      tg1 = ng1;
    }
    __syncthreads();          // tile t+1 landed (vmcnt(0) rides on the barrier); buffer cur free
  };
  for (int64_t t = t_beg; t < t_end; t += 2) {
    tile(t, sB0, sB1);
    if (t + 1 < t_end) tile(t + 1, sB1, sB0);
  }
  if (want_rest) {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int ro = (e & 3) + 8 * (e >> 2);
      const float t = s_rt[wave * 32 + 4 * lhi + ro];
      RmMass x{rm_m[e], rm_s[e]};
#pragma unroll
      for (int o = 16; o > 0; o >>= 1)                              // the row's 32 lanes (one half wave)
        x = rm_join(x, RmMass{__shfl_xor(x.m, o, 64), __shfl_xor(x.s, o, 64)}, t);
      const int64_t row = m0 + wave * 32 + 4 * lhi + ro;
      if (l31 == 0 && row < M) {
        flt.m_part[row * flt.ldl + part] = x.m;
        flt.s_part[row * flt.ldl + part] = x.s;
      }
    }
  }
  if (want_topk && ovf) *flt.overflow = 1;
  if (want_lse) {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      float mx = lm[e], sm = ls[e];
#pragma unroll
      for (int o = 16; o > 0; o >>= 1) {                            // the row's 32 lanes (one half wave)
        const float m2 = __shfl_xor(mx, o, 64), s2 = __shfl_xor(sm, o, 64);
        const float mn = fmaxf(mx, m2);
        sm = (mx == -__builtin_inff() ? 0.f : sm * __expf(mx - mn)) + (m2 == -__builtin_inff() ? 0.f : s2 * __expf(m2 - mn));
        mx = mn;
      }
      const int64_t row = m0 + wave * 32 + 4 * lhi + (e & 3) + 8 * (e >> 2);
      if (l31 == 0 && row < M) flt.lse_part[row * flt.ldl + part] = mx + __logf(sm);
    }
  }
  if (want_relu) {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      float sm = rsum[e];
#pragma unroll
      for (int o = 16; o > 0; o >>= 1) sm += __shfl_xor(sm, o, 64);
      const int64_t row = m0 + wave * 32 + 4 * lhi + (e & 3) + 8 * (e >> 2);
      if (want_rank) {
        if (l31 == e && row < M) flt.relu_part[row * flt.ldl + part] = (float)acnt + sm;
      } else if (l31 == 0 && row < M) {
        flt.relu_part[row * flt.ldl + part] = sm;
      }
    }
  }
  if (want_rank) {
    const int64_t row = m0 + wave * 32 + 4 * lhi + (l31 & 3) + 8 * (l31 >> 2);
    if (l31 < 16 && row < M) flt.cnt_part[row * flt.ldl + part] = rcnt;
  }
}

}  // namespace

// Returns ARX_EUNSUPPORTED when the shape is not this kernel's (caller falls back to the
// tiled kernel): K in {32, 64, 128}, 16-byte aligned operands.
int gemm_nt_smallk(int64_t M, int64_t N, int64_t K, float alpha, const float* A, int64_t lda,
                   const float* B, int64_t ldb, float* C, int64_t ldc, const float* col_bias,
                   hipStream_t s) {
  if (!(K == 32 || K == 64 || K == 128)) return ARX_EUNSUPPORTED;
  if ((reinterpret_cast<uintptr_t>(A) & 15) || (reinterpret_cast<uintptr_t>(B) & 15) ||
      (lda % 4) || (ldb % 4))
    return ARX_EUNSUPPORTED;
  const int64_t panels = ceil_div(M, (int64_t)kNtBM);
  const int64_t tiles_n = ceil_div(N, (int64_t)kNtBN);
  // enough workgroups for two per CU; each keeps >= 1 tile
  int64_t nsplit = ceil_div((int64_t)cu_count() * 2, panels);
  if (nsplit > tiles_n) nsplit = tiles_n;
  if (nsplit < 1) nsplit = 1;
  const int64_t tpb = ceil_div(tiles_n, nsplit);
  nsplit = ceil_div(tiles_n, tpb);
  const int64_t grid = panels * nsplit;
  if (grid > 0x7fffffff) return ARX_EUNSUPPORTED;
  if (K == 128)
    k_gemm_nt_areg<128><<<(int)grid, 256, 0, s>>>(M, N, A, lda, B, ldb, alpha, C, ldc, col_bias,
                                                   (int)tpb, (int)nsplit, NtFilter{});
  else if (K == 64)
    k_gemm_nt_areg<64><<<(int)grid, 256, 0, s>>>(M, N, A, lda, B, ldb, alpha, C, ldc, col_bias,
                                                  (int)tpb, (int)nsplit, NtFilter{});
  else
    k_gemm_nt_areg<32><<<(int)grid, 256, 0, s>>>(M, N, A, lda, B, ldb, alpha, C, ldc, col_bias,
                                                  (int)tpb, (int)nsplit, NtFilter{});
  ARX_CHECK_LAUNCH();
  return ARX_OK;
}

static void nt_split(int64_t M, int64_t N, int64_t* tpb, int64_t* nsplit) {
  const int64_t panels = ceil_div(M, (int64_t)kNtBM);
  const int64_t tiles_n = ceil_div(N, (int64_t)kNtBN);
  int64_t ns = ceil_div((int64_t)cu_count() * 2, panels);
  if (ns > tiles_n) ns = tiles_n;
  if (ns < 1) ns = 1;
  *tpb = ceil_div(tiles_n, ns);
  *nsplit = ceil_div(tiles_n, *tpb);
}

template <int MODE>
static void nt_launch_mode(int64_t K, int64_t grid, hipStream_t s, int64_t M, int64_t N, const float* A, int64_t lda,
                           const float* Bm, int64_t ldb, const float* col_bias, int tpb, int ns, const NtFilter& f) {
  if (K == 128)
    k_gemm_nt_areg<128, MODE><<<(int)grid, 256, 0, s>>>(M, N, A, lda, Bm, ldb, 1.f, nullptr, 0, col_bias, tpb, ns, f);
  else if (K == 64)
    k_gemm_nt_areg<64, MODE><<<(int)grid, 256, 0, s>>>(M, N, A, lda, Bm, ldb, 1.f, nullptr, 0, col_bias, tpb, ns, f);
  else
    k_gemm_nt_areg<32, MODE><<<(int)grid, 256, 0, s>>>(M, N, A, lda, Bm, ldb, 1.f, nullptr, 0, col_bias, tpb, ns, f);
}

template <int MODE>
static void nt_launch_sample(bool excl, bool tags, int64_t K, int64_t grid, hipStream_t s, int64_t M, int64_t N,
                             const float* A, int64_t lda, const float* Bm, int64_t ldb, const float* col_bias, int tpb,
                             int ns, const NtFilter& f) {
  if (excl && tags)
    nt_launch_mode<MODE | kNtTags | kNtExcl>(K, grid, s, M, N, A, lda, Bm, ldb, col_bias, tpb, ns, f);
  else if (tags)
    nt_launch_mode<MODE | kNtTags>(K, grid, s, M, N, A, lda, Bm, ldb, col_bias, tpb, ns, f);
  else if (excl)
    nt_launch_mode<MODE | kNtExcl>(K, grid, s, M, N, A, lda, Bm, ldb, col_bias, tpb, ns, f);
  else
    nt_launch_mode<MODE>(K, grid, s, M, N, A, lda, Bm, ldb, col_bias, tpb, ns, f);
}

}  // namespace arx

using namespace arx;

extern "C" {

int arx_gemm_nt_topk_parts(int64_t M, int64_t N, int* parts) {
  ARX_CHECK_ARG(M > 0 && N > 0 && parts, "arx_gemm_nt_topk_parts: bad argument");
  int64_t tpb, ns;
  nt_split(M, N, &tpb, &ns);
  *parts = (int)ns;
  return ARX_OK;
}

int arx_gemm_nt_topk_filter(const float* A, int64_t lda, int64_t M, const float* Bm, int64_t ldb, int64_t N, int64_t K,
                            const float* col_bias, const float* thr, int64_t ldthr, int32_t col_base, float* cand_v,
                            int32_t* cand_i, int64_t ldcand, int capp, int* overflow, float* lse_part, int64_t ldl,
                            void* stream) {
  ARX_CHECK_ARG(A && Bm && thr && cand_v && cand_i && overflow && M > 0 && N > 0 && capp > 0,
                "arx_gemm_nt_topk_filter: bad argument");
  ARX_CHECK_ARG(K == 32 || K == 64 || K == 128, "arx_gemm_nt_topk_filter: K must be 32, 64 or 128");
  ARX_CHECK_ARG(!((reinterpret_cast<uintptr_t>(A) | reinterpret_cast<uintptr_t>(Bm)) & 15) && lda % 4 == 0 &&
                    ldb % 4 == 0,
                "arx_gemm_nt_topk_filter: operands must be 16-byte aligned");
  int64_t tpb, ns;
  nt_split(M, N, &tpb, &ns);
  ARX_CHECK_ARG(ns * capp <= ldcand, "arx_gemm_nt_topk_filter: candidate rows too short (parts * capp > ldcand)");
  const int64_t grid = ceil_div(M, (int64_t)kNtBM) * ns;
  ARX_CHECK_ARG(grid <= 0x7fffffff, "arx_gemm_nt_topk_filter: grid too large");
  ARX_CHECK_ARG(!lse_part || ldl >= ns, "arx_gemm_nt_topk_filter: lse_part rows too short (ldl < parts)");
  const NtFilter f{thr, ldthr, cand_v, cand_i, ldcand, capp, col_base, overflow, lse_part, ldl, nullptr, nullptr};
  hipStream_t s = as_stream(stream);
  if (lse_part)
    nt_launch_mode<kNtTopk | kNtLse>(K, grid, s, M, N, A, lda, Bm, ldb, col_bias, (int)tpb, (int)ns, f);
  else
    nt_launch_mode<kNtTopk>(K, grid, s, M, N, A, lda, Bm, ldb, col_bias, (int)tpb, (int)ns, f);
  ARX_CHECK_LAUNCH();
  return ARX_OK;
}

int arx_gemm_nt_topk_filter_excl(const float* A, int64_t lda, int64_t M, const float* Bm, int64_t ldb, int64_t N,
                                 int64_t K, const float* col_bias, const float* thr, int64_t ldthr, int32_t col_base,
                                 float* cand_v, int32_t* cand_i, int64_t ldcand, int capp, int* overflow, float* lse_part,
                                 int64_t ldl, const int32_t* row_keys, int64_t key_rows, const int32_t* ex_ptr,
                                 const int32_t* ex_cols, void* stream) {
  ARX_CHECK_ARG(A && Bm && thr && cand_v && cand_i && overflow && M > 0 && N > 0 && capp > 0,
                "arx_gemm_nt_topk_filter_excl: bad argument");
  ARX_CHECK_ARG(row_keys && ex_ptr && ex_cols && key_rows > 0,
                "arx_gemm_nt_topk_filter_excl: need row_keys, ex_ptr, ex_cols and key_rows > 0");
  ARX_CHECK_ARG(col_base >= 0, "arx_gemm_nt_topk_filter_excl: col_base < 0");
  ARX_CHECK_ARG(K == 32 || K == 64 || K == 128, "arx_gemm_nt_topk_filter_excl: K must be 32, 64 or 128");
  ARX_CHECK_ARG(!((reinterpret_cast<uintptr_t>(A) | reinterpret_cast<uintptr_t>(Bm)) & 15) && lda % 4 == 0 &&
                    ldb % 4 == 0,
                "arx_gemm_nt_topk_filter_excl: operands must be 16-byte aligned");
  int64_t tpb, ns;
  nt_split(M, N, &tpb, &ns);
  ARX_CHECK_ARG(ns * capp <= ldcand,
                "arx_gemm_nt_topk_filter_excl: candidate rows too short (parts * capp > ldcand)");
  const int64_t grid = ceil_div(M, (int64_t)kNtBM) * ns;
  ARX_CHECK_ARG(grid <= 0x7fffffff, "arx_gemm_nt_topk_filter_excl: grid too large");
  ARX_CHECK_ARG(!lse_part || ldl >= ns, "arx_gemm_nt_topk_filter_excl: lse_part rows too short (ldl < parts)");
  const NtFilter f{thr,      ldthr,   cand_v,   cand_i,   ldcand,   capp,   col_base, overflow, lse_part,
                   ldl,      nullptr, nullptr,  row_keys, key_rows, ex_ptr, ex_cols};
  hipStream_t s = as_stream(stream);
  if (lse_part)
    nt_launch_mode<kNtTopk | kNtLse | kNtExcl>(K, grid, s, M, N, A, lda, Bm, ldb, col_bias, (int)tpb, (int)ns, f);
  else
    nt_launch_mode<kNtTopk | kNtExcl>(K, grid, s, M, N, A, lda, Bm, ldb, col_bias, (int)tpb, (int)ns, f);
  ARX_CHECK_LAUNCH();
  return ARX_OK;
}

int arx_gemm_nt_topk_filter_tags(const float* A, int64_t lda, int64_t M, const float* Bm, int64_t ldb, int64_t N,
                                 int64_t K, const float* col_bias, const float* thr, int64_t ldthr, int32_t col_base,
                                 float* cand_v, int32_t* cand_i, int64_t ldcand, int capp, int* overflow, float* lse_part,
                                 int64_t ldl, const int32_t* row_keys, int64_t key_rows, const int32_t* ex_ptr,
                                 const int32_t* ex_cols, const int32_t* col_tags, const int32_t* want_any,
                                 const int32_t* want_all, int64_t want_rows, void* stream) {
  ARX_CHECK_ARG(A && Bm && thr && cand_v && cand_i && overflow,
                "arx_gemm_nt_topk_filter_tags: null pointer (col_bias, lse_part and the exclusion lists may be NULL)");
  ARX_CHECK_ARG(M > 0 && N > 0 && capp > 0 && ldcand > 0 && lda >= K && ldb >= K,
                "arx_gemm_nt_topk_filter_tags: need M > 0, N > 0, capp > 0, ldcand > 0, lda >= K, ldb >= K");
  ARX_CHECK_ARG(col_tags && want_any && want_all && want_rows > 0,
                "arx_gemm_nt_topk_filter_tags: need col_tags, want_any, want_all and want_rows > 0");
  const bool excl = row_keys || ex_ptr || ex_cols;
  ARX_CHECK_ARG(!excl || (row_keys && ex_ptr && ex_cols && key_rows > 0),
                "arx_gemm_nt_topk_filter_tags: row_keys, ex_ptr, ex_cols go together (all NULL: no lists), key_rows > 0");
  ARX_CHECK_ARG(col_base >= 0 && (int64_t)col_base + N <= 0x7fffffff,
                "arx_gemm_nt_topk_filter_tags: need col_base >= 0 and col_base + N < 2^31");
  ARX_CHECK_ARG(K == 32 || K == 64 || K == 128, "arx_gemm_nt_topk_filter_tags: K must be 32, 64 or 128");
  ARX_CHECK_ARG(!((reinterpret_cast<uintptr_t>(A) | reinterpret_cast<uintptr_t>(Bm)) & 15) && lda % 4 == 0 &&
                    ldb % 4 == 0,
                "arx_gemm_nt_topk_filter_tags: operands must be 16-byte aligned");
  int64_t tpb, ns;
  nt_split(M, N, &tpb, &ns);
  ARX_CHECK_ARG(ns * capp <= ldcand,
                "arx_gemm_nt_topk_filter_tags: candidate rows too short (parts * capp > ldcand)");
  const int64_t grid = ceil_div(M, (int64_t)kNtBM) * ns;
  ARX_CHECK_ARG(grid <= 0x7fffffff, "arx_gemm_nt_topk_filter_tags: grid too large");
  ARX_CHECK_ARG(!lse_part || ldl >= ns, "arx_gemm_nt_topk_filter_tags: lse_part rows too short (ldl < parts)");
  NtFilter f{thr,      ldthr,   cand_v,   cand_i,   ldcand,   capp,   col_base, overflow, lse_part,
             ldl,      nullptr, nullptr,  row_keys, key_rows, ex_ptr, ex_cols};
  f.col_tags = col_tags;
  f.want_any = want_any;
  f.want_all = want_all;
  f.want_rows = want_rows;
  hipStream_t s = as_stream(stream);
  const int itpb = (int)tpb, ins = (int)ns;
  if (excl && lse_part)
    nt_launch_mode<kNtTopk | kNtTags | kNtExcl | kNtLse>(K, grid, s, M, N, A, lda, Bm, ldb, col_bias, itpb, ins, f);
  else if (excl)
    nt_launch_mode<kNtTopk | kNtTags | kNtExcl>(K, grid, s, M, N, A, lda, Bm, ldb, col_bias, itpb, ins, f);
  else if (lse_part)
    nt_launch_mode<kNtTopk | kNtTags | kNtLse>(K, grid, s, M, N, A, lda, Bm, ldb, col_bias, itpb, ins, f);
  else
    nt_launch_mode<kNtTopk | kNtTags>(K, grid, s, M, N, A, lda, Bm, ldb, col_bias, itpb, ins, f);
  ARX_CHECK_LAUNCH();
  return ARX_OK;
}

static int filter_sample(const char* fn, const float* A, int64_t lda, int64_t M, const float* Bm, int64_t ldb,
                         int64_t N, int64_t K, const float* col_bias, const float* thr, int64_t ldthr, int32_t col_base,
                         float* cand_v, int32_t* cand_i, int64_t ldcand, int capp, int* overflow, float* lse_part,
                         int64_t ldl, const int32_t* row_keys, int64_t key_rows, const int32_t* ex_ptr,
                         const int32_t* ex_cols, const int32_t* col_tags, const int32_t* want_any,
                         const int32_t* want_all, int64_t want_rows, const float* tau, int64_t tau_rows,
                         const int32_t* seed_words, int32_t col_mul, int32_t col_add, const int32_t* noise_rows,
                         void* stream) {
  ARX_CHECK_ARG(A && Bm && thr && cand_v && cand_i && overflow && tau && seed_words,
                "%s: null pointer (col_bias, lse_part, the exclusion lists and the tag "
                "arrays may be NULL)", fn);
  ARX_CHECK_ARG(M > 0 && N > 0 && capp > 0 && ldcand > 0 && lda >= K && ldb >= K && tau_rows > 0,
                "%s: need M > 0, N > 0, capp > 0, ldcand > 0, lda >= K, ldb >= K, "
                "tau_rows > 0", fn);
  const bool tags = col_tags || want_any || want_all;
  ARX_CHECK_ARG(!tags || (col_tags && want_any && want_all && want_rows > 0),
                "%s: col_tags, want_any, want_all go together (all NULL: no tags), "
                "want_rows > 0", fn);
  const bool excl = row_keys || ex_ptr || ex_cols;
  ARX_CHECK_ARG(!excl || (row_keys && ex_ptr && ex_cols && key_rows > 0),
                "%s: row_keys, ex_ptr, ex_cols go together (all NULL: no lists), "
                "key_rows > 0", fn);
  ARX_CHECK_ARG(col_base >= 0 && (int64_t)col_base + N <= 0x7fffffff,
                "%s: need col_base >= 0 and col_base + N < 2^31", fn);
  ARX_CHECK_ARG(col_mul >= 1 && col_add >= 0 && col_add < col_mul &&
                    (int64_t)col_base + N - 1 <= (0x7fffffffll - col_add) / col_mul,
                "%s: need col_mul >= 1, 0 <= col_add < col_mul and every noise column (col_base + c) * col_mul + "
                "col_add < 2^31", fn);
  ARX_CHECK_ARG(K == 32 || K == 64 || K == 128, "%s: K must be 32, 64 or 128", fn);
  ARX_CHECK_ARG(!((reinterpret_cast<uintptr_t>(A) | reinterpret_cast<uintptr_t>(Bm)) & 15) && lda % 4 == 0 &&
                    ldb % 4 == 0,
                "%s: operands must be 16-byte aligned", fn);
  int64_t tpb, ns;
  nt_split(M, N, &tpb, &ns);
  ARX_CHECK_ARG(ns * capp <= ldcand,
                "%s: candidate rows too short (parts * capp > ldcand)", fn);
  const int64_t grid = ceil_div(M, (int64_t)kNtBM) * ns;
  ARX_CHECK_ARG(grid <= 0x7fffffff, "%s: grid too large", fn);
  ARX_CHECK_ARG(!lse_part || ldl >= ns, "%s: lse_part rows too short (ldl < parts)", fn);
  NtFilter f{thr,      ldthr,   cand_v,   cand_i,   ldcand,   capp,   col_base, overflow, lse_part,
             ldl,      nullptr, nullptr,  row_keys, key_rows, ex_ptr, ex_cols};
  f.col_tags = col_tags;
  f.want_any = want_any;
  f.want_all = want_all;
  f.want_rows = want_rows;
  f.tau = tau;
  f.tau_rows = tau_rows;
  f.seed_words = seed_words;
  f.noise_rows = noise_rows;
  f.noise_mul = (uint32_t)col_mul;
  f.noise_add = (uint32_t)col_base * (uint32_t)col_mul + (uint32_t)col_add;
  hipStream_t s = as_stream(stream);
  const bool keyed = col_mul != 1 || col_add != 0 || noise_rows != nullptr;    // (1, 0, NULL): the plain instances
  if (lse_part && keyed)
    nt_launch_sample<kNtTopk | kNtGumbel | kNtKeyed | kNtLse>(excl, tags, K, grid, s, M, N, A, lda, Bm, ldb, col_bias,
                                                              (int)tpb, (int)ns, f);
  else if (keyed)
    nt_launch_sample<kNtTopk | kNtGumbel | kNtKeyed>(excl, tags, K, grid, s, M, N, A, lda, Bm, ldb, col_bias, (int)tpb,
                                                     (int)ns, f);
  else if (lse_part)
    nt_launch_sample<kNtTopk | kNtGumbel | kNtLse>(excl, tags, K, grid, s, M, N, A, lda, Bm, ldb, col_bias, (int)tpb,
                                                   (int)ns, f);
  else
    nt_launch_sample<kNtTopk | kNtGumbel>(excl, tags, K, grid, s, M, N, A, lda, Bm, ldb, col_bias, (int)tpb, (int)ns, f);
  ARX_CHECK_LAUNCH();
  return ARX_OK;
}

int arx_gemm_nt_topk_filter_sample(const float* A, int64_t lda, int64_t M, const float* Bm, int64_t ldb, int64_t N,
                                   int64_t K, const float* col_bias, const float* thr, int64_t ldthr, int32_t col_base,
                                   float* cand_v, int32_t* cand_i, int64_t ldcand, int capp, int* overflow,
                                   float* lse_part, int64_t ldl, const int32_t* row_keys, int64_t key_rows,
                                   const int32_t* ex_ptr, const int32_t* ex_cols, const int32_t* col_tags,
                                   const int32_t* want_any, const int32_t* want_all, int64_t want_rows, const float* tau,
                                   int64_t tau_rows, const int32_t* seed_words, void* stream) {
  return filter_sample("arx_gemm_nt_topk_filter_sample", A, lda, M, Bm, ldb, N, K, col_bias, thr, ldthr, col_base,
                       cand_v, cand_i, ldcand, capp, overflow, lse_part, ldl, row_keys, key_rows, ex_ptr, ex_cols,
                       col_tags, want_any, want_all, want_rows, tau, tau_rows, seed_words, 1, 0, nullptr, stream);
}

int arx_gemm_nt_topk_filter_sample_keyed(const float* A, int64_t lda, int64_t M, const float* Bm, int64_t ldb,
                                         int64_t N, int64_t K, const float* col_bias, const float* thr, int64_t ldthr,
                                         int32_t col_base, float* cand_v, int32_t* cand_i, int64_t ldcand, int capp,
                                         int* overflow, float* lse_part, int64_t ldl, const int32_t* row_keys,
                                         int64_t key_rows, const int32_t* ex_ptr, const int32_t* ex_cols,
                                         const int32_t* col_tags, const int32_t* want_any, const int32_t* want_all,
                                         int64_t want_rows, const float* tau, int64_t tau_rows,
                                         const int32_t* seed_words, int32_t col_mul, int32_t col_add,
                                         const int32_t* noise_rows, void* stream) {
  return filter_sample("arx_gemm_nt_topk_filter_sample_keyed", A, lda, M, Bm, ldb, N, K, col_bias, thr, ldthr, col_base,
                       cand_v, cand_i, ldcand, capp, overflow, lse_part, ldl, row_keys, key_rows, ex_ptr, ex_cols,
                       col_tags, want_any, want_all, want_rows, tau, tau_rows, seed_words, col_mul, col_add, noise_rows,
                       stream);
}

int arx_gemm_nt_rest_mass(const float* A, int64_t lda, int64_t M, const float* Bm, int64_t ldb, int64_t N, int64_t K,
                          const float* col_bias, int32_t col_base, const float* tau, int64_t tau_rows,
                          const int32_t* row_keys, int64_t key_rows, const int32_t* ex_ptr, const int32_t* ex_cols,
                          const int32_t* col_tags, const int32_t* want_any, const int32_t* want_all, int64_t want_rows,
                          const int32_t* pk_cols, const int32_t* pk_slot, int64_t ldp, int k, float* m_part,
                          float* s_part, int64_t ldl, float* pick_score, int64_t ldps, void* stream) {
  ARX_CHECK_ARG(A && Bm && tau && pk_cols && pk_slot && m_part && s_part && pick_score,
                "arx_gemm_nt_rest_mass: null pointer (col_bias, the exclusion lists and the tag arrays may be NULL)");
  ARX_CHECK_ARG(M >= 0 && N > 0 && lda >= K && ldb >= K && tau_rows > 0,
                "arx_gemm_nt_rest_mass: need M >= 0, N > 0, lda >= K, ldb >= K, tau_rows > 0");
  const bool tags = col_tags || want_any || want_all;
  ARX_CHECK_ARG(!tags || (col_tags && want_any && want_all && want_rows > 0),
                "arx_gemm_nt_rest_mass: col_tags, want_any, want_all go together (all NULL: no tags), want_rows > 0");
  const bool excl = row_keys || ex_ptr || ex_cols;
  ARX_CHECK_ARG(!excl || (row_keys && ex_ptr && ex_cols && key_rows > 0),
                "arx_gemm_nt_rest_mass: row_keys, ex_ptr, ex_cols go together (all NULL: no lists), key_rows > 0");
  ARX_CHECK_ARG(col_base >= 0 && (int64_t)col_base + N <= 0x7fffffff,
                "arx_gemm_nt_rest_mass: need col_base >= 0 and col_base + N < 2^31");
  ARX_CHECK_ARG(k >= 1 && k <= 1024 && ldp >= k && ldps >= k,
                "arx_gemm_nt_rest_mass: need 1 <= k <= 1024, ldp >= k, ldps >= k (k=%d ldp=%lld ldps=%lld)", k,
                (long long)ldp, (long long)ldps);
  if (!(K == 32 || K == 64 || K == 128)) {
    set_error("arx_gemm_nt_rest_mass: K=%lld unsupported (K must be 32, 64 or 128)", (long long)K);
    return ARX_EUNSUPPORTED;
  }
  ARX_CHECK_ARG(!((reinterpret_cast<uintptr_t>(A) | reinterpret_cast<uintptr_t>(Bm)) & 15) && lda % 4 == 0 &&
                    ldb % 4 == 0,
                "arx_gemm_nt_rest_mass: operands must be 16-byte aligned");
  if (M == 0) return ARX_OK;
  int64_t tpb, ns;
  nt_split(M, N, &tpb, &ns);
  ARX_CHECK_ARG(ldl >= ns, "arx_gemm_nt_rest_mass: part rows too short (ldl < parts)");
  const int64_t grid = ceil_div(M, (int64_t)kNtBM) * ns;
  ARX_CHECK_ARG(grid <= 0x7fffffff, "arx_gemm_nt_rest_mass: grid too large");
  NtFilter f{};
  f.col_base = col_base;
  f.ldl = ldl;
  f.row_keys = row_keys;
  f.key_rows = key_rows;
  f.ex_ptr = ex_ptr;
  f.ex_cols = ex_cols;
  f.col_tags = col_tags;
  f.want_any = want_any;
  f.want_all = want_all;
  f.want_rows = want_rows;
  f.tau = tau;
  f.tau_rows = tau_rows;
  f.pk_cols = pk_cols;
  f.pk_slot = pk_slot;
  f.ldp = ldp;
  f.pk_k = k;
  f.m_part = m_part;
  f.s_part = s_part;
  f.pick_score = pick_score;
  f.ldps = ldps;
  nt_launch_mode<kNtRest>(K, grid, as_stream(stream), M, N, A, lda, Bm, ldb, col_bias, (int)tpb, (int)ns, f);
  ARX_CHECK_LAUNCH();
  return ARX_OK;
}

int arx_gemm_nt_topk_filter_cos(const float* A, int64_t lda, int64_t M, const float* Bm, int64_t ldb, int64_t N,
                                int64_t K, const float* col_scale, const int32_t* self_col, const float* thr,
                                int64_t ldthr, int32_t col_base, float* cand_v, int32_t* cand_i, int64_t ldcand, int capp,
                                int* overflow, void* stream) {
  ARX_CHECK_ARG(A && Bm && col_scale && thr && cand_v && cand_i && overflow,
                "arx_gemm_nt_topk_filter_cos: null pointer (only self_col may be NULL)");
  ARX_CHECK_ARG(M > 0 && N > 0 && capp > 0 && ldcand > 0 && lda >= K && ldb >= K,
                "arx_gemm_nt_topk_filter_cos: need M > 0, N > 0, capp > 0, ldcand > 0, lda >= K, ldb >= K");
  ARX_CHECK_ARG(col_base >= 0 && (int64_t)col_base + N <= 0x7fffffff,
                "arx_gemm_nt_topk_filter_cos: need col_base >= 0 and col_base + N < 2^31");
  ARX_CHECK_ARG(K == 32 || K == 64 || K == 128, "arx_gemm_nt_topk_filter_cos: K must be 32, 64 or 128");
  ARX_CHECK_ARG(!((reinterpret_cast<uintptr_t>(A) | reinterpret_cast<uintptr_t>(Bm)) & 15) && lda % 4 == 0 &&
                    ldb % 4 == 0,
                "arx_gemm_nt_topk_filter_cos: operands must be 16-byte aligned");
  int64_t tpb, ns;
  nt_split(M, N, &tpb, &ns);
  ARX_CHECK_ARG(ns * capp <= ldcand, "arx_gemm_nt_topk_filter_cos: candidate rows too short (parts * capp > ldcand)");
  const int64_t grid = ceil_div(M, (int64_t)kNtBM) * ns;
  ARX_CHECK_ARG(grid <= 0x7fffffff, "arx_gemm_nt_topk_filter_cos: grid too large");
  NtFilter f{thr, ldthr, cand_v, cand_i, ldcand, capp, col_base, overflow};
  f.tcol = self_col;
  hipStream_t s = as_stream(stream);
  if (self_col)
    nt_launch_mode<kNtTopk | kNtCos | kNtSelf>(K, grid, s, M, N, A, lda, Bm, ldb, col_scale, (int)tpb, (int)ns, f);
  else
    nt_launch_mode<kNtTopk | kNtCos>(K, grid, s, M, N, A, lda, Bm, ldb, col_scale, (int)tpb, (int)ns, f);
  ARX_CHECK_LAUNCH();
  return ARX_OK;
}

int arx_gemm_nt_eval_parts(const float* A, int64_t lda, int64_t M, const float* Bm, int64_t ldb, int64_t N, int64_t K,
                           const float* col_bias, const float* tscore, float* lse_part, float* relu_part, int64_t ldl,
                           void* stream) {
  ARX_CHECK_ARG(A && Bm && M > 0 && N > 0 && (lse_part || relu_part), "arx_gemm_nt_eval_parts: bad argument");
  ARX_CHECK_ARG(!relu_part || tscore, "arx_gemm_nt_eval_parts: the margin sums need the target scores");
  ARX_CHECK_ARG(K == 32 || K == 64 || K == 128, "arx_gemm_nt_eval_parts: K must be 32, 64 or 128");
  ARX_CHECK_ARG(!((reinterpret_cast<uintptr_t>(A) | reinterpret_cast<uintptr_t>(Bm)) & 15) && lda % 4 == 0 &&
                    ldb % 4 == 0,
                "arx_gemm_nt_eval_parts: operands must be 16-byte aligned");
  int64_t tpb, ns;
  nt_split(M, N, &tpb, &ns);
  ARX_CHECK_ARG(ldl >= ns, "arx_gemm_nt_eval_parts: part rows too short (ldl < parts)");
  const int64_t grid = ceil_div(M, (int64_t)kNtBM) * ns;
  ARX_CHECK_ARG(grid <= 0x7fffffff, "arx_gemm_nt_eval_parts: grid too large");
  const NtFilter f{nullptr, 0, nullptr, nullptr, 0, 0, 0, nullptr, lse_part, ldl, tscore, relu_part};
  hipStream_t s = as_stream(stream);
  if (lse_part && relu_part)
    nt_launch_mode<kNtLse | kNtRelu>(K, grid, s, M, N, A, lda, Bm, ldb, col_bias, (int)tpb, (int)ns, f);
  else if (lse_part)
    nt_launch_mode<kNtLse>(K, grid, s, M, N, A, lda, Bm, ldb, col_bias, (int)tpb, (int)ns, f);
  else
    nt_launch_mode<kNtRelu>(K, grid, s, M, N, A, lda, Bm, ldb, col_bias, (int)tpb, (int)ns, f);
  ARX_CHECK_LAUNCH();
  return ARX_OK;
}

int arx_gemm_nt_eval_rank_parts(const float* A, int64_t lda, int64_t M, const float* Bm, int64_t ldb, int64_t N,
                                int64_t K, const float* col_bias, const float* tscore, const int32_t* tcol,
                                float* relu_part, int32_t* cnt_part, int64_t ldl, void* stream) {
  ARX_CHECK_ARG(A && Bm && tscore && tcol && relu_part && cnt_part, "arx_gemm_nt_eval_rank_parts: null pointer");
  ARX_CHECK_ARG(M > 0 && N > 0 && N <= 0x7fffffff, "arx_gemm_nt_eval_rank_parts: need M > 0, 0 < N < 2^31");
  ARX_CHECK_ARG(K == 32 || K == 64 || K == 128, "arx_gemm_nt_eval_rank_parts: K must be 32, 64 or 128");
  ARX_CHECK_ARG(!((reinterpret_cast<uintptr_t>(A) | reinterpret_cast<uintptr_t>(Bm)) & 15) && lda % 4 == 0 &&
                    ldb % 4 == 0,
                "arx_gemm_nt_eval_rank_parts: operands must be 16-byte aligned");
  int64_t tpb, ns;
  nt_split(M, N, &tpb, &ns);
  ARX_CHECK_ARG(ldl >= ns, "arx_gemm_nt_eval_rank_parts: part rows too short (ldl < parts)");
  const int64_t grid = ceil_div(M, (int64_t)kNtBM) * ns;
  ARX_CHECK_ARG(grid <= 0x7fffffff, "arx_gemm_nt_eval_rank_parts: grid too large");
  NtFilter f{};
  f.ldl = ldl;
  f.tsc = tscore;
  f.relu_part = relu_part;
  f.tcol = tcol;
  f.cnt_part = cnt_part;
  nt_launch_mode<kNtRelu | kNtRank>(K, grid, as_stream(stream), M, N, A, lda, Bm, ldb, col_bias, (int)tpb, (int)ns, f);
  ARX_CHECK_LAUNCH();
  return ARX_OK;
}

}  // extern "C"

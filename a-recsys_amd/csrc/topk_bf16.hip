// topk_bf16.hip -- recommend(scan_dtype='bf16') (arx_topk_bf16.h): the FILTER scan of the streaming top-k on the bf16
// matrix pipe.  The scan of gemm_nt.hip multiplies with v_mfma_f32_32x32x2_f32; here both operands are rounded to bf16
// and one v_mfma_f32_32x32x16_bf16 does the work of sixteen of those.  The product is only a filter: a logit passes
// when  fmaf(rowm[row], coln[col], v~) > thr[row]  -- the margin rowm * coln bounds the rounding error (DESIGN.md
// section 4 item 20), so no column whose f32 score beats the threshold is lost -- and arx_cand_rescore then overwrites
// every survivor's value with the exact f32 score in arx_slate_scores' arithmetic.
//
// k_topk_filter_bf16 keeps the decomposition of k_gemm_nt_areg's FILTER modes -- 128 rows per workgroup (4 waves x 32),
// the column ranges of arx_gemm_nt_topk_parts, the XCD-aware block order, 64-column tiles double-buffered in LDS by
// LDS-DMA with a source-side XOR swizzle, survivors placed by ballot + prefix count in ascending column order -- but is
// a kernel of its own: that body holds 246 VGPRs and has no room for one more mode.  What differs:
//   * A: a lane rounds its row's f32 values to bf16 in registers (4 VGPRs per 16-wide k step); the row's 2-norm comes
//     from the same registers (the two lanes of a row meet by one shuffle), so rowm costs no launch;
//   * B: the bf16 image of arx_rows_bf16_norm, rows of 2 K bytes; lane (r = l & 31, h = l >> 5) reads the 16-byte chunk
//     2 s + h of pool row r (+ 32) for step s: k = 16 s + 8 h + j, j = 0..7, what the 32x32x16 operand map wants;
//   * 16 / CPR pool rows share one 256-byte bank row (CPR = K / 8 chunks per row), so chunk c of row r lives at slot
//     c ^ ((r / (16 / CPR)) & (CPR - 1)): the 16 rows of a ds_read_b128 lane group hit 16 distinct 16-byte slots;
//   * the epilogue forms all 32 predicates of a tile first, as one wave-uniform word; the placement (tags, exclusion
//     lists, ballot) is one copy of code entered once per set bit, and the rows' list lengths are registers, not LDS
//     words -- with the matrix work 16 times shorter the epilogue is what the scan pays for;
//   * exclusion lists and tag words are nullable run-time operands of the survivor path, not template modes.
#include "common.h"

namespace arx {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

constexpr int kBfBM = 128;   // rows per workgroup
constexpr int kBfBN = 64;    // pool rows (output columns) per tile
constexpr float kNormUp = 1.f + 0x1p-20f;   // a computed norm times this is >= the exact one (arx_topk_bf16.h)

// round-to-nearest-even bf16 of a float (ties to the even 8-bit significand); a NaN becomes the quiet NaN
__device__ __forceinline__ uint32_t bf16_rne(float x) {
  const uint32_t u = __float_as_uint(x);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0u;
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}
__device__ __forceinline__ uint32_t bf16_pack(float lo, float hi) { return bf16_rne(lo) | (bf16_rne(hi) << 16); }

// x0^2 + .. + x7^2: one multiply, seven fused multiply-adds, in that order
__device__ __forceinline__ float sumsq8(const float4& a, const float4& b) {
  float s = a.x * a.x;
  s = fmaf(a.y, a.y, s);
  s = fmaf(a.z, a.z, s);
  s = fmaf(a.w, a.w, s);
  s = fmaf(b.x, b.x, s);
  s = fmaf(b.y, b.y, s);
  s = fmaf(b.z, b.z, s);
  s = fmaf(b.w, b.w, s);
  return s;
}

// ---- arx_rows_bf16_norm: L lanes per row, 8 elements per lane; waves stride the row groups ----
template <int L>
__global__ __launch_bounds__(256) void k_rows_bf16_norm(const float* __restrict__ P, int64_t ldp, int64_t N, int K,
                                                        uint16_t* __restrict__ img, int64_t ldi,
                                                        float* __restrict__ norms) {
  constexpr int R = 64 / L;                                       // rows per wave
  const int lane = threadIdx.x & 63, li = lane & (L - 1), g = lane / L;
  const bool live = li * 8 < K;
  const int64_t wave = blockIdx.x * (int64_t)(blockDim.x >> 6) + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x >> 6);
  const int64_t units = ceil_div(N, (int64_t)R);
  for (int64_t w = wave; w < units; w += nwaves) {                // (wave-uniform bounds: every lane shuffles)
    const int64_t n = w * R + g;
    const bool ok = live && n < N;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
    if (ok) {
      const float* p = P + n * ldp + li * 8;
      a = *reinterpret_cast<const float4*>(p);
      b = *reinterpret_cast<const float4*>(p + 4);
    }
    float ss = sumsq8(a, b);
#pragma unroll
    for (int o = 1; o < L; o <<= 1) ss += __shfl_xor(ss, o, 64);
    if (ok) {
      *reinterpret_cast<uint4*>(img + n * ldi + li * 8) =
          make_uint4(bf16_pack(a.x, a.y), bf16_pack(a.z, a.w), bf16_pack(b.x, b.y), bf16_pack(b.z, b.w));
      if (li == 0) norms[n] = sqrtf(ss) * kNormUp;
    }
  }
}

// ---- arx_cand_rescore: arx_slate_scores' gather and dot over the occupied candidate slots, in place ----
constexpr int kRescoreUnroll = 4;    // pool rows in flight per group
constexpr int kRescoreMaxPasses = 8;

template <int L>
__global__ __launch_bounds__(256) void k_cand_rescore(const float* __restrict__ U, int64_t ldu,
                                                      const float* __restrict__ P, int64_t ldp,
                                                      const float* __restrict__ pbias, int32_t V, int d,
                                                      float* __restrict__ cand_v, const int32_t* __restrict__ cand_i,
                                                      int64_t ldcand, int64_t C, int64_t units, int64_t nruns, int run) {
  constexpr int S = 64 / L;                                       // slots per wave and load
  const int lane = threadIdx.x & 63, li = lane & (L - 1), gw = lane / L;
  const bool live = li * 4 < d;
  const int64_t wave = blockIdx.x * (int64_t)(blockDim.x >> 6) + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x >> 6);
  for (int64_t w = wave; w < units; w += nwaves) {                // (wave-uniform bounds: every lane shuffles)
    const int64_t r = w / nruns;
    const int64_t j0 = (w - r * nruns) * run;
    const int64_t j1 = j0 + run < C ? j0 + run : C;
    float4 u = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live) u = *reinterpret_cast<const float4*>(U + r * ldu + li * 4);
    const int32_t* cr = cand_i + r * ldcand;
    float* sr = cand_v + r * ldcand;
    for (int64_t j = j0; j < j1; j += kRescoreUnroll * S) {
      bool occ[kRescoreUnroll];
      int32_t c[kRescoreUnroll];
      float4 p[kRescoreUnroll];
      float b[kRescoreUnroll];
#pragma unroll
      for (int t = 0; t < kRescoreUnroll; ++t) {
        const int64_t jj = j + t * S + gw;
        occ[t] = jj < j1 && !(sr[jj] == -__builtin_inff());       // an empty slot holds -inf: its index is stale
        c[t] = occ[t] ? cr[jj] : -1;
      }
#pragma unroll
      for (int t = 0; t < kRescoreUnroll; ++t) {
        const bool ok = (uint32_t)c[t] < (uint32_t)V;
        p[t] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (ok && live) p[t] = *reinterpret_cast<const float4*>(P + (int64_t)c[t] * ldp + li * 4);
        b[t] = ok && pbias ? pbias[c[t]] : 0.f;
      }
#pragma unroll
      for (int t = 0; t < kRescoreUnroll; ++t) {
        float s = u.x * p[t].x;                                   // (the order of arx_slate.h, add for add)
        s = fmaf(u.y, p[t].y, s);
        s = fmaf(u.z, p[t].z, s);
        s = fmaf(u.w, p[t].w, s);
#pragma unroll
        for (int o = 1; o < L; o <<= 1) s += __shfl_xor(s, o, 64);
        const int64_t jj = j + t * S + gw;
        if (li == 0 && occ[t]) {
          const bool ok = (uint32_t)c[t] < (uint32_t)V;
          sr[jj] = ok ? (pbias ? s + b[t] : s) : -__builtin_inff();
        }
      }
    }
  }
}

// ---- the filter ----
struct BfFilter {
  const float* thr; int64_t ldthr;
  float* cand_v; int32_t* cand_i; int64_t ldcand;
  int capp; int32_t col_base;
  int* overflow;
  float coeff;
  // row r's excluded ABSOLUTE columns: ex_cols[ex_ptr[key] .. ex_ptr[key + 1]), sorted, key = row_keys[r % key_rows]
  // (< 0: nothing excluded); row_keys == nullptr: no lists
  const int32_t* row_keys; int64_t key_rows;
  const int32_t* ex_ptr; const int32_t* ex_cols;
  // column c of this launch carries col_tags[c], row r the words want_any / want_all [r % want_rows] (arx_tags.h);
  // col_tags == nullptr: no tags
  const int32_t* col_tags; const int32_t* want_any; const int32_t* want_all; int64_t want_rows;
};

// the float two steps below a finite t: what the comparison of the widened logit runs against (the roundings of the
// bias add and of the fmaf; arx_topk_bf16.h).  -inf, +inf and NaN stay
__device__ __forceinline__ float two_below(float t) {
  if (!(fabsf(t) < __builtin_inff())) return t;
  return nextafterf(nextafterf(t, -__builtin_inff()), -__builtin_inff());
}

template <int KT>
__global__ __launch_bounds__(256, 2) void k_topk_filter_bf16(
    int64_t M, int64_t N, const float* __restrict__ A, int64_t lda, const uint16_t* __restrict__ Bi, int64_t ldbi,
    const float* __restrict__ coln, const float* __restrict__ col_bias, int tiles_per_block, int nsplit, BfFilter flt) {
  constexpr int NS = KT / 16;                 // MFMA steps (two MFMAs each: the tile's two column halves)
  constexpr int CPR = KT / 8;                 // 16-B chunks per image row
  constexpr int RPB = 16 / CPR;               // image rows per 256-B bank row
  constexpr int NLB = kBfBN * CPR / 256;      // DMA pieces per thread per tile
  static_assert(NLB >= 1 && RPB >= 1, "tile too small");
  // two separate arrays: the DMA destination and the buffer being read must not look like aliases (gemm_nt.hip)
  __shared__ __attribute__((aligned(1024))) uint16_t sB0[kBfBN * KT];
  __shared__ __attribute__((aligned(1024))) uint16_t sB1[kBfBN * KT];
  __shared__ __attribute__((aligned(16))) float s_th[kBfBM];
  __shared__ __attribute__((aligned(16))) float s_rm[kBfBM];
  __shared__ int s_xb[kBfBM], s_xe[kBfBM];
  __shared__ uint32_t s_wa[kBfBM], s_wl[kBfBM];

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
  const int64_t m0 = (int64_t)panel * kBfBM;
  const int64_t tiles_n = ceil_div(N, (int64_t)kBfBN);
  const int64_t t_beg = (int64_t)part * tiles_per_block;
  const int64_t t_end = min(tiles_n, t_beg + tiles_per_block);
  if (t_beg >= t_end) return;

  // LDS-DMA of one image tile: piece f = threadIdx.x + 256 i lands at chunk f of the LDS image; it fetches chunk
  // (f % CPR) ^ swz(row) of image row n0 + f / CPR (rows past N clamped: their columns never pass)
  auto dma_b = [&](int64_t t, uint16_t* img) {
    const int64_t n0 = t * kBfBN;
#pragma unroll
    for (int i = 0; i < NLB; ++i) {
      const int f = threadIdx.x + i * 256;
      const int r = f / CPR, slot = f % CPR;
      const int c = slot ^ ((r / RPB) & (CPR - 1));
      const int64_t gr = min(n0 + r, N - 1);
      const uint16_t* src = Bi + gr * ldbi + c * 8;
      uint16_t* dst = img + (f - lane) * 8;        // wave-uniform base; HW adds 16 B x lane
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                       (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
    }
  };
  dma_b(t_beg, sB0);

  // ---- A operand: this lane's row, k = 16 s + 8 lhi + {0..7}, rounded to bf16; the row's norm on the way ----
  bf16x8 a[NS];
  {
    const int64_t row = m0 + wave * 32 + l31;
    const bool ok = row < M;
    const float* ap = A + (ok ? row : 0) * lda + 8 * lhi;
    float part_ss[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      float4 x = *reinterpret_cast<const float4*>(ap + 16 * s);
      float4 y = *reinterpret_cast<const float4*>(ap + 16 * s + 4);
      if (!ok) x = y = make_float4(0.f, 0.f, 0.f, 0.f);
      a[s] = __builtin_bit_cast(bf16x8, make_uint4(bf16_pack(x.x, x.y), bf16_pack(x.z, x.w), bf16_pack(y.x, y.y),
                                                   bf16_pack(y.z, y.w)));
      part_ss[s] = sumsq8(x, y);
    }
    // 8 + log2(NS) + 1 roundings at most (a chain of 8, a tree over the steps, the other half of the row): the bound
    // kNormUp was sized for
#pragma unroll
    for (int w = 1; w < NS; w <<= 1)
#pragma unroll
      for (int s = 0; s + w < NS; s += 2 * w) part_ss[s] += part_ss[s + w];
    const float ss = part_ss[0] + __shfl_xor(part_ss[0], 32, 64);
    if (lhi == 0) s_rm[wave * 32 + l31] = flt.coeff * (sqrtf(ss) * kNormUp);
  }
  if (threadIdx.x < kBfBM) {
    const int64_t row = m0 + threadIdx.x;
    s_th[threadIdx.x] = row < M ? two_below(flt.thr[row * flt.ldthr]) : __builtin_inff();
    int xb = 0, xe = 0;
    if (row < M && flt.row_keys) {
      const int32_t key = flt.row_keys[row % flt.key_rows];
      if (key >= 0) {
        // narrowed to this workgroup's columns [c_lo, c_hi) once here: the survivor searches get shorter
        const int32_t c_lo = flt.col_base + (int32_t)(t_beg * kBfBN);
        const int32_t c_hi = flt.col_base + (int32_t)min(t_end * kBfBN, N);
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
    const bool tg = row < M && flt.col_tags != nullptr;
    s_wa[threadIdx.x] = tg ? (uint32_t)flt.want_any[row % flt.want_rows] : 0u;
    s_wl[threadIdx.x] = tg ? (uint32_t)flt.want_all[row % flt.want_rows] : 0u;
  }
  // bias and norm of the tile's two columns (later tiles: fetched one tile ahead, behind the DMA issue).  A column
  // past N gets bias -inf: its widened logit is -inf and passes no threshold
  auto col_consts = [&](int64_t t, float& b0, float& b1, float& c0, float& c1) {
    const int64_t x0 = t * kBfBN + l31, x1 = x0 + 32;
    b0 = x0 < N ? (col_bias ? col_bias[x0] : 0.f) : -__builtin_inff();
    b1 = x1 < N ? (col_bias ? col_bias[x1] : 0.f) : -__builtin_inff();
    c0 = coln[min(x0, N - 1)];
    c1 = coln[min(x1, N - 1)];
  };
  float bias0, bias1, cn0, cn1;
  col_consts(t_beg, bias0, bias1, cn0, cn1);
  __syncthreads();

  // the thresholds and margins of the lane's 16 rows (row = rl0 + (e & 3) + 8 (e >> 2)): registers for the whole run
  const int rl0 = wave * 32 + 4 * lhi;
  float th[16], rm[16];
#pragma unroll
  for (int g4 = 0; g4 < 4; ++g4) {
    const float4 t4 = *reinterpret_cast<const float4*>(&s_th[rl0 + 8 * g4]);
    const float4 m4 = *reinterpret_cast<const float4*>(&s_rm[rl0 + 8 * g4]);
    th[4 * g4] = t4.x; th[4 * g4 + 1] = t4.y; th[4 * g4 + 2] = t4.z; th[4 * g4 + 3] = t4.w;
    rm[4 * g4] = m4.x; rm[4 * g4 + 1] = m4.y; rm[4 * g4 + 2] = m4.z; rm[4 * g4 + 3] = m4.w;
  }
  // the list lengths of the same 16 rows: every lane of a half wave sees the half's ballots, so each keeps its own
  // copy of the 16 counters in step -- no LDS, no atomics, one writer per segment (the wave owns its rows)
  int cnt[16];
#pragma unroll
  for (int e = 0; e < 16; ++e) cnt[e] = 0;
  const bool has_tags = flt.col_tags != nullptr, has_excl = flt.row_keys != nullptr;
  bool ovf = false;

  // read-side swizzle: chunk 2 s + lhi of image row l31 (+ 32); swz(l31) == swz(l31 + 32)
  const int sw = (l31 / RPB) & (CPR - 1);
  auto tile = [&](int64_t t, const uint16_t* cur_img, uint16_t* nxt_img) {
    float nb0 = 0.f, nb1 = 0.f, nc0 = 0.f, nc1 = 0.f;
    if (t + 1 < t_end) {
      col_consts(t + 1, nb0, nb1, nc0, nc1);
      dma_b(t + 1, nxt_img);
    }
    f32x16 acc0, acc1;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      acc0[e] = 0.f;
      acc1[e] = 0.f;
    }
    const uint16_t* b0p = cur_img + l31 * KT;
    const uint16_t* b1p = b0p + 32 * KT;
    // operands of step s + 1 are fetched from LDS before the MFMAs of step s issue (gemm_nt.hip)
    uint4 b0 = *reinterpret_cast<const uint4*>(b0p + ((lhi ^ sw) * 8));
    uint4 b1 = *reinterpret_cast<const uint4*>(b1p + ((lhi ^ sw) * 8));
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      uint4 n0 = b0, n1 = b1;
      if (s + 1 < NS) {
        const int off = ((2 * (s + 1) + lhi) ^ sw) * 8;
        n0 = *reinterpret_cast<const uint4*>(b0p + off);
        n1 = *reinterpret_cast<const uint4*>(b1p + off);
      }
      __builtin_amdgcn_sched_barrier(0);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[s], __builtin_bit_cast(bf16x8, b0), acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[s], __builtin_bit_cast(bf16x8, b1), acc1, 0, 0, 0);
      b0 = n0;
      b1 = n1;
    }
    // epilogue.  C/D map of the 32x32 MFMA: col = lane & 31, row = (e & 3) + 8 (e >> 2) + 4 (lane >> 5).  All 32
    // predicates first, as one wave-uniform word: bit 16 j + e says that logit (j, e) passes in some lane
    uint32_t wm = 0u;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      if (__ballot(fmaf(rm[e], cn0, acc0[e] + bias0) > th[e]) != 0ull) wm |= 1u << e;
      if (__ballot(fmaf(rm[e], cn1, acc1[e] + bias1) > th[e]) != 0ull) wm |= 1u << (16 + e);
    }
    wm = (uint32_t)__builtin_amdgcn_readfirstlane((int)wm);
    // the placement, ONE copy of it, entered once per set bit in (j, e) order -- a row's columns ascend.  (Unrolled
    // over the 32 logits like gemm_nt.hip's, it spilled 1.5 KB per lane: nothing of it may cost registers between
    // survivors.)  The logit, its row's threshold, margin and list length come from registers by a switch on the bit:
    // a trip of a scan without tags and lists touches no LDS (four survivors per wave and tile at 1 M columns: with the
    // constants and the lengths read from LDS in the trip the scan took 4.45 ms at 4096 x 1 M x 128, now 3.68)
    const int64_t n0 = t * kBfBN;
    while (wm != 0u) {
      const int bit = __builtin_ctz(wm);
      wm &= wm - 1u;
      const int e = bit & 15, j = bit >> 4;
      float x = 0.f, thv = 0.f, rmv = 0.f;
      int c0 = 0;
      switch (bit) {
#define ARX_BF_PICK(E)        \
  case E:                     \
    x = acc0[E];              \
    thv = th[E];              \
    rmv = rm[E];              \
    c0 = cnt[E];              \
    break;                    \
  case 16 + E:                \
    x = acc1[E];              \
    thv = th[E];              \
    rmv = rm[E];              \
    c0 = cnt[E];              \
    break;
        ARX_BF_PICK(0) ARX_BF_PICK(1) ARX_BF_PICK(2) ARX_BF_PICK(3) ARX_BF_PICK(4) ARX_BF_PICK(5) ARX_BF_PICK(6)
        ARX_BF_PICK(7) ARX_BF_PICK(8) ARX_BF_PICK(9) ARX_BF_PICK(10) ARX_BF_PICK(11) ARX_BF_PICK(12) ARX_BF_PICK(13)
        ARX_BF_PICK(14) ARX_BF_PICK(15)
#undef ARX_BF_PICK
      }
      const int rl = rl0 + (e & 3) + 8 * (e >> 2);
      const int64_t col = n0 + j * 32 + l31;
      const float v = x + (j == 0 ? bias0 : bias1);
      bool pred = fmaf(rmv, j == 0 ? cn0 : cn1, v) > thv;                  // (the test above, bit for bit)
      if (has_tags && pred) {
        // a survivor: its column's tag word comes from global memory here, BEFORE the ballot, so an ineligible
        // column takes no position; a row of two zero words loads nothing
        const uint32_t wa = s_wa[rl], wl = s_wl[rl];
        if ((wa | wl) != 0u) {
          const uint32_t tg = (uint32_t)flt.col_tags[col];
          if ((wa != 0u && (tg & wa) == 0u) || (tg & wl) != wl) pred = false;
        }
      }
      if (has_excl && pred) {
        // lower_bound of its absolute column in the row's exclusion list, BEFORE the ballot
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
      if (m == 0ull) continue;
      const uint32_t mh = lhi ? (uint32_t)(m >> 32) : (uint32_t)m;         // the survivors of THIS half's row
      const int pos = c0 + __popc(mh & ((1u << l31) - 1u));
      if (pred) {
        if (pos < flt.capp) {
          const int64_t at = (m0 + rl) * flt.ldcand + (int64_t)part * flt.capp + pos;
          flt.cand_v[at] = v;
          flt.cand_i[at] = flt.col_base + (int32_t)col;
        } else {
          ovf = true;
        }
      }
      const int add = __popc(mh);
      switch (e) {
#define ARX_BF_COUNT(E)       \
  case E:                     \
    cnt[E] += add;            \
    break;
        ARX_BF_COUNT(0) ARX_BF_COUNT(1) ARX_BF_COUNT(2) ARX_BF_COUNT(3) ARX_BF_COUNT(4) ARX_BF_COUNT(5)
        ARX_BF_COUNT(6) ARX_BF_COUNT(7) ARX_BF_COUNT(8) ARX_BF_COUNT(9) ARX_BF_COUNT(10) ARX_BF_COUNT(11)
        ARX_BF_COUNT(12) ARX_BF_COUNT(13) ARX_BF_COUNT(14) ARX_BF_COUNT(15)
#undef ARX_BF_COUNT
      }
    }
    bias0 = nb0;
    bias1 = nb1;
    cn0 = nc0;
    cn1 = nc1;
    __syncthreads();          // tile t + 1 landed (vmcnt(0) rides on the barrier); buffer cur free
  };
  for (int64_t t = t_beg; t < t_end; t += 2) {
    tile(t, sB0, sB1);
    if (t + 1 < t_end) tile(t + 1, sB1, sB0);
  }
  if (ovf) *flt.overflow = 1;
}

template <int L>
void rows_launch(int g, hipStream_t s, const float* P, int64_t ldp, int64_t N, int K, uint16_t* img, int64_t ldi,
                 float* norms) {
  k_rows_bf16_norm<L><<<g, 256, 0, s>>>(P, ldp, N, K, img, ldi, norms);
}

template <int L>
void rescore_launch(int g, hipStream_t s, const float* U, int64_t ldu, const float* P, int64_t ldp, const float* pbias,
                    int32_t V, int d, float* cand_v, const int32_t* cand_i, int64_t ldcand, int64_t C, int64_t units,
                    int64_t nruns, int run) {
  k_cand_rescore<L><<<g, 256, 0, s>>>(U, ldu, P, ldp, pbias, V, d, cand_v, cand_i, ldcand, C, units, nruns, run);
}

}  // namespace
}  // namespace arx

using namespace arx;

extern "C" {

int arx_rows_bf16_norm(const float* P, int64_t ldp, int64_t N, int64_t K, uint16_t* img, int64_t ldi, float* norms,
                       void* stream) {
  ARX_CHECK_ARG(P && img && norms, "arx_rows_bf16_norm: null pointer");
  ARX_CHECK_ARG(N >= 0 && K > 0, "arx_rows_bf16_norm: need N >= 0 and K > 0 (N=%lld K=%lld)", (long long)N, (long long)K);
  if (K % 8 != 0 || K > 512) {
    set_error("arx_rows_bf16_norm: row width K=%lld unsupported (need K %% 8 == 0 and K <= 512)", (long long)K);
    return ARX_EUNSUPPORTED;
  }
  ARX_CHECK_ARG(ldp >= K && ldp % 4 == 0 && ldi >= K && ldi % 8 == 0,
                "arx_rows_bf16_norm: need ldp >= K, ldp %% 4 == 0, ldi >= K, ldi %% 8 == 0 (ldp=%lld ldi=%lld K=%lld)",
                (long long)ldp, (long long)ldi, (long long)K);
  ARX_CHECK_ARG(!((reinterpret_cast<uintptr_t>(P) | reinterpret_cast<uintptr_t>(img)) & 15),
                "arx_rows_bf16_norm: P and img must be 16-byte aligned");
  if (N == 0) return ARX_OK;
  int L = 1;
  while (L * 8 < K) L <<= 1;
  int64_t g = ceil_div(ceil_div(N, (int64_t)(64 / L)), (int64_t)4);
  const int64_t cap = (int64_t)cu_count() * 16;
  if (g > cap) g = cap;
  hipStream_t s = as_stream(stream);
#define ARX_ROWS_CASE(LL)                                                \
  case LL:                                                               \
    rows_launch<LL>((int)g, s, P, ldp, N, (int)K, img, ldi, norms);      \
    break;
  switch (L) {
    ARX_ROWS_CASE(1)
    ARX_ROWS_CASE(2)
    ARX_ROWS_CASE(4)
    ARX_ROWS_CASE(8)
    ARX_ROWS_CASE(16)
    ARX_ROWS_CASE(32)
    ARX_ROWS_CASE(64)
  }
#undef ARX_ROWS_CASE
  ARX_CHECK_LAUNCH();
  return ARX_OK;
}

int arx_gemm_nt_topk_filter_bf16(const float* A, int64_t lda, int64_t M, const uint16_t* Bimg, int64_t ldbi,
                                 const float* coln, int64_t N, int64_t K, float coeff, const float* col_bias,
                                 const float* thr, int64_t ldthr, int32_t col_base, float* cand_v, int32_t* cand_i,
                                 int64_t ldcand, int capp, int* overflow, const int32_t* row_keys, int64_t key_rows,
                                 const int32_t* ex_ptr, const int32_t* ex_cols, const int32_t* col_tags,
                                 const int32_t* want_any, const int32_t* want_all, int64_t want_rows, void* stream) {
  ARX_CHECK_ARG(A && Bimg && coln && thr && cand_v && cand_i && overflow,
                "arx_gemm_nt_topk_filter_bf16: null pointer (col_bias, the exclusion lists and the tag arrays may be "
                "NULL)");
  if (!(K == 32 || K == 64 || K == 128)) {
    set_error("arx_gemm_nt_topk_filter_bf16: K must be 32, 64 or 128 (K=%lld)", (long long)K);
    return ARX_EUNSUPPORTED;
  }
  ARX_CHECK_ARG(M > 0 && N > 0 && capp > 0 && ldcand > 0 && lda >= K && ldbi >= K,
                "arx_gemm_nt_topk_filter_bf16: need M > 0, N > 0, capp > 0, ldcand > 0, lda >= K, ldbi >= K");
  ARX_CHECK_ARG(coeff >= 0.f && coeff < __builtin_inff(),
                "arx_gemm_nt_topk_filter_bf16: coeff must be finite and >= 0");
  const bool excl = row_keys || ex_ptr || ex_cols;
  ARX_CHECK_ARG(!excl || (row_keys && ex_ptr && ex_cols && key_rows > 0),
                "arx_gemm_nt_topk_filter_bf16: row_keys, ex_ptr, ex_cols go together (all NULL: no lists), key_rows > 0");
  const bool tags = col_tags || want_any || want_all;
  ARX_CHECK_ARG(!tags || (col_tags && want_any && want_all && want_rows > 0),
                "arx_gemm_nt_topk_filter_bf16: col_tags, want_any, want_all go together (all NULL: no tags), "
                "want_rows > 0");
  ARX_CHECK_ARG(col_base >= 0 && (int64_t)col_base + N <= 0x7fffffff,
                "arx_gemm_nt_topk_filter_bf16: need col_base >= 0 and col_base + N < 2^31");
  ARX_CHECK_ARG(!((reinterpret_cast<uintptr_t>(A) | reinterpret_cast<uintptr_t>(Bimg)) & 15) && lda % 4 == 0 &&
                    ldbi % 8 == 0,
                "arx_gemm_nt_topk_filter_bf16: operands must be 16-byte aligned (lda %% 4 == 0, ldbi %% 8 == 0)");
  int ns = 0;
  const int rc = arx_gemm_nt_topk_parts(M, N, &ns);               // the split the candidate rows were sized for
  if (rc != ARX_OK) return rc;
  const int64_t tiles_n = ceil_div(N, (int64_t)kBfBN);
  const int64_t tpb = ceil_div(tiles_n, (int64_t)ns);
  ARX_CHECK_ARG((int64_t)ns * capp <= ldcand,
                "arx_gemm_nt_topk_filter_bf16: candidate rows too short (parts * capp > ldcand)");
  const int64_t grid = ceil_div(M, (int64_t)kBfBM) * ns;
  ARX_CHECK_ARG(grid <= 0x7fffffff, "arx_gemm_nt_topk_filter_bf16: grid too large");
  const BfFilter f{thr,      ldthr,    cand_v, cand_i,  ldcand,   capp,     col_base, overflow,
                   coeff,    row_keys, key_rows, ex_ptr, ex_cols, col_tags, want_any, want_all, want_rows};
  hipStream_t s = as_stream(stream);
  if (K == 128)
    k_topk_filter_bf16<128><<<(int)grid, 256, 0, s>>>(M, N, A, lda, Bimg, ldbi, coln, col_bias, (int)tpb, ns, f);
  else if (K == 64)
    k_topk_filter_bf16<64><<<(int)grid, 256, 0, s>>>(M, N, A, lda, Bimg, ldbi, coln, col_bias, (int)tpb, ns, f);
  else
    k_topk_filter_bf16<32><<<(int)grid, 256, 0, s>>>(M, N, A, lda, Bimg, ldbi, coln, col_bias, (int)tpb, ns, f);
  ARX_CHECK_LAUNCH();
  return ARX_OK;
}

int arx_cand_rescore(const float* U, int64_t ldu, int64_t B, const float* P, int64_t ldp, const float* pbias, int64_t V,
                     int d, float* cand_v, const int32_t* cand_i, int64_t ldcand, int64_t ncand, void* stream) {
  ARX_CHECK_ARG(U && P && cand_v && cand_i, "arx_cand_rescore: null pointer (only pbias may be NULL)");
  ARX_CHECK_ARG(B >= 0 && ncand >= 0 && V >= 0 && V <= 0x7fffffffll,
                "arx_cand_rescore: need B >= 0, ncand >= 0, 0 <= V < 2^31 (B=%lld ncand=%lld V=%lld)", (long long)B,
                (long long)ncand, (long long)V);
  ARX_CHECK_ARG(d >= 4 && d % 4 == 0, "arx_cand_rescore: need d %% 4 == 0 and d >= 4 (d=%d)", d);
  if (d > 256) {
    set_error("arx_cand_rescore: embedding size d=%d unsupported (need d <= 256)", d);
    return ARX_EUNSUPPORTED;
  }
  ARX_CHECK_ARG(ldu >= d && ldu % 4 == 0 && ldp >= d && ldp % 4 == 0,
                "arx_cand_rescore: ldu, ldp must be multiples of 4 and >= d (ldu=%lld ldp=%lld d=%d)", (long long)ldu,
                (long long)ldp, d);
  ARX_CHECK_ARG(!((reinterpret_cast<uintptr_t>(U) | reinterpret_cast<uintptr_t>(P)) & 15),
                "arx_cand_rescore: U and P must be 16-byte aligned");
  ARX_CHECK_ARG(ldcand >= ncand, "arx_cand_rescore: need ldcand >= ncand (ldcand=%lld ncand=%lld)", (long long)ldcand,
                (long long)ncand);
  ARX_CHECK_ARG(B == 0 || ncand <= 0x7fffffffll / B, "arx_cand_rescore: need B * ncand < 2^31 (B=%lld ncand=%lld)",
                (long long)B, (long long)ncand);
  if (B == 0 || ncand == 0) return ARX_OK;
  const int L = lanes_per_row(d);
  const int per_pass = kRescoreUnroll * (64 / L);
  const int64_t want = (int64_t)cu_count() * 64;
  int passes = kRescoreMaxPasses;
  while (passes > 1 && B * ceil_div(ncand, (int64_t)per_pass * passes) < want) passes >>= 1;
  const int run = per_pass * passes;
  const int64_t nruns = ceil_div(ncand, (int64_t)run);
  const int64_t units = B * nruns;
  int64_t g = ceil_div(units, (int64_t)4);
  const int64_t cap = (int64_t)cu_count() * 16;
  if (g > cap) g = cap;
  hipStream_t s = as_stream(stream);
#define ARX_RESCORE_CASE(LL)                                                                                        \
  case LL:                                                                                                          \
    rescore_launch<LL>((int)g, s, U, ldu, P, ldp, pbias, (int32_t)V, d, cand_v, cand_i, ldcand, ncand, units, nruns, \
                       run);                                                                                        \
    break;
  switch (L) {
    ARX_RESCORE_CASE(1)
    ARX_RESCORE_CASE(2)
    ARX_RESCORE_CASE(4)
    ARX_RESCORE_CASE(8)
    ARX_RESCORE_CASE(16)
    ARX_RESCORE_CASE(32)
    ARX_RESCORE_CASE(64)
  }
#undef ARX_RESCORE_CASE
  ARX_CHECK_LAUNCH();
  return ARX_OK;
}

}  // extern "C"

// neg_hard.hip -- arx_neg_draw_hardest (arx_neg_hard.h): per batch row, C candidate negatives drawn, scored against the
// row's user and the best one picked, in one launch.
//
// One wave owns one batch row at a time.  Lane j < C runs candidate j's rank-select -- the statement of
// k_neg_draw_uniform / k_neg_draw_weighted (pair.hip), restated here at counter + j; tests/test_neg_draw_hard_gpu.py
// holds the two equal column for column -- and keeps the column and its table row; the scoring reads them by shuffle.
// A group of L lanes (the layout and the order of adds of slate.hip) owns one (row, candidate) pair: 64 / L candidates
// per trip, the user's float4 in registers for the whole row, kHardUnroll trips' table rows loaded before the first
// fold.  Every group keeps the best (v, j) of its own trips; one xor-shuffle fold on (v desc, j asc) gives the pick.
// No LDS, no atomics, nothing depends on the grid.
//
// The chain users[r] -> ex_ptr -> binary search -> col2row -> table row is a string of dependent loads per wave: it is
// hidden by the other 7 waves of the SIMD (8 x cu workgroups of 4 waves fill the chip), not inside the wave.
#include "common.h"

namespace arx {
namespace {

constexpr int kHardUnroll = 4;       // trips whose table rows are in flight together (kSlateUnroll)

struct HardArgs {
  const int32_t* users;
  int64_t B, n_users;
  const int32_t* ex_ptr;
  const int32_t* ex_cols;
  const int64_t* ex_cum;
  const int64_t* cum;
  int32_t V;
  const int32_t* col2item;
  uint64_t seed;
  const uint64_t* step_dev;
  uint64_t counter;
  int C;
  const float* U;
  int64_t ldu, n_urows;
  const int32_t* umap;
  int64_t n_umap;
  const float* P;
  int64_t ldp, n_prows;
  const float* pbias;
  const int32_t* col2row;
  int d;
  int32_t* neg_items;
  int32_t* lookup_items;
  int32_t* out_pick;
  int32_t* out_cand;
  int64_t ldc;
  float* out_score;
  int64_t lds;
};

// k_neg_draw_uniform's column of row r under `seed` (already advanced by the step): the k-th eligible column, -1 where
// that kernel reports -1 for a list that is not sorted and unique.  n_elig > 0 and len >= 0 are the caller's.
__device__ __forceinline__ int32_t hard_col_uniform(const int32_t* __restrict__ ex_cols, int32_t lo, int32_t len,
                                                    int32_t n_elig, int32_t V, uint64_t seed, int64_t r) {
  const uint32_t rnd = mix32(seed * 0x100000001b3ull + (uint64_t)r);
  const int32_t k = (int32_t)__umulhi(rnd, (uint32_t)n_elig);
  int32_t a = 0, b = len;                                 // first j with p_j - j > k
  while (a < b) {
    const int32_t m = a + ((b - a) >> 1);
    if (ex_cols[lo + m] - m <= k) a = m + 1; else b = m;
  }
  const int32_t col = k + a;
  return col < V ? col : -1;
}

// k_neg_draw_weighted's column: the point t of the eligible mass M (> 0, the caller's), its two binary searches.
__device__ __forceinline__ int32_t hard_col_weighted(const int32_t* __restrict__ ex_cols,
                                                     const int64_t* __restrict__ ex_cum,
                                                     const int64_t* __restrict__ cum, int32_t lo, int32_t len,
                                                     int64_t h_len, int64_t M, int32_t V, uint64_t seed, int64_t r) {
  const uint64_t rnd = mix64(seed * 0x100000001b3ull + (uint64_t)r);
  const int64_t t = (int64_t)__umul64hi(rnd, (uint64_t)M);
  int32_t a = 0, b = len;                                 // first j with cum[p_j] - H(j) > t
  while (a < b) {
    const int32_t m = a + ((b - a) >> 1);
    const int32_t p = ex_cols[lo + m];
    const int32_t pc = p < 0 ? 0 : (p > V ? V : p);
    if (cum[pc] - ex_cum[lo + m] <= t) a = m + 1; else b = m;
  }
  const int64_t tp = t + (a < len ? ex_cum[lo + a] : h_len);
  int32_t c0 = 0, c1 = V;                                 // cum[c0] <= t' (cum[0] = 0), c1 = V or cum[c1] > t'
  while (c1 - c0 > 1) {
    const int32_t m = c0 + ((c1 - c0) >> 1);
    if (cum[m] <= tp) c0 = m; else c1 = m;
  }
  return c0;
}

template <int L>
__global__ __launch_bounds__(256) void k_neg_draw_hardest(const HardArgs a) {
  constexpr int S = 64 / L;                               // candidates per trip
  const int lane = threadIdx.x & 63, li = lane & (L - 1), gw = lane / L;
  const bool incol = li * 4 < a.d;
  const int C = a.C;
  const int trips = (C + S - 1) / S;
  const int64_t wave = blockIdx.x * (int64_t)(blockDim.x >> 6) + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x >> 6);
  const uint64_t step = (a.step_dev ? *a.step_dev : 0ull) + a.counter;
  // candidate j = lane: the seed of the plain draw at counter + j
  const uint64_t seed = a.seed + (step + (uint64_t)lane) * 0x9e3779b97f4a7c15ull;
  const bool weighted = a.cum != nullptr;
  const int64_t total = weighted ? a.cum[a.V] : 0;
  const float ninf = -__builtin_inff();
  for (int64_t r = wave; r < a.B; r += nwaves) {          // (everything up to `draws` is wave-uniform)
    const int32_t u = a.users[r];
    int64_t urow = u;
    if (a.umap) urow = (u >= 0 && u < a.n_umap) ? a.umap[u] : -1;
    const bool has_u = urow >= 0 && urow < a.n_urows;
    int32_t lo = 0, len = 0;
    if (u >= 0 && u < a.n_users) {
      lo = a.ex_ptr[u];
      len = a.ex_ptr[u + 1] - lo;
    }
    int64_t h_len = 0, M = 0;
    bool draws;                                           // the plain draw is not void
    if (weighted) {
      if (len > 0) {
        const int32_t p = a.ex_cols[lo + len - 1];
        const int32_t pc = p < 0 ? 0 : (p > a.V ? a.V : p);
        const int32_t pn = p < 0 ? 0 : (p >= a.V ? a.V : p + 1);
        h_len = a.ex_cum[lo + len - 1] + (a.cum[pn] - a.cum[pc]);
      }
      M = total - h_len;
      draws = M > 0 && len >= 0;
    } else {
      draws = a.V - len > 0 && len >= 0;
    }
    if (!(draws && has_u)) {                              // a void row
      if (lane < C) {
        if (a.out_cand) a.out_cand[r * a.ldc + lane] = -1;
        if (a.out_score) a.out_score[r * a.lds + lane] = ninf;
      }
      if (lane == 0) {
        a.neg_items[r] = -1;
        if (a.lookup_items) a.lookup_items[r] = a.col2item ? a.col2item[0] : 0;
        if (a.out_pick) a.out_pick[r] = -1;
      }
      continue;
    }
    int32_t col = -1, prow = -1;                          // lane j < C: candidate j's column and its row of P
    if (lane < C) {
      col = weighted ? hard_col_weighted(a.ex_cols, a.ex_cum, a.cum, lo, len, h_len, M, a.V, seed, r)
                     : hard_col_uniform(a.ex_cols, lo, len, a.V - len, a.V, seed, r);
      if (col >= 0) {
        const int64_t pr = a.col2row ? a.col2row[col] : col;
        if (pr >= 0 && pr < a.n_prows) prow = (int32_t)pr;
      }
      if (a.out_cand) a.out_cand[r * a.ldc + lane] = col;
    }
    float4 uu = make_float4(0.f, 0.f, 0.f, 0.f);
    if (incol) uu = *reinterpret_cast<const float4*>(a.U + urow * a.ldu + li * 4);
    float bv = ninf;                                      // this group's best (v, j); no candidate yet
    int bj = 64;
    for (int t0 = 0; t0 < trips; t0 += kHardUnroll) {     // (wave-uniform bounds: every lane shuffles)
      int32_t pr[kHardUnroll];
      float4 p[kHardUnroll];
      float b[kHardUnroll];
#pragma unroll
      for (int t = 0; t < kHardUnroll; ++t) {
        const int jj = (t0 + t) * S + gw;
        pr[t] = __shfl(prow, jj & 63, 64);
        if (jj >= C) pr[t] = -1;
      }
#pragma unroll
      for (int t = 0; t < kHardUnroll; ++t) {
        const bool ok = pr[t] >= 0;
        p[t] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (ok && incol) p[t] = *reinterpret_cast<const float4*>(a.P + (int64_t)pr[t] * a.ldp + li * 4);
        b[t] = ok && a.pbias ? a.pbias[pr[t]] : 0.f;
      }
#pragma unroll
      for (int t = 0; t < kHardUnroll; ++t) {
        float s = uu.x * p[t].x;                          // (arx_slate.h: the order of the adds)
        s = fmaf(uu.y, p[t].y, s);
        s = fmaf(uu.z, p[t].z, s);
        s = fmaf(uu.w, p[t].w, s);
#pragma unroll
        for (int o = 1; o < L; o <<= 1) s += __shfl_xor(s, o, 64);
        const int jj = (t0 + t) * S + gw;
        if (jj < C) {
          const float sc = pr[t] >= 0 ? (a.pbias ? s + b[t] : s) : ninf;
          if (li == 0 && a.out_score) a.out_score[r * a.lds + jj] = sc;
          const float v = sc != sc ? ninf : sc;
          if (v > bv || (v == bv && jj < bj)) {
            bv = v;
            bj = jj;
          }
        }
      }
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {                    // (v desc, j asc) is a total order: every lane ends equal
      const float ov = __shfl_xor(bv, o, 64);
      const int oj = __shfl_xor(bj, o, 64);
      if (ov > bv || (ov == bv && oj < bj)) {
        bv = ov;
        bj = oj;
      }
    }
    const int32_t cp = __shfl(col, bj & 63, 64);          // (candidate 0 always competes: bj < C)
    if (lane == 0) {
      const int32_t item = cp >= 0 ? (a.col2item ? a.col2item[cp] : cp) : -1;
      a.neg_items[r] = item;
      if (a.lookup_items) a.lookup_items[r] = item >= 0 ? item : (a.col2item ? a.col2item[0] : 0);
      if (a.out_pick) a.out_pick[r] = bj;
    }
  }
}

template <int L>
void hard_launch(int g, hipStream_t s, const HardArgs& a) {
  k_neg_draw_hardest<L><<<g, 256, 0, s>>>(a);
}

}  // namespace
}  // namespace arx

using namespace arx;

extern "C" {

int arx_neg_draw_hardest(const int32_t* users, int64_t B, int64_t n_users, const int32_t* ex_ptr,
                         const int32_t* ex_cols, const int64_t* ex_cum, const int64_t* cum, int64_t V,
                         const int32_t* col2item, uint64_t seed, const uint64_t* step_dev, uint64_t counter, int C,
                         const float* U, int64_t ldu, int64_t n_urows, const int32_t* umap, int64_t n_umap,
                         const float* P, int64_t ldp, int64_t n_prows, const float* pbias, const int32_t* col2row,
                         int d, int32_t* neg_items, int32_t* lookup_items, int32_t* out_pick, int32_t* out_cand,
                         int64_t ldc, float* out_score, int64_t lds, void* stream) {
  ARX_CHECK_ARG(B >= 0 && n_users >= 0 && n_umap >= 0, "arx_neg_draw_hardest: B < 0, n_users < 0 or n_umap < 0");
  ARX_CHECK_ARG(V > 0 && V < ((int64_t)1 << 31), "arx_neg_draw_hardest: need 0 < V < 2^31");
  ARX_CHECK_ARG(C >= 2 && C <= 64, "arx_neg_draw_hardest: need 2 <= C <= 64 candidates (C=%d)", C);
  ARX_CHECK_ARG(users && ex_ptr && ex_cols && U && P && neg_items,
                "arx_neg_draw_hardest: null pointer (users, ex_ptr, ex_cols, U, P and neg_items are required)");
  ARX_CHECK_ARG((cum != nullptr) == (ex_cum != nullptr),
                "arx_neg_draw_hardest: cum and ex_cum are both null (uniform) or both set (weighted)");
  if (d < 4 || d % 4 != 0 || d > 256) {
    set_error("arx_neg_draw_hardest: embedding size d=%d unsupported (need d %% 4 == 0 and 4 <= d <= 256)", d);
    return ARX_EUNSUPPORTED;
  }
  ARX_CHECK_ARG(n_urows >= 0 && n_urows < ((int64_t)1 << 31) && n_prows >= 0 && n_prows < ((int64_t)1 << 31),
                "arx_neg_draw_hardest: need 0 <= n_urows, n_prows < 2^31");
  ARX_CHECK_ARG(ldu >= d && ldu % 4 == 0 && ldp >= d && ldp % 4 == 0,
                "arx_neg_draw_hardest: ldu, ldp must be multiples of 4 and >= d (ldu=%lld ldp=%lld d=%d)",
                (long long)ldu, (long long)ldp, d);
  ARX_CHECK_ARG(!((reinterpret_cast<uintptr_t>(U) | reinterpret_cast<uintptr_t>(P)) & 15),
                "arx_neg_draw_hardest: U and P must be 16-byte aligned");
  ARX_CHECK_ARG((!out_cand || ldc >= C) && (!out_score || lds >= C),
                "arx_neg_draw_hardest: need ldc >= C and lds >= C (ldc=%lld lds=%lld C=%d)", (long long)ldc,
                (long long)lds, C);
  if (B == 0) return ARX_OK;
  const HardArgs a = {users, B, n_users, ex_ptr, ex_cols, ex_cum, cum, (int32_t)V, col2item, seed, step_dev, counter,
                      C, U, ldu, n_urows, umap, n_umap, P, ldp, n_prows, pbias, col2row, d, neg_items, lookup_items,
                      out_pick, out_cand, ldc, out_score, lds};
  int64_t g = ceil_div(B, (int64_t)4);                    // one wave per row, 4 waves per workgroup
  const int64_t cap = (int64_t)cu_count() * 8;
  if (g > cap) g = cap;
  hipStream_t s = as_stream(stream);
#define ARX_HARD_CASE(LL) \
  case LL:                \
    hard_launch<LL>((int)g, s, a); \
    break;
  switch (lanes_per_row(d)) {
    ARX_HARD_CASE(1)
    ARX_HARD_CASE(2)
    ARX_HARD_CASE(4)
    ARX_HARD_CASE(8)
    ARX_HARD_CASE(16)
    ARX_HARD_CASE(32)
    ARX_HARD_CASE(64)
  }
#undef ARX_HARD_CASE
  ARX_CHECK_LAUNCH();
  return ARX_OK;
}

}  // extern "C"

// explain.hip -- explain_items: the score of every (row, slot) pair of a candidate slate taken apart into the
// contributions of the item's output features and of the tokens of its bags (arx_explain.h).  A dependent gather chain
// like k_gather_mulhot (slot -> starts / lens -> vals -> table rows) with a dot per fetched row; bound by the row
// fetches (HBM / L2), not by arithmetic.  [B, C, len, d] is never materialised.
//
// A GROUP of L lanes (L the smallest power of two >= d / 4; 64 / L groups per wave) owns one (row, slot) pair: it holds
// its u fragment in registers (one float4 per lane, lanes past d / 4 hold zeros), walks the item's features in index
// order and a bag L tokens at a time -- lane j of the group loads token j and its bias coalesced, the group broadcasts
// them by shuffles and issues the row loads of four tokens back to back before the first reduction --, folds every dot
// by xor shuffles 1, 2, 4, ... and keeps the running top T in registers (every lane of the group holds the same list:
// after the fold all of them know the value).  No LDS, no atomics, no loop over pairs: the grid is not capped.  The
// order of the adds of one pair depends on d, F and the item's bags only (the header states it; tests check the bits).
#include "common.h"

namespace arx {
namespace {

struct ExplainFeats {
  const float* E[ARX_EXPLAIN_MAX_FEATS];
  const float* bias[ARX_EXPLAIN_MAX_FEATS];     // null: no bias
  const int32_t* map[ARX_EXPLAIN_MAX_FEATS];    // cat: cat_map (null: identity); mulhot: vals
  const int32_t* starts[ARX_EXPLAIN_MAX_FEATS];
  const int32_t* lens[ARX_EXPLAIN_MAX_FEATS];
  int64_t lde[ARX_EXPLAIN_MAX_FEATS];
  int kind[ARX_EXPLAIN_MAX_FEATS];
};

template <int L>
__device__ __forceinline__ float group_dot(const float4& u, const float4& e) {
  float s = u.x * e.x;
  s = fmaf(u.y, e.y, s);
  s = fmaf(u.z, e.z, s);
  s = fmaf(u.w, e.w, s);
#pragma unroll
  for (int o = 1; o < L; o <<= 1) s += __shfl_xor(s, o, 64);
  return s;
}

// The running top TT by (value desc, arrival asc): entries arrive in (feature asc, position asc) order, so a newcomer
// goes in front of the first entry it beats STRICTLY -- or of the first free place -- and everything behind moves down
// one.  A NaN beats nothing and takes no free place.
template <int TT>
struct TopList {
  float v[TT > 0 ? TT : 1];
  int32_t id[TT > 0 ? TT : 1];
  int32_t ft[TT > 0 ? TT : 1];
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int k = 0; k < TT; ++k) {
      v[k] = -__builtin_inff();
      id[k] = -1;
      ft[k] = -1;
    }
  }
  __device__ __forceinline__ void push(float x, int32_t tok, int32_t f) {
    bool moving = false;
#pragma unroll
    for (int k = 0; k < TT; ++k) {
      moving = moving || x > v[k] || (id[k] < 0 && x == x);
      const float ov = v[k];
      const int32_t oi = id[k], of = ft[k];
      v[k] = moving ? x : ov;
      id[k] = moving ? tok : oi;
      ft[k] = moving ? f : of;
      x = moving ? ov : x;
      tok = moving ? oi : tok;
      f = moving ? of : f;
    }
  }
};

// pair p = r * C + j of n = B * C: group (wave, p % GPW) of the launch, no loop (the grid covers n)
template <int L, int TT>
__global__ __launch_bounds__(256) void k_explain_slate(const float* __restrict__ U, int64_t ldu, int d,
                                                       const int32_t* __restrict__ cand, int64_t ldc, int64_t C,
                                                       int32_t V, int64_t n, int F, const ExplainFeats ft, int T,
                                                       float* __restrict__ feat, int64_t ldf,
                                                       float* __restrict__ bias, int64_t ldb,
                                                       float* __restrict__ tok_val, int32_t* __restrict__ tok_id,
                                                       int32_t* __restrict__ tok_feat, int64_t ldt) {
  constexpr int GPW = 64 / L;
  const int lane = threadIdx.x & 63, li = lane & (L - 1), gid = lane / L;
  const bool live = li * 4 < d;
  const int64_t wave = blockIdx.x * (int64_t)(blockDim.x >> 6) + (threadIdx.x >> 6);
  const int64_t p = wave * GPW + gid;
  if (p >= n) return;                                              // (a whole group leaves: shuffles stay inside one)
  const int64_t r = p / C, j = p - r * C;
  const int32_t c = cand[r * ldc + j];
  const bool ok = (uint32_t)c < (uint32_t)V;                       // (an empty slot: nothing is read)
  float* fo = feat ? feat + r * ldf + j * F : nullptr;
  TopList<TT> top;
  top.clear();
  float btot = 0.f;
  if (ok) {
    float4 u = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live) u = *reinterpret_cast<const float4*>(U + r * ldu + li * 4);
    const float invF = 1.0f / (float)F;
    for (int f = 0; f < F; ++f) {
      const float* __restrict__ E = ft.E[f] + li * 4;
      const float* __restrict__ fb = ft.bias[f];
      const int32_t* __restrict__ map = ft.map[f];
      const int64_t lde = ft.lde[f];
      if (ft.kind[f] == ARX_EXPLAIN_CAT) {
        const int32_t row = map ? map[c] : c;
        float4 e = make_float4(0.f, 0.f, 0.f, 0.f);
        if (live) e = *reinterpret_cast<const float4*>(E + (int64_t)row * lde);
        const float b = fb ? fb[row] : 0.f;
        const float s = group_dot<L>(u, e);
        if (fo && li == 0) fo[f] = (s + b) * invF;
        btot += b * invF;
        continue;
      }
      const int32_t st = ft.starts[f][c];
      const int32_t len = ft.lens[f][c];
      const float coef = 1.0f / ((float)F * (float)len);
      float fsum = 0.f, bsum = 0.f;
      for (int32_t j0 = 0; j0 < len; j0 += L) {
        const int32_t myj = j0 + li;
        const int32_t mytok = myj < len ? map[st + myj] : 0;
        const float myb = (fb && myj < len) ? fb[mytok] : 0.f;
        const int cnt = min(L, len - j0);
        int t = 0;
        for (; t + 4 <= cnt; t += 4) {                            // (L >= 4 only: four rows in flight per lane)
          int32_t tk[4];
          float4 e[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) tk[q] = __shfl(mytok, t + q, L);
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            e[q] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (live) e[q] = *reinterpret_cast<const float4*>(E + (int64_t)tk[q] * lde);
          }
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const float b = __shfl(myb, t + q, L);
            const float x = group_dot<L>(u, e[q]) + b;
            const bool first = j0 + t + q == 0;
            fsum = first ? x : fsum + x;
            bsum = first ? b : bsum + b;
            if (TT > 0) top.push(x * coef, tk[q], f);
          }
        }
        for (; t < cnt; ++t) {
          const int32_t tk = __shfl(mytok, t, L);
          float4 e = make_float4(0.f, 0.f, 0.f, 0.f);
          if (live) e = *reinterpret_cast<const float4*>(E + (int64_t)tk * lde);
          const float b = __shfl(myb, t, L);
          const float x = group_dot<L>(u, e) + b;
          const bool first = j0 + t == 0;
          fsum = first ? x : fsum + x;
          bsum = first ? b : bsum + b;
          if (TT > 0) top.push(x * coef, tk, f);
        }
      }
      if (fo && li == 0) fo[f] = fsum * coef;
      btot += bsum * coef;
    }
  } else if (fo && li == 0) {
    for (int f = 0; f < F; ++f) fo[f] = 0.f;
  }
  if (li != 0) return;
  if (bias) bias[r * ldb + j] = btot;
  if (TT > 0) {
    const int64_t o = r * ldt + j * T;
#pragma unroll
    for (int k = 0; k < TT; ++k) {
      if (k < T) {
        tok_val[o + k] = top.v[k];
        tok_id[o + k] = top.id[k];
        tok_feat[o + k] = top.ft[k];
      }
    }
  }
}

template <int L>
void explain_launch(int tt, int64_t g, hipStream_t s, const float* U, int64_t ldu, int d, const int32_t* cand,
                    int64_t ldc, int64_t C, int32_t V, int64_t n, int F, const ExplainFeats& ft, int T, float* feat,
                    int64_t ldf, float* bias, int64_t ldb, float* tok_val, int32_t* tok_id, int32_t* tok_feat,
                    int64_t ldt) {
#define ARX_EXPLAIN_GO(TT)                                                                                          \
  k_explain_slate<L, TT><<<(unsigned)g, 256, 0, s>>>(U, ldu, d, cand, ldc, C, V, n, F, ft, T, feat, ldf, bias, ldb, \
                                                     tok_val, tok_id, tok_feat, ldt)
  if (tt == 0) ARX_EXPLAIN_GO(0);
  else if (tt <= 4) ARX_EXPLAIN_GO(4);
  else ARX_EXPLAIN_GO(16);
#undef ARX_EXPLAIN_GO
}

}  // namespace
}  // namespace arx

using namespace arx;

extern "C" {

int arx_explain_slate(const float* U, int64_t ldu, int64_t B, int d, const int32_t* cand, int64_t ldc, int64_t C,
                      int64_t V, int F, const int* kind, const float* const* E, const int64_t* lde,
                      const float* const* fbias, const int32_t* const* cat_map, const int32_t* const* vals,
                      const int32_t* const* starts, const int32_t* const* lens, int T, float* feat, int64_t ldf,
                      float* bias, int64_t ldb, float* tok_val, int32_t* tok_id, int32_t* tok_feat, int64_t ldt,
                      void* stream) {
  ARX_CHECK_ARG(U && cand && kind && E && lde, "arx_explain_slate: null pointer (U, cand, kind, E, lde are required)");
  ARX_CHECK_ARG(F >= 1 && F <= ARX_EXPLAIN_MAX_FEATS, "arx_explain_slate: need 1 <= F <= 8 (F=%d)", F);
  ARX_CHECK_ARG(T >= 0 && T <= ARX_EXPLAIN_MAX_TOP, "arx_explain_slate: need 0 <= T <= 16 (T=%d)", T);
  if (d < 4 || d > 256 || d % 4) {
    set_error("arx_explain_slate: embedding size d=%d unsupported (need d %% 4 == 0 and 4 <= d <= 256)", d);
    return ARX_EUNSUPPORTED;
  }
  ARX_CHECK_ARG(B >= 0 && C >= 0 && V >= 0 && V <= 0x7fffffffll,
                "arx_explain_slate: need B >= 0, C >= 0, 0 <= V < 2^31 (B=%lld C=%lld V=%lld)", (long long)B,
                (long long)C, (long long)V);
  ARX_CHECK_ARG(ldu >= d && ldu % 4 == 0, "arx_explain_slate: ldu must be a multiple of 4 and >= d (ldu=%lld d=%d)",
                (long long)ldu, d);
  ARX_CHECK_ARG(!(reinterpret_cast<uintptr_t>(U) & 15), "arx_explain_slate: U must be 16-byte aligned");
  const bool any_tok = tok_val || tok_id || tok_feat, all_tok = tok_val && tok_id && tok_feat;
  ARX_CHECK_ARG(any_tok == all_tok, "arx_explain_slate: tok_val, tok_id and tok_feat are NULL together");
  ARX_CHECK_ARG(!(any_tok && T == 0), "arx_explain_slate: tok_* given with T == 0");
  ExplainFeats ft = {};
  for (int f = 0; f < F; ++f) {
    ARX_CHECK_ARG(kind[f] == ARX_EXPLAIN_CAT || kind[f] == ARX_EXPLAIN_MULHOT,
                  "arx_explain_slate: feature %d: kind %d is neither ARX_EXPLAIN_CAT nor ARX_EXPLAIN_MULHOT", f, kind[f]);
    ARX_CHECK_ARG(E[f] && !(reinterpret_cast<uintptr_t>(E[f]) & 15),
                  "arx_explain_slate: feature %d: the table must be set and 16-byte aligned", f);
    ARX_CHECK_ARG(lde[f] >= d && lde[f] % 4 == 0,
                  "arx_explain_slate: feature %d: lde must be a multiple of 4 and >= d (lde=%lld d=%d)", f,
                  (long long)lde[f], d);
    ft.kind[f] = kind[f];
    ft.E[f] = E[f];
    ft.lde[f] = lde[f];
    ft.bias[f] = fbias ? fbias[f] : nullptr;
    if (kind[f] == ARX_EXPLAIN_CAT) {
      ft.map[f] = cat_map ? cat_map[f] : nullptr;
    } else {
      ARX_CHECK_ARG(vals && starts && lens && vals[f] && starts[f] && lens[f],
                    "arx_explain_slate: feature %d: a mulhot feature needs vals / starts / lens", f);
      ft.map[f] = vals[f];
      ft.starts[f] = starts[f];
      ft.lens[f] = lens[f];
    }
  }
  ARX_CHECK_ARG(ldc >= C && (!feat || ldf >= C * F) && (!bias || ldb >= C) && (!any_tok || ldt >= C * T),
                "arx_explain_slate: need ldc >= C, ldf >= C * F, ldb >= C, ldt >= C * T (ldc=%lld ldf=%lld ldb=%lld "
                "ldt=%lld C=%lld F=%d T=%d)", (long long)ldc, (long long)ldf, (long long)ldb, (long long)ldt,
                (long long)C, F, T);
  ARX_CHECK_ARG(B == 0 || C <= 0x7fffffffll / B, "arx_explain_slate: need B * C < 2^31 (B=%lld C=%lld)", (long long)B,
                (long long)C);
  if (B == 0 || C == 0) return ARX_OK;
  if (!feat && !bias && !any_tok) return ARX_OK;
  const int L = lanes_per_row(d);
  const int64_t n = B * C;
  const int64_t g = ceil_div(ceil_div(n, (int64_t)(64 / L)), (int64_t)4);      // (< 2^29: not capped, no pair loop)
  const int tt = any_tok ? T : 0;
  hipStream_t s = as_stream(stream);
#define ARX_EXPLAIN_CASE(LL)                                                                                       \
  case LL:                                                                                                         \
    explain_launch<LL>(tt, g, s, U, ldu, d, cand, ldc, C, (int32_t)V, n, F, ft, T, feat, ldf, bias, ldb, tok_val,  \
                       tok_id, tok_feat, ldt);                                                                     \
    break;
  switch (L) {
    ARX_EXPLAIN_CASE(1)
    ARX_EXPLAIN_CASE(2)
    ARX_EXPLAIN_CASE(4)
    ARX_EXPLAIN_CASE(8)
    ARX_EXPLAIN_CASE(16)
    ARX_EXPLAIN_CASE(32)
    ARX_EXPLAIN_CASE(64)
  }
#undef ARX_EXPLAIN_CASE
  ARX_CHECK_LAUNCH();
  return ARX_OK;
}

}  // extern "C"

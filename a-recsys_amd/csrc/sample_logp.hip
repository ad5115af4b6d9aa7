// sample_logp.hip -- recommend(sample_temperature=, return_logprob=True) (arx_sample_logp.h): the kernels around the
// mass pass.  The streaming form of the pass itself is a mode of the scorer GEMM (gemm_nt.hip, kNtRest); here:
//   k_logp_sort     one wave per row: the row's k picks ranked by column in LDS (a rank sort: k <= 1024), written as
//                   (column, slot) with the -1 entries last -- what both forms of the mass pass walk;
//   k_rest_chunk    the materialised form: one workgroup per row folds a chunk of logits (-inf where ineligible) into
//                   the row's running REST pair, leaves the picks out and writes their scores;
//   k_logp_finish   one wave per row: the P parts (of each of W shard slabs, arx_sample_shard.h) joined in order, then the backward join over the picks in
//                   selection order -- lane l owns the picks [l E, l E + E), E = ceil(k / 64): its own suffix, a suffix
//                   scan over the lanes, its own suffix again on top of what lies above.
// Rows walk grid-stride loops under capped grids; every LDS word is rewritten on every trip.  The order of every join
// depends on k, P and the chunk's width only.
#include "common.h"
#include "rest_mass.h"

namespace arx {
namespace {

constexpr int kLpMaxK = 1024;
constexpr int kLpThreads = 256;
constexpr int kLpWaves = kLpThreads / kWave;

__device__ __forceinline__ RmMass rm_shfl_down(const RmMass a, int o) {
  return RmMass{__shfl_down(a.m, o, 64), __shfl_down(a.s, o, 64)};
}

__global__ __launch_bounds__(kLpThreads) void k_logp_sort(const int32_t* __restrict__ indices, int64_t ldi, int64_t B,
                                                          int k, int32_t* __restrict__ pk_cols,
                                                          int32_t* __restrict__ pk_slot, int64_t ldp) {
  __shared__ uint32_t cols[kLpWaves][kLpMaxK];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t base = (int64_t)blockIdx.x * kLpWaves; base < B; base += (int64_t)gridDim.x * kLpWaves) {
    const int64_t r = base + wave;
    __syncthreads();                                               // (the last trip's readers are done with the LDS)
    if (r < B)
      for (int j = lane; j < k; j += 64) cols[wave][j] = (uint32_t)indices[r * ldi + j];
    __syncthreads();
    if (r < B)
      for (int j = lane; j < k; j += 64) {
        const uint32_t c = cols[wave][j];
        int rank = 0;
        for (int i = 0; i < k; ++i) {
          const uint32_t x = cols[wave][i];
          rank += (x < c || (x == c && i < j)) ? 1 : 0;
        }
        pk_cols[r * ldp + rank] = (int32_t)c;
        pk_slot[r * ldp + rank] = j;
      }
  }
}

__global__ __launch_bounds__(kLpThreads) void k_rest_chunk(
    const float* __restrict__ logits, int64_t ld, int64_t B, int32_t col0, int64_t ncols, const float* __restrict__ tau,
    int64_t tau_rows, const int32_t* __restrict__ pk_cols, const int32_t* __restrict__ pk_slot, int64_t ldp, int k,
    int first, float* __restrict__ m_run, float* __restrict__ s_run, float* __restrict__ pick_score, int64_t ldps) {
  __shared__ uint32_t pc[kLpMaxK];
  __shared__ int32_t ps[kLpMaxK];
  __shared__ RmMass wt[kLpWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t c_lo = (uint32_t)col0, c_hi = (uint32_t)col0 + (uint32_t)ncols;
  for (int64_t r = blockIdx.x; r < B; r += gridDim.x) {
    __syncthreads();
    for (int j = tid; j < k; j += kLpThreads) {
      pc[j] = (uint32_t)pk_cols[r * ldp + j];
      ps[j] = pk_slot[r * ldp + j];
    }
    __syncthreads();
    const float t = rm_tau(tau[r % tau_rows]);
    const float itau = rm_itau(t);
    // the row's picks inside this chunk: [pb, pe) of the sorted list
    int pb, pe;
    {
      int lo = 0, hi = k;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (pc[mid] < c_lo) lo = mid + 1;
        else hi = mid;
      }
      pb = lo;
      hi = k;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (pc[mid] < c_hi) lo = mid + 1;
        else hi = mid;
      }
      pe = lo;
    }
    float m = -__FLT_MAX__, s = 0.f;
    const float* lr = logits + r * ld;
    for (int64_t c = tid; c < ncols; c += kLpThreads) {
      float v = lr[c];
      if (pb < pe) {
        const uint32_t ac = c_lo + (uint32_t)c;
        int lo = pb, hi = pe;
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (pc[mid] < ac) lo = mid + 1;
          else hi = mid;
        }
        if (lo < pe && pc[lo] == ac) {                             // a pick: its score leaves here, it adds no mass
          pick_score[r * ldps + ps[lo]] = v;
          v = -__builtin_inff();
        }
      }
      rm_add(m, s, v, itau);
    }
    RmMass tot{m, s};
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) tot = rm_join(tot, rm_shfl_down(tot, o), t);
    if (lane == 0) wt[wave] = tot;
    __syncthreads();
    if (tid == 0) {
      RmMass run = first ? rm_empty() : RmMass{m_run[r], s_run[r]};
      for (int w = 0; w < kLpWaves; ++w) run = rm_join(run, wt[w], t);
      m_run[r] = run.m;
      s_run[r] = run.s;
    }
  }
}

// W slabs (arx_sample_logp_finish_shards; W == 1, strides 0: the single-device finish): shard w's parts of row r at
// m_part[w * slab_l + r * ldl + p], its pick scores at pick_score[w * slab_ps + r * ldps + t]; the parts join in
// (shard, part) order and pick t's score is read from the slab of its owner, indices[t] % W
__global__ __launch_bounds__(kLpThreads) void k_logp_finish(
    const int32_t* __restrict__ indices, int64_t ldi, const float* __restrict__ pick_score, int64_t ldps,
    int64_t slab_ps, const float* __restrict__ m_part, const float* __restrict__ s_part, int64_t ldl, int64_t slab_l,
    int W, int P, const float* __restrict__ tau, int64_t tau_rows, int64_t B, int k, float* __restrict__ logp,
    int64_t ldo, float* __restrict__ values, int64_t ldv) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int E = (k + 63) / 64;
  const int lo = min(k, lane * E), hi = min(k, lane * E + E);
  for (int64_t r = (int64_t)blockIdx.x * kLpWaves + wave; r < B; r += (int64_t)gridDim.x * kLpWaves) {
    const float tau0 = tau[r % tau_rows];
    const float t = rm_tau(tau0);
    RmMass rest = rm_empty();
    for (int w = 0; w < W; ++w)
      for (int p = 0; p < P; ++p) {
        const int64_t at = w * slab_l + r * ldl + p;
        rest = rm_join(rest, RmMass{m_part[at], s_part[at]}, t);
      }
    const int32_t* ir = indices + r * ldi;
    const float* sr = pick_score + r * ldps;
    // (an index < 0 reads slab 0: the value is not used)
    auto score = [&](int j) { return sr[(ir[j] >= 0 ? ir[j] % W : 0) * slab_ps + j]; };
    RmMass acc = rm_empty();
    for (int j = hi - 1; j >= lo; --j) {
      const float sj = score(j);
      if (ir[j] >= 0 && sj > -__builtin_inff()) acc = rm_join(RmMass{sj, 1.f}, acc, t);
    }
    // the wave: tot = this lane's picks and those of the lanes above it
    RmMass tot = acc;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const RmMass j = rm_join(tot, rm_shfl_down(tot, o), t);
      if (lane + o < 64) tot = j;
    }
    RmMass above = rm_shfl_down(tot, 1);
    if (lane == 63) above = rm_empty();
    acc = rm_join(above, rest, t);
    for (int j = hi - 1; j >= lo; --j) {
      const float sj = score(j);
      const bool live = ir[j] >= 0 && sj > -__builtin_inff();        // (a -inf score is not eligible: a -1 column)
      const float s = live ? sj : -__builtin_inff();
      float lp = 0.f;
      if (live) {
        acc = rm_join(RmMass{s, 1.f}, acc, t);
        if (tau0 > 0.f) lp = (s - acc.m) / t - logf(acc.s);
      }
      logp[r * ldo + j] = lp;
      if (values) values[r * ldv + j] = s;
    }
  }
}

inline int lp_grid(int64_t units) {
  const int64_t cap = (int64_t)cu_count() * 8;
  return (int)(units < cap ? units : cap);
}

}  // namespace
}  // namespace arx

using namespace arx;

extern "C" {

int arx_sample_logp_sort(const int32_t* indices, int64_t ldi, int64_t B, int k, int32_t* pk_cols, int32_t* pk_slot,
                         int64_t ldp, void* stream) {
  ARX_CHECK_ARG(indices && pk_cols && pk_slot, "arx_sample_logp_sort: null pointer");
  ARX_CHECK_ARG(B >= 0, "arx_sample_logp_sort: need B >= 0 (B=%lld)", (long long)B);
  ARX_CHECK_ARG(k >= 1 && k <= kLpMaxK, "arx_sample_logp_sort: need 1 <= k <= %d (k=%d)", kLpMaxK, k);
  ARX_CHECK_ARG(ldi >= k && ldp >= k, "arx_sample_logp_sort: need ldi >= k and ldp >= k (ldi=%lld ldp=%lld k=%d)",
                (long long)ldi, (long long)ldp, k);
  if (B == 0) return ARX_OK;
  k_logp_sort<<<lp_grid(ceil_div(B, (int64_t)kLpWaves)), kLpThreads, 0, as_stream(stream)>>>(indices, ldi, B, k,
                                                                                              pk_cols, pk_slot, ldp);
  ARX_CHECK_LAUNCH();
  return ARX_OK;
}

int arx_rest_mass_chunk(const float* logits, int64_t ld, int64_t B, int32_t col0, int64_t ncols, const float* tau,
                        int64_t tau_rows, const int32_t* pk_cols, const int32_t* pk_slot, int64_t ldp, int k, int first,
                        float* m_run, float* s_run, float* pick_score, int64_t ldps, void* stream) {
  ARX_CHECK_ARG(logits && tau && pk_cols && pk_slot && m_run && s_run && pick_score,
                "arx_rest_mass_chunk: null pointer");
  ARX_CHECK_ARG(B >= 0 && ncols >= 0 && ld >= ncols, "arx_rest_mass_chunk: need B >= 0, ncols >= 0, ld >= ncols "
                "(B=%lld ncols=%lld ld=%lld)", (long long)B, (long long)ncols, (long long)ld);
  ARX_CHECK_ARG(tau_rows > 0, "arx_rest_mass_chunk: need tau_rows > 0 (tau_rows=%lld)", (long long)tau_rows);
  ARX_CHECK_ARG(col0 >= 0 && (int64_t)col0 + ncols <= 0x7fffffff,
                "arx_rest_mass_chunk: need col0 >= 0 and col0 + ncols < 2^31");
  ARX_CHECK_ARG(k >= 1 && k <= kLpMaxK, "arx_rest_mass_chunk: need 1 <= k <= %d (k=%d)", kLpMaxK, k);
  ARX_CHECK_ARG(ldp >= k && ldps >= k, "arx_rest_mass_chunk: need ldp >= k and ldps >= k (ldp=%lld ldps=%lld k=%d)",
                (long long)ldp, (long long)ldps, k);
  if (B == 0) return ARX_OK;
  k_rest_chunk<<<lp_grid(B), kLpThreads, 0, as_stream(stream)>>>(logits, ld, B, col0, ncols, tau, tau_rows, pk_cols,
                                                                 pk_slot, ldp, k, first, m_run, s_run, pick_score,
                                                                 ldps);
  ARX_CHECK_LAUNCH();
  return ARX_OK;
}

static int logp_finish(const char* fn, const int32_t* indices, int64_t ldi, const float* pick_score, int64_t ldps,
                       int64_t slab_ps, const float* m_part, const float* s_part, int64_t ldl, int64_t slab_l, int W,
                       int P, const float* tau, int64_t tau_rows, int64_t B, int k, float* logp, int64_t ldo,
                       float* values, int64_t ldv, void* stream) {
  ARX_CHECK_ARG(indices && pick_score && m_part && s_part && tau && logp,
                "%s: null pointer (only values may be NULL)", fn);
  ARX_CHECK_ARG(B >= 0, "%s: need B >= 0 (B=%lld)", fn, (long long)B);
  ARX_CHECK_ARG(tau_rows > 0, "%s: need tau_rows > 0 (tau_rows=%lld)", fn, (long long)tau_rows);
  ARX_CHECK_ARG(k >= 1 && k <= kLpMaxK, "%s: need 1 <= k <= %d (k=%d)", fn, kLpMaxK, k);
  ARX_CHECK_ARG(P >= 1 && ldl >= P, "%s: need P >= 1 and ldl >= P (P=%d ldl=%lld)", fn, P, (long long)ldl);
  ARX_CHECK_ARG(ldi >= k && ldps >= k && ldo >= k && (!values || ldv >= k),
                "%s: need ldi, ldps, ldo (and ldv with values) >= k (k=%d)", fn, k);
  ARX_CHECK_ARG(W >= 1 && W <= 64 && (W == 1 || (slab_ps >= 0 && slab_l >= 0)),
                "%s: need 1 <= W <= 64 and slab strides >= 0 (W=%d)", fn, W);
  if (B == 0) return ARX_OK;
  k_logp_finish<<<lp_grid(ceil_div(B, (int64_t)kLpWaves)), kLpThreads, 0, as_stream(stream)>>>(
      indices, ldi, pick_score, ldps, slab_ps, m_part, s_part, ldl, slab_l, W, P, tau, tau_rows, B, k, logp, ldo, values,
      ldv);
  ARX_CHECK_LAUNCH();
  return ARX_OK;
}

int arx_sample_logp_finish(const int32_t* indices, int64_t ldi, const float* pick_score, int64_t ldps,
                           const float* m_part, const float* s_part, int64_t ldl, int P, const float* tau,
                           int64_t tau_rows, int64_t B, int k, float* logp, int64_t ldo, float* values, int64_t ldv,
                           void* stream) {
  return logp_finish("arx_sample_logp_finish", indices, ldi, pick_score, ldps, 0, m_part, s_part, ldl, 0, 1, P, tau,
                     tau_rows, B, k, logp, ldo, values, ldv, stream);
}

int arx_sample_logp_finish_shards(const int32_t* indices, int64_t ldi, const float* pick_score, int64_t ldps,
                                  int64_t slab_ps, const float* m_part, const float* s_part, int64_t ldl,
                                  int64_t slab_l, int W, int P, const float* tau, int64_t tau_rows, int64_t B, int k,
                                  float* logp, int64_t ldo, float* values, int64_t ldv, void* stream) {
  return logp_finish("arx_sample_logp_finish_shards", indices, ldi, pick_score, ldps, slab_ps, m_part, s_part, ldl,
                     slab_l, W, P, tau, tau_rows, B, k, logp, ldo, values, ldv, stream);
}

}  // extern "C"

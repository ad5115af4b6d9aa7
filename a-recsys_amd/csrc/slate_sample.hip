// slate_sample.hip -- score_items(sample_temperature=): k draws without replacement from softmax(score / tau) over a
// scored slate, with the log-probability of every draw (arx_slate_sample.h).  One workgroup owns a request row and
// keeps the row in LDS:
//   1. every slot becomes a 64-bit sort word -- the key's order-preserving image (arx_topk's) in the high half, ~slot
//      in the low half; 0 for a slot that is not live and for the padding up to N, the next power of two (>= 64);
//   2. one descending bitonic sort over the N words gives (key desc, slot asc), everything that is not live last;
//   3. position p of the sorted order belongs to thread p / E (E = N / threads in {1, 2, 4}): it takes its slot's score
//      and id into registers and rewrites its word as (key image, id); a backward walk over the run of equal keys finds
//      an earlier slot with the same id -- that slot does not compete;
//   4. one suffix scan over the sorted order of (largest score, sum of exp((s - largest) / tau), competitors): serial
//      over the thread's E positions, shuffles inside a wave, the waves' totals through LDS;
//   5. the competitor of rank t < k writes column t of the outputs; the columns past the last competitor are padding.
// Threads: 64 up to N = 128, 128 at N = 256, 256 above.  The grid is capped at 8 workgroups per CU and rows walk a
// grid-stride loop: every LDS word is rewritten on every trip.
#include "common.h"
#include "gumbel.h"

namespace arx {
namespace {

constexpr int kSsMaxC = 1024;
constexpr int kSsMaxThreads = 256;
constexpr int kSsMaxWaves = kSsMaxThreads / kWave;

// larger float <-> larger unsigned, as arx_topk orders its values (topk.hip ord_key): -0 < +0
__device__ __forceinline__ uint32_t ss_ord(float x) {
  const uint32_t b = __float_as_uint(x);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ bool ss_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

// what is left from a position on: m the largest score, s = sum exp((score - m) / tau), n competitors (n == 0: nothing)
struct SsMass {
  float m, s;
  int n;
};

// MASS false: the counts only (logp == NULL, or a tau == 0 row)
template <bool MASS>
__device__ __forceinline__ SsMass ss_join(const SsMass a, const SsMass b, float tau) {
  SsMass o;
  o.n = a.n + b.n;
  o.m = 0.f;
  o.s = 0.f;
  if (MASS) {
    const bool ge = a.m >= b.m;
    const float hi = ge ? a.m : b.m, lo = ge ? b.m : a.m;
    const float sh = ge ? a.s : b.s, sl = ge ? b.s : a.s;
    const float f = expf((lo - hi) / tau);
    o.m = hi;
    o.s = fmaf(sl, f, sh);
    // (an empty side: -inf - -inf has no value)
    if (a.n == 0) { o.m = b.m; o.s = b.s; }
    if (b.n == 0) { o.m = a.m; o.s = a.s; }
  }
  return o;
}

__device__ __forceinline__ SsMass ss_shfl_down(const SsMass a, int o) {
  SsMass b;
  b.m = __shfl_down(a.m, o, 64);
  b.s = __shfl_down(a.s, o, 64);
  b.n = __shfl_down(a.n, o, 64);
  return b;
}

template <int E, bool MASS>
__device__ __forceinline__ void ss_finish(const float (&s)[E], const bool (&comp)[E], float tau, SsMass* wt, int tid,
                                          int waves, SsMass (&full)[E], int& total) {
  const int lane = tid & 63, wave = tid >> 6;
  const float ninf = -__builtin_inff();
  SsMass acc = {ninf, 0.f, 0};
#pragma unroll
  for (int e = E - 1; e >= 0; --e) {
    const SsMass leaf = {comp[e] ? s[e] : ninf, comp[e] ? 1.f : 0.f, comp[e] ? 1 : 0};
    acc = ss_join<MASS>(leaf, acc, tau);
    full[e] = acc;
  }
  // the wave: tot = this lane's positions and everything of the lanes above it
  SsMass tot = acc;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const SsMass up = ss_shfl_down(tot, o);
    const SsMass j = ss_join<MASS>(tot, up, tau);
    if (lane + o < 64) tot = j;
  }
  SsMass ex = ss_shfl_down(tot, 1);
  if (lane == 63) ex = SsMass{ninf, 0.f, 0};
  if (lane == 0) wt[wave] = tot;
  __syncthreads();
  SsMass above = {ninf, 0.f, 0};
  total = 0;
  for (int w = waves - 1; w >= 0; --w) {
    const SsMass x = wt[w];
    total += x.n;
    if (w > wave) above = ss_join<MASS>(x, above, tau);
  }
  ex = ss_join<MASS>(ex, above, tau);
#pragma unroll
  for (int e = 0; e < E; ++e) full[e] = ss_join<MASS>(full[e], ex, tau);
}

template <int E>
__global__ __launch_bounds__(kSsMaxThreads) void k_slate_sample(
    const int32_t* __restrict__ cand, int64_t ldc, const float* __restrict__ scores, int64_t lds, int64_t B, int C,
    int N, const float* __restrict__ tau, int64_t tau_rows, const int32_t* __restrict__ seed_words, int k,
    int32_t* __restrict__ ids, int64_t ldi, float* __restrict__ values, int64_t ldv, int32_t* __restrict__ pos,
    int64_t ldq, float* __restrict__ logp, int64_t ldl) {
  extern __shared__ uint64_t ss_lds[];
  __shared__ SsMass wt[kSsMaxWaves];
  uint64_t* words = ss_lds;                                        // [N]
  float* sc = reinterpret_cast<float*>(words + N);                 // [N] by slot
  int32_t* cid = reinterpret_cast<int32_t*>(sc + N);               // [N] by slot
  const int tid = threadIdx.x, T = blockDim.x, waves = T >> 6;
  const float ninf = -__builtin_inff();

  for (int64_t r = blockIdx.x; r < B; r += gridDim.x) {
    __syncthreads();                                               // (the last row's readers are done with the LDS)
    const int32_t* cr = cand + r * ldc;
    const float* sr = scores + r * lds;
    const int64_t nr = r % tau_rows;
    const float t = tau[nr];
    const GumbelRow gr = gumbel_row(seed_words, nr);
    // ---- 1. the sort words
    for (int j = tid; j < N; j += T) {
      uint64_t w = 0;
      float s = ninf;
      int32_t c = -1;
      if (j < C) {
        c = cr[j];
        s = sr[j];
        if (c >= 0 && ss_finite(s)) {
          const float key = t == 0.f ? s : fmaf(t, gumbel_of_bits(gumbel_bits(gr.b0, gr.b1, (uint32_t)c)), s);
          w = ((uint64_t)ss_ord(key) << 32) | (uint32_t)~j;
        }
      }
      words[j] = w;
      sc[j] = s;
      cid[j] = c;
    }
    __syncthreads();
    // ---- 2. bitonic, descending
    for (int k2 = 2; k2 <= N; k2 <<= 1) {
      for (int j = k2 >> 1; j > 0; j >>= 1) {
        for (int i = tid; i < (N >> 1); i += T) {
          const int l = ((i & ~(j - 1)) << 1) | (i & (j - 1));
          const int h = l | j;
          const uint64_t a = words[l], b = words[h];
          const bool desc = (l & k2) == 0;
          if ((a < b) == desc) {
            words[l] = b;
            words[h] = a;
          }
        }
        __syncthreads();
      }
    }
    // ---- 3. this thread's positions; the same item in a lower slot
    const int p0 = tid * E;
    uint32_t kimg[E];
    int slot[E];
    int32_t id[E];
    float s[E];
    bool comp[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const uint64_t w = words[p0 + e];
      comp[e] = w != 0;
      kimg[e] = (uint32_t)(w >> 32);
      slot[e] = comp[e] ? (int)~(uint32_t)w : 0;
      s[e] = sc[slot[e]];
      id[e] = cid[slot[e]];
      if (comp[e]) words[p0 + e] = (w & 0xffffffff00000000ull) | (uint32_t)id[e];   // (its own word: no reader yet)
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < E; ++e) {
      if (!comp[e]) continue;
      for (int q = p0 + e - 1; q >= 0; --q) {
        const uint64_t x = words[q];
        if ((uint32_t)(x >> 32) != kimg[e]) break;
        if ((uint32_t)x == (uint32_t)id[e]) {
          comp[e] = false;
          break;
        }
      }
    }
    // ---- 4. what is left from every position on
    SsMass full[E];
    int total;
    const bool mass = logp != nullptr && t > 0.f;                  // (the same for every thread)
    if (mass)
      ss_finish<E, true>(s, comp, t, wt, tid, waves, full, total);
    else
      ss_finish<E, false>(s, comp, t, wt, tid, waves, full, total);
    // ---- 5. the picks
    int32_t* ids_r = ids + r * ldi;
    float* val_r = values + r * ldv;
    int32_t* pos_r = pos + r * ldq;
    float* lp_r = logp ? logp + r * ldl : nullptr;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int rank = total - full[e].n;
      if (comp[e] && rank < k) {
        ids_r[rank] = id[e];
        val_r[rank] = s[e];
        pos_r[rank] = slot[e];
        if (lp_r) lp_r[rank] = mass ? (s[e] - full[e].m) / t - logf(full[e].s) : 0.f;
      }
    }
    for (int c = total + tid; c < k; c += T) {
      ids_r[c] = -1;
      val_r[c] = ninf;
      pos_r[c] = -1;
      if (lp_r) lp_r[c] = 0.f;
    }
  }
}

inline bool ss_supported(int64_t C) { return C >= 1 && C <= kSsMaxC; }

}  // namespace
}  // namespace arx

using namespace arx;

extern "C" {

int arx_slate_sample_supported(int64_t C) { return ss_supported(C) ? 1 : 0; }

int arx_slate_sample(const int32_t* cand, int64_t ldc, const float* scores, int64_t lds, int64_t B, int64_t C,
                     const float* tau, int64_t tau_rows, const int32_t* seed_words, int k, int32_t* ids, int64_t ldi,
                     float* values, int64_t ldv, int32_t* pos, int64_t ldq, float* logp, int64_t ldl, void* stream) {
  ARX_CHECK_ARG(cand && scores && tau && seed_words && ids && values && pos,
                "arx_slate_sample: null pointer (only logp may be NULL)");
  ARX_CHECK_ARG(B >= 0 && C >= 0, "arx_slate_sample: need B >= 0 and C >= 0 (B=%lld C=%lld)", (long long)B,
                (long long)C);
  ARX_CHECK_ARG(tau_rows > 0, "arx_slate_sample: need tau_rows > 0 (tau_rows=%lld)", (long long)tau_rows);
  ARX_CHECK_ARG(ldc >= C && lds >= C, "arx_slate_sample: need ldc >= C and lds >= C (ldc=%lld lds=%lld C=%lld)",
                (long long)ldc, (long long)lds, (long long)C);
  ARX_CHECK_ARG(k >= 1 && k <= C, "arx_slate_sample: need 1 <= k <= C (k=%d C=%lld)", k, (long long)C);
  ARX_CHECK_ARG(ldi >= k && ldv >= k && ldq >= k,
                "arx_slate_sample: need ldi, ldv, ldq >= k (ldi=%lld ldv=%lld ldq=%lld k=%d)", (long long)ldi,
                (long long)ldv, (long long)ldq, k);
  ARX_CHECK_ARG(!logp || ldl >= k, "arx_slate_sample: need ldl >= k with logp (ldl=%lld k=%d)", (long long)ldl, k);
  if (!ss_supported(C)) {
    set_error("arx_slate_sample: C=%lld unsupported (arx_slate_sample_supported: need 1 <= C <= %d)", (long long)C,
              kSsMaxC);
    return ARX_EUNSUPPORTED;
  }
  if (B == 0) return ARX_OK;
  int N = kWave;
  while (N < C) N <<= 1;
  const int threads = N <= 128 ? 64 : N == 256 ? 128 : kSsMaxThreads;
  const int E = N / threads;                                       // 1, 2 or 4
  const size_t lds_bytes = (size_t)N * 16;                         // <= 16 KiB: under the default limit
  int64_t g = B;
  const int64_t cap = (int64_t)cu_count() * 8;
  if (g > cap) g = cap;
  auto kern = E == 1 ? k_slate_sample<1> : E == 2 ? k_slate_sample<2> : k_slate_sample<4>;
  kern<<<(int)g, threads, lds_bytes, as_stream(stream)>>>(cand, ldc, scores, lds, B, (int)C, N, tau, tau_rows,
                                                          seed_words, k, ids, ldi, values, ldv, pos, ldq, logp, ldl);
  ARX_CHECK_LAUNCH();
  return ARX_OK;
}

}  // extern "C"

// diverse.hip -- score_items(diversify=): the greedy MMR re-rank of a scored slate (arx_diverse.h).  k dependent
// arg-max steps over C candidates with a cosine update between them: latency bound, so ONE workgroup of 256 threads
// owns a request row and keeps the row's C unit rows in LDS for all k steps.
//
// Thread t owns slots t and t + 256 (C <= 512): their score, rel, pen, group, group count and id live in its registers
// for the whole row.  A round is
//   1. every thread forms the objective of its eligible slots and keeps the better one by (obj, s, -slot);
//   2. a wave folds by xor shuffles, lane 0 writes the wave's best to LDS, ONE barrier, every thread reads the four
//      entries and finds the same winner j* (the entries alternate between two sets by the parity of the round: a
//      thread can be at most one round ahead of the slowest reader);
//   3. the owner of j* writes the outputs; every thread dots its slots' rows with row j* -- a broadcast read -- and
//      updates pen and the group count of its slots.  The rows are not written after the prologue.
// At d = 128 and C <= 256 (one slot per thread) the thread's own row is held in registers for the whole row, so a round
// reads only the winner's row from LDS (k_slate_mmr<32>; every other shape: k_slate_mmr<0>).
// LDS rows have a stride of d floats where d / 4 is odd and d + 4 where it is even: the stride in 16-byte slots is odd,
// so the 16 lanes a ds_read_b128 serves together (consecutive slots, the same column) fall on 16 different slots of the
// 256-byte bank row.
#include "common.h"
#include "sim_norm.h"

namespace arx {
namespace {

constexpr int kMmrThreads = 256;
constexpr int kMmrWaves = kMmrThreads / kWave;
constexpr int kMmrSlots = 2;                          // slots a thread owns
constexpr int kMmrMaxC = kMmrThreads * kMmrSlots;     // 512
constexpr int kMmrMaxD = 128;
constexpr int kMmrMaxCD = 32768;                      // floats of unpadded candidate rows (128 KiB)
constexpr int kMmrRegD4 = 32;                         // d = 128: the row width served by the register form
constexpr int kMmrPad = 4;                            // floats a row is padded by, at most
// LDS, in bytes: [0, 128) the waves' best of a round, two sets of four 16-byte keys; [128, 192) the waves' (min, max)
// of the prologue; then the rows [C][stride] float; then the slots' groups [C rounded up to 4] int32
constexpr int kMmrFixedBytes = 2 * kMmrWaves * 16 + kMmrWaves * 16;
constexpr int kMmrLdsLimit = 160 * 1024;              // what one workgroup may declare on gfx950
static_assert((kMmrMaxCD + kMmrMaxC * kMmrPad) * 4 + kMmrMaxC * 4 + kMmrFixedBytes <= kMmrLdsLimit,
              "arx_slate_mmr: the envelope of arx_slate_mmr_supported must fit one workgroup's LDS");

__host__ __device__ inline int mmr_stride(int d) { return ((d / 4) & 1) ? d : d + kMmrPad; }

inline size_t mmr_lds_bytes(int64_t C, int d) {
  return (size_t)kMmrFixedBytes + (size_t)C * mmr_stride(d) * 4 + (size_t)((C + 3) & ~(int64_t)3) * 4;
}

inline bool mmr_supported(int64_t C, int d) {
  return d % 4 == 0 && d >= 4 && d <= kMmrMaxD && C >= 1 && C <= kMmrMaxC && C * d <= kMmrMaxCD;
}

struct MmrKey {
  float obj, s;
  int slot;                                           // < 0: no eligible slot
};

// best = the earlier of best and a in the order of the selection: obj desc, score desc, slot asc.  One predicate and
// three selects, no branches: every lane of a wave runs this between two shuffles.
__device__ __forceinline__ void mmr_keep_earlier(MmrKey& best, float obj, float s, int slot) {
  const bool gt = obj > best.obj || (obj == best.obj && (s > best.s || (s == best.s && slot < best.slot)));
  const bool take = slot >= 0 && (best.slot < 0 || gt);
  best.obj = take ? obj : best.obj;
  best.s = take ? s : best.s;
  best.slot = take ? slot : best.slot;
}

__device__ __forceinline__ bool mmr_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

// D4R > 0: the register form for d = 4 * D4R and C <= 256 -- one slot per thread, whose unit row is copied from LDS into
// D4R float4 registers after the prologue, so that a round reads only the winner's row (same adds, same order).
template <int D4R>
__global__ __launch_bounds__(kMmrThreads) void k_slate_mmr(
    const float* __restrict__ P, int64_t ldp, int32_t V, int d, const int32_t* __restrict__ cand, int64_t ldc,
    const float* __restrict__ scores, int64_t lds, int64_t B, int C, const float* __restrict__ lam,
    const int32_t* __restrict__ groups, const int32_t* __restrict__ max_per_group, int k, int32_t* __restrict__ ids,
    int64_t ldi, float* __restrict__ values, int64_t ldv, int32_t* __restrict__ pos, int64_t ldq) {
  extern __shared__ float4 mmr_lds[];
  float4* red = mmr_lds;                                           // [2][kMmrWaves]
  float4* mm = mmr_lds + 2 * kMmrWaves;                            // [kMmrWaves]
  float* rows = reinterpret_cast<float*>(mmr_lds + 3 * kMmrWaves);
  const int stride = mmr_stride(d);
  int32_t* grp = reinterpret_cast<int32_t*>(rows + (size_t)C * stride);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int L = sim_group(d, true), li = lane & (L - 1), gw = lane / L, rpw = 64 / L;
  const int d4 = d >> 2;
  const float ninf = -__builtin_inff();

  for (int64_t r = blockIdx.x; r < B; r += gridDim.x) {
    __syncthreads();                                               // (the last row's readers are done with the LDS)
    const int32_t* cr = cand + r * ldc;
    const float* sr = scores + r * lds;
    // ---- the slots this thread owns
    int32_t id[kMmrSlots], g[kMmrSlots], cnt[kMmrSlots];
    float sc[kMmrSlots], rel[kMmrSlots], pen[kMmrSlots];
    bool act[kMmrSlots];                                           // live and not selected yet
    float mn = __builtin_inff(), mx = ninf;
#pragma unroll
    for (int u = 0; u < kMmrSlots; ++u) {
      const int j = tid + u * kMmrThreads;
      id[u] = -1; g[u] = -1; cnt[u] = 0; sc[u] = ninf; rel[u] = 0.f; pen[u] = 0.f; act[u] = false;
      if (j < C) {
        const int32_t c = cr[j];
        const float s = sr[j];
        if ((uint32_t)c < (uint32_t)V && mmr_finite(s)) {
          act[u] = true; id[u] = c; sc[u] = s;
          if (groups) g[u] = groups[c];
          mn = fminf(mn, s); mx = fmaxf(mx, s);
        }
        grp[j] = g[u];
      }
    }
    // ---- the unit rows: a group of L lanes per slot, the sum of sim_row_sq (wave-uniform bound: every lane shuffles)
    for (int j0 = wave * rpw; j0 < C; j0 += kMmrWaves * rpw) {
      const int j = j0 + gw;
      const bool in = j < C;
      const int32_t c = in ? cr[j] : -1;
      const bool ok = in && (uint32_t)c < (uint32_t)V && mmr_finite(sr[j]);
      const float* row = P + (ok ? (int64_t)c : 0) * ldp;
      const float inv = sim_inv(sim_row_sq<true>(row, d, L, li, ok));
      if (in && li < d4) {
        float4 x = make_float4(0.f, 0.f, 0.f, 0.f);                // (a dead slot: a zero row, nothing read)
        if (ok) {
          x = *reinterpret_cast<const float4*>(row + li * 4);
          x.x *= inv; x.y *= inv; x.z *= inv; x.w *= inv;
        }
        *reinterpret_cast<float4*>(rows + (size_t)j * stride + li * 4) = x;
      }
    }
    // ---- smin / smax, rel
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      mn = fminf(mn, __shfl_xor(mn, o, 64));
      mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    }
    if (lane == 0) mm[wave] = make_float4(mn, mx, 0.f, 0.f);
    __syncthreads();                                               // (publishes rows, grp and mm)
    float smin = mm[0].x, smax = mm[0].y;
#pragma unroll
    for (int w = 1; w < kMmrWaves; ++w) {
      smin = fminf(smin, mm[w].x);
      smax = fmaxf(smax, mm[w].y);
    }
    float4 own[D4R > 0 ? D4R : 1];
    if (D4R > 0) {
      const float4* a4 = reinterpret_cast<const float4*>(rows + (size_t)(tid < C ? tid : 0) * stride);
#pragma unroll
      for (int q = 0; q < D4R; ++q) own[q] = a4[q];
    }
    const bool spread = smax > smin;
    const float span = smax - smin;
#pragma unroll
    for (int u = 0; u < kMmrSlots; ++u)
      if (act[u]) rel[u] = spread ? (sc[u] - smin) / span : 1.f;
    const float la = lam[r], om = 1.0f - la;
    int cap = 0x7fffffff;
    if (groups) {
      cap = max_per_group[r];
      if (cap < 1) cap = 1;
    }
    int32_t* ids_r = ids + r * ldi;
    float* val_r = values + r * ldv;
    int32_t* pos_r = pos + r * ldq;

    // ---- k rounds
    int done = 0;
    for (int t = 0; t < k; ++t) {
      MmrKey best = {0.f, 0.f, -1};
#pragma unroll
      for (int u = 0; u < kMmrSlots; ++u) {
        const bool open = act[u] && !(g[u] >= 0 && cnt[u] >= cap);
        mmr_keep_earlier(best, la * rel[u] - om * pen[u], sc[u], open ? tid + u * kMmrThreads : -1);
      }
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) {
        const float oo = __shfl_xor(best.obj, o, 64), os = __shfl_xor(best.s, o, 64);
        const int oj = __shfl_xor(best.slot, o, 64);
        mmr_keep_earlier(best, oo, os, oj);
      }
      float4* set = red + (t & 1) * kMmrWaves;
      if (lane == 0) set[wave] = make_float4(best.obj, best.s, __int_as_float(best.slot), 0.f);
      __syncthreads();
      best.slot = -1;
#pragma unroll
      for (int w = 0; w < kMmrWaves; ++w) {
        const float4 e = set[w];
        mmr_keep_earlier(best, e.x, e.y, __float_as_int(e.z));
      }
      if (best.slot < 0) break;                                    // (the same for every thread)
      const int js = best.slot;
      const int32_t gs = grp[js];
#pragma unroll
      for (int u = 0; u < kMmrSlots; ++u) {
        if (js == tid + u * kMmrThreads) {
          ids_r[t] = id[u];
          val_r[t] = sc[u];
          pos_r[t] = js;
          act[u] = false;
        }
      }
      done = t + 1;
      if (done == k) break;
      // the cosines of this thread's slots with the winner (selected and dead slots need none)
      const float4* w4 = reinterpret_cast<const float4*>(rows + (size_t)js * stride);
#pragma unroll
      for (int u = 0; u < kMmrSlots; ++u) {
        if (g[u] >= 0 && g[u] == gs) ++cnt[u];
        if (!act[u]) continue;
        float p0 = 0.f, p1 = 0.f, p2 = 0.f, p3 = 0.f;
        if (D4R > 0) {
          if (u == 0) {
#pragma unroll
            for (int q = 0; q < D4R; ++q) {
              const float4 a = own[q], w = w4[q];
              p0 = fmaf(a.x, w.x, p0);
              p1 = fmaf(a.y, w.y, p1);
              p2 = fmaf(a.z, w.z, p2);
              p3 = fmaf(a.w, w.w, p3);
            }
          }
        } else {
          const float4* a4 = reinterpret_cast<const float4*>(rows + (size_t)(tid + u * kMmrThreads) * stride);
#pragma unroll 8
          for (int q = 0; q < d4; ++q) {
            const float4 a = a4[q], w = w4[q];
            p0 = fmaf(a.x, w.x, p0);
            p1 = fmaf(a.y, w.y, p1);
            p2 = fmaf(a.z, w.z, p2);
            p3 = fmaf(a.w, w.w, p3);
          }
        }
        pen[u] = fmaxf(pen[u], (p0 + p1) + (p2 + p3));
      }
    }
    for (int t = done + tid; t < k; t += kMmrThreads) {
      ids_r[t] = -1;
      val_r[t] = ninf;
      pos_r[t] = -1;
    }
  }
}

}  // namespace
}  // namespace arx

using namespace arx;

extern "C" {

int arx_slate_mmr_supported(int64_t C, int d) { return mmr_supported(C, d) ? 1 : 0; }

int arx_slate_mmr(const float* P, int64_t ldp, int64_t V, int d, const int32_t* cand, int64_t ldc, const float* scores,
                  int64_t lds, int64_t B, int64_t C, const float* lam, const int32_t* groups,
                  const int32_t* max_per_group, int k, int32_t* ids, int64_t ldi, float* values, int64_t ldv,
                  int32_t* pos, int64_t ldq, void* stream) {
  ARX_CHECK_ARG(P && cand && scores && lam && ids && values && pos,
                "arx_slate_mmr: null pointer (only groups and max_per_group may be NULL)");
  ARX_CHECK_ARG(!groups == !max_per_group,
                "arx_slate_mmr: groups and max_per_group go together (both NULL or both given)");
  ARX_CHECK_ARG(B >= 0 && C >= 0 && V >= 0 && V <= 0x7fffffffll,
                "arx_slate_mmr: need B >= 0, C >= 0, 0 <= V < 2^31 (B=%lld C=%lld V=%lld)", (long long)B, (long long)C,
                (long long)V);
  ARX_CHECK_ARG(d >= 4 && d % 4 == 0, "arx_slate_mmr: need d %% 4 == 0 and d >= 4 (d=%d)", d);
  ARX_CHECK_ARG(ldp >= d && ldp % 4 == 0, "arx_slate_mmr: ldp must be a multiple of 4 and >= d (ldp=%lld d=%d)",
                (long long)ldp, d);
  ARX_CHECK_ARG(!(reinterpret_cast<uintptr_t>(P) & 15), "arx_slate_mmr: P must be 16-byte aligned");
  ARX_CHECK_ARG(ldc >= C && lds >= C, "arx_slate_mmr: need ldc >= C and lds >= C (ldc=%lld lds=%lld C=%lld)",
                (long long)ldc, (long long)lds, (long long)C);
  ARX_CHECK_ARG(k >= 1 && k <= C, "arx_slate_mmr: need 1 <= k <= C (k=%d C=%lld)", k, (long long)C);
  ARX_CHECK_ARG(ldi >= k && ldv >= k && ldq >= k,
                "arx_slate_mmr: need ldi, ldv, ldq >= k (ldi=%lld ldv=%lld ldq=%lld k=%d)", (long long)ldi,
                (long long)ldv, (long long)ldq, k);
  if (!mmr_supported(C, d)) {
    set_error("arx_slate_mmr: C=%lld d=%d unsupported (arx_slate_mmr_supported: need d %% 4 == 0, 4 <= d <= %d, "
              "1 <= C <= %d, C * d <= %d)", (long long)C, d, kMmrMaxD, kMmrMaxC, kMmrMaxCD);
    return ARX_EUNSUPPORTED;
  }
  if (B == 0) return ARX_OK;
  const size_t lds_bytes = mmr_lds_bytes(C, d);
  // (per call: the attribute is per device and the call is cheap)
  const bool in_regs = d == 4 * kMmrRegD4 && C <= kMmrThreads;
  auto kern = in_regs ? k_slate_mmr<kMmrRegD4> : k_slate_mmr<0>;
  ARX_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    kMmrLdsLimit));
  int64_t g = B;
  const int64_t cap = (int64_t)cu_count() * 8;
  if (g > cap) g = cap;
  kern<<<(int)g, kMmrThreads, lds_bytes, as_stream(stream)>>>(P, ldp, (int32_t)V, d, cand, ldc, scores, lds, B, (int)C,
                                                             lam, groups, max_per_group, k, ids, ldi, values, ldv,
                                                             pos, ldq);
  ARX_CHECK_LAUNCH();
  return ARX_OK;
}

}  // extern "C"

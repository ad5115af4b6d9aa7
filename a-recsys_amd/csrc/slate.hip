// slate.hip -- score_items: every row of a batch against its OWN list of candidate items (arx_slate.h).  A gather and a
// dot over rows x C randomly addressed pool rows; [rows, C, d] is never materialised.  Bound by the row fetches (HBM /
// L2), not by arithmetic.
//
// A GROUP of L lanes (L the smallest power of two >= d / 4; 64 / L groups per wave) owns one (row, slot) pair: every
// lane loads one float4 of the pool row -- a 512-B row at d = 128 is one coalesced request of 32 lanes --, lanes past
// d / 4 hold zeros.  A wave takes one row and a run of its slots: the row's U fragment stays in registers for the whole
// run, and kSlateUnroll loads per lane (that many pool rows per group) are issued before the first reduction.  The
// group folds by xor shuffles 1, 2, 4, ... and its lane 0 stores.  No LDS, no atomics; the order of the adds of one
// pair depends on d only (the header states it; tests check the bit patterns).
#include "common.h"

namespace arx {
namespace {

constexpr int kSlateUnroll = 4;      // pool rows in flight per group (4 x 64 / L per wave)
constexpr int kSlateMaxPasses = 8;   // unrolled passes of one wave's run, at most

// unit w of `units` = (row w / nruns, slots [(w % nruns) * run, + run)); waves stride the units, so no grid dimension
// bounds B or C
template <int L>
__global__ __launch_bounds__(256) void k_slate_scores(const float* __restrict__ U, int64_t ldu,
                                                      const float* __restrict__ P, int64_t ldp,
                                                      const float* __restrict__ pbias, int32_t V, int d,
                                                      const int32_t* __restrict__ cand, int64_t ldc, int64_t C,
                                                      float* __restrict__ scores, int64_t lds, int64_t units,
                                                      int64_t nruns, int run) {
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
    const int32_t* cr = cand + r * ldc;
    float* sr = scores + r * lds;
    for (int64_t j = j0; j < j1; j += kSlateUnroll * S) {
      int32_t c[kSlateUnroll];
      float4 p[kSlateUnroll];
      float b[kSlateUnroll];
#pragma unroll
      for (int t = 0; t < kSlateUnroll; ++t) {
        const int64_t jj = j + t * S + gw;
        c[t] = jj < j1 ? cr[jj] : -1;
      }
#pragma unroll
      for (int t = 0; t < kSlateUnroll; ++t) {
        const bool ok = (uint32_t)c[t] < (uint32_t)V;             // (negative ids and ARX_KEY_NONE: nothing is read)
        p[t] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (ok && live) p[t] = *reinterpret_cast<const float4*>(P + (int64_t)c[t] * ldp + li * 4);
        b[t] = ok && pbias ? pbias[c[t]] : 0.f;
      }
#pragma unroll
      for (int t = 0; t < kSlateUnroll; ++t) {
        float s = u.x * p[t].x;
        s = fmaf(u.y, p[t].y, s);
        s = fmaf(u.z, p[t].z, s);
        s = fmaf(u.w, p[t].w, s);
#pragma unroll
        for (int o = 1; o < L; o <<= 1) s += __shfl_xor(s, o, 64);
        const int64_t jj = j + t * S + gw;
        if (li == 0 && jj < j1) {
          const bool ok = (uint32_t)c[t] < (uint32_t)V;
          sr[jj] = ok ? (pbias ? s + b[t] : s) : -__builtin_inff();
        }
      }
    }
  }
}

__global__ __launch_bounds__(256) void k_slate_merge_shards(const float* __restrict__ parts, int64_t n, int64_t C,
                                                            int W, float* __restrict__ out, int64_t ldo) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    float m = parts[i];
    for (int s = 1; s < W; ++s) {
      const float v = parts[s * n + i];
      m = (v > m || v != v) ? v : m;                              // (the owner's bits; its NaN stays)
    }
    const int64_t r = i / C;
    out[r * ldo + (i - r * C)] = m;
  }
}

template <int L>
void slate_launch(int g, hipStream_t s, const float* U, int64_t ldu, const float* P, int64_t ldp, const float* pbias,
                  int32_t V, int d, const int32_t* cand, int64_t ldc, int64_t C, float* scores, int64_t lds,
                  int64_t units, int64_t nruns, int run) {
  k_slate_scores<L><<<g, 256, 0, s>>>(U, ldu, P, ldp, pbias, V, d, cand, ldc, C, scores, lds, units, nruns, run);
}

}  // namespace
}  // namespace arx

using namespace arx;

extern "C" {

int arx_slate_scores(const float* U, int64_t ldu, int64_t B, const float* P, int64_t ldp, const float* pbias, int64_t V,
                     int d, const int32_t* cand, int64_t ldc, int64_t C, float* scores, int64_t lds, void* stream) {
  ARX_CHECK_ARG(U && P && cand && scores, "arx_slate_scores: null pointer (only pbias may be NULL)");
  ARX_CHECK_ARG(B >= 0 && C >= 0 && V >= 0 && V <= 0x7fffffffll,
                "arx_slate_scores: need B >= 0, C >= 0, 0 <= V < 2^31 (B=%lld C=%lld V=%lld)", (long long)B,
                (long long)C, (long long)V);
  ARX_CHECK_ARG(d >= 4 && d % 4 == 0, "arx_slate_scores: need d %% 4 == 0 and d >= 4 (d=%d)", d);
  if (d > 256) {
    set_error("arx_slate_scores: embedding size d=%d unsupported (need d <= 256)", d);
    return ARX_EUNSUPPORTED;
  }
  ARX_CHECK_ARG(ldu >= d && ldu % 4 == 0 && ldp >= d && ldp % 4 == 0,
                "arx_slate_scores: ldu, ldp must be multiples of 4 and >= d (ldu=%lld ldp=%lld d=%d)", (long long)ldu,
                (long long)ldp, d);
  ARX_CHECK_ARG(!((reinterpret_cast<uintptr_t>(U) | reinterpret_cast<uintptr_t>(P)) & 15),
                "arx_slate_scores: U and P must be 16-byte aligned");
  ARX_CHECK_ARG(ldc >= C && lds >= C, "arx_slate_scores: need ldc >= C and lds >= C (ldc=%lld lds=%lld C=%lld)",
                (long long)ldc, (long long)lds, (long long)C);
  ARX_CHECK_ARG(B == 0 || C <= 0x7fffffffll / B, "arx_slate_scores: need B * C < 2^31 (B=%lld C=%lld)", (long long)B,
                (long long)C);
  if (B == 0 || C == 0) return ARX_OK;
  const int L = lanes_per_row(d);
  const int per_pass = kSlateUnroll * (64 / L);
  // a wave's run of slots: as long as the chip stays full (the U fragment is loaded once per run)
  const int64_t want = (int64_t)cu_count() * 64;
  int passes = kSlateMaxPasses;
  while (passes > 1 && B * ceil_div(C, (int64_t)per_pass * passes) < want) passes >>= 1;
  const int run = per_pass * passes;
  const int64_t nruns = ceil_div(C, (int64_t)run);
  const int64_t units = B * nruns;
  int64_t g = ceil_div(units, (int64_t)4);
  const int64_t cap = (int64_t)cu_count() * 16;
  if (g > cap) g = cap;
  hipStream_t s = as_stream(stream);
#define ARX_SLATE_CASE(LL)                                                                                       \
  case LL:                                                                                                       \
    slate_launch<LL>((int)g, s, U, ldu, P, ldp, pbias, (int32_t)V, d, cand, ldc, C, scores, lds, units, nruns, run); \
    break;
  switch (L) {
    ARX_SLATE_CASE(1)
    ARX_SLATE_CASE(2)
    ARX_SLATE_CASE(4)
    ARX_SLATE_CASE(8)
    ARX_SLATE_CASE(16)
    ARX_SLATE_CASE(32)
    ARX_SLATE_CASE(64)
  }
#undef ARX_SLATE_CASE
  ARX_CHECK_LAUNCH();
  return ARX_OK;
}

int arx_slate_merge_shards(const float* parts, int64_t B, int64_t C, int W, float* out, int64_t ldo, void* stream) {
  ARX_CHECK_ARG(parts && out, "arx_slate_merge_shards: null pointer");
  ARX_CHECK_ARG(B >= 0 && C >= 0 && ldo >= C, "arx_slate_merge_shards: need B >= 0, C >= 0, ldo >= C (B=%lld C=%lld ldo=%lld)",
                (long long)B, (long long)C, (long long)ldo);
  ARX_CHECK_ARG(W >= 1 && W <= 64, "arx_slate_merge_shards: need 1 <= W <= 64 (W=%d)", W);
  ARX_CHECK_ARG(B == 0 || C <= 0x7fffffffll / B, "arx_slate_merge_shards: need B * C < 2^31 (B=%lld C=%lld)",
                (long long)B, (long long)C);
  if (B == 0 || C == 0) return ARX_OK;
  const int64_t n = B * C;
  int64_t g = ceil_div(n, (int64_t)256);
  const int64_t cap = (int64_t)cu_count() * 16;
  if (g > cap) g = cap;
  k_slate_merge_shards<<<(int)g, 256, 0, as_stream(stream)>>>(parts, n, C, W, out, ldo);
  ARX_CHECK_LAUNCH();
  return ARX_OK;
}

}  // extern "C"

// sim_norm.h -- how a row's sum of squares is added and turned into an inverse norm: the one definition shared by the
// kernels that must agree on a row norm bit for bit (similar.hip: arx_rows_inv_norm, arx_gather_rows_unit;
// diverse.hip: arx_slate_mmr).  The order is stated at the head of similar.hip.
#pragma once
#include "common.h"

namespace arx {
namespace {

__host__ __device__ inline int sim_group(int d, bool vec) {
  const int q = vec ? d / 4 : d;
  int l = 1;
  while (l < q && l < 64) l <<= 1;
  return l;
}

// sum of squares of `row` over the calling group (every lane of the wave calls it; ok == false: contributes nothing);
// every lane of the group returns the same sum
template <bool VEC>
__device__ __forceinline__ float sim_row_sq(const float* __restrict__ row, int d, int L, int li, bool ok) {
  float s = 0.f;
  if (ok) {
    if (VEC) {
      for (int c = li * 4; c < d; c += L * 4) {
        const float4 x = *reinterpret_cast<const float4*>(row + c);
        s += x.x * x.x;
        s += x.y * x.y;
        s += x.z * x.z;
        s += x.w * x.w;
      }
    } else {
      for (int c = li; c < d; c += L) s += row[c] * row[c];
    }
  }
  for (int o = 1; o < L; o <<= 1) s += __shfl_xor(s, o, 64);
  return s;
}

__device__ __forceinline__ float sim_inv(float s) { return s > 0.f ? 1.0f / sqrtf(s) : 0.f; }

}  // namespace
}  // namespace arx

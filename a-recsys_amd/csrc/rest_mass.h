// rest_mass.h -- the (m, S) mass arithmetic of arx_sample_logp.h, ONE definition for the streaming scan
// (gemm_nt.hip), the materialised form and the finishing kernel (sample_logp.hip).  A mass is a pair: m the largest
// SCORE in it, s = sum exp((score - m) / tau) >= 1; the empty mass is (-FLT_MAX, 0), so no join ever forms
// -inf - -inf.  tau here is always > 0: a tau == 0 row (its logp is 0 by rule) is walked with tau = 1.
#pragma once
#include "common.h"

namespace arx {

struct RmMass {
  float m, s;
};

__device__ __forceinline__ RmMass rm_empty() { return RmMass{-__FLT_MAX__, 0.f}; }

// tau as the mass kernels use it: the row's own where it is > 0, else 1
__device__ __forceinline__ float rm_tau(float tau) { return tau > 0.f ? tau : 1.f; }

// 1 / tau for the per-logit path, kept finite (a denormal tau): 0 * itau stays 0
__device__ __forceinline__ float rm_itau(float tau) { return fminf(1.f / tau, __FLT_MAX__); }

// (max, S_hi + S_lo * exp((m_lo - m_hi) / tau)); an empty side adds 0 * exp(..) = 0
__device__ __forceinline__ RmMass rm_join(const RmMass a, const RmMass b, float tau) {
  const bool ge = a.m >= b.m;
  const float hi = ge ? a.m : b.m, lo = ge ? b.m : a.m;
  const float sh = ge ? a.s : b.s, sl = ge ? b.s : a.s;
  return RmMass{hi, fmaf(sl, expf((lo - hi) / tau), sh)};
}

// one score into a running mass, the per-logit form: ONE exp; v == -inf adds nothing (itau = rm_itau(tau))
__device__ __forceinline__ void rm_add(float& m, float& s, float v, float itau) {
  const float dd = (v - m) * itau;
  const float ex = __expf(-fabsf(dd));
  s = dd > 0.f ? fmaf(s, ex, 1.f) : s + ex;
  m = fmaxf(m, v);
}

}  // namespace arx

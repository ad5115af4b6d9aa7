// gate_fn.h -- the gate non-linearities of the recurrent forward kernels (lstm.hip, gru.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace arx {

// Gate non-linearities on the transcendental unit (v_exp_f32, v_rcp_f32: 1 ulp each), no libm call and no IEEE
// division: ~6 / ~14 instructions instead of ~15 / ~45.  tanh: (1 - e) / (1 + e) with e = exp(-2|x|) loses the
// small-|x| digits to 1 - e, so |x| < 1/16 takes the odd series (relative error < 1e-10 there); both within ~5e-7
// relative of tanh over the whole range (tests/test_lstm_kernels_gpu.py::test_gate_functions and ::test_cell_tanh run
// both functions alone, through one-hot weights, against float64: 4.3e-7 measured for sigmoid at x = -9.1, 4.1e-7 for
// tanh just above 1/16, 1e-6 asserted; where the exact sigmoid is below 2^-126, x < -87.3, the result is 0 or
// subnormal).  FORWARD kernels only: k_lstm_fwd_r4 83.8 -> 75.2 us at L = 50,
// B = 1024; in the backward kernels the same replacement measured SLOWER (k_lstm_bwd_r4 46.8 -> 56.8 us), they keep
// libm's tanhf.  Also measured and dropped: the x half of step t + 1 issued between the gate arithmetic of step t
// (82.5 us compiler-scheduled, 93 us with a sched_group_barrier interleave that needs > 256 registers).
__device__ __forceinline__ float sigmoidf_(float x) { return __builtin_amdgcn_rcpf(1.f + __expf(-x)); }
__device__ __forceinline__ float tanhf_(float x) {
  const float ax = fabsf(x);
  const float e = __expf(-2.f * ax);
  const float big = (1.f - e) * __builtin_amdgcn_rcpf(1.f + e);
  const float x2 = ax * ax;
  const float small = ax * (1.f + x2 * (-0.33333334f + x2 * (0.13333334f + x2 * -0.053968254f)));
  return copysignf(ax < 0.0625f ? small : big, x);
}

}  // namespace arx

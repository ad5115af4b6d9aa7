// gumbel.h -- the noise of the sampled recommend (arx_sample.h): ONE definition for the dense, the chunked and the fused
// path.  g(seed, row, col) is standard Gumbel noise as a pure function of its three arguments, so every path draws the
// same sample and a request re-run after a candidate overflow returns the same items.  key = fmaf(tau, g, v): the top-k
// of the keys is k draws without replacement with probability proportional to exp(v / tau) (Plackett-Luce).
// All integer arithmetic is unsigned and wrapping.  Per row, once (64-bit): gumbel_row; per column, 32-bit ops and two
// multiplies: gumbel_bits; the two ACCURATE logarithms (the draws that win have u next to 1, where the fast form loses
// all relative accuracy in -log u): gumbel_of_bits.
#ifndef ARX_GUMBEL_H_
#define ARX_GUMBEL_H_
#include <stdint.h>
#include <hip/hip_runtime.h>

namespace arx {

struct GumbelRow { uint32_t b0, b1; };

// the row's two words: the splitmix64 finaliser (sampler.hip's mix32s with all 64 bits kept) of seed and row
__device__ __forceinline__ GumbelRow gumbel_row(const int32_t* __restrict__ seed_words, int64_t row) {
  const uint64_t seed = (uint64_t)(uint32_t)seed_words[0] | ((uint64_t)(uint32_t)seed_words[1] << 32);
  uint64_t z = seed * 0x9E3779B97F4A7C15ull + ((uint64_t)row + 1ull) * 0xD1B54A32D192ED03ull;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  z = z ^ (z >> 31);
  return GumbelRow{(uint32_t)z, (uint32_t)(z >> 32)};
}

// the column's hash; its top 23 bits m = x >> 9 are the draw
__device__ __forceinline__ uint32_t gumbel_bits(uint32_t b0, uint32_t b1, uint32_t col) {
  uint32_t x = col + b0;
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x ^= b1;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

// g = -log(-log(u)), u = (m + 0.5) 2^-23 in [2^-24, 1 - 2^-24] (exact in float32): g in [-2.8116, 16.6356], finite
__device__ __forceinline__ float gumbel_of_bits(uint32_t x) {
  const float u = ((float)(x >> 9) + 0.5f) * (1.0f / 8388608.0f);
  return -logf(-logf(u));
}

// An upper bound of gumbel_of_bits(x) without a logarithm, for the fused filter's rejection test.  With
// w = 2^24 - 2 m - 1 (odd, < 2^24: exact in float32), 1 - u = w 2^-24 exactly, and
//     -log u >= 1 - u            =>  g <= -log(1 - u) = ln 2 (24 - log2 w)
//     log2(1 + f) >= f on [0, 1] =>  log2 w >= e + f,  the float's exponent and mantissa fraction, i.e.
//                                    (bits(w) - bits(1.0f)) 2^-23
// so g <= ln 2 (24 - (bits(w) - bits(1)) 2^-23).  The bound is tight to 0.06 where it matters (u next to 1).  Float
// rounding: the integer (< 2^28) rounds by 2^-24 relative (1.4e-6 of the 23 it scales to), the fma once more (2e-6),
// the accurate logf pair is good to a few ulp of g (< 1e-5): kGumbelSlack = 1e-3 covers all of it a hundred times
// and costs a factor e^0.001 of false passes.
constexpr float kGumbelSlack = 1e-3f;
__device__ __forceinline__ float gumbel_upper(uint32_t x) {
  const uint32_t w = 0x1000000u - 2u * (x >> 9) - 1u;
  const int32_t lb = (int32_t)__float_as_uint((float)w) - 0x3f800000;
  return fmaf((float)lb, -0.69314718f / 8388608.0f, 24.f * 0.69314718f + kGumbelSlack);
}

}  // namespace arx
#endif  // ARX_GUMBEL_H_

// similar.hip -- the small kernels of the item-to-item scan (model.similar_items: cosine nearest neighbours over the
// full item vocabulary).  The scan itself is the streaming top-k of recommend with the cosine scale in the scorer
// GEMM's epilogue (gemm_nt.hip, kNtCos); here: the inverse row norms of the table (one streaming read), the queries as
// unit rows, and the finish of a MATERIALISED chunk of logits (the first chunk and the chunked path).
//
// A row of d floats is summed by a GROUP of L lanes (L a power of two, <= 64; 64 / L rows per wave): lane i of the
// group adds the squares of its elements i, i + L, i + 2L, ... (float4 elements on the vector path) in that order, then
// the group folds by xor shuffles 1, 2, 4, ... -- one fixed order whatever the grid, so the sums are deterministic and
// the two kernels that need a row's norm agree bit for bit.  1.0f / sqrtf(s): both correctly rounded in this build (no
// fast-math), so s = 4^e gives exactly 2^-e.
#include "common.h"
#include "sim_norm.h"

namespace arx {
namespace {

template <bool VEC>
__global__ __launch_bounds__(256) void k_rows_inv_norm(const float* __restrict__ E, int64_t ld, int64_t n, int d, int L,
                                                       float* __restrict__ out) {
  const int lane = threadIdx.x & 63, li = lane & (L - 1), gw = lane / L, rpw = 64 / L;
  const int64_t wave = blockIdx.x * (int64_t)(blockDim.x >> 6) + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x >> 6);
  for (int64_t r0 = wave * rpw; r0 < n; r0 += nwaves * rpw) {      // (wave-uniform bound: every lane shuffles)
    const int64_t r = r0 + gw;
    const bool ok = r < n;
    const float s = sim_row_sq<VEC>(E + (ok ? r : 0) * ld, d, L, li, ok);
    if (ok && li == 0) out[r] = sim_inv(s);
  }
}

template <bool VEC>
__global__ __launch_bounds__(256) void k_gather_rows_unit(const float* __restrict__ E, int64_t ld,
                                                          const int32_t* __restrict__ rows, int64_t B, int d, int L,
                                                          float* __restrict__ out, int64_t ldo) {
  const int lane = threadIdx.x & 63, li = lane & (L - 1), gw = lane / L, rpw = 64 / L;
  const int64_t wave = blockIdx.x * (int64_t)(blockDim.x >> 6) + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x >> 6);
  for (int64_t r0 = wave * rpw; r0 < B; r0 += nwaves * rpw) {
    const int64_t r = r0 + gw;
    const bool in = r < B;
    const int32_t src = in ? rows[r] : -1;
    const bool ok = src >= 0;                                      // (src < 0: a zero row, nothing read through it)
    const float* row = E + (ok ? (int64_t)src : 0) * ld;
    const float inv = sim_inv(sim_row_sq<VEC>(row, d, L, li, ok));
    if (!in) continue;
    float* o = out + r * ldo;
    if (VEC) {
      for (int c = li * 4; c < d; c += L * 4) {
        float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
        if (ok) {
          x = *reinterpret_cast<const float4*>(row + c);
          x.x *= inv; x.y *= inv; x.z *= inv; x.w *= inv;
        }
        *reinterpret_cast<float4*>(o + c) = x;
      }
    } else {
      for (int c = li; c < d; c += L) o[c] = ok ? row[c] * inv : 0.f;
    }
  }
}

// logits[r, c] = logits[r, c] * col_scale[col0 + c] + 0 (a product -0 becomes +0, as in the fused filter), then -inf at
// the row's own column; blockIdx.y strides the rows, x the columns
__global__ __launch_bounds__(256) void k_cos_chunk_finish(float* __restrict__ logits, int64_t ld, int64_t B,
                                                          int32_t col0, int64_t ncols,
                                                          const float* __restrict__ col_scale,
                                                          const int32_t* __restrict__ self_col) {
  for (int64_t r = blockIdx.y; r < B; r += gridDim.y) {
    const int64_t sc = self_col ? (int64_t)self_col[r] - col0 : -1;
    float* lp = logits + r * ld;
    for (int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; c < ncols; c += (int64_t)gridDim.x * blockDim.x)
      lp[c] = c == sc ? -__builtin_inff() : lp[c] * col_scale[(int64_t)col0 + c] + 0.f;
  }
}

int sim_grid(int64_t rows, int L) {
  const int64_t waves = ceil_div(rows, (int64_t)(64 / L));
  int64_t g = ceil_div(waves, (int64_t)4);
  const int64_t cap = (int64_t)cu_count() * 8;
  if (g > cap) g = cap;
  return (int)(g < 1 ? 1 : g);
}

}  // namespace
}  // namespace arx

using namespace arx;

extern "C" {

int arx_rows_inv_norm(const float* E, int64_t ld, int64_t n, int64_t d, float* out, void* stream) {
  ARX_CHECK_ARG(E && out, "arx_rows_inv_norm: null pointer");
  ARX_CHECK_ARG(n >= 0 && d >= 1 && d <= 0x7fffffff && ld >= d, "arx_rows_inv_norm: need n >= 0, d >= 1, ld >= d");
  if (n == 0) return ARX_OK;
  const bool vec = d % 4 == 0 && ld % 4 == 0 && !(reinterpret_cast<uintptr_t>(E) & 15);
  const int L = sim_group((int)d, vec);
  const int g = sim_grid(n, L);
  if (vec)
    k_rows_inv_norm<true><<<g, 256, 0, as_stream(stream)>>>(E, ld, n, (int)d, L, out);
  else
    k_rows_inv_norm<false><<<g, 256, 0, as_stream(stream)>>>(E, ld, n, (int)d, L, out);
  ARX_CHECK_LAUNCH();
  return ARX_OK;
}

int arx_gather_rows_unit(const float* E, int64_t ld, const int32_t* rows, int64_t B, int64_t d, float* out, int64_t ldo,
                         void* stream) {
  ARX_CHECK_ARG(E && rows && out, "arx_gather_rows_unit: null pointer");
  ARX_CHECK_ARG(B >= 0 && d >= 1 && d <= 0x7fffffff && ld >= d && ldo >= d,
                "arx_gather_rows_unit: need B >= 0, d >= 1, ld >= d, ldo >= d");
  if (B == 0) return ARX_OK;
  const bool vec = d % 4 == 0 && ld % 4 == 0 && ldo % 4 == 0 &&
                   !((reinterpret_cast<uintptr_t>(E) | reinterpret_cast<uintptr_t>(out)) & 15);
  const int L = sim_group((int)d, vec);
  const int g = sim_grid(B, L);
  if (vec)
    k_gather_rows_unit<true><<<g, 256, 0, as_stream(stream)>>>(E, ld, rows, B, (int)d, L, out, ldo);
  else
    k_gather_rows_unit<false><<<g, 256, 0, as_stream(stream)>>>(E, ld, rows, B, (int)d, L, out, ldo);
  ARX_CHECK_LAUNCH();
  return ARX_OK;
}

int arx_cos_chunk_finish(float* logits, int64_t ld, int64_t B, int32_t col0, int64_t ncols, const float* col_scale,
                         const int32_t* self_col, void* stream) {
  ARX_CHECK_ARG(logits && col_scale, "arx_cos_chunk_finish: null pointer (only self_col may be NULL)");
  ARX_CHECK_ARG(B >= 0 && ncols >= 0 && ld >= ncols && col0 >= 0 && (int64_t)col0 + ncols <= 0x7fffffff,
                "arx_cos_chunk_finish: need B >= 0, ncols >= 0, ld >= ncols, col0 >= 0, col0 + ncols < 2^31");
  if (B == 0 || ncols == 0) return ARX_OK;
  int64_t gx = ceil_div(ncols, (int64_t)256);
  if (gx > 256) gx = 256;
  const dim3 grid((unsigned)gx, (unsigned)(B < 4096 ? B : 4096));
  k_cos_chunk_finish<<<grid, 256, 0, as_stream(stream)>>>(logits, ld, B, col0, ncols, col_scale, self_col);
  ARX_CHECK_LAUNCH();
  return ARX_OK;
}

}  // extern "C"

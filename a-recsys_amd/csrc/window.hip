// window.hip -- the context window of the skip-gram / CBOW recommenders (word2vec/cbow_model.py:83-90) as one
// lookup: the n one-hot lookups of a batch row are summed in registers instead of travelling through an
// [n*mb, d] buffer, and their gradient is ONE [mb, d] row per batch row that all n lookups of the window share.
//
//  arx_gather_window_fwd  : out[b] = base_scale * base[b] + scale * sum_t E[cat_map[ids[t*mb + b]]]
//  arx_sparse_site_window : K7 contributions of such a lookup (keys per lookup, source row per batch row)
//  arx_window_slots_fwd   : the same sum over the rows of a RECEIVED block named by slot (the row-sharded model:
//                           out[b] = base_scale * base[b] + scale * sum_t R[slots[t*mb + b]], rows ldr floats apart)
//  arx_window_slots_bwd   : dbase[b] (+)= base_scale * dX[b], dR[slots[t*mb + b]] = scale * dX[b] for every t
//
// Layout as in gather.hip: a row of d fp32 is read by a sub-group of LPR = pow2ceil(d/4) lanes, one float4 per
// lane.  The kernel is a bandwidth-bound gather of n rows per output row: every lane keeps up to four 16-byte
// row loads in flight (the ids of the window first, then the rows), and adds them in ascending t.
#include "common.h"

namespace arx {

__device__ __forceinline__ void f4_fma(float4& a, float s, const float4& v) {
  a.x += s * v.x;
  a.y += s * v.y;
  a.z += s * v.z;
  a.w += s * v.w;
}

template <int LPR>
__global__ __launch_bounds__(256) void k_gather_window(
    const float* __restrict__ E, int64_t lde, const int32_t* __restrict__ cat_map, const int32_t* __restrict__ ids,
    int n, int64_t mb, int d, float scale, const float* __restrict__ base, int64_t ldb, float base_scale,
    float* __restrict__ out, int64_t ldo) {
  constexpr int GPW = 64 / LPR;
  const int lane = threadIdx.x & 63;
  const int lig = lane % LPR;
  const int gid = lane / LPR;
  const int col = lig * 4;
  const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  const int64_t nwave = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t b = wave * GPW + gid; b < mb; b += nwave * GPW) {
    if (col >= d) continue;
    // sum_t of the raw rows, ascending t, one chain of fp32 adds: the order never depends on the launch shape
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    int t = 0;
    for (; t + 4 <= n; t += 4) {
      const int i0 = ids[(int64_t)t * mb + b];
      const int i1 = ids[(int64_t)(t + 1) * mb + b];
      const int i2 = ids[(int64_t)(t + 2) * mb + b];
      const int i3 = ids[(int64_t)(t + 3) * mb + b];
      const int r0 = cat_map ? cat_map[i0] : i0;
      const int r1 = cat_map ? cat_map[i1] : i1;
      const int r2 = cat_map ? cat_map[i2] : i2;
      const int r3 = cat_map ? cat_map[i3] : i3;
      const float4 v0 = *reinterpret_cast<const float4*>(E + (int64_t)r0 * lde + col);
      const float4 v1 = *reinterpret_cast<const float4*>(E + (int64_t)r1 * lde + col);
      const float4 v2 = *reinterpret_cast<const float4*>(E + (int64_t)r2 * lde + col);
      const float4 v3 = *reinterpret_cast<const float4*>(E + (int64_t)r3 * lde + col);
      f4_fma(acc, 1.f, v0);
      f4_fma(acc, 1.f, v1);
      f4_fma(acc, 1.f, v2);
      f4_fma(acc, 1.f, v3);
    }
    for (; t < n; ++t) {
      const int i0 = ids[(int64_t)t * mb + b];
      const int r0 = cat_map ? cat_map[i0] : i0;
      f4_fma(acc, 1.f, *reinterpret_cast<const float4*>(E + (int64_t)r0 * lde + col));
    }
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    if (base) f4_fma(o, base_scale, *reinterpret_cast<const float4*>(base + b * ldb + col));
    f4_fma(o, scale, acc);
    *reinterpret_cast<float4*>(out + b * ldo + col) = o;
  }
}

// One dX row in, n + 1 rows out: every lane reads its float4 of dX[b] once, loads the slots of the window (four at a
// time) and then issues the stores.  One slot has one writer (the route gives every request its own slot), so there
// are no atomics; rows of dR that no slot names are not touched.  Every output element is ONE fp32 multiply
// (acc: one multiply and one add, not contracted), so the result does not depend on the launch shape.
template <int LPR>
__global__ __launch_bounds__(256) void k_window_slots_bwd(
    const float* __restrict__ dX, int64_t ldx, const int32_t* __restrict__ slots, int n, int64_t mb, int d,
    float scale, float base_scale, float* __restrict__ dbase, int64_t ldbase, int acc, float* __restrict__ dR,
    int64_t ldr) {
  constexpr int GPW = 64 / LPR;
  const int lane = threadIdx.x & 63;
  const int lig = lane % LPR;
  const int gid = lane / LPR;
  const int col = lig * 4;
  const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  const int64_t nwave = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t b = wave * GPW + gid; b < mb; b += nwave * GPW) {
    if (col >= d) continue;
    const float4 g = *reinterpret_cast<const float4*>(dX + b * ldx + col);
    float4 u = make_float4(__fmul_rn(base_scale, g.x), __fmul_rn(base_scale, g.y), __fmul_rn(base_scale, g.z),
                           __fmul_rn(base_scale, g.w));
    float* ub = dbase + b * ldbase + col;
    if (acc) {
      const float4 o = *reinterpret_cast<const float4*>(ub);
      u = make_float4(__fadd_rn(o.x, u.x), __fadd_rn(o.y, u.y), __fadd_rn(o.z, u.z), __fadd_rn(o.w, u.w));
    }
    *reinterpret_cast<float4*>(ub) = u;
    const float4 r = make_float4(__fmul_rn(scale, g.x), __fmul_rn(scale, g.y), __fmul_rn(scale, g.z),
                                 __fmul_rn(scale, g.w));
    int t = 0;
    for (; t + 4 <= n; t += 4) {
      const int s0 = slots[(int64_t)t * mb + b];
      const int s1 = slots[(int64_t)(t + 1) * mb + b];
      const int s2 = slots[(int64_t)(t + 2) * mb + b];
      const int s3 = slots[(int64_t)(t + 3) * mb + b];
      *reinterpret_cast<float4*>(dR + (int64_t)s0 * ldr + col) = r;
      *reinterpret_cast<float4*>(dR + (int64_t)s1 * ldr + col) = r;
      *reinterpret_cast<float4*>(dR + (int64_t)s2 * ldr + col) = r;
      *reinterpret_cast<float4*>(dR + (int64_t)s3 * ldr + col) = r;
    }
    for (; t < n; ++t) {
      const int s0 = slots[(int64_t)t * mb + b];
      *reinterpret_cast<float4*>(dR + (int64_t)s0 * ldr + col) = r;
    }
  }
}

__global__ void k_site_window(const int32_t* __restrict__ cat_map, const int32_t* __restrict__ ids, int64_t total,
                              int64_t mb, int32_t row_base, float coef, int32_t* __restrict__ keys_out,
                              int32_t* __restrict__ src_out, float* __restrict__ coef_out) {
  int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; k < total; k += stride) {
    const int id = ids[k];
    keys_out[k] = id < 0 ? ARX_KEY_NONE : (cat_map ? cat_map[id] : id);     // (as k_site_onehot: id < 0, no update)
    if (src_out) src_out[k] = row_base + (int32_t)(k % mb);
    if (coef_out) coef_out[k] = coef;
  }
}

#define ARX_WINDOW_DISPATCH_LPR(lpr, CALL)           \
  switch (lpr) {                                     \
    case 1: { constexpr int LPR = 1; CALL; } break;  \
    case 2: { constexpr int LPR = 2; CALL; } break;  \
    case 4: { constexpr int LPR = 4; CALL; } break;  \
    case 8: { constexpr int LPR = 8; CALL; } break;  \
    case 16: { constexpr int LPR = 16; CALL; } break;\
    case 32: { constexpr int LPR = 32; CALL; } break;\
    default: { constexpr int LPR = 64; CALL; } break;\
  }

static bool window_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace arx

using namespace arx;

extern "C" {

int arx_gather_window_fwd(const float* E, const int32_t* cat_map, const int32_t* ids, int n, int64_t mb, int d,
                          float scale, const float* base, int64_t ldb, float base_scale, float* out, int64_t ldo,
                          void* stream) {
  ARX_CHECK_ARG(E && ids && out, "arx_gather_window_fwd: null pointer");
  ARX_CHECK_ARG(n >= 1 && mb >= 0 && (int64_t)n * mb < (1ll << 31), "arx_gather_window_fwd: n >= 1 and n * mb < 2^31");
  if (d <= 0 || d % 4 != 0 || d > 256) {
    set_error("arx_gather_window_fwd: embedding size d=%d unsupported (need d %% 4 == 0 and d <= 256)", d);
    return ARX_EUNSUPPORTED;
  }
  ARX_CHECK_ARG(ldo % 4 == 0 && ldo >= d && window_aligned16(E) && window_aligned16(out),
                "arx_gather_window_fwd: ldo %% 4 and 16-byte alignment required");
  ARX_CHECK_ARG(!base || (ldb % 4 == 0 && ldb >= d && window_aligned16(base)),
                "arx_gather_window_fwd: base needs ldb %% 4, ldb >= d and 16-byte alignment");
  if (mb <= 0) return ARX_OK;
  const int lpr = lanes_per_row(d);
  const int64_t nwaves = ceil_div(mb, 64 / lpr);
  int64_t g = ceil_div(nwaves, 4);
  const int64_t cap = (int64_t)cu_count() * 8;
  if (g > cap) g = cap;
  ARX_WINDOW_DISPATCH_LPR(lpr, (k_gather_window<LPR><<<(int)g, 256, 0, as_stream(stream)>>>(
                                   E, d, cat_map, ids, n, mb, d, scale, base, ldb, base_scale, out, ldo)));
  ARX_CHECK_LAUNCH();
  return ARX_OK;
}

static int window_grid(int64_t mb, int lpr) {
  const int64_t nwaves = ceil_div(mb, 64 / lpr);
  int64_t g = ceil_div(nwaves, 4);
  const int64_t cap = (int64_t)cu_count() * 8;
  return (int)(g > cap ? cap : g);
}

int arx_window_slots_fwd(const float* R, int64_t ldr, const int32_t* slots, int n, int64_t mb, int d, float scale,
                         const float* base, int64_t ldb, float base_scale, float* out, int64_t ldo, void* stream) {
  ARX_CHECK_ARG(R && slots && out, "arx_window_slots_fwd: null pointer");
  ARX_CHECK_ARG(n >= 1 && mb >= 0 && (int64_t)n * mb < (1ll << 31), "arx_window_slots_fwd: n >= 1 and n * mb < 2^31");
  if (d <= 0 || d % 4 != 0 || d > 256) {
    set_error("arx_window_slots_fwd: embedding size d=%d unsupported (need d %% 4 == 0 and d <= 256)", d);
    return ARX_EUNSUPPORTED;
  }
  ARX_CHECK_ARG(ldr % 4 == 0 && ldr >= d && ldo % 4 == 0 && ldo >= d && window_aligned16(R) && window_aligned16(out),
                "arx_window_slots_fwd: ldr / ldo %% 4, >= d and 16-byte alignment required");
  ARX_CHECK_ARG(!base || (ldb % 4 == 0 && ldb >= d && window_aligned16(base)),
                "arx_window_slots_fwd: base needs ldb %% 4, ldb >= d and 16-byte alignment");
  if (mb <= 0) return ARX_OK;
  const int lpr = lanes_per_row(d);
  // the window kernel itself: the block is the table (rows ldr floats apart), the slots are the ids, no map
  ARX_WINDOW_DISPATCH_LPR(lpr, (k_gather_window<LPR><<<window_grid(mb, lpr), 256, 0, as_stream(stream)>>>(
                                   R, ldr, nullptr, slots, n, mb, d, scale, base, ldb, base_scale, out, ldo)));
  ARX_CHECK_LAUNCH();
  return ARX_OK;
}

int arx_window_slots_bwd(const float* dX, int64_t ldx, const int32_t* slots, int n, int64_t mb, int d, float scale,
                         float base_scale, float* dbase, int64_t ldbase, int acc_dbase, float* dR, int64_t ldr,
                         void* stream) {
  ARX_CHECK_ARG(dX && slots && dbase && dR, "arx_window_slots_bwd: null pointer");
  ARX_CHECK_ARG(n >= 1 && mb >= 0 && (int64_t)n * mb < (1ll << 31), "arx_window_slots_bwd: n >= 1 and n * mb < 2^31");
  if (d <= 0 || d % 4 != 0 || d > 256) {
    set_error("arx_window_slots_bwd: embedding size d=%d unsupported (need d %% 4 == 0 and d <= 256)", d);
    return ARX_EUNSUPPORTED;
  }
  ARX_CHECK_ARG(ldx % 4 == 0 && ldx >= d && ldbase % 4 == 0 && ldbase >= d && ldr % 4 == 0 && ldr >= d,
                "arx_window_slots_bwd: ldx / ldbase / ldr %% 4 and >= d required");
  ARX_CHECK_ARG(window_aligned16(dX) && window_aligned16(dbase) && window_aligned16(dR),
                "arx_window_slots_bwd: 16-byte alignment required");
  ARX_CHECK_ARG(acc_dbase == 0 || acc_dbase == 1, "arx_window_slots_bwd: acc_dbase is 0 or 1");
  if (mb <= 0) return ARX_OK;
  const int lpr = lanes_per_row(d);
  ARX_WINDOW_DISPATCH_LPR(lpr, (k_window_slots_bwd<LPR><<<window_grid(mb, lpr), 256, 0, as_stream(stream)>>>(
                                   dX, ldx, slots, n, mb, d, scale, base_scale, dbase, ldbase, acc_dbase, dR, ldr)));
  ARX_CHECK_LAUNCH();
  return ARX_OK;
}

int arx_sparse_site_window(const int32_t* cat_map, const int32_t* ids, int n, int64_t mb, int32_t row_base,
                           float coef, int32_t* keys_out, int32_t* src_out, float* coef_out, void* stream) {
  ARX_CHECK_ARG(ids && keys_out, "arx_sparse_site_window: null pointer");
  ARX_CHECK_ARG(n >= 1 && mb >= 0 && (int64_t)n * mb < (1ll << 31) && (int64_t)row_base + mb < (1ll << 31),
                "arx_sparse_site_window: n >= 1, n * mb < 2^31 and row_base + mb < 2^31");
  if (mb <= 0) return ARX_OK;
  const int64_t total = (int64_t)n * mb;
  int64_t g = ceil_div(total, 256);
  const int64_t cap = (int64_t)cu_count() * 8;
  if (g > cap) g = cap;
  k_site_window<<<(int)g, 256, 0, as_stream(stream)>>>(cat_map, ids, total, mb, row_base, coef, keys_out, src_out,
                                                       coef_out);
  ARX_CHECK_LAUNCH();
  return ARX_OK;
}

}  // extern "C"

// pair.hip -- the pairwise losses 'bpr' / 'bpr-hinge' of the HMF model and their negative draw.
//
//  arx_pair_loss_fwdbwd : pair scores + loss + all five gradients, one launch (hmf_model.py:104-106,
//                         embed_attribute.py:541-544)
//  arx_pair_loss_slots  : the same arithmetic over packed rows named by slot (the sharded step: the positive and the
//                         negative row of an interaction are two rows of ONE received block, arx/dist.py)
//  arx_pair_auc         : auc = 0.5 - 0.5 * mean sign(neg_score - pos_score) (hmf_model.py:107)
//  arx_neg_draw_uniform : one negative per row, uniform over the columns that are NOT in the user's list
//  arx_neg_draw_weighted: the same with integer column weights (popularity^power), two binary searches per row
//
// The loss kernel streams: 3 B d floats in, 3 B d out, nothing is read twice.  A row of d floats belongs to a sub-group
// of LPR = pow2ceil(d / 4) lanes, one float4 per lane (the layout of gather.hip), so a wave holds 64 / LPR rows -- 8 at
// d = 32, 4 at d = 64 -- and every lane of it carries 16 bytes of each operand.  The two dots are butterfly sums inside
// the sub-group: every lane ends with the same bits, whatever the grid.  Each row is written by exactly one sub-group
// and there are no atomics, so the result does not depend on the launch shape.
#include "common.h"

namespace arx {

template <int LPR>
__global__ __launch_bounds__(256) void k_pair_loss(
    const float* __restrict__ U, int64_t ldu, const float* __restrict__ P, int64_t ldp,
    const float* __restrict__ pbias, const float* __restrict__ N, int64_t ldn, const float* __restrict__ nbias,
    const int32_t* __restrict__ neg_ids, const float* __restrict__ row_w, int64_t B, int d, int kind, float gscale,
    float* __restrict__ pos_score, float* __restrict__ neg_score, float* __restrict__ batch_loss,
    float* dU, int64_t lddu, int acc_dU, float* __restrict__ dP, int64_t lddp, float* __restrict__ dpbias,
    float* __restrict__ dN, int64_t lddn, float* __restrict__ dnbias) {
  constexpr int GPW = 64 / LPR;
  const int lane = threadIdx.x & 63;
  const int lig = lane % LPR;
  const int gid = lane / LPR;
  const int col = lig * 4;
  const bool incol = col < d;
  const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  const int64_t nwave = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int64_t r = wave * GPW + gid; r < B; r += nwave * GPW) {
    float4 u = z4, p = z4, n = z4;
    if (incol) {
      u = *reinterpret_cast<const float4*>(U + r * ldu + col);
      p = *reinterpret_cast<const float4*>(P + r * ldp + col);
      n = *reinterpret_cast<const float4*>(N + r * ldn + col);
    }
    float sp = u.x * p.x + u.y * p.y + u.z * p.z + u.w * p.w;
    float sn = u.x * n.x + u.y * n.y + u.z * n.z + u.w * n.w;
#pragma unroll
    for (int o = LPR / 2; o > 0; o >>= 1) {
      sp += __shfl_xor(sp, o, LPR);
      sn += __shfl_xor(sn, o, LPR);
    }
    const float ps = sp + pbias[r];                       // hmf_model.py:104
    const float ns = sn + nbias[r];                       // :105
    const float x = ns - ps;                              // :106 neg_pos
    const bool live = !(neg_ids && neg_ids[r] < 0);       // void row: no eligible negative (arx_neg_draw_uniform)
    float loss, g;
    if (kind == 0) {                                      // embed_attribute.py:542 log(1 + exp(x)), stable form
      const float e = expf(-fabsf(x));
      loss = fmaxf(x, 0.f) + log1pf(e);
      g = x >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);     // sigmoid(x)
    } else {                                              // :544 max(1 + x, 0)
      const float h = 1.f + x;
      loss = fmaxf(h, 0.f);
      g = h > 0.f ? 1.f : 0.f;
    }
    const float c = live ? gscale * (row_w ? row_w[r] : 1.f) * g : 0.f;
    if (lig == 0) {
      pos_score[r] = ps;
      neg_score[r] = ns;
      batch_loss[r] = live ? loss : 0.f;
      if (dU) {
        dpbias[r] = live ? -c : 0.f;
        dnbias[r] = c;
      }
    }
    if (dU && incol) {
      float4* up = reinterpret_cast<float4*>(dU + r * lddu + col);
      float4 o = acc_dU ? *up : z4;
      float4 gp = z4, gn = z4;
      if (live) {
        o.x += c * (n.x - p.x);
        o.y += c * (n.y - p.y);
        o.z += c * (n.z - p.z);
        o.w += c * (n.w - p.w);
        gn = make_float4(c * u.x, c * u.y, c * u.z, c * u.w);
        gp = make_float4(-gn.x, -gn.y, -gn.z, -gn.w);
      }
      *up = o;
      *reinterpret_cast<float4*>(dP + r * lddp + col) = gp;
      *reinterpret_cast<float4*>(dN + r * lddn + col) = gn;
    }
  }
}

// One workgroup; the sum of signs and the number of live rows are integers, so any order gives the same float.
__global__ __launch_bounds__(256) void k_pair_auc(const float* __restrict__ pos_score,
                                                  const float* __restrict__ neg_score,
                                                  const int32_t* __restrict__ neg_ids, int64_t B,
                                                  float* __restrict__ auc) {
  __shared__ int s_sign[256];
  __shared__ int s_cnt[256];
  int sg = 0, cnt = 0;
  for (int64_t r = threadIdx.x; r < B; r += blockDim.x) {
    if (neg_ids && neg_ids[r] < 0) continue;
    const float x = neg_score[r] - pos_score[r];
    sg += (x > 0.f) - (x < 0.f);
    cnt += 1;
  }
  s_sign[threadIdx.x] = sg;
  s_cnt[threadIdx.x] = cnt;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      s_sign[threadIdx.x] += s_sign[threadIdx.x + o];
      s_cnt[threadIdx.x] += s_cnt[threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) *auc = s_cnt[0] > 0 ? 0.5f - 0.5f * ((float)s_sign[0] / (float)s_cnt[0]) : 0.5f;
}

// The slot-indirect, packed-row sibling of k_pair_loss: P and N of row r are rows pos_slot[r] / neg_slot[r] of ONE
// block R [n_slots, ldr] with the bias in column d, and their gradient rows go to the same rows of dR (-c U | -c and
// c U | c).  Every slot is named by at most one batch row (the caller's precondition), so a row of dR has one
// writer, nothing is atomic, and rows no slot names are not touched.  neg_slot < 0: a void row -- its negative is not
// read, its loss is 0, its dU and its positive's dR row are exact zeros.  A slot outside [0, n_slots) is never
// dereferenced: such a row counts as void and its missing score is 0.
template <int LPR>
__global__ __launch_bounds__(256) void k_pair_loss_slots(
    const float* __restrict__ U, int64_t ldu, const float* __restrict__ R, int64_t ldr, int64_t n_slots,
    const int32_t* __restrict__ pos_slot, const int32_t* __restrict__ neg_slot, const float* __restrict__ row_w,
    int64_t B, int d, int kind, float gscale, float* __restrict__ pos_score, float* __restrict__ neg_score,
    float* __restrict__ batch_loss, float* dU, int64_t lddu, int acc_dU, float* __restrict__ dR, int64_t lddr) {
  constexpr int GPW = 64 / LPR;
  const int lane = threadIdx.x & 63;
  const int lig = lane % LPR;
  const int gid = lane / LPR;
  const int col = lig * 4;
  const bool incol = col < d;
  const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  const int64_t nwave = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int64_t r = wave * GPW + gid; r < B; r += nwave * GPW) {
    const int64_t sp_ = pos_slot[r], sn_ = neg_slot[r];
    const bool has_p = sp_ >= 0 && sp_ < n_slots;
    const bool has_n = sn_ >= 0 && sn_ < n_slots;
    const bool live = has_p && has_n;
    float4 u = z4, p = z4, n = z4;
    if (incol) {
      u = *reinterpret_cast<const float4*>(U + r * ldu + col);
      if (has_p) p = *reinterpret_cast<const float4*>(R + sp_ * ldr + col);
      if (has_n) n = *reinterpret_cast<const float4*>(R + sn_ * ldr + col);
    }
    float sp = u.x * p.x + u.y * p.y + u.z * p.z + u.w * p.w;
    float sn = u.x * n.x + u.y * n.y + u.z * n.z + u.w * n.w;
#pragma unroll
    for (int o = LPR / 2; o > 0; o >>= 1) {
      sp += __shfl_xor(sp, o, LPR);
      sn += __shfl_xor(sn, o, LPR);
    }
    const float ps = has_p ? sp + R[sp_ * ldr + d] : 0.f;
    const float ns = has_n ? sn + R[sn_ * ldr + d] : 0.f;
    const float x = ns - ps;
    float loss, g;
    if (kind == 0) {                                      // (the arithmetic of k_pair_loss, term for term)
      const float e = expf(-fabsf(x));
      loss = fmaxf(x, 0.f) + log1pf(e);
      g = x >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
    } else {
      const float h = 1.f + x;
      loss = fmaxf(h, 0.f);
      g = h > 0.f ? 1.f : 0.f;
    }
    const float c = live ? gscale * (row_w ? row_w[r] : 1.f) * g : 0.f;
    if (lig == 0) {
      pos_score[r] = ps;
      neg_score[r] = ns;
      batch_loss[r] = live ? loss : 0.f;
      if (dU) {
        if (has_p) dR[sp_ * lddr + d] = live ? -c : 0.f;
        if (has_n) dR[sn_ * lddr + d] = c;
      }
    }
    if (dU && incol) {
      float4* up = reinterpret_cast<float4*>(dU + r * lddu + col);
      float4 o = acc_dU ? *up : z4;
      float4 gp = z4, gn = z4;
      if (live) {
        o.x += c * (n.x - p.x);
        o.y += c * (n.y - p.y);
        o.z += c * (n.z - p.z);
        o.w += c * (n.w - p.w);
        gn = make_float4(c * u.x, c * u.y, c * u.z, c * u.w);
        gp = make_float4(-gn.x, -gn.y, -gn.z, -gn.w);
      }
      *up = o;
      if (has_p) *reinterpret_cast<float4*>(dR + sp_ * lddr + col) = gp;
      if (has_n) *reinterpret_cast<float4*>(dR + sn_ * lddr + col) = gn;
    }
  }
}

// The two integers of the auc -- the sum of signs and the number of live rows -- for a caller that sums them over
// several ranks before it divides.  One workgroup of 1024 threads, integer sums (any order gives the same numbers);
// four rows per thread and round, their loads independent of each other: the kernel is a chain of load latencies,
// 4 rounds at B = 16384.
__global__ __launch_bounds__(1024) void k_pair_auc_counts(const float* __restrict__ pos_score,
                                                          const float* __restrict__ neg_score,
                                                          const int32_t* __restrict__ neg_slot, int64_t B,
                                                          int64_t n_slots, int32_t* __restrict__ counts) {
  __shared__ int s_sign[1024];
  __shared__ int s_cnt[1024];
  int sg = 0, cnt = 0;
  for (int64_t r0 = threadIdx.x; r0 < B; r0 += 4 * 1024) {
    int32_t sl[4];
    float ps[4], ns[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t r = r0 + j * 1024;
      const bool in = r < B;
      sl[j] = in ? neg_slot[r] : -1;
      ps[j] = in ? pos_score[r] : 0.f;
      ns[j] = in ? neg_score[r] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (sl[j] < 0 || sl[j] >= n_slots) continue;
      const float x = ns[j] - ps[j];
      sg += (x > 0.f) - (x < 0.f);
      cnt += 1;
    }
  }
  s_sign[threadIdx.x] = sg;
  s_cnt[threadIdx.x] = cnt;
  __syncthreads();
  for (int o = 512; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      s_sign[threadIdx.x] += s_sign[threadIdx.x + o];
      s_cnt[threadIdx.x] += s_cnt[threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    counts[0] = s_sign[0];
    counts[1] = s_cnt[0];
  }
}

// Rank-select draw.  The user's list p_0 < p_1 < ... < p_{len-1} leaves n_elig = V - len columns; the k-th of them
// (k from 0) is k + #{ j : p_j - j <= k }: p_j - j counts the eligible columns below p_j and does not decrease with j,
// so the count is one binary search.  Nothing is rejected and nothing loops.
__global__ __launch_bounds__(256) void k_neg_draw_uniform(
    const int32_t* __restrict__ users, int64_t B, int64_t n_users, const int32_t* __restrict__ ex_ptr,
    const int32_t* __restrict__ ex_cols, int32_t V, const int32_t* __restrict__ col2item, uint64_t seed,
    const uint64_t* __restrict__ step_dev, uint64_t counter, int32_t* __restrict__ neg_items,
    int32_t* __restrict__ lookup_items, int32_t* __restrict__ out_rank) {
  const uint64_t step = (step_dev ? *step_dev : 0ull) + counter;
  seed += step * 0x9e3779b97f4a7c15ull;                   // (the keying of k_dropout_fwd)
  for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < B;
       r += (int64_t)gridDim.x * blockDim.x) {
    const int32_t u = users[r];
    int32_t lo = 0, len = 0;
    if (u >= 0 && u < n_users) {
      lo = ex_ptr[u];
      len = ex_ptr[u + 1] - lo;
    }
    const int32_t n_elig = V - len;
    int32_t k = -1, item = -1;
    if (n_elig > 0 && len >= 0) {
      const uint32_t rnd = mix32(seed * 0x100000001b3ull + (uint64_t)r);
      k = (int32_t)__umulhi(rnd, (uint32_t)n_elig);
      int32_t a = 0, b = len;                             // first j with p_j - j > k
      while (a < b) {
        const int32_t m = a + ((b - a) >> 1);
        if (ex_cols[lo + m] - m <= k) a = m + 1; else b = m;
      }
      const int32_t col = k + a;
      if (col < V) item = col2item ? col2item[col] : col;     // (col >= V: a list that is not sorted and unique)
    }
    neg_items[r] = item;
    if (lookup_items) lookup_items[r] = item >= 0 ? item : (col2item ? col2item[0] : 0);
    if (out_rank) out_rank[r] = item >= 0 ? k : -1;
  }
}

// Weighted rank-select draw.  Column c weighs q[c] >= 0, cum[c] = sum_{i<c} q[i] (cum[V]: the whole mass), and the
// user's list p_0 < ... < p_{len-1} comes with H(j) = sum_{i<j} q[p_i] (ex_cum[lo + j]; H(len) adds the last entry's
// weight).  The eligible mass is M = cum[V] - H(len) and t = mulhi64(rnd64, M) is a point of it.  cum[p_j] - H(j) is the
// eligible mass below p_j and does not decrease with j, so a = #{ j : cum[p_j] - H(j) <= t } is one binary search; the
// point sits at t' = t + H(a) of the whole mass, and the column is the LARGEST c with cum[c] <= t' -- a second binary
// search, which steps over zero-weight columns.  Nothing is rejected and no loop depends on the weights.
// A list entry is clamped to [0, V] before it indexes cum, and the second search never leaves [0, V): lists that are
// not sorted, unique and in range give some column of [0, V), never a read outside the tables.
__global__ __launch_bounds__(256) void k_neg_draw_weighted(
    const int32_t* __restrict__ users, int64_t B, int64_t n_users, const int32_t* __restrict__ ex_ptr,
    const int32_t* __restrict__ ex_cols, const int64_t* __restrict__ ex_cum, const int64_t* __restrict__ cum,
    int32_t V, const int32_t* __restrict__ col2item, uint64_t seed, const uint64_t* __restrict__ step_dev,
    uint64_t counter, int32_t* __restrict__ neg_items, int32_t* __restrict__ lookup_items,
    int64_t* __restrict__ out_mass) {
  const uint64_t step = (step_dev ? *step_dev : 0ull) + counter;
  seed += step * 0x9e3779b97f4a7c15ull;                   // (the keying of k_neg_draw_uniform)
  const int64_t total = cum[V];
  for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < B;
       r += (int64_t)gridDim.x * blockDim.x) {
    const int32_t u = users[r];
    int32_t lo = 0, len = 0;
    if (u >= 0 && u < n_users) {
      lo = ex_ptr[u];
      len = ex_ptr[u + 1] - lo;
    }
    int64_t h_len = 0;                                    // H(len)
    if (len > 0) {
      const int32_t p = ex_cols[lo + len - 1];
      const int32_t pc = p < 0 ? 0 : (p > V ? V : p);
      const int32_t pn = p < 0 ? 0 : (p >= V ? V : p + 1);
      h_len = ex_cum[lo + len - 1] + (cum[pn] - cum[pc]);
    }
    const int64_t M = total - h_len;
    int64_t t = -1;
    int32_t item = -1;
    if (M > 0 && len >= 0) {
      const uint64_t rnd = mix64(seed * 0x100000001b3ull + (uint64_t)r);
      t = (int64_t)__umul64hi(rnd, (uint64_t)M);
      int32_t a = 0, b = len;                             // first j with cum[p_j] - H(j) > t
      while (a < b) {
        const int32_t m = a + ((b - a) >> 1);
        const int32_t p = ex_cols[lo + m];
        const int32_t pc = p < 0 ? 0 : (p > V ? V : p);
        if (cum[pc] - ex_cum[lo + m] <= t) a = m + 1; else b = m;
      }
      const int64_t tp = t + (a < len ? ex_cum[lo + a] : h_len);
      int32_t c0 = 0, c1 = V;                             // cum[c0] <= t' (cum[0] = 0), c1 = V or cum[c1] > t'
      while (c1 - c0 > 1) {
        const int32_t m = c0 + ((c1 - c0) >> 1);
        if (cum[m] <= tp) c0 = m; else c1 = m;
      }
      item = col2item ? col2item[c0] : c0;
    }
    neg_items[r] = item;
    if (lookup_items) lookup_items[r] = item >= 0 ? item : (col2item ? col2item[0] : 0);
    if (out_mass) out_mass[r] = item >= 0 ? t : -1;
  }
}

}  // namespace arx

using namespace arx;

#define ARX_PAIR_DISPATCH_LPR(lpr, CALL)             \
  switch (lpr) {                                     \
    case 1: { constexpr int LPR = 1; CALL; } break;  \
    case 2: { constexpr int LPR = 2; CALL; } break;  \
    case 4: { constexpr int LPR = 4; CALL; } break;  \
    case 8: { constexpr int LPR = 8; CALL; } break;  \
    case 16: { constexpr int LPR = 16; CALL; } break;\
    case 32: { constexpr int LPR = 32; CALL; } break;\
    default: { constexpr int LPR = 64; CALL; } break;\
  }

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

extern "C" {

int arx_pair_loss_fwdbwd(const float* U, int64_t ldu, const float* P, int64_t ldp, const float* pbias,
                         const float* N, int64_t ldn, const float* nbias, const int32_t* neg_ids,
                         const float* row_w, int64_t B, int d, int kind, float gscale, float* pos_score,
                         float* neg_score, float* batch_loss, float* dU, int64_t lddu, int acc_dU, float* dP,
                         int64_t lddp, float* dpbias, float* dN, int64_t lddn, float* dnbias, void* stream) {
  ARX_CHECK_ARG(B >= 0, "arx_pair_loss_fwdbwd: B < 0");
  ARX_CHECK_ARG(kind == 0 || kind == 1, "arx_pair_loss_fwdbwd: kind must be 0 (bpr) or 1 (bpr-hinge)");
  ARX_CHECK_ARG(d > 0 && d % 4 == 0 && d <= 256, "arx_pair_loss_fwdbwd: need d %% 4 == 0 and 0 < d <= 256 (d=%d)", d);
  ARX_CHECK_ARG(U && P && pbias && N && nbias && pos_score && neg_score && batch_loss,
                "arx_pair_loss_fwdbwd: null pointer");
  const bool any_grad = dU || dP || dpbias || dN || dnbias;
  ARX_CHECK_ARG(!any_grad || (dU && dP && dpbias && dN && dnbias),
                "arx_pair_loss_fwdbwd: the five gradient pointers are all null (forward only) or all set");
  ARX_CHECK_ARG(ldu % 4 == 0 && ldp % 4 == 0 && ldn % 4 == 0 && ldu >= d && ldp >= d && ldn >= d && aligned16(U) &&
                    aligned16(P) && aligned16(N),
                "arx_pair_loss_fwdbwd: leading dims %% 4, >= d and 16-byte alignment required");
  ARX_CHECK_ARG(!any_grad || (lddu % 4 == 0 && lddp % 4 == 0 && lddn % 4 == 0 && lddu >= d && lddp >= d &&
                              lddn >= d && aligned16(dU) && aligned16(dP) && aligned16(dN)),
                "arx_pair_loss_fwdbwd: gradient leading dims %% 4, >= d and 16-byte alignment required");
  if (B == 0) return ARX_OK;
  const int lpr = lanes_per_row(d);
  const int64_t nwaves = ceil_div(B, 64 / lpr);
  int64_t g = ceil_div(nwaves, 4);
  const int64_t cap = (int64_t)cu_count() * 8;
  if (g > cap) g = cap;
  ARX_PAIR_DISPATCH_LPR(lpr, (k_pair_loss<LPR><<<(int)g, 256, 0, as_stream(stream)>>>(
                                 U, ldu, P, ldp, pbias, N, ldn, nbias, neg_ids, row_w, B, d, kind, gscale, pos_score,
                                 neg_score, batch_loss, dU, lddu, acc_dU, dP, lddp, dpbias, dN, lddn, dnbias)));
  ARX_CHECK_LAUNCH();
  return ARX_OK;
}

int arx_pair_loss_slots(const float* U, int64_t ldu, const float* R, int64_t ldr, int64_t n_slots,
                        const int32_t* pos_slot, const int32_t* neg_slot, const float* row_w, int64_t B, int d,
                        int kind, float gscale, float* pos_score, float* neg_score, float* batch_loss, float* dU,
                        int64_t lddu, int acc_dU, float* dR, int64_t lddr, int32_t* auc_counts, void* stream) {
  ARX_CHECK_ARG(B >= 0 && n_slots >= 0, "arx_pair_loss_slots: B < 0 or n_slots < 0");
  ARX_CHECK_ARG(B < ((int64_t)1 << 31) && n_slots < ((int64_t)1 << 31),
                "arx_pair_loss_slots: at most 2^31 - 1 rows and slots (int32 slots, integer sums)");
  ARX_CHECK_ARG(kind == 0 || kind == 1, "arx_pair_loss_slots: kind must be 0 (bpr) or 1 (bpr-hinge)");
  ARX_CHECK_ARG(d > 0 && d % 4 == 0 && d <= 256, "arx_pair_loss_slots: need d %% 4 == 0 and 0 < d <= 256 (d=%d)", d);
  ARX_CHECK_ARG(U && R && pos_slot && neg_slot && pos_score && neg_score && batch_loss,
                "arx_pair_loss_slots: null pointer");
  ARX_CHECK_ARG((dU != nullptr) == (dR != nullptr),
                "arx_pair_loss_slots: dU and dR are both null (forward only) or both set");
  ARX_CHECK_ARG(ldu % 4 == 0 && ldr % 4 == 0 && ldu >= d && ldr >= d + 4 && aligned16(U) && aligned16(R),
                "arx_pair_loss_slots: leading dims %% 4, ldu >= d, ldr >= d + 4 (packed rows: bias in column d) and "
                "16-byte alignment required");
  ARX_CHECK_ARG(!dU || (lddu % 4 == 0 && lddr % 4 == 0 && lddu >= d && lddr >= d + 4 && aligned16(dU) &&
                        aligned16(dR)),
                "arx_pair_loss_slots: gradient leading dims %% 4, lddu >= d, lddr >= d + 4 and 16-byte alignment "
                "required");
  if (B == 0) return ARX_OK;
  const int lpr = lanes_per_row(d);
  const int64_t nwaves = ceil_div(B, 64 / lpr);
  int64_t g = ceil_div(nwaves, 4);
  const int64_t cap = (int64_t)cu_count() * 8;
  if (g > cap) g = cap;
  ARX_PAIR_DISPATCH_LPR(lpr, (k_pair_loss_slots<LPR><<<(int)g, 256, 0, as_stream(stream)>>>(
                                 U, ldu, R, ldr, n_slots, pos_slot, neg_slot, row_w, B, d, kind, gscale, pos_score,
                                 neg_score, batch_loss, dU, lddu, acc_dU, dR, lddr)));
  ARX_CHECK_LAUNCH();
  if (auc_counts) {
    k_pair_auc_counts<<<1, 1024, 0, as_stream(stream)>>>(pos_score, neg_score, neg_slot, B, n_slots, auc_counts);
    ARX_CHECK_LAUNCH();
  }
  return ARX_OK;
}

int arx_pair_auc(const float* pos_score, const float* neg_score, const int32_t* neg_ids, int64_t B, float* auc,
                 void* stream) {
  ARX_CHECK_ARG(B >= 0, "arx_pair_auc: B < 0");
  ARX_CHECK_ARG(pos_score && neg_score && auc, "arx_pair_auc: null pointer");
  ARX_CHECK_ARG(B < ((int64_t)1 << 31), "arx_pair_auc: at most 2^31 - 1 rows (integer sums)");
  if (B == 0) return ARX_OK;
  k_pair_auc<<<1, 256, 0, as_stream(stream)>>>(pos_score, neg_score, neg_ids, B, auc);
  ARX_CHECK_LAUNCH();
  return ARX_OK;
}

int arx_neg_draw_uniform(const int32_t* users, int64_t B, int64_t n_users, const int32_t* ex_ptr,
                         const int32_t* ex_cols, int64_t V, const int32_t* col2item, uint64_t seed,
                         const uint64_t* step_dev, uint64_t counter, int32_t* neg_items, int32_t* lookup_items,
                         int32_t* out_rank, void* stream) {
  ARX_CHECK_ARG(B >= 0 && n_users >= 0, "arx_neg_draw_uniform: B < 0 or n_users < 0");
  ARX_CHECK_ARG(V > 0 && V < ((int64_t)1 << 31), "arx_neg_draw_uniform: need 0 < V < 2^31");
  ARX_CHECK_ARG(users && ex_ptr && ex_cols && neg_items, "arx_neg_draw_uniform: null pointer");
  if (B == 0) return ARX_OK;
  int64_t g = ceil_div(B, 256);
  const int64_t cap = (int64_t)cu_count() * 8;
  if (g > cap) g = cap;
  k_neg_draw_uniform<<<(int)g, 256, 0, as_stream(stream)>>>(users, B, n_users, ex_ptr, ex_cols, (int32_t)V, col2item,
                                                            seed, step_dev, counter, neg_items, lookup_items,
                                                            out_rank);
  ARX_CHECK_LAUNCH();
  return ARX_OK;
}

int arx_neg_draw_weighted(const int32_t* users, int64_t B, int64_t n_users, const int32_t* ex_ptr,
                          const int32_t* ex_cols, const int64_t* ex_cum, const int64_t* cum, int64_t V,
                          const int32_t* col2item, uint64_t seed, const uint64_t* step_dev, uint64_t counter,
                          int32_t* neg_items, int32_t* lookup_items, int64_t* out_mass, void* stream) {
  ARX_CHECK_ARG(B >= 0 && n_users >= 0, "arx_neg_draw_weighted: B < 0 or n_users < 0");
  ARX_CHECK_ARG(V > 0 && V < ((int64_t)1 << 31), "arx_neg_draw_weighted: need 0 < V < 2^31");
  ARX_CHECK_ARG(users && ex_ptr && ex_cols && ex_cum && cum && neg_items, "arx_neg_draw_weighted: null pointer");
  if (B == 0) return ARX_OK;
  int64_t g = ceil_div(B, 256);
  const int64_t cap = (int64_t)cu_count() * 8;
  if (g > cap) g = cap;
  k_neg_draw_weighted<<<(int)g, 256, 0, as_stream(stream)>>>(users, B, n_users, ex_ptr, ex_cols, ex_cum, cum,
                                                             (int32_t)V, col2item, seed, step_dev, counter, neg_items,
                                                             lookup_items, out_mass);
  ARX_CHECK_LAUNCH();
  return ARX_OK;
}

}  // extern "C"

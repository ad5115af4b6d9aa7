// gru.hip -- GRU sequence encoder: SeqModel(cell='gru').
//
// tf.contrib.rnn GRUCell(h) (TF 1.0): [r | u] = sigmoid([x_t, h_{t-1}] . Wg + bg), c = tanh([x_t, r * h_{t-1}] . Wc + bc),
// h_t = u * h_{t-1} + (1 - u) * c; zero initial state; static_rnn runs all L steps.  The reset is applied BEFORE the
// candidate's product (not cuDNN's form), so a time step is two dependent products with a workgroup barrier between
// them, forward and backward.
//
// The kernels have the shape of lstm.hip's: ONE persistent launch walks all L steps, a workgroup owns 16 batch rows
// (the M of v_mfma_f32_16x16x4_f32), its 4 waves own h/4 units each -- r, u and c of those units, so the state update
// is register-local; h_{t-1} lives in LDS (double-buffered, stride h + 2), r * h_{t-1} in a third buffer, the wave's own
// units of h_{t-1} in registers, x_{t+1} is prefetched into LDS while step t computes.
//   phase 1: zg = [x, h] . Wg for the wave's units, the gates, r * h_prev into LDS; the x half of the candidate's
//            product (it does not depend on r) is issued here too, so the barrier waits behind MFMAs;  barrier
//   phase 2: zc += rh . Wc_h, c, h_t into the other h buffer;  barrier
// Backward, per step: dzc into LDS; barrier; q = dzc . Wc_h^T, dzr, [dzr | dzu] into LDS; barrier; the second product
// against Wg_h^T; dh_prev stays in registers.  Two barriers per step are enough because each buffer is written in one
// span only: dzc ahead of the first barrier (its readers sit between the two barriers of the step before), BOTH halves
// of [dzr | dzu] between the two barriers (its readers sit behind the second barrier of the step before; dzu, known
// ahead of the first barrier, waits in a register).
//
// Compiler resource report (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
//   k_gru_fwd_wreg<64>: 154 VGPRs + 24 AGPRs, scratch 0, no spill, LDS 21120 B, 2 waves / SIMD
//   k_gru_bwd_wreg<64>: 148 VGPRs +  8 AGPRs, scratch 0, no spill, LDS 12544 B, 3 waves / SIMD
//   (the streaming and generic kernels: 22 .. 94 VGPRs, scratch 0)
#include <stdlib.h>

#include "common.h"
#include "gate_fn.h"

namespace arx {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kGruRows = 16;  // batch rows per workgroup (MFMA M)

// ---- h in {64, 128}, din % 4 == 0: Wg and Wc streamed from L2 as the MFMA B operands ----------------------
// TPG = 16-unit tiles per wave = h / 64
template <int TPG>
__global__ __launch_bounds__(256) void k_gru_fwd(
    const float* __restrict__ x, const float* __restrict__ Wg, const float* __restrict__ bg,
    const float* __restrict__ Wc, const float* __restrict__ bc, int64_t L, int64_t B, int din, int h,
    float* __restrict__ hs, float* __restrict__ gates, float* __restrict__ rh) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int SX = din + 2, SH = h + 2;
  float* xbuf = smem;                            // [2][16][SX]
  float* hbuf = smem + 2 * kGruRows * SX;        // [2][16][SH]
  float* rbuf = hbuf + 2 * kGruRows * SH;        // [16][SH]: r * h_{t-1}
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l15 = lane & 15, lq = lane >> 4;
  const int64_t row0 = (int64_t)blockIdx.x * kGruRows;
  const int ubase = wave * (h / 4);
  const int H2 = 2 * h, H3 = 3 * h;

  // zero h_{-1}, stage x_0
  for (int i = threadIdx.x; i < kGruRows * SH; i += 256) hbuf[i] = 0.f;
  for (int i = threadIdx.x; i < kGruRows * din; i += 256) {
    const int r = i / din, c = i % din;
    const int64_t gr = row0 + r;
    xbuf[r * SX + c] = (gr < B) ? x[gr * din + c] : 0.f;
  }
  float hprev[TPG][4];
#pragma unroll
  for (int tp = 0; tp < TPG; ++tp)
#pragma unroll
    for (int r = 0; r < 4; ++r) hprev[tp][r] = 0.f;
  __syncthreads();

  for (int64_t t = 0; t < L; ++t) {
    const int cur = (int)(t & 1), nxt = cur ^ 1;
    const float* xb = xbuf + cur * kGruRows * SX;
    const float* hb = hbuf + cur * kGruRows * SH;
    // prefetch x_{t+1}
    if (t + 1 < L) {
      float* xn = xbuf + nxt * kGruRows * SX;
      const float* xs = x + (t + 1) * B * din;
      for (int i = threadIdx.x; i < kGruRows * din; i += 256) {
        const int r = i / din, c = i % din;
        const int64_t gr = row0 + r;
        xn[r * SX + c] = (gr < B) ? xs[gr * din + c] : 0.f;
      }
    }
    f32x4 ar[TPG], au[TPG], ac[TPG];
#pragma unroll
    for (int tp = 0; tp < TPG; ++tp) {
      const int unit = ubase + tp * 16 + l15;
      const float br = bg[unit], bu = bg[h + unit], bcv = bc[unit];
      ar[tp] = (f32x4){br, br, br, br};
      au[tp] = (f32x4){bu, bu, bu, bu};
      ac[tp] = (f32x4){bcv, bcv, bcv, bcv};
    }
    // ---- phase 1.  x part: both gates and the candidate's x half
    for (int kk = 0; kk < din; kk += 4) {
      const float a = xb[l15 * SX + kk + lq];
      const float* wg = Wg + (int64_t)(kk + lq) * H2 + ubase + l15;
      const float* wc = Wc + (int64_t)(kk + lq) * h + ubase + l15;
#pragma unroll
      for (int tp = 0; tp < TPG; ++tp) {
        ar[tp] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, wg[tp * 16], ar[tp], 0, 0, 0);
        au[tp] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, wg[h + tp * 16], au[tp], 0, 0, 0);
        ac[tp] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, wc[tp * 16], ac[tp], 0, 0, 0);
      }
    }
    // h part of the gates
    for (int kk = 0; kk < h; kk += 4) {
      const float a = hb[l15 * SH + kk + lq];
      const float* wg = Wg + (int64_t)(din + kk + lq) * H2 + ubase + l15;
#pragma unroll
      for (int tp = 0; tp < TPG; ++tp) {
        ar[tp] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, wg[tp * 16], ar[tp], 0, 0, 0);
        au[tp] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, wg[h + tp * 16], au[tp], 0, 0, 0);
      }
    }
    // gates; C/D map of 16x16: col = lane&15 (unit), row = (lane>>4)*4 + reg
    float gu[TPG][4];
#pragma unroll
    for (int tp = 0; tp < TPG; ++tp) {
      const int unit = ubase + tp * 16 + l15;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int lrow = lq * 4 + r;
        const int64_t gr = row0 + lrow;
        const float g_r = sigmoidf_(ar[tp][r]);
        gu[tp][r] = sigmoidf_(au[tp][r]);
        const float v = g_r * hprev[tp][r];
        rbuf[lrow * SH + unit] = v;
        if (gr < B) {
          const int64_t o = t * B + gr;
          rh[o * h + unit] = v;
          gates[o * H3 + unit] = g_r;
          gates[o * H3 + h + unit] = gu[tp][r];
        }
      }
    }
    __syncthreads();
    // ---- phase 2: the candidate's h half reads r * h_{t-1}
    for (int kk = 0; kk < h; kk += 4) {
      const float a = rbuf[l15 * SH + kk + lq];
      const float* wc = Wc + (int64_t)(din + kk + lq) * h + ubase + l15;
#pragma unroll
      for (int tp = 0; tp < TPG; ++tp)
        ac[tp] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, wc[tp * 16], ac[tp], 0, 0, 0);
    }
    float* hn = hbuf + nxt * kGruRows * SH;
#pragma unroll
    for (int tp = 0; tp < TPG; ++tp) {
      const int unit = ubase + tp * 16 + l15;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int lrow = lq * 4 + r;
        const int64_t gr = row0 + lrow;
        const float c = tanhf_(ac[tp][r]);
        const float u = gu[tp][r];
        const float hh = u * hprev[tp][r] + (1.f - u) * c;
        hprev[tp][r] = hh;
        hn[lrow * SH + unit] = hh;
        if (gr < B) {
          const int64_t o = t * B + gr;
          hs[o * h + unit] = hh;
          gates[o * H3 + 2 * h + unit] = c;
        }
      }
    }
    __syncthreads();
  }
}

template <int TPG>
__global__ __launch_bounds__(256) void k_gru_bwd(
    const float* __restrict__ Wg, const float* __restrict__ Wc, const float* __restrict__ hs,
    const float* __restrict__ gates, const float* __restrict__ dhs, int64_t L, int64_t B, int din, int h,
    float* __restrict__ dzg, float* __restrict__ dzc) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int H2 = 2 * h, H3 = 3 * h, SC = h + 2, SG = H2 + 2;
  float* cbuf = smem;                       // [16][SC]: dzc
  float* gbuf = smem + kGruRows * SC;       // [16][SG]: [dzr | dzu]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l15 = lane & 15, lq = lane >> 4;
  const int64_t row0 = (int64_t)blockIdx.x * kGruRows;
  const int ubase = wave * (h / 4);
  float dh_rec[TPG][4];
#pragma unroll
  for (int tp = 0; tp < TPG; ++tp)
#pragma unroll
    for (int r = 0; r < 4; ++r) dh_rec[tp][r] = 0.f;

  for (int64_t t = L - 1; t >= 0; --t) {
    float g_r[TPG][4], hp[TPG][4], keep[TPG][4], zus[TPG][4];      // keep = dh * u, the direct part of dh_{t-1}
#pragma unroll
    for (int tp = 0; tp < TPG; ++tp) {
      const int unit = ubase + tp * 16 + l15;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int lrow = lq * 4 + r;
        const int64_t gr = row0 + lrow;
        float zc = 0.f, zu = 0.f;
        g_r[tp][r] = hp[tp][r] = keep[tp][r] = 0.f;
        if (gr < B) {
          const int64_t o = t * B + gr;
          const float* gp = gates + o * H3 + unit;
          const float rr = gp[0], u = gp[h], c = gp[2 * h];
          const float hprev = (t > 0) ? hs[(o - B) * h + unit] : 0.f;
          const float dh = dhs[o * h + unit] + dh_rec[tp][r];
          const float du = dh * (hprev - c);
          const float dc = dh * (1.f - u);
          zc = dc * (1.f - c * c);
          zu = du * u * (1.f - u);
          g_r[tp][r] = rr;
          hp[tp][r] = hprev;
          keep[tp][r] = dh * u;
          dzc[o * h + unit] = zc;
          dzg[o * H2 + h + unit] = zu;
        }
        cbuf[lrow * SC + unit] = zc;
        zus[tp][r] = zu;                // (into LDS behind the barrier, with dzr: the buffer may still be read here)
      }
    }
    __syncthreads();
    // q[row, unit] = sum_k dzc[row, k] * Wc[din + unit, k]
    f32x4 acc[TPG];
#pragma unroll
    for (int tp = 0; tp < TPG; ++tp) acc[tp] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int kk = 0; kk < h; kk += 4) {
      const float a = cbuf[l15 * SC + kk + lq];
#pragma unroll
      for (int tp = 0; tp < TPG; ++tp) {
        const float b = Wc[(int64_t)(din + ubase + tp * 16 + l15) * h + kk + lq];
        acc[tp] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[tp], 0, 0, 0);
      }
    }
#pragma unroll
    for (int tp = 0; tp < TPG; ++tp) {
      const int unit = ubase + tp * 16 + l15;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int lrow = lq * 4 + r;
        const int64_t gr = row0 + lrow;
        float zr = 0.f;
        if (gr < B) {
          const float q = acc[tp][r], rr = g_r[tp][r];
          zr = q * hp[tp][r] * rr * (1.f - rr);
          keep[tp][r] += q * rr;
          dzg[(t * B + gr) * H2 + unit] = zr;
        }
        gbuf[lrow * SG + unit] = zr;
        gbuf[lrow * SG + h + unit] = zus[tp][r];
      }
    }
    __syncthreads();
    if (t > 0) {
      // dh_{t-1}[row, unit] = dh * u + q * r + sum_k [dzr | dzu][row, k] * Wg[din + unit, k]
#pragma unroll
      for (int tp = 0; tp < TPG; ++tp) acc[tp] = (f32x4){0.f, 0.f, 0.f, 0.f};
      for (int kk = 0; kk < H2; kk += 4) {
        const float a = gbuf[l15 * SG + kk + lq];
#pragma unroll
        for (int tp = 0; tp < TPG; ++tp) {
          const float b = Wg[(int64_t)(din + ubase + tp * 16 + l15) * H2 + kk + lq];
          acc[tp] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[tp], 0, 0, 0);
        }
      }
#pragma unroll
      for (int tp = 0; tp < TPG; ++tp)
#pragma unroll
        for (int r = 0; r < 4; ++r) dh_rec[tp][r] = keep[tp][r] + acc[tp][r];
    }
  }
}

// ---- d = h = 64 (config C4): weights register-resident -------------------------------------------------
// The wave's slice of Wg, Wc and the biases is loaded ONCE: (64 + 64) rows x (16 r + 16 u + 16 c) columns = 96 VGPRs
// per lane.  A step is then LDS operand reads plus back-to-back MFMAs.  Backward holds its slices of Wg_h^T (32 VGPRs)
// and Wc_h^T (16) and prefetches the next step's gates, h_prev and dh into registers under the current products.
template <int DIN>
__global__ __launch_bounds__(256, 1) void k_gru_fwd_wreg(
    const float* __restrict__ x, const float* __restrict__ Wg, const float* __restrict__ bg,
    const float* __restrict__ Wc, const float* __restrict__ bc, int64_t L, int64_t B,
    float* __restrict__ hs, float* __restrict__ gates, float* __restrict__ rh) {
  constexpr int H = 64, H2 = 128, H3 = 192, SX = DIN + 2, SH = H + 2;
  constexpr int NKX = DIN / 4, NKH = H / 4, NX = kGruRows * DIN / 256;
  __shared__ __attribute__((aligned(16))) float xbuf[2][kGruRows * SX];
  __shared__ __attribute__((aligned(16))) float hbuf[2][kGruRows * SH];
  __shared__ __attribute__((aligned(16))) float rbuf[kGruRows * SH];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l15 = lane & 15, lq = lane >> 4;
  const int64_t row0 = (int64_t)blockIdx.x * kGruRows;
  const int unit = wave * 16 + l15;
  // weight slices: k = 4*ks + lq; columns unit (r), H + unit (u) of Wg, unit of Wc
  float wgx[NKX][2], wgh[NKH][2], wcx[NKX], wch[NKH];
#pragma unroll
  for (int ks = 0; ks < NKX; ++ks) {
    wgx[ks][0] = Wg[(int64_t)(4 * ks + lq) * H2 + unit];
    wgx[ks][1] = Wg[(int64_t)(4 * ks + lq) * H2 + H + unit];
    wcx[ks] = Wc[(int64_t)(4 * ks + lq) * H + unit];
  }
#pragma unroll
  for (int ks = 0; ks < NKH; ++ks) {
    wgh[ks][0] = Wg[(int64_t)(DIN + 4 * ks + lq) * H2 + unit];
    wgh[ks][1] = Wg[(int64_t)(DIN + 4 * ks + lq) * H2 + H + unit];
    wch[ks] = Wc[(int64_t)(DIN + 4 * ks + lq) * H + unit];
  }
  const float br = bg[unit], bu = bg[H + unit], bcv = bc[unit];
  for (int i = threadIdx.x; i < kGruRows * SH; i += 256) hbuf[0][i] = 0.f;
  for (int i = threadIdx.x; i < kGruRows * DIN; i += 256) {
    const int r = i / DIN, c = i % DIN;
    const int64_t gr = row0 + r;
    xbuf[0][r * SX + c] = (gr < B) ? x[gr * DIN + c] : 0.f;
  }
  float hprev[4] = {0.f, 0.f, 0.f, 0.f};
  __syncthreads();
  for (int64_t t = 0; t < L; ++t) {
    const int cur = (int)(t & 1), nxt = cur ^ 1;
    const float* xb = xbuf[cur];
    const float* hb = hbuf[cur];
    float xn[NX];                                // x_{t+1}: loads fly under the MFMAs
    if (t + 1 < L) {
      const float* xs = x + (t + 1) * B * DIN;
#pragma unroll
      for (int q = 0; q < NX; ++q) {
        const int i = threadIdx.x + q * 256;
        const int64_t gr = row0 + i / DIN;
        xn[q] = xs[min(gr, B - 1) * DIN + i % DIN];
      }
    }
    f32x4 ar = (f32x4){br, br, br, br}, au = (f32x4){bu, bu, bu, bu}, ac = (f32x4){bcv, bcv, bcv, bcv};
    // ---- phase 1 (the candidate's x half rides along: it does not depend on r)
#pragma unroll
    for (int ks = 0; ks < NKX; ++ks) {
      const float a = xb[l15 * SX + 4 * ks + lq];
      ar = __builtin_amdgcn_mfma_f32_16x16x4f32(a, wgx[ks][0], ar, 0, 0, 0);
      au = __builtin_amdgcn_mfma_f32_16x16x4f32(a, wgx[ks][1], au, 0, 0, 0);
      ac = __builtin_amdgcn_mfma_f32_16x16x4f32(a, wcx[ks], ac, 0, 0, 0);
    }
#pragma unroll
    for (int ks = 0; ks < NKH; ++ks) {
      const float a = hb[l15 * SH + 4 * ks + lq];
      ar = __builtin_amdgcn_mfma_f32_16x16x4f32(a, wgh[ks][0], ar, 0, 0, 0);
      au = __builtin_amdgcn_mfma_f32_16x16x4f32(a, wgh[ks][1], au, 0, 0, 0);
    }
    // C/D map of 16x16: col = lane&15 (unit), row = (lane>>4)*4 + reg
    float gu[4], gr_[4], rhv[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      gr_[r] = sigmoidf_(ar[r]);
      gu[r] = sigmoidf_(au[r]);
      rhv[r] = gr_[r] * hprev[r];
      rbuf[(lq * 4 + r) * SH + unit] = rhv[r];
    }
    __syncthreads();
    // ---- phase 2
    f32x4 ac1 = (f32x4){0.f, 0.f, 0.f, 0.f};     // two chains: MFMA latency
#pragma unroll
    for (int ks = 0; ks < NKH; ks += 2) {
      const float a0 = rbuf[l15 * SH + 4 * ks + lq];
      const float a1 = rbuf[l15 * SH + 4 * (ks + 1) + lq];
      ac = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, wch[ks], ac, 0, 0, 0);
      ac1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, wch[ks + 1], ac1, 0, 0, 0);
    }
    float* hn = hbuf[nxt];
    float cv[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      cv[r] = tanhf_(ac[r] + ac1[r]);
      const float hh = gu[r] * hprev[r] + (1.f - gu[r]) * cv[r];
      hprev[r] = hh;
      hn[(lq * 4 + r) * SH + unit] = hh;
    }
    // (x_{t+1} goes to LDS BEFORE the step's global stores are issued: loads and stores share the vmcnt counter)
    if (t + 1 < L) {
      float* xw = xbuf[nxt];
#pragma unroll
      for (int q = 0; q < NX; ++q) {
        const int i = threadIdx.x + q * 256;
        const int64_t gr = row0 + i / DIN;
        xw[(i / DIN) * SX + i % DIN] = (gr < B) ? xn[q] : 0.f;
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t gr = row0 + lq * 4 + r;
      if (gr < B) {
        const int64_t o = t * B + gr;
        hs[o * H + unit] = hprev[r];
        rh[o * H + unit] = rhv[r];
        float* gp = gates + o * H3 + unit;
        gp[0] = gr_[r];
        gp[H] = gu[r];
        gp[2 * H] = cv[r];
      }
    }
    __syncthreads();
  }
}

template <int DIN>
__global__ __launch_bounds__(256, 1) void k_gru_bwd_wreg(
    const float* __restrict__ Wg, const float* __restrict__ Wc, const float* __restrict__ hs,
    const float* __restrict__ gates, const float* __restrict__ dhs, int64_t L, int64_t B,
    float* __restrict__ dzg, float* __restrict__ dzc) {
  constexpr int H = 64, H2 = 128, H3 = 192, SC = H + 2, SG = H2 + 2, NKC = H / 4, NKG = H2 / 4;
  __shared__ __attribute__((aligned(16))) float cbuf[kGruRows * SC];
  __shared__ __attribute__((aligned(16))) float gbuf[kGruRows * SG];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l15 = lane & 15, lq = lane >> 4;
  const int64_t row0 = (int64_t)blockIdx.x * kGruRows;
  const int unit = wave * 16 + l15;
  // B operand element (k = 4*ks + lq, unit) of Wc_h^T and Wg_h^T
  float wct[NKC], wgt[NKG];
#pragma unroll
  for (int ks = 0; ks < NKC; ++ks) wct[ks] = Wc[(int64_t)(DIN + unit) * H + 4 * ks + lq];
#pragma unroll
  for (int ks = 0; ks < NKG; ++ks) wgt[ks] = Wg[(int64_t)(DIN + unit) * H2 + 4 * ks + lq];
  float dh_rec[4] = {0.f, 0.f, 0.f, 0.f};
  // step-t inputs of this lane's 4 rows: r, u, c, h_prev, dh
  float pr[4], pu[4], pc[4], php[4], pdh[4];
  auto prefetch = [&](int64_t t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t gr = min(row0 + lq * 4 + r, B - 1);
      const int64_t o = t * B + gr;
      const float* gp = gates + o * H3 + unit;
      pr[r] = gp[0];
      pu[r] = gp[H];
      pc[r] = gp[2 * H];
      php[r] = (t > 0) ? hs[(o - B) * H + unit] : 0.f;
      pdh[r] = dhs[o * H + unit];
    }
  };
  if (L > 0) prefetch(L - 1);
  for (int64_t t = L - 1; t >= 0; --t) {
    float g_r[4], hp[4], keep[4], zus[4];         // keep = dh * u, the direct part of dh_{t-1}
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int lrow = lq * 4 + r;
      const int64_t gr = row0 + lrow;
      float zc = 0.f, zu = 0.f;
      g_r[r] = hp[r] = keep[r] = 0.f;
      if (gr < B) {
        const float u = pu[r], c = pc[r];
        const float dh = pdh[r] + dh_rec[r];
        const float du = dh * (php[r] - c);
        const float dc = dh * (1.f - u);
        zc = dc * (1.f - c * c);
        zu = du * u * (1.f - u);
        g_r[r] = pr[r];
        hp[r] = php[r];
        keep[r] = dh * u;
        dzc[(t * B + gr) * H + unit] = zc;
        dzg[(t * B + gr) * H2 + H + unit] = zu;
      }
      cbuf[lrow * SC + unit] = zc;
      zus[r] = zu;                      // (into LDS behind the barrier, with dzr: the buffer may still be read here)
    }
    __syncthreads();
    if (t > 0) prefetch(t - 1);                   // in flight under the two products
    // q[row, unit] = sum_k dzc[row, k] * Wc[DIN + unit, k]
    f32x4 acc0 = (f32x4){0.f, 0.f, 0.f, 0.f}, acc1 = acc0;   // two chains: MFMA latency
#pragma unroll
    for (int ks = 0; ks < NKC; ks += 2) {
      const float a0 = cbuf[l15 * SC + 4 * ks + lq];
      const float a1 = cbuf[l15 * SC + 4 * (ks + 1) + lq];
      acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, wct[ks], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, wct[ks + 1], acc1, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int lrow = lq * 4 + r;
      const int64_t gr = row0 + lrow;
      float zr = 0.f;
      if (gr < B) {
        const float q = acc0[r] + acc1[r], rr = g_r[r];
        zr = q * hp[r] * rr * (1.f - rr);
        keep[r] += q * rr;
        dzg[(t * B + gr) * H2 + unit] = zr;
      }
      gbuf[lrow * SG + unit] = zr;
      gbuf[lrow * SG + H + unit] = zus[r];
    }
    __syncthreads();
    if (t > 0) {
      // dh_{t-1}[row, unit] = dh * u + q * r + sum_k [dzr | dzu][row, k] * Wg[DIN + unit, k]
      acc0 = (f32x4){0.f, 0.f, 0.f, 0.f};
      acc1 = acc0;
#pragma unroll
      for (int ks = 0; ks < NKG; ks += 2) {
        const float a0 = gbuf[l15 * SG + 4 * ks + lq];
        const float a1 = gbuf[l15 * SG + 4 * (ks + 1) + lq];
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, wgt[ks], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, wgt[ks + 1], acc1, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) dh_rec[r] = keep[r] + (acc0[r] + acc1[r]);
    }
  }
}

// ---- generic fallback (any din, h): one workgroup per batch row -------------
__global__ __launch_bounds__(256) void k_gru_fwd_generic(
    const float* __restrict__ x, const float* __restrict__ Wg, const float* __restrict__ bg,
    const float* __restrict__ Wc, const float* __restrict__ bc, int64_t L, int64_t B, int din, int h,
    float* __restrict__ hs, float* __restrict__ gates, float* __restrict__ rh) {
  extern __shared__ float smem[];
  float* in = smem;            // [din + h]: x_t, h_{t-1}
  float* g = smem + din + h;   // [2h]: r, u
  float* rv = g + 2 * h;       // [h]: r * h_{t-1}
  const int64_t b = blockIdx.x;
  const int K = din + h, H2 = 2 * h, H3 = 3 * h;
  for (int i = threadIdx.x; i < h; i += 256) in[din + i] = 0.f;
  for (int64_t t = 0; t < L; ++t) {
    const int64_t o = t * B + b;
    for (int i = threadIdx.x; i < din; i += 256) in[i] = x[o * din + i];
    __syncthreads();
    for (int c = threadIdx.x; c < H2; c += 256) {
      float s = bg[c];
      for (int k = 0; k < K; ++k) s = fmaf(in[k], Wg[(int64_t)k * H2 + c], s);
      const float v = sigmoidf_(s);
      g[c] = v;
      gates[o * H3 + c] = v;
      if (c < h) {
        const float p = v * in[din + c];
        rv[c] = p;
        rh[o * h + c] = p;
      }
    }
    __syncthreads();
    for (int u = threadIdx.x; u < h; u += 256) {
      float s = bc[u];
      for (int k = 0; k < din; ++k) s = fmaf(in[k], Wc[(int64_t)k * h + u], s);
      for (int k = 0; k < h; ++k) s = fmaf(rv[k], Wc[(int64_t)(din + k) * h + u], s);
      const float c = tanhf_(s);
      const float uu = g[h + u];
      const float hh = uu * in[din + u] + (1.f - uu) * c;     // (in[din + u] is read by this thread alone here)
      in[din + u] = hh;
      hs[o * h + u] = hh;
      gates[o * H3 + 2 * h + u] = c;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void k_gru_bwd_generic(
    const float* __restrict__ Wg, const float* __restrict__ Wc, const float* __restrict__ hs,
    const float* __restrict__ gates, const float* __restrict__ dhs, int64_t L, int64_t B, int din, int h,
    float* __restrict__ dzg, float* __restrict__ dzc) {
  extern __shared__ float smem[];
  float* zc = smem;            // [h]
  float* zg = smem + h;        // [2h]: dzr, dzu
  float* dhr = zg + 2 * h;     // [h]: the recurrent part of dh_t
  float* keep = dhr + h;       // [h]: dh * u, then + q * r
  const int64_t b = blockIdx.x;
  const int H2 = 2 * h, H3 = 3 * h;
  for (int i = threadIdx.x; i < h; i += 256) dhr[i] = 0.f;
  __syncthreads();
  for (int64_t t = L - 1; t >= 0; --t) {
    const int64_t o = t * B + b;
    for (int u = threadIdx.x; u < h; u += 256) {
      const float uu = gates[o * H3 + h + u], c = gates[o * H3 + 2 * h + u];
      const float hprev = (t > 0) ? hs[(o - B) * h + u] : 0.f;
      const float dh = dhs[o * h + u] + dhr[u];
      const float du = dh * (hprev - c);
      const float dc = dh * (1.f - uu);
      const float vc = dc * (1.f - c * c), vu = du * uu * (1.f - uu);
      zc[u] = vc;
      zg[h + u] = vu;
      keep[u] = dh * uu;
      dzc[o * h + u] = vc;
      dzg[o * H2 + h + u] = vu;
    }
    __syncthreads();
    for (int u = threadIdx.x; u < h; u += 256) {
      float q = 0.f;
      const float* wr = Wc + (int64_t)(din + u) * h;
      for (int k = 0; k < h; ++k) q = fmaf(zc[k], wr[k], q);
      const float rr = gates[o * H3 + u];
      const float hprev = (t > 0) ? hs[(o - B) * h + u] : 0.f;
      const float vr = q * hprev * rr * (1.f - rr);
      zg[u] = vr;
      keep[u] += q * rr;
      dzg[o * H2 + u] = vr;
    }
    __syncthreads();
    if (t > 0) {
      for (int u = threadIdx.x; u < h; u += 256) {
        float s = 0.f;
        const float* wr = Wg + (int64_t)(din + u) * H2;
        for (int k = 0; k < H2; ++k) s = fmaf(zg[k], wr[k], s);
        dhr[u] = keep[u] + s;
      }
      __syncthreads();
    }
  }
}

// Dynamic LDS of the streaming and generic kernels grows with din and h: up to the CU's 160 KB, an argument error past
// it; past 64 KB the kernel is opted in (lstm.hip states the rule).
constexpr size_t kGruLdsLimit = 160 * 1024;

static int gru_raise_lds(const void* kern, size_t lds) {
  if (lds > 64 * 1024)
    ARX_CHECK_HIP(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  return ARX_OK;
}

// 0 wreg, 1 mfma, 2 generic -- the same rule forward and backward (tests/gru_paths.py restates it)
static int gru_path(int din, int h) {
  if (h == 64 && din == 64) return 0;
  if ((h == 64 || h == 128) && din % 4 == 0) return 1;
  return 2;
}

}  // namespace arx

using namespace arx;

extern "C" {

int arx_gru_fwd(const float* x, const float* Wg, const float* bg, const float* Wc, const float* bc, int64_t L,
                int64_t B, int din, int h, float* hs, float* gates, float* rh, void* stream) {
  ARX_CHECK_ARG(x && Wg && bg && Wc && bc && hs && gates && rh, "arx_gru_fwd: null pointer");
  ARX_CHECK_ARG(L >= 0 && B >= 0 && din > 0 && h > 0, "arx_gru_fwd: bad size");
  const int path = gru_path(din, h);
  const size_t lds = path == 1 ? ((size_t)2 * kGruRows * ((size_t)din + 2) + 3 * kGruRows * ((size_t)h + 2)) * sizeof(float)
                   : path == 2 ? ((size_t)din + 4 * (size_t)h) * sizeof(float) : 0;
  ARX_CHECK_ARG(lds <= kGruLdsLimit, "arx_gru_fwd: sizes exceed LDS");       // ahead of any launch
  if (L == 0 || B == 0) return ARX_OK;
  hipStream_t s = as_stream(stream);
  if (path == 0) {
    k_gru_fwd_wreg<64><<<(int)ceil_div(B, kGruRows), 256, 0, s>>>(x, Wg, bg, Wc, bc, L, B, hs, gates, rh);
  } else if (path == 1) {
    auto kern = h == 64 ? k_gru_fwd<1> : k_gru_fwd<2>;
    if (const int rc = gru_raise_lds(reinterpret_cast<const void*>(kern), lds)) return rc;
    kern<<<(int)ceil_div(B, kGruRows), 256, lds, s>>>(x, Wg, bg, Wc, bc, L, B, din, h, hs, gates, rh);
  } else {
    if (const int rc = gru_raise_lds(reinterpret_cast<const void*>(k_gru_fwd_generic), lds)) return rc;
    k_gru_fwd_generic<<<(int)B, 256, lds, s>>>(x, Wg, bg, Wc, bc, L, B, din, h, hs, gates, rh);
  }
  ARX_CHECK_LAUNCH();
  return ARX_OK;
}

int arx_gru_bwd(const float* Wg, const float* Wc, const float* hs, const float* gates, const float* dhs, int64_t L,
                int64_t B, int din, int h, float* dzg, float* dzc, void* stream) {
  ARX_CHECK_ARG(Wg && Wc && hs && gates && dhs && dzg && dzc, "arx_gru_bwd: null pointer");
  ARX_CHECK_ARG(L >= 0 && B >= 0 && din > 0 && h > 0, "arx_gru_bwd: bad size");
  const int path = gru_path(din, h);
  const size_t lds = path == 1 ? (size_t)kGruRows * (3 * (size_t)h + 4) * sizeof(float)
                   : path == 2 ? 5 * (size_t)h * sizeof(float) : 0;
  ARX_CHECK_ARG(lds <= kGruLdsLimit, "arx_gru_bwd: sizes exceed LDS");       // ahead of any launch
  if (L == 0 || B == 0) return ARX_OK;
  hipStream_t s = as_stream(stream);
  if (path == 0) {
    k_gru_bwd_wreg<64><<<(int)ceil_div(B, kGruRows), 256, 0, s>>>(Wg, Wc, hs, gates, dhs, L, B, dzg, dzc);
  } else if (path == 1) {
    const int grid = (int)ceil_div(B, kGruRows);
    if (h == 64) k_gru_bwd<1><<<grid, 256, lds, s>>>(Wg, Wc, hs, gates, dhs, L, B, din, h, dzg, dzc);
    else k_gru_bwd<2><<<grid, 256, lds, s>>>(Wg, Wc, hs, gates, dhs, L, B, din, h, dzg, dzc);
  } else {
    if (const int rc = gru_raise_lds(reinterpret_cast<const void*>(k_gru_bwd_generic), lds)) return rc;
    k_gru_bwd_generic<<<(int)B, 256, lds, s>>>(Wg, Wc, hs, gates, dhs, L, B, din, h, dzg, dzc);
  }
  ARX_CHECK_LAUNCH();
  return ARX_OK;
}

}  // extern "C"

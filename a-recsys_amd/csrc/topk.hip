// topk.hip -- tf.nn.top_k(logits, k, sorted=True) for the recommend / eval path
// (hmf_model.py:154, seqModel.py:514-517) over rows of up to ~10^8 columns, and the merge step
// of the streaming full-vocabulary scorer.
//
// k_topk in misc.hip makes k passes over the row (k = 100, V = 1 M: 10^8 reads per row).
// Here one workgroup per row does a 3-level radix SELECT on the order-preserving integer image
// of the floats (11 + 11 + 10 bits, histogram in LDS) to find the k-th largest value T, then
// one collecting pass: everything > T, plus as many == T as still needed, lowest column first
// (tf.nn.top_k's tie rule); the <= 1024 winners are rank-sorted in LDS.  Four passes over the
// row in total, whatever k is.
// Recommend without each user's seen items: arx_topk_exclude_fill masks them in a logits chunk, arx_topk_mark_empty
// turns the -inf tails of short rows into index -1.
// Recommend of the row-sharded model: arx_topk_merge_shards folds the W shards' lists into global ids in one launch;
// arx_topk_softmax_merge_shards does it for lists of logit ids and turns the winners' values into softmax values.
#include "common.h"
#include "gumbel.h"

namespace arx {

namespace {

constexpr int kSelThreads = 256;
constexpr int kSelBins = 2048;
constexpr int kMaxK = 1024;

// larger float <-> larger unsigned (NaNs sort above +inf; -0 < +0)
__device__ __forceinline__ uint32_t ord_key(float x) {
  const uint32_t b = __float_as_uint(x);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float ord_val(uint32_t k) {
  const uint32_t b = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
  return __uint_as_float(b);
}

// From a histogram over `bins` digit values (larger digit = larger key): the digit D that holds
// the need-th largest key, and how many keys sit in digits above D.  All threads get both.
__device__ __forceinline__ void pick_digit(const int* hist, int bins, int need, int* s_scan,
                                           int& digit, int& above) {
  // suffix counts per thread chunk (8 digits per thread at 2048 bins)
  const int per = bins / kSelThreads;
  const int t = threadIdx.x;
  int mine = 0;
  for (int u = 0; u < per; ++u) mine += hist[t * per + u];
  s_scan[t] = mine;
  __syncthreads();
  // exclusive suffix sum over threads (256 entries: serial by thread 0 is 256 adds -- fine)
  if (t == 0) {
    int run = 0;
    for (int i = kSelThreads - 1; i >= 0; --i) {
      const int v = s_scan[i];
      s_scan[i] = run;          // keys in chunks above chunk i
      run += v;
    }
  }
  __syncthreads();
  const int ab = s_scan[t];
  __shared__ int s_digit, s_above;
  if (ab < need && ab + mine >= need) {   // exactly one thread: the need-th largest is in my chunk
    int run = ab;
    for (int u = per - 1; u >= 0; --u) {
      const int c = hist[t * per + u];
      if (run + c >= need) {
        s_digit = t * per + u;
        s_above = run;
        break;
      }
      run += c;
    }
  }
  __syncthreads();
  digit = s_digit;
  above = s_above;
  __syncthreads();
}

__global__ __launch_bounds__(kSelThreads) void k_topk_select(const float* __restrict__ logits,
                                                             int64_t ld, int64_t V, int k,
                                                             int32_t idx_base,
                                                             float* __restrict__ values,
                                                             int32_t* __restrict__ indices) {
  __shared__ int hist[kSelBins];
  __shared__ int s_scan[kSelThreads];
  __shared__ uint32_t c_key[kMaxK];
  __shared__ int32_t c_idx[kMaxK];
  __shared__ int s_cnt, s_tie;
  const int64_t r = blockIdx.x;
  const float* x = logits + r * ld;
  const int t = threadIdx.x;
  // ---- level 1: top 11 bits ----
  for (int b = t; b < kSelBins; b += kSelThreads) hist[b] = 0;
  __syncthreads();
  for (int64_t c = t; c < V; c += kSelThreads) atomicAdd(&hist[ord_key(x[c]) >> 21], 1);
  __syncthreads();
  int d1, above1;
  pick_digit(hist, kSelBins, k, s_scan, d1, above1);
  // ---- level 2: next 11 bits among keys whose top digit is d1 ----
  for (int b = t; b < kSelBins; b += kSelThreads) hist[b] = 0;
  __syncthreads();
  for (int64_t c = t; c < V; c += kSelThreads) {
    const uint32_t key = ord_key(x[c]);
    if ((int)(key >> 21) == d1) atomicAdd(&hist[(key >> 10) & 2047u], 1);
  }
  __syncthreads();
  int d2, above2;
  pick_digit(hist, kSelBins, k - above1, s_scan, d2, above2);
  // ---- level 3: low 10 bits among keys with prefix (d1, d2) ----
  for (int b = t; b < kSelBins; b += kSelThreads) hist[b] = 0;
  __syncthreads();
  const uint32_t pre = ((uint32_t)d1 << 11) | (uint32_t)d2;
  for (int64_t c = t; c < V; c += kSelThreads) {
    const uint32_t key = ord_key(x[c]);
    if ((key >> 10) == pre) atomicAdd(&hist[key & 1023u], 1);
  }
  __syncthreads();
  int d3, above3;
  pick_digit(hist, 1024, k - above1 - above2, s_scan, d3, above3);
  const uint32_t T = (pre << 10) | (uint32_t)d3;               // the k-th largest key
  const int n_gt = above1 + above2 + above3;                    // keys strictly above T
  const int need_tie = k - n_gt;                                // keys == T to take, lowest column first
  // ---- collect ----
  if (t == 0) {
    s_cnt = 0;
    s_tie = 0;
  }
  __syncthreads();
  for (int64_t c = t; c < V; c += kSelThreads) {
    const uint32_t key = ord_key(x[c]);
    if (key > T) {
      const int p = atomicAdd(&s_cnt, 1);
      c_key[p] = key;
      c_idx[p] = (int32_t)c;
    }
  }
  __syncthreads();
  // ties in column order: ordered compaction, 256 columns per round, until need_tie are taken
  for (int64_t c0 = 0; c0 < V; c0 += kSelThreads) {
    if (s_tie >= need_tie) break;                               // uniform: read after a barrier below
    const int64_t c = c0 + t;
    const bool is = (c < V) && (ord_key(x[c]) == T);
    const unsigned long long bal = __ballot(is);
    const int lane = t & 63, wv = t >> 6;
    s_scan[wv] = __popcll(bal);
    __syncthreads();
    int before = 0;
    for (int w = 0; w < wv; ++w) before += s_scan[w];
    const int tot = s_scan[0] + s_scan[1] + s_scan[2] + s_scan[3];
    const int pos = s_tie + before + __popcll(bal & ((lane == 0) ? 0ull : (~0ull >> (64 - lane))));
    if (is && pos < need_tie) {
      c_key[n_gt + pos] = T;
      c_idx[n_gt + pos] = (int32_t)c;
    }
    __syncthreads();
    if (t == 0) s_tie += tot;
    __syncthreads();
  }
  __syncthreads();
  // ---- rank sort the k winners: descending key, ascending column ----
  for (int i = t; i < k; i += kSelThreads) {
    const uint32_t ki = c_key[i];
    const int32_t ci = c_idx[i];
    int rank = 0;
    for (int j = 0; j < k; ++j) {
      const uint32_t kj = c_key[j];
      rank += (kj > ki) || (kj == ki && c_idx[j] < ci);
    }
    if (values) values[r * k + rank] = ord_val(ki);
    indices[r * k + rank] = ci + idx_base;
  }
}

// merge two per-row top-k lists (each sorted: descending value, ascending index) into one;
// on equal values list A wins (A holds the lower column indices: earlier vocabulary chunks)
__global__ void k_topk_merge(const float* __restrict__ va, const int32_t* __restrict__ ia,
                             const float* __restrict__ vb, const int32_t* __restrict__ ib, int64_t B,
                             int ka, int kb, int k, float* __restrict__ vo, int32_t* __restrict__ io) {
  const int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (r >= B) return;
  int a = 0, b = 0;
  for (int j = 0; j < k; ++j) {
    const bool has_a = a < ka, has_b = b < kb;
    bool take_a;
    if (has_a && has_b) {
      const float xa = va[r * ka + a], xb = vb[r * kb + b];
      take_a = (xa > xb) || (xa == xb && ia[r * ka + a] <= ib[r * kb + b]);
    } else {
      take_a = has_a;
    }
    if (take_a) {
      vo[r * k + j] = va[r * ka + a];
      io[r * k + j] = ia[r * ka + a];
      ++a;
    } else {
      vo[r * k + j] = vb[r * kb + b];
      io[r * k + j] = ib[r * kb + b];
      ++b;
    }
  }
}

// out[r][j] = table[r][pos[r][j]]: positions inside a row's candidate list -> the candidates' column indices
__global__ void k_take_rows_i32(const int32_t* __restrict__ table, int64_t ld, const int32_t* __restrict__ pos,
                                int64_t ldp, int64_t B, int k, int32_t* __restrict__ out, int64_t ldo) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= B * k) return;
  const int64_t r = i / k;
  const int j = (int)(i % k);
  out[r * ldo + j] = table[r * ld + pos[r * ldp + j]];
}

// Exclusion lists (recommend with each user's seen items left out): row r's list is ex_cols[ex_ptr[key] ..
// ex_ptr[key + 1]), sorted ascending, key = row_keys[r % key_rows] (< 0: none).  One wave per row writes -inf at the
// listed columns in [col0, col0 + ncols) of its logits row (column c lands at logits[r * ld + c - col0]): a lower_bound
// finds the first one, the wave then strides through the list until it leaves the range.
constexpr int kExRowsPerBlock = 4;

__global__ __launch_bounds__(64 * kExRowsPerBlock) void k_topk_exclude_fill(
    float* __restrict__ logits, int64_t ld, int64_t B, int32_t col0, int64_t ncols, const int32_t* __restrict__ row_keys,
    int64_t key_rows, const int32_t* __restrict__ ex_ptr, const int32_t* __restrict__ ex_cols) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * kExRowsPerBlock + (threadIdx.x >> 6);
  if (r >= B) return;
  const int32_t key = row_keys[r % key_rows];
  if (key < 0) return;
  const int beg = ex_ptr[key], end = ex_ptr[key + 1];
  int lo = beg, hi = end;                        // first entry >= col0 (the same search in every lane)
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (ex_cols[mid] < col0) lo = mid + 1;
    else hi = mid;
  }
  const int64_t c1 = (int64_t)col0 + ncols;
  float* row = logits + r * ld;
  for (int i = lo + lane; i < end; i += 64) {
    const int64_t c = ex_cols[i];
    if (c >= c1) break;                          // sorted: the rest lies past the range
    if (c >= col0) row[c - col0] = -__builtin_inff();
  }
}

// Item tags (recommend within "only this category / in stock / this market"): absolute column c carries 32 tag bits
// col_tags[c], row r the two words want_any / want_all [r % want_rows]; c is eligible for r iff
// (any == 0 || (tags & any) != 0) && (tags & all) == all.  One workgroup per row strides over [col0, col0 + ncols) and
// writes -inf at the ineligible columns (the logits themselves are never read); a row of two zero words returns.
__global__ __launch_bounds__(256) void k_topk_tags_fill(float* __restrict__ logits, int64_t ld, int32_t col0,
                                                        int64_t ncols, const int32_t* __restrict__ col_tags,
                                                        const int32_t* __restrict__ want_any,
                                                        const int32_t* __restrict__ want_all, int64_t want_rows) {
  const int64_t r = blockIdx.x;
  const uint32_t wa = (uint32_t)want_any[r % want_rows], wl = (uint32_t)want_all[r % want_rows];
  if ((wa | wl) == 0u) return;
  float* row = logits + r * ld;
  const int32_t* tg = col_tags + col0;
  for (int64_t c = threadIdx.x; c < ncols; c += 256) {
    const uint32_t t = (uint32_t)tg[c];
    if ((wa != 0u && (t & wa) == 0u) || (t & wl) != wl) row[c] = -__builtin_inff();
  }
}

// The sampled recommend (arx_sample.h, arx_sample_shard.h): key = fmaf(tau, g(noise row, noise column), logit) in place,
// g the Gumbel noise of gumbel.h.  The noise row of batch row r is noise_rows[r % tau_rows] (nullptr: r % tau_rows), the
// noise column of absolute column c is c * col_mul + col_add (unsigned, wrapping) -- (1, 0, nullptr) is the plain
// convention of arx_sample.h, (W, s, user ids) the row-sharded one.  One workgroup per row strides over
// [col0, col0 + ncols); a row of tau == 0 or of a negative noise row returns (its keys ARE its logits); a -inf logit
// stays -inf (g is finite).
__global__ __launch_bounds__(256) void k_topk_gumbel_add(float* __restrict__ logits, int64_t ld, int32_t col0,
                                                         int64_t ncols, const float* __restrict__ tau, int64_t tau_rows,
                                                         const int32_t* __restrict__ seed_words, uint32_t col_mul,
                                                         uint32_t col_add, const int32_t* __restrict__ noise_rows) {
  const int64_t r = blockIdx.x, tr = r % tau_rows;
  const int64_t nr = noise_rows ? (int64_t)noise_rows[tr] : tr;
  const float t = tau[tr];
  if (t == 0.f || nr < 0) return;
  const GumbelRow gr = gumbel_row(seed_words, nr);
  float* row = logits + r * ld;
  for (int64_t c = threadIdx.x; c < ncols; c += 256) {
    const uint32_t nc = ((uint32_t)col0 + (uint32_t)c) * col_mul + col_add;
    row[c] = fmaf(t, gumbel_of_bits(gumbel_bits(gr.b0, gr.b1, nc)), row[c]);
  }
}

// the winners' keys back into the model's scores: value = fmaf(-tau, g(noise row, index * col_mul + col_add), key);
// index -1: -inf; a negative noise row is a tau == 0 row
__global__ void k_topk_gumbel_strip(float* __restrict__ values, int64_t ldv, const int32_t* __restrict__ indices,
                                    int64_t ldi, int64_t B, int k, const float* __restrict__ tau, int64_t tau_rows,
                                    const int32_t* __restrict__ seed_words, uint32_t col_mul, uint32_t col_add,
                                    const int32_t* __restrict__ noise_rows) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= B * k) return;
  const int64_t r = i / k, tr = r % tau_rows;
  const int j = (int)(i % k);
  const int32_t c = indices[r * ldi + j];
  float* v = values + r * ldv + j;
  if (c < 0) {
    *v = -__builtin_inff();
    return;
  }
  const int64_t nr = noise_rows ? (int64_t)noise_rows[tr] : tr;
  const float t = tau[tr];
  if (t == 0.f || nr < 0) return;
  const GumbelRow gr = gumbel_row(seed_words, nr);
  *v = fmaf(-t, gumbel_of_bits(gumbel_bits(gr.b0, gr.b1, (uint32_t)c * col_mul + col_add)), *v);
}

// the picks of the merged lists as columns of ONE shard (arx_sample_shard.h): global id -> id / W where id % W == s,
// -1 for a pick of another shard and for an id -1
__global__ void k_picks_to_shard(const int32_t* __restrict__ ids, int64_t ldi, int64_t B, int k, int W, int s,
                                 int32_t* __restrict__ cols, int64_t ldc) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < B * k; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i / k;
    const int j = (int)(i % k);
    const int32_t id = ids[r * ldi + j];
    cols[r * ldc + j] = (id >= 0 && id % W == s) ? id / W : -1;
  }
}

// a winner whose value is -inf is no item (a row with fewer eligible columns than k): index -1
__global__ void k_topk_mark_empty(const float* __restrict__ values, int64_t ldv, int32_t* __restrict__ indices,
                                  int64_t ldi, int64_t B, int k) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= B * k) return;
  const int64_t r = i / k;
  const int j = (int)(i % k);
  if (values[r * ldv + j] == -__builtin_inff()) indices[r * ldi + j] = -1;
}

// W-way merge of per-shard top-k lists (row-sharded recommend, owner = id % W): v / c [W][B][k], list (s, r) sorted
// by (value desc, local column asc), c < 0 = empty.  One wave per row; lane s < W holds the head of list s as one
// 64-bit key (order-preserving value image << 32 | ~global id: the larger key is the better entry, so the lower id
// wins a tie -- tf.nn.top_k's rule), 0 when the list is used up.  Round j: a 64-lane max, the winning lane steps to
// its next non-empty entry; lane j % 64 keeps round j's winner and the wave stores 64 results at a time.
constexpr int kMergeRowsPerBlock = 4;

__device__ __forceinline__ uint64_t shard_head(const float* __restrict__ v, const int32_t* __restrict__ c,
                                               int64_t base, int& pos, int k, int W, int s) {
  for (; pos < k; ++pos) {
    const int32_t col = c[base + pos];
    if (col < 0) continue;                                   // an empty entry is no candidate
    const uint32_t gid = (uint32_t)((int64_t)col * W + s);
    return ((uint64_t)ord_key(v[base + pos]) << 32) | (uint64_t)(0xffffffffu - gid);
  }
  return 0;
}

__global__ __launch_bounds__(64 * kMergeRowsPerBlock) void k_topk_merge_shards(
    const float* __restrict__ v, const int32_t* __restrict__ c, int64_t B, int W, int k, float* __restrict__ vo,
    int32_t* __restrict__ io) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * kMergeRowsPerBlock + (threadIdx.x >> 6);
  if (r >= B) return;                                        // (whole waves: B is per wave)
  const int64_t base = ((int64_t)lane * B + r) * k;          // list of shard `lane` for row r
  int pos = 0;
  uint64_t head = lane < W ? shard_head(v, c, base, pos, k, W, lane) : 0;
  float keep_v = -__builtin_inff();
  int32_t keep_i = -1;
  for (int j = 0; j < k; ++j) {
    uint64_t best = head;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      const uint32_t lo = __shfl_xor((uint32_t)best, m, 64), hi = __shfl_xor((uint32_t)(best >> 32), m, 64);
      const uint64_t o = ((uint64_t)hi << 32) | lo;
      best = o > best ? o : best;
    }
    if (best != 0 && head == best) {                         // the one winning lane (global ids are distinct)
      ++pos;
      head = shard_head(v, c, base, pos, k, W, lane);
    }
    if (lane == (j & 63)) {
      const float bv = ord_val((uint32_t)(best >> 32));
      const bool none = best == 0 || bv == -__builtin_inff();
      keep_v = none ? -__builtin_inff() : bv;
      keep_i = none ? -1 : (int32_t)(0xffffffffu - (uint32_t)best);
    }
    if ((j & 63) == 63 || j == k - 1) {
      const int64_t o = r * k + (j & ~63) + lane;
      if (lane <= (j & 63)) {
        vo[o] = keep_v;
        io[o] = keep_i;
      }
    }
  }
}

// The softmax twin of k_topk_merge_shards (recommend of the row-striped SeqModel): the lists carry GLOBAL logit ids
// (the owner mapped its columns before sending), lse_part [W][B] is each shard's log-sum-exp of the row over ALL of
// its vocabulary columns.  The lanes s < W that hold the list heads also hold the parts: a wave max, a wave sum of
// exp(part - max) -> the row's lse (-inf when every part is -inf: no NaN out of -inf - -inf); the merge then stores
// exp(value - lse) for each winner, 0 next to an index -1.
__device__ __forceinline__ uint64_t shard_head_gid(const float* __restrict__ v, const int32_t* __restrict__ id,
                                                   int64_t base, int& pos, int k) {
  for (; pos < k; ++pos) {
    const int32_t g = id[base + pos];
    if (g < 0) continue;                                     // an empty entry is no candidate
    return ((uint64_t)ord_key(v[base + pos]) << 32) | (uint64_t)(0xffffffffu - (uint32_t)g);
  }
  return 0;
}

__global__ __launch_bounds__(64 * kMergeRowsPerBlock) void k_topk_softmax_merge_shards(
    const float* __restrict__ v, const int32_t* __restrict__ id, const float* __restrict__ lse_part, int64_t B, int W,
    int k, float* __restrict__ po, int32_t* __restrict__ io, float* __restrict__ lse_out) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * kMergeRowsPerBlock + (threadIdx.x >> 6);
  if (r >= B) return;                                        // (whole waves: B is per wave)
  const float ninf = -__builtin_inff();
  const float part = lane < W ? lse_part[(int64_t)lane * B + r] : ninf;
  float mx = part;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) mx = fmaxf(mx, __shfl_xor(mx, m, 64));
  float sum = part == ninf ? 0.f : expf(part - mx);          // (mx = -inf only when every part is)
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) sum += __shfl_xor(sum, m, 64);
  const float lse = mx == ninf ? ninf : mx + logf(sum);
  if (lse_out && lane == 0) lse_out[r] = lse;
  const int64_t base = ((int64_t)lane * B + r) * k;          // list of shard `lane` for row r
  int pos = 0;
  uint64_t head = lane < W ? shard_head_gid(v, id, base, pos, k) : 0;
  float keep_p = 0.f;
  int32_t keep_i = -1;
  for (int j = 0; j < k; ++j) {
    uint64_t best = head;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      const uint32_t lo = __shfl_xor((uint32_t)best, m, 64), hi = __shfl_xor((uint32_t)(best >> 32), m, 64);
      const uint64_t o = ((uint64_t)hi << 32) | lo;
      best = o > best ? o : best;
    }
    if (best != 0 && head == best) {                         // the one winning lane (logit ids are distinct)
      ++pos;
      head = shard_head_gid(v, id, base, pos, k);
    }
    if (lane == (j & 63)) {
      const float bv = ord_val((uint32_t)(best >> 32));
      const bool none = best == 0 || bv == ninf;
      keep_p = none ? 0.f : expf(bv - lse);
      keep_i = none ? -1 : (int32_t)(0xffffffffu - (uint32_t)best);
    }
    if ((j & 63) == 63 || j == k - 1) {
      const int64_t o = r * k + (j & ~63) + lane;
      if (lane <= (j & 63)) {
        po[o] = keep_p;
        io[o] = keep_i;
      }
    }
  }
}

}  // namespace

int topk_select_launch(const float* logits, int64_t ld, int64_t B, int64_t V, int k, int32_t idx_base,
                       float* values, int32_t* indices, hipStream_t s) {
  k_topk_select<<<(int)B, kSelThreads, 0, s>>>(logits, ld, V, k, idx_base, values, indices);
  ARX_CHECK_LAUNCH();
  return ARX_OK;
}

}  // namespace arx

using namespace arx;

extern "C" {

int arx_topk_chunk(const float* logits, int64_t ld, int64_t B, int64_t V, int k, int32_t idx_base,
                   float* values, int32_t* indices, void* stream) {
  ARX_CHECK_ARG(logits && values && indices, "arx_topk_chunk: null pointer");
  ARX_CHECK_ARG(k > 0 && k <= V && k <= kMaxK, "arx_topk_chunk: need 0 < k <= min(V, 1024)");
  if (B <= 0) return ARX_OK;
  return topk_select_launch(logits, ld, B, V, k, idx_base, values, indices, as_stream(stream));
}

int arx_topk_merge(const float* va, const int32_t* ia, const float* vb, const int32_t* ib, int64_t B,
                   int ka, int kb, int k, float* vo, int32_t* io, void* stream) {
  ARX_CHECK_ARG(va && ia && vb && ib && vo && io, "arx_topk_merge: null pointer");
  ARX_CHECK_ARG(ka >= 0 && kb >= 0 && k > 0 && k <= ka + kb, "arx_topk_merge: need 0 < k <= ka + kb");
  if (B <= 0) return ARX_OK;
  k_topk_merge<<<(int)ceil_div(B, 64), 64, 0, as_stream(stream)>>>(va, ia, vb, ib, B, ka, kb, k, vo, io);
  ARX_CHECK_LAUNCH();
  return ARX_OK;
}

int arx_take_rows_i32(const int32_t* table, int64_t ld, const int32_t* pos, int64_t ldp, int64_t B, int k,
                      int32_t* out, int64_t ldo, void* stream) {
  ARX_CHECK_ARG(table && pos && out && k > 0, "arx_take_rows_i32: bad argument");
  if (B <= 0) return ARX_OK;
  k_take_rows_i32<<<(int)ceil_div(B * k, 256), 256, 0, as_stream(stream)>>>(table, ld, pos, ldp, B, k, out, ldo);
  ARX_CHECK_LAUNCH();
  return ARX_OK;
}

int arx_topk_exclude_fill(float* logits, int64_t ld, int64_t B, int32_t col0, int64_t ncols, const int32_t* row_keys,
                          int64_t key_rows, const int32_t* ex_ptr, const int32_t* ex_cols, void* stream) {
  ARX_CHECK_ARG(logits && row_keys && ex_ptr && ex_cols, "arx_topk_exclude_fill: null pointer");
  ARX_CHECK_ARG(B >= 0 && ncols >= 0 && col0 >= 0 && key_rows > 0,
                "arx_topk_exclude_fill: need B >= 0, ncols >= 0, col0 >= 0, key_rows > 0");
  ARX_CHECK_ARG(B <= 1 || ld >= ncols, "arx_topk_exclude_fill: ld < ncols");
  ARX_CHECK_ARG(ceil_div(B, (int64_t)kExRowsPerBlock) <= 0x7fffffff, "arx_topk_exclude_fill: too many rows");
  if (B == 0 || ncols == 0) return ARX_OK;
  k_topk_exclude_fill<<<(int)ceil_div(B, (int64_t)kExRowsPerBlock), 64 * kExRowsPerBlock, 0, as_stream(stream)>>>(
      logits, ld, B, col0, ncols, row_keys, key_rows, ex_ptr, ex_cols);
  ARX_CHECK_LAUNCH();
  return ARX_OK;
}

int arx_topk_tags_fill(float* logits, int64_t ld, int64_t M, int32_t col0, int64_t ncols, const int32_t* col_tags,
                       const int32_t* want_any, const int32_t* want_all, int64_t want_rows, void* stream) {
  ARX_CHECK_ARG(logits && col_tags && want_any && want_all, "arx_topk_tags_fill: null pointer");
  ARX_CHECK_ARG(M >= 0 && ncols >= 0 && col0 >= 0 && want_rows > 0,
                "arx_topk_tags_fill: need M >= 0, ncols >= 0, col0 >= 0, want_rows > 0");
  ARX_CHECK_ARG((int64_t)col0 + ncols <= 0x7fffffff, "arx_topk_tags_fill: need col0 + ncols < 2^31");
  ARX_CHECK_ARG(M <= 1 || ld >= ncols, "arx_topk_tags_fill: ld < ncols");
  ARX_CHECK_ARG(M <= 0x7fffffff, "arx_topk_tags_fill: too many rows");
  if (M == 0 || ncols == 0) return ARX_OK;
  k_topk_tags_fill<<<(int)M, 256, 0, as_stream(stream)>>>(logits, ld, col0, ncols, col_tags, want_any, want_all,
                                                          want_rows);
  ARX_CHECK_LAUNCH();
  return ARX_OK;
}

// the column map of arx_sample_shard.h: the largest noise column of the columns [col0, col0 + ncols) stays below 2^31
static bool noise_cols_ok(int64_t col0, int64_t ncols, int32_t col_mul, int32_t col_add) {
  if (col_mul < 1 || col_add < 0 || col_add >= col_mul) return false;
  if (ncols <= 0) return true;
  return (col0 + ncols - 1) <= (0x7fffffffll - col_add) / col_mul;
}

static int gumbel_add(const char* fn, float* logits, int64_t ld, int64_t M, int32_t col0, int64_t ncols,
                      const float* tau, int64_t tau_rows, const int32_t* seed_words, int32_t col_mul, int32_t col_add,
                      const int32_t* noise_rows, void* stream) {
  ARX_CHECK_ARG(logits && tau && seed_words, "%s: null pointer", fn);
  ARX_CHECK_ARG(M >= 0 && ncols >= 0 && col0 >= 0 && tau_rows > 0,
                "%s: need M >= 0, ncols >= 0, col0 >= 0, tau_rows > 0", fn);
  ARX_CHECK_ARG((int64_t)col0 + ncols <= 0x7fffffff, "%s: need col0 + ncols < 2^31", fn);
  ARX_CHECK_ARG(noise_cols_ok(col0, ncols, col_mul, col_add),
                "%s: need col_mul >= 1, 0 <= col_add < col_mul and every noise column (col0 + c) * col_mul + col_add "
                "< 2^31", fn);
  ARX_CHECK_ARG(M <= 1 || ld >= ncols, "%s: ld < ncols", fn);
  ARX_CHECK_ARG(M <= 0x7fffffff, "%s: too many rows", fn);
  if (M == 0 || ncols == 0) return ARX_OK;
  k_topk_gumbel_add<<<(int)M, 256, 0, as_stream(stream)>>>(logits, ld, col0, ncols, tau, tau_rows, seed_words,
                                                           (uint32_t)col_mul, (uint32_t)col_add, noise_rows);
  ARX_CHECK_LAUNCH();
  return ARX_OK;
}

static int gumbel_strip(const char* fn, float* values, int64_t ldv, const int32_t* indices, int64_t ldi, int64_t B,
                        int k, const float* tau, int64_t tau_rows, const int32_t* seed_words, int32_t col_mul,
                        int32_t col_add, const int32_t* noise_rows, void* stream) {
  ARX_CHECK_ARG(values && indices && tau && seed_words, "%s: null pointer", fn);
  ARX_CHECK_ARG(B >= 0 && k > 0 && tau_rows > 0 && (B <= 1 || (ldv >= k && ldi >= k)),
                "%s: need B >= 0, k > 0, tau_rows > 0, ldv >= k, ldi >= k", fn);
  ARX_CHECK_ARG(col_mul >= 1 && col_add >= 0 && col_add < col_mul, "%s: need col_mul >= 1, 0 <= col_add < col_mul", fn);
  ARX_CHECK_ARG(ceil_div(B * k, (int64_t)256) <= 0x7fffffff, "%s: too many entries", fn);
  if (B == 0) return ARX_OK;
  k_topk_gumbel_strip<<<(int)ceil_div(B * k, (int64_t)256), 256, 0, as_stream(stream)>>>(
      values, ldv, indices, ldi, B, k, tau, tau_rows, seed_words, (uint32_t)col_mul, (uint32_t)col_add, noise_rows);
  ARX_CHECK_LAUNCH();
  return ARX_OK;
}

int arx_topk_gumbel_add(float* logits, int64_t ld, int64_t M, int32_t col0, int64_t ncols, const float* tau,
                        int64_t tau_rows, const int32_t* seed_words, void* stream) {
  return gumbel_add("arx_topk_gumbel_add", logits, ld, M, col0, ncols, tau, tau_rows, seed_words, 1, 0, nullptr, stream);
}

int arx_topk_gumbel_add_keyed(float* logits, int64_t ld, int64_t M, int32_t col0, int64_t ncols, const float* tau,
                              int64_t tau_rows, const int32_t* seed_words, int32_t col_mul, int32_t col_add,
                              const int32_t* noise_rows, void* stream) {
  return gumbel_add("arx_topk_gumbel_add_keyed", logits, ld, M, col0, ncols, tau, tau_rows, seed_words, col_mul,
                    col_add, noise_rows, stream);
}

int arx_topk_gumbel_strip(float* values, int64_t ldv, const int32_t* indices, int64_t ldi, int64_t B, int k,
                          const float* tau, int64_t tau_rows, const int32_t* seed_words, void* stream) {
  return gumbel_strip("arx_topk_gumbel_strip", values, ldv, indices, ldi, B, k, tau, tau_rows, seed_words, 1, 0,
                      nullptr, stream);
}

int arx_topk_gumbel_strip_keyed(float* values, int64_t ldv, const int32_t* indices, int64_t ldi, int64_t B, int k,
                                const float* tau, int64_t tau_rows, const int32_t* seed_words, int32_t col_mul,
                                int32_t col_add, const int32_t* noise_rows, void* stream) {
  return gumbel_strip("arx_topk_gumbel_strip_keyed", values, ldv, indices, ldi, B, k, tau, tau_rows, seed_words,
                      col_mul, col_add, noise_rows, stream);
}

int arx_picks_to_shard(const int32_t* ids, int64_t ldi, int64_t B, int k, int W, int s, int32_t* cols, int64_t ldc,
                       void* stream) {
  ARX_CHECK_ARG(ids && cols, "arx_picks_to_shard: null pointer");
  ARX_CHECK_ARG(B >= 0 && k >= 1 && ldi >= k && ldc >= k, "arx_picks_to_shard: need B >= 0, k >= 1, ldi >= k, ldc >= k");
  ARX_CHECK_ARG(W >= 1 && s >= 0 && s < W, "arx_picks_to_shard: need W >= 1 and 0 <= s < W");
  if (B == 0) return ARX_OK;
  const int64_t blocks = ceil_div(B * k, (int64_t)256);
  k_picks_to_shard<<<(int)(blocks < 65536 ? blocks : 65536), 256, 0, as_stream(stream)>>>(ids, ldi, B, k, W, s, cols,
                                                                                            ldc);
  ARX_CHECK_LAUNCH();
  return ARX_OK;
}

int arx_topk_mark_empty(const float* values, int64_t ldv, int32_t* indices, int64_t ldi, int64_t B, int k,
                        void* stream) {
  ARX_CHECK_ARG(values && indices, "arx_topk_mark_empty: null pointer");
  ARX_CHECK_ARG(B >= 0 && k > 0 && (B <= 1 || (ldv >= k && ldi >= k)),
                "arx_topk_mark_empty: need B >= 0, k > 0, ldv >= k, ldi >= k");
  if (B == 0) return ARX_OK;
  k_topk_mark_empty<<<(int)ceil_div(B * k, (int64_t)256), 256, 0, as_stream(stream)>>>(values, ldv, indices, ldi, B, k);
  ARX_CHECK_LAUNCH();
  return ARX_OK;
}

int arx_topk_merge_shards(const float* v, const int32_t* c, int64_t B, int W, int k, float* vo, int32_t* io,
                          void* stream) {
  ARX_CHECK_ARG(v && c && vo && io, "arx_topk_merge_shards: null pointer");
  ARX_CHECK_ARG(W >= 1 && W <= 64, "arx_topk_merge_shards: need 1 <= W <= 64");
  ARX_CHECK_ARG(k > 0 && k <= kMaxK, "arx_topk_merge_shards: need 0 < k <= 1024");
  ARX_CHECK_ARG(B >= 0 && ceil_div(B, (int64_t)kMergeRowsPerBlock) <= 0x7fffffff,
                "arx_topk_merge_shards: need 0 <= B, B / 4 < 2^31");
  if (B == 0) return ARX_OK;
  k_topk_merge_shards<<<(int)ceil_div(B, (int64_t)kMergeRowsPerBlock), 64 * kMergeRowsPerBlock, 0, as_stream(stream)>>>(
      v, c, B, W, k, vo, io);
  ARX_CHECK_LAUNCH();
  return ARX_OK;
}

int arx_topk_softmax_merge_shards(const float* v, const int32_t* id, const float* lse_part, int64_t B, int W, int k,
                                  float* po, int32_t* io, float* lse_out, void* stream) {
  ARX_CHECK_ARG(v && id && lse_part && po && io, "arx_topk_softmax_merge_shards: null pointer");
  ARX_CHECK_ARG(W >= 1 && W <= 64, "arx_topk_softmax_merge_shards: need 1 <= W <= 64");
  ARX_CHECK_ARG(k > 0 && k <= kMaxK, "arx_topk_softmax_merge_shards: need 0 < k <= 1024");
  ARX_CHECK_ARG(B >= 0 && ceil_div(B, (int64_t)kMergeRowsPerBlock) <= 0x7fffffff,
                "arx_topk_softmax_merge_shards: need 0 <= B, B / 4 < 2^31");
  if (B == 0) return ARX_OK;
  k_topk_softmax_merge_shards<<<(int)ceil_div(B, (int64_t)kMergeRowsPerBlock), 64 * kMergeRowsPerBlock, 0,
                                as_stream(stream)>>>(v, id, lse_part, B, W, k, po, io, lse_out);
  ARX_CHECK_LAUNCH();
  return ARX_OK;
}

}  // extern "C"

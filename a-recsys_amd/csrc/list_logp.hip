// list_logp.hip -- list_logprob (arx_list_logp.h): the two kernels around the unchanged mass pass and finish of
// arx_sample_logp.h that let them take a list the policy did not draw itself.
//   k_list_prepare  one wave per row: every entry gets its reason code (range, exclusion list by binary search, tag
//                   test), the survivors are held in LDS as unsigned columns (0xffffffff: no pick), a first O(k^2 / 64)
//                   sweep finds the repeats (an earlier slot with the same column), a second one is the rank sort of
//                   k_logp_sort (sample_logp.hip) over the cleaned row -- the same comparator, so (pk_cols, pk_slot) are
//                   what arx_sample_logp_sort writes for `clean`.  kShard (arx_list_logp_shard.h): the lists hold GLOBAL
//                   ids and this is shard s of W -- an in-range entry of another shard is no pick (code 0), an owned one
//                   is tested and kept as the LOCAL column v / W; off, the body is the single-device one, unchanged;
//   k_list_merge    one thread per entry of the owner's global list: the code of the entry's owner shard, and the global
//                   clean list the finish reads;
//   k_list_stamp    one thread per entry, after the finish: NOSCORE where a clean pick's score came out -inf, then
//                   logp = value = -inf at every code >= 2.
// Rows walk grid-stride loops under capped grids; every LDS word a trip reads is rewritten on that trip.
#include "common.h"

namespace arx {
namespace {

constexpr int kLlMaxK = 1024;
constexpr int kLlThreads = 256;
constexpr int kLlWaves = kLlThreads / kWave;
constexpr uint32_t kLlNone = 0xffffffffu;                      // (uint32_t)-1: what k_logp_sort sorts last

template <bool kShard>
__global__ __launch_bounds__(kLlThreads) void k_list_prepare(
    const int32_t* __restrict__ lists, int64_t ldl, int64_t B, int k, int64_t V, int W, int s,
    const int32_t* __restrict__ row_keys, int64_t key_rows, const int32_t* __restrict__ ex_ptr,
    const int32_t* __restrict__ ex_cols,
    const int32_t* __restrict__ col_tags, const int32_t* __restrict__ want_any, const int32_t* __restrict__ want_all,
    int64_t want_rows, int32_t* __restrict__ clean, int64_t ldc, int32_t* __restrict__ why, int64_t ldw,
    int32_t* __restrict__ pk_cols, int32_t* __restrict__ pk_slot, int64_t ldp) {
  __shared__ uint32_t cols[kLlWaves][kLlMaxK];
  __shared__ uint8_t code[kLlWaves][kLlMaxK];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t base = (int64_t)blockIdx.x * kLlWaves; base < B; base += (int64_t)gridDim.x * kLlWaves) {
    const int64_t r = base + wave;
    const bool on = r < B;
    __syncthreads();                                               // (the last trip's readers are done with the LDS)
    if (on) {
      int ex_lo = 0, ex_hi = 0;
      if (row_keys) {
        const int32_t key = row_keys[r % key_rows];
        if (key >= 0) {
          ex_lo = ex_ptr[key];
          ex_hi = ex_ptr[key + 1];
        }
      }
      uint32_t wa = 0u, wl = 0u;
      if (col_tags) {
        wa = (uint32_t)want_any[r % want_rows];
        wl = (uint32_t)want_all[r % want_rows];
      }
      for (int j = lane; j < k; j += 64) {
        const int32_t v = lists[r * ldl + j];
        int c = ARX_LIST_OK;
        int32_t col = v;
        bool mine = true;
        if (v == -1) c = ARX_LIST_EMPTY;
        else if (v < 0 || (int64_t)v >= V) c = ARX_LIST_RANGE;
        else if (kShard && v % W != s) mine = false;               // another shard's: no pick here, nothing to say
        else {
          col = kShard ? v / W : v;                                // the column of THIS pool
          int lo = ex_lo, hi = ex_hi;                              // the first listed column >= col
          while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (ex_cols[mid] < col) lo = mid + 1;
            else hi = mid;
          }
          if (lo < ex_hi && ex_cols[lo] == col) c = ARX_LIST_EXCLUDED;
          else if (col_tags) {
            const uint32_t t = (uint32_t)col_tags[col];
            if ((wa != 0u && (t & wa) == 0u) || (t & wl) != wl) c = ARX_LIST_TAGS;
          }
        }
        cols[wave][j] = (c == ARX_LIST_OK && mine) ? (uint32_t)col : kLlNone;
        code[wave][j] = (uint8_t)c;
      }
    }
    __syncthreads();
    // the repeats among the survivors: an earlier slot holds the same column (that slot survived too: it holds v)
    uint32_t rep = 0u;                                             // bit e: slot lane + 64 e is a repeat
    for (int e = 0; e < kLlMaxK / 64; ++e) {
      const int j = lane + e * 64;
      if (on && j < k) {
        const uint32_t c = cols[wave][j];
        if (c != kLlNone) {
          bool hit = false;
          for (int i = 0; i < j; ++i) hit = hit || cols[wave][i] == c;
          rep |= hit ? 1u << e : 0u;
        }
      }
    }
    __syncthreads();                                               // (every slot was compared before one changes)
    for (int e = 0; e < kLlMaxK / 64; ++e) {
      const int j = lane + e * 64;
      if (on && j < k) {
        if ((rep >> e) & 1u) {
          cols[wave][j] = kLlNone;
          code[wave][j] = (uint8_t)ARX_LIST_REPEAT;
        }
        clean[r * ldc + j] = (int32_t)cols[wave][j];
        why[r * ldw + j] = (int32_t)code[wave][j];
      }
    }
    __syncthreads();
    if (on)
      for (int j = lane; j < k; j += 64) {                         // the rank sort of k_logp_sort over the cleaned row
        const uint32_t c = cols[wave][j];
        int rank = 0;
        for (int i = 0; i < k; ++i) {
          const uint32_t x = cols[wave][i];
          rank += (x < c || (x == c && i < j)) ? 1 : 0;
        }
        pk_cols[r * ldp + rank] = (int32_t)c;
        pk_slot[r * ldp + rank] = j;
      }
  }
}

__global__ __launch_bounds__(256) void k_list_stamp(const int32_t* __restrict__ clean, int64_t ldc,
                                                    const float* __restrict__ pick_score, int64_t ldps, int64_t B, int k,
                                                    int32_t* __restrict__ why, int64_t ldw, float* __restrict__ logp,
                                                    int64_t ldo, float* __restrict__ values, int64_t ldv) {
  const int64_t n = B * k;
  const float ninf = -__builtin_inff();
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i / k;
    const int j = (int)(i - r * k);
    int32_t c = why[r * ldw + j];
    if (clean[r * ldc + j] >= 0 && pick_score[r * ldps + j] == ninf) {
      c = ARX_LIST_NOSCORE;
      why[r * ldw + j] = c;
    }
    if (c >= ARX_LIST_RANGE) {
      logp[r * ldo + j] = ninf;
      if (values) values[r * ldv + j] = ninf;
    }
  }
}

__global__ __launch_bounds__(256) void k_list_merge(const int32_t* __restrict__ lists, int64_t ldl, int64_t B, int k,
                                                    int64_t V, const int32_t* __restrict__ codes, int64_t ldcode,
                                                    int64_t slab, int W, int32_t* __restrict__ clean, int64_t ldc,
                                                    int32_t* __restrict__ why, int64_t ldw) {
  const int64_t n = B * k;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i / k;
    const int j = (int)(i - r * k);
    const int32_t v = lists[r * ldl + j];
    int32_t c;
    if (v == -1) c = ARX_LIST_EMPTY;
    else if (v < 0 || (int64_t)v >= V) c = ARX_LIST_RANGE;
    else c = codes[(int64_t)(v % W) * slab + r * ldcode + j];      // the owner's verdict
    why[r * ldw + j] = c;
    clean[r * ldc + j] = c == ARX_LIST_OK ? v : -1;
  }
}

inline int ll_grid(int64_t units) {
  const int64_t cap = (int64_t)cu_count() * 8;
  return (int)(units < cap ? units : cap);
}

// the one body of arx_list_logp_prepare (shard off: W = 1, s = 0) and arx_list_logp_prepare_shard
int ll_prepare(const char* fn, bool shard, const int32_t* lists, int64_t ldl, int64_t B, int k, int64_t V, int W, int s,
               const int32_t* row_keys, int64_t key_rows, const int32_t* ex_ptr, const int32_t* ex_cols,
               const int32_t* col_tags, const int32_t* want_any, const int32_t* want_all, int64_t want_rows,
               int32_t* clean, int64_t ldc, int32_t* why, int64_t ldw, int32_t* pk_cols, int32_t* pk_slot, int64_t ldp,
               void* stream) {
  ARX_CHECK_ARG(lists && clean && why && pk_cols && pk_slot, "%s: null pointer", fn);
  ARX_CHECK_ARG(B >= 0, "%s: need B >= 0 (B=%lld)", fn, (long long)B);
  ARX_CHECK_ARG(k >= 1 && k <= kLlMaxK, "%s: need 1 <= k <= %d (k=%d)", fn, kLlMaxK, k);
  ARX_CHECK_ARG(V > 0 && V <= 0x7fffffffll, "%s: need 0 < V < 2^31 (V=%lld)", fn, (long long)V);
  ARX_CHECK_ARG(W >= 1 && s >= 0 && s < W, "%s: need W >= 1 and 0 <= s < W (W=%d s=%d)", fn, W, s);
  ARX_CHECK_ARG(ldl >= k && ldc >= k && ldw >= k && ldp >= k,
                "%s: need ldl, ldc, ldw and ldp >= k (ldl=%lld ldc=%lld ldw=%lld ldp=%lld k=%d)", fn, (long long)ldl,
                (long long)ldc, (long long)ldw, (long long)ldp, k);
  const bool ex_all = row_keys && ex_ptr && ex_cols, ex_none = !row_keys && !ex_ptr && !ex_cols;
  ARX_CHECK_ARG(ex_all || ex_none, "%s: row_keys, ex_ptr and ex_cols go together (all or none)", fn);
  ARX_CHECK_ARG(!ex_all || key_rows > 0, "%s: need key_rows > 0 with exclusion lists (key_rows=%lld)", fn,
                (long long)key_rows);
  const bool tg_all = col_tags && want_any && want_all, tg_none = !col_tags && !want_any && !want_all;
  ARX_CHECK_ARG(tg_all || tg_none, "%s: col_tags, want_any and want_all go together (all or none)", fn);
  ARX_CHECK_ARG(!tg_all || want_rows > 0, "%s: need want_rows > 0 with tags (want_rows=%lld)", fn, (long long)want_rows);
  if (B == 0) return ARX_OK;
  const int grid = ll_grid(ceil_div(B, (int64_t)kLlWaves));
  if (shard)
    k_list_prepare<true><<<grid, kLlThreads, 0, as_stream(stream)>>>(
        lists, ldl, B, k, V, W, s, row_keys, key_rows, ex_ptr, ex_cols, col_tags, want_any, want_all, want_rows, clean,
        ldc, why, ldw, pk_cols, pk_slot, ldp);
  else
    k_list_prepare<false><<<grid, kLlThreads, 0, as_stream(stream)>>>(
        lists, ldl, B, k, V, W, s, row_keys, key_rows, ex_ptr, ex_cols, col_tags, want_any, want_all, want_rows, clean,
        ldc, why, ldw, pk_cols, pk_slot, ldp);
  ARX_CHECK_LAUNCH();
  return ARX_OK;
}

}  // namespace
}  // namespace arx

using namespace arx;

extern "C" {

int arx_list_logp_prepare(const int32_t* lists, int64_t ldl, int64_t B, int k, int64_t V, const int32_t* row_keys,
                          int64_t key_rows, const int32_t* ex_ptr, const int32_t* ex_cols, const int32_t* col_tags,
                          const int32_t* want_any, const int32_t* want_all, int64_t want_rows, int32_t* clean,
                          int64_t ldc, int32_t* why, int64_t ldw, int32_t* pk_cols, int32_t* pk_slot, int64_t ldp,
                          void* stream) {
  return ll_prepare("arx_list_logp_prepare", false, lists, ldl, B, k, V, 1, 0, row_keys, key_rows, ex_ptr, ex_cols,
                    col_tags, want_any, want_all, want_rows, clean, ldc, why, ldw, pk_cols, pk_slot, ldp, stream);
}

int arx_list_logp_prepare_shard(const int32_t* lists, int64_t ldl, int64_t B, int k, int64_t V_global, int W, int s,
                                const int32_t* row_keys, int64_t key_rows, const int32_t* ex_ptr,
                                const int32_t* ex_cols, const int32_t* col_tags, const int32_t* want_any,
                                const int32_t* want_all, int64_t want_rows, int32_t* clean, int64_t ldc, int32_t* why,
                                int64_t ldw, int32_t* pk_cols, int32_t* pk_slot, int64_t ldp, void* stream) {
  return ll_prepare("arx_list_logp_prepare_shard", true, lists, ldl, B, k, V_global, W, s, row_keys, key_rows, ex_ptr,
                    ex_cols, col_tags, want_any, want_all, want_rows, clean, ldc, why, ldw, pk_cols, pk_slot, ldp, stream);
}

int arx_list_logp_merge_shards(const int32_t* lists, int64_t ldl, int64_t B, int k, int64_t V_global,
                               const int32_t* codes, int64_t ldcode, int64_t slab, int W, int32_t* clean, int64_t ldc,
                               int32_t* why, int64_t ldw, void* stream) {
  ARX_CHECK_ARG(lists && codes && clean && why, "arx_list_logp_merge_shards: null pointer");
  ARX_CHECK_ARG(B >= 0, "arx_list_logp_merge_shards: need B >= 0 (B=%lld)", (long long)B);
  ARX_CHECK_ARG(k >= 1 && k <= kLlMaxK, "arx_list_logp_merge_shards: need 1 <= k <= %d (k=%d)", kLlMaxK, k);
  ARX_CHECK_ARG(V_global > 0 && V_global <= 0x7fffffffll, "arx_list_logp_merge_shards: need 0 < V_global < 2^31 (%lld)",
                (long long)V_global);
  ARX_CHECK_ARG(W >= 1 && W <= 64, "arx_list_logp_merge_shards: need 1 <= W <= 64 (W=%d)", W);
  ARX_CHECK_ARG(ldl >= k && ldcode >= k && ldc >= k && ldw >= k && slab >= 0,
                "arx_list_logp_merge_shards: need ldl, ldcode, ldc and ldw >= k, slab >= 0 (ldl=%lld ldcode=%lld "
                "ldc=%lld ldw=%lld slab=%lld k=%d)",
                (long long)ldl, (long long)ldcode, (long long)ldc, (long long)ldw, (long long)slab, k);
  if (B == 0) return ARX_OK;
  k_list_merge<<<ll_grid(ceil_div(B * k, (int64_t)256)), 256, 0, as_stream(stream)>>>(lists, ldl, B, k, V_global, codes,
                                                                                      ldcode, slab, W, clean, ldc, why,
                                                                                      ldw);
  ARX_CHECK_LAUNCH();
  return ARX_OK;
}

int arx_list_logp_stamp(const int32_t* clean, int64_t ldc, const float* pick_score, int64_t ldps, int64_t B, int k,
                        int32_t* why, int64_t ldw, float* logp, int64_t ldo, float* values, int64_t ldv, void* stream) {
  ARX_CHECK_ARG(clean && pick_score && why && logp, "arx_list_logp_stamp: null pointer (only values may be NULL)");
  ARX_CHECK_ARG(B >= 0, "arx_list_logp_stamp: need B >= 0 (B=%lld)", (long long)B);
  ARX_CHECK_ARG(k >= 1 && k <= kLlMaxK, "arx_list_logp_stamp: need 1 <= k <= %d (k=%d)", kLlMaxK, k);
  ARX_CHECK_ARG(ldc >= k && ldps >= k && ldw >= k && ldo >= k && (!values || ldv >= k),
                "arx_list_logp_stamp: need ldc, ldps, ldw, ldo (and ldv with values) >= k (k=%d)", k);
  if (B == 0) return ARX_OK;
  k_list_stamp<<<ll_grid(ceil_div(B * k, (int64_t)256)), 256, 0, as_stream(stream)>>>(clean, ldc, pick_score, ldps, B, k,
                                                                                      why, ldw, logp, ldo, values, ldv);
  ARX_CHECK_LAUNCH();
  return ARX_OK;
}

}  // extern "C"

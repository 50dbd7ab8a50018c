// rank_keys.h -- how a double becomes a key and how ties are counted: the one statement behind gss_auc_rows (auc.hip), gss_rank_metrics_rows
// (rank_metrics.hip) and gss_profile_rank (profile_rank.hip).  A score becomes an order-preserving uint64 key (-0.0 folded into +0.0), a
// power-of-two block of keys is bitonic-sorted in LDS, and "below" and "tied" are a lower-bound and an upper-bound binary search: every
// rule of the three files depends on those integer counts alone.  The row kernels (auc.hip, rank_metrics.hip, rank_strata.hip) also
// share what they refuse on the device: the positives' list of a row, checked while its bitmap is built.  What those three share above
// this -- the limits, the scoring body of the two that rank with cut-offs, the argument checks and the refusals' way back to the host --
// is rank_score.h, which includes this file.  Inline code only.
#pragma once
#include "device_scope.h"

namespace gss {

constexpr uint64_t kBehind = ~0ull;   // the key of whatever sorts behind the keys that count (the other class, padding, NaN): above every other key

// the sort buffer's length: the least power of two >= c, at least 64
__host__ __device__ inline int32_t pow2_at_least(int32_t c) {
  int32_t p = 64;
  while (p < c) p <<= 1;
  return p;
}

__device__ __forceinline__ bool finite_bits(uint64_t b) { return (b & 0x7ff0000000000000ull) != 0x7ff0000000000000ull; }

// order-preserving key of a double under IEEE comparison (no NaN); +0.0 and -0.0 are one value.  No value maps to kBehind
__device__ __forceinline__ uint64_t order_key(double x) {
  const uint64_t b = (uint64_t)__double_as_longlong(x == 0.0 ? 0.0 : x);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

// order_key with NaN -> kBehind (above +inf's key)
__device__ __forceinline__ uint64_t order_key_nan_behind(double x) { return x != x ? kBehind : order_key(x); }

// first index in [lo, hi) whose key is >= k (strict = false) or > k (strict = true); hi if there is none
__device__ __forceinline__ int32_t search(const uint64_t *key, int32_t lo, int32_t hi, uint64_t k, bool strict) {
  while (lo < hi) {
    const int32_t mid = (lo + hi) >> 1;
    const uint64_t m = key[mid];
    if (strict ? m <= k : m < k) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// bitonic sort of the cpad keys, ascending (cpad a power of two), by a workgroup of THREADS; ends behind a barrier.  It is made of
// barriers: EVERY thread of the workgroup must reach the call, with the same cpad (never call it under a condition that threads disagree on)
template <int THREADS>
__device__ __forceinline__ void sort_keys(uint64_t *key, int32_t cpad, int32_t tid) {
  for (int32_t k = 2; k <= cpad; k <<= 1) {
    for (int32_t j = k >> 1; j > 0; j >>= 1) {
      for (int32_t i = tid; i < cpad / 2; i += THREADS) {
        const int32_t lo = ((i & ~(j - 1)) << 1) | (i & (j - 1)), hi = lo + j;
        const uint64_t x = key[lo], y = key[hi];
        if ((x > y) == ((lo & k) == 0)) {
          key[lo] = y;
          key[hi] = x;
        }
      }
      __syncthreads();
    }
  }
}

// sort_keys over the pairs (key[i], idx[i]), ascending by key, then by index: with distinct indices the order is total, so equal keys cannot
// make it depend on the network.  perm_null.h's seeded permutations are idx after this sort of counter-based keys.  Made of barriers, as
// sort_keys is
template <int THREADS>
__device__ __forceinline__ void sort_pairs(uint64_t *key, int32_t *idx, int32_t cpad, int32_t tid) {
  for (int32_t k = 2; k <= cpad; k <<= 1) {
    for (int32_t j = k >> 1; j > 0; j >>= 1) {
      for (int32_t i = tid; i < cpad / 2; i += THREADS) {
        const int32_t lo = ((i & ~(j - 1)) << 1) | (i & (j - 1)), hi = lo + j;
        const uint64_t x = key[lo], y = key[hi];
        const int32_t ix = idx[lo], iy = idx[hi];
        const bool above = x > y || (x == y && ix > iy);
        if (above == ((lo & k) == 0)) {
          key[lo] = y;
          key[hi] = x;
          idx[lo] = iy;
          idx[hi] = ix;
        }
      }
      __syncthreads();
    }
  }
}

// ---- the positives of a row: what the two row kernels check before they sort ------------------------------------------------------------
// per-row refusal, written to n_pos[r] as -code with the offending column (kBadPtr: the row's length) in n_neg[r]
enum RowRefusal { kBadPtr = 1, kColRange = 2, kColRepeat = 3, kNonFinite = 4 };

// row r's slice [b, b + P) of pos_col -> whether pos_ptr[r], pos_ptr[r + 1] can be a CSR row pointer's; if not, the refusal is written.
// Uniform over the workgroup: every thread reads the same two words
__device__ __forceinline__ bool row_positives(const int32_t *__restrict__ pos_ptr, int32_t r, int32_t C, int32_t tid, int32_t *__restrict__ n_pos,
                                              int32_t *__restrict__ n_neg, int32_t &b, int32_t &P) {
  b = pos_ptr[r];
  P = pos_ptr[r + 1] - b;
  if (b < 0 || P < 0 || P > C || (r == 0 && b != 0)) {
    if (tid == 0) {
      n_pos[r] = -kBadPtr;
      n_neg[r] = P;
    }
    return false;
  }
  return true;
}

// Marks the row's P positives pos[0 .. P) in the bitmap is_pos [cpad / 32] (an LDS atomicOr per entry also finds a repeated column) and
// fills key [cpad] with the keys of one class -- the positives (POSITIVES) or the negatives -- and kBehind for the other class and the
// padding.  -> whether the row goes on to the sort: a column outside [0, C), a repeated column or a score that is not finite is a
// refusal (the first in that order of precedence; the first offending list entry, the least repeated column, the least such column), and
// a row of one class only has its counts; either way n_pos[r] and n_neg[r] are written here and the caller writes its NaNs.  The answer
// is uniform, and the function is made of barriers: EVERY thread of the workgroup (of THREADS) must reach the call.  It ends behind one
template <int THREADS, bool POSITIVES>
__device__ __forceinline__ bool mark_and_fill(int32_t C, int32_t cpad, const double *__restrict__ row, const int32_t *__restrict__ pos, int32_t P,
                                              int32_t tid, uint64_t *key, uint32_t *is_pos, int32_t *__restrict__ n_pos_r,
                                              int32_t *__restrict__ n_neg_r) {
  __shared__ int32_t bad_range, bad_repeat, bad_finite;
  if (tid == 0) {
    bad_range = INT32_MAX;
    bad_repeat = INT32_MAX;
    bad_finite = INT32_MAX;
  }
  for (int32_t w = tid; w < cpad / 32; w += THREADS) is_pos[w] = 0u;
  __syncthreads();
  for (int32_t k = tid; k < P; k += THREADS) {
    const int32_t c = pos[k];
    if (c < 0 || c >= C) {
      atomicMin(&bad_range, k);     // the first offending entry in list order
      continue;
    }
    const uint32_t bit = 1u << (c & 31);
    if (atomicOr(&is_pos[c >> 5], bit) & bit) atomicMin(&bad_repeat, c);
  }
  __syncthreads();
  for (int32_t c = tid; c < cpad; c += THREADS) {
    uint64_t k = kBehind;
    if (c < C) {
      const double x = row[c];
      if (!finite_bits((uint64_t)__double_as_longlong(x))) atomicMin(&bad_finite, c);
      else if ((((is_pos[c >> 5] >> (c & 31)) & 1u) != 0) == POSITIVES) k = order_key(x);
    }
    key[c] = k;
  }
  __syncthreads();
  const int32_t N = C - P;
  if (bad_range == INT32_MAX && bad_repeat == INT32_MAX && bad_finite == INT32_MAX && P != 0 && N != 0) return true;
  if (tid == 0) {
    if (bad_range != INT32_MAX) {
      *n_pos_r = -kColRange;
      *n_neg_r = pos[bad_range];
    } else if (bad_repeat != INT32_MAX) {
      *n_pos_r = -kColRepeat;
      *n_neg_r = bad_repeat;
    } else if (bad_finite != INT32_MAX) {
      *n_pos_r = -kNonFinite;
      *n_neg_r = bad_finite;
    } else {
      *n_pos_r = P;
      *n_neg_r = N;
    }
  }
  return false;
}

}  // namespace gss

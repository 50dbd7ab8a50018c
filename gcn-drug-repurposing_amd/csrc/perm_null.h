// perm_null.h -- what the seeded permutation nulls share (class_cohesion.hip, matrix_mantel.hip, enrich.hip): the
// key and padding rule of a permutation, the order of a row sum, the entry points' host checks.  Unnamed namespace: nothing is exported.
#pragma once
#include "rank_keys.h"
#include "counter_rng.h"
#include "device_scope.h"

namespace gss {
namespace {

// the sort key of place i in sample s of the null `tag` (an RngTag).  A kernel fills (key, idx)[0 .. cpad) in LDS with (perm_key, i) for i < n
// and pads with (kBehind, i >= n), which sorts behind every real pair; sort_pairs<THREADS>(key, idx, cpad, tid) then leaves pi_s in idx.  The
// four-line fill stays in each kernel: as a shared function it changed cc_random_kernel's register allocation and cost 0.3 % of its time
__device__ __forceinline__ uint64_t perm_key(uint64_t seed, uint64_t tag, uint64_t s, int32_t i) { return rng_key(seed, tag, s, (uint64_t)i, 0); }

// the sum of term(i), i < j, in the row sum's order, by a whole wave; every lane returns it.  The terms of AHEAD strides are formed (their
// loads issued) before their additions, which stay in order and are never contracted with a term's product
template <int AHEAD, typename Term>
__device__ __forceinline__ double wave_ordered_sum(int32_t j, int lane, Term term) {
#pragma clang fp contract(off)
  double v = 0.0;
  int32_t i = lane;
  if constexpr (AHEAD > 1) {
    for (; i + (AHEAD - 1) * kWave < j; i += AHEAD * kWave) {
      double x[AHEAD];
#pragma unroll
      for (int u = 0; u < AHEAD; ++u) x[u] = term(i + u * kWave);
#pragma unroll
      for (int u = 0; u < AHEAD; ++u) v = v + x[u];
    }
  }
  for (; i < j; i += kWave) v = v + term(i);
  return wave_sum_d(v);
}

// samples s0 .. s0 + P - 1 must be sample numbers: the kernels count them in 31 bits
inline int check_sample_window(const char *who, int64_t s0, int32_t P) {
  GSS_REQUIRE(s0 >= 0 && s0 + (int64_t)P <= (int64_t)1 << 31, "%s: samples s0=%lld .. s0 + P=%lld are outside [0, 2^31]", who, (long long)s0,
              (long long)(s0 + (int64_t)P));
  return GSS_OK;
}

// h = a host copy of the n_sizes set sizes at d_sizes: each in [lo, hi] (hi_words: the refusal's words for hi), strictly ascending
inline int check_sizes(const char *who, const int32_t *d_sizes, int32_t n_sizes, int32_t lo, int32_t hi, const char *hi_words, hipStream_t st,
                       std::unique_ptr<int32_t[]> &h) {
  if (int rc = host_copy(h, d_sizes, (size_t)n_sizes, st, "%s: host copy of %d sizes", who, n_sizes)) return rc;
  for (int32_t k = 0; k < n_sizes; ++k) {
    GSS_REQUIRE(h[k] >= lo && h[k] <= hi, "%s: sizes[%d] = %d is outside [%d, %s]", who, k, h[k], lo, hi_words);
    GSS_REQUIRE(k == 0 || h[k] > h[k - 1], "%s: sizes[%d] = %d is not above sizes[%d] = %d (strictly ascending)", who, k, h[k], k - 1, h[k - 1]);
  }
  return GSS_OK;
}

// h = a host copy of the C + 1 offsets at d_ptr of C lists packed one after another: 0 first, non-decreasing
inline int check_list_offsets(const char *who, const int32_t *d_ptr, int32_t C, hipStream_t st, std::unique_ptr<int32_t[]> &h) {
  if (int rc = host_copy(h, d_ptr, (size_t)C + 1, st, "%s: host copy of ptr, %d lists", who, C)) return rc;
  GSS_REQUIRE(h[0] == 0, "%s: ptr[0] = %d must be 0", who, h[0]);
  for (int32_t c = 0; c < C; ++c) GSS_REQUIRE(h[c + 1] >= h[c], "%s: ptr[%d] = %d is below ptr[%d] = %d", who, c + 1, h[c + 1], c, h[c]);
  return GSS_OK;
}

}  // namespace
}  // namespace gss

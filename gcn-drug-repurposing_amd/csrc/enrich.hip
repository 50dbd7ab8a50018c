// enrich.hip -- preranked gene-set enrichment of diffusion profiles: does a set of proteins as a whole sit higher in a profile than random
// sets of its size do?  The Kolmogorov-Smirnov-like running sum of Subramanian et al. 2005 with a gene-set permutation null.
//
// include/gssgcn.h has the contract, DESIGN.md section 9.16 the definitions, the limits and the measurements.  Three entry points:
//   gss_profile_order   the order of a profile's column over a universe of M nodes: pos[u] = the place of u in
//                       np.argsort(-x[universe, c], kind="stable") and w[u] = |x[universe[u], c]|.  A rank needs no sorted payload, only a
//                       count: with the descending key k_u = ~order_key(x_u) (rank_keys.h), pos[u] = the number of pairs (k_v, v) below
//                       (k_u, u), summed over chunks of kOrdChunk pairs that sort_pairs orders in LDS and every place searches.
//                         ord_keys_kernel   one thread per (column, place): the key into the workspace, |x| into w_out;
//                         ord_rank_kernel   one workgroup per column: per chunk sort, then every place adds its lower bound to its own
//                                           word of pos_out (the first chunk stores); a column with a NaN is rewritten as -1 / NaN.
//   gss_enrich_lists    ES and its peak of listed sets: one workgroup per (set, column) sorts the members' (pos, place) pairs in LDS and
//                       one lane walks them (es_walk, the one statement of the score).
//   gss_enrich_random   the null: one workgroup per sample s selects the kmax smallest of the M keys perm_key(seed, kRngEnrichPerm, s, i)
//                       exactly -- the keys at or under a threshold are collected in LDS, the threshold is bisected when fewer than kmax or
//                       more than the buffer holds came, and sort_pairs orders what came by (key, i): the result is the prefix of the
//                       permutation whatever the thresholds were -- then per column sorts the prefix by pos, keeping each member's rank
//                       rho in the permutation; the set of size m is the subsequence with rho < m, and one lane per size walks it with
//                       es_walk: every size in exactly the order of the definition, bit-equal to gss_enrich_lists on the prefix.
// All arithmetic of the score is fp64, every operation rounded on its own; nothing is accumulated with atomics (the only atomics are
// integer counters and bitmaps in LDS and the refusal's status word), and every output word has one owner.
#include "profile_front.h"

#include "perm_null.h"

namespace gss {
namespace {

constexpr int kOrdThreads = 1024;
constexpr int kOrdChunk = 4096;        // (key, place) pairs sorted in LDS at a time: 48 KiB
constexpr int kOrdMaxM = 65536;        // the count is quadratic in M / kOrdChunk
constexpr int kEsThreads = 256;
constexpr int kEsMaxSet = 1024;        // members of a set: sorted in LDS and walked by one lane
constexpr int kEsMaxCols = 65535;      // gss_enrich_lists: the grid's second dimension
constexpr int kSelCap = 2048;          // gss_enrich_random: keys collected under the threshold, at most
constexpr int kSelRounds = 80;         // a bisection over 64-bit thresholds ends within 64 rounds
constexpr uint64_t kNanKey = 0;        // no value's descending key: ~order_key(x) = 0 only for order_key(x) = kBehind

__device__ __forceinline__ double quiet_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// the number of pairs of the sorted (key, idx)[0 .. hi) below (k, u)
__device__ __forceinline__ int32_t pairs_below(const uint64_t *key, const int32_t *idx, int32_t hi, uint64_t k, int32_t u) {
  int32_t lo = 0;
  while (lo < hi) {
    const int32_t mid = (lo + hi) >> 1;
    const uint64_t m = key[mid];
    if (m < k || (m == k && idx[mid] < u)) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// ---- gss_profile_order ------------------------------------------------------------------------------------------------------------------
// status[2]: the first position of universe whose entry is outside [0, n) or not above its predecessor
__global__ __launch_bounds__(kListThreads) void ord_universe_kernel(int32_t n, int32_t M, const int32_t *__restrict__ universe,
                                                                     uint32_t *__restrict__ status) {
  const int32_t t = blockIdx.x * kListThreads + threadIdx.x;
  if (t >= M) return;
  const int32_t e = universe[t];
  if (e < 0 || e >= n || (t > 0 && e <= universe[t - 1])) atomicMin(&status[2], (uint32_t)t);
}

__global__ __launch_bounds__(kListThreads) void ord_keys_kernel(int32_t M, const double *__restrict__ x, int64_t ld, const int32_t *__restrict__ cols,
                                                                 const int32_t *__restrict__ universe, uint64_t *__restrict__ keys,
                                                                 double *__restrict__ w_out) {
  const int32_t u = blockIdx.x * kListThreads + threadIdx.x, j = blockIdx.y;
  if (u >= M) return;
  const int32_t c = cols ? cols[j] : j;
  const double v = x[(int64_t)universe[u] * ld + c];
  keys[(size_t)j * M + u] = v != v ? kNanKey : ~order_key(v);
  w_out[(size_t)j * M + u] = fabs(v);
}

// workgroup = list position blockIdx.x; place i belongs to thread i mod kOrdThreads in every chunk round
__global__ __launch_bounds__(kOrdThreads) void ord_rank_kernel(int32_t M, const uint64_t *__restrict__ keys, int32_t *__restrict__ pos_out,
                                                                double *__restrict__ w_out) {
  __shared__ uint64_t srt[kOrdChunk];
  __shared__ int32_t plc[kOrdChunk];
  const int32_t tid = threadIdx.x;
  const uint64_t *key = keys + (size_t)blockIdx.x * M;
  int32_t *pos = pos_out + (size_t)blockIdx.x * M;
  int nan_here = 0;
  for (int32_t c0 = 0; c0 < M; c0 += kOrdChunk) {
    const int32_t len = min(kOrdChunk, M - c0), cpad = pow2_at_least(len);
    for (int32_t i = tid; i < cpad; i += kOrdThreads) {
      const uint64_t k = i < len ? key[c0 + i] : kBehind;
      nan_here |= (i < len && k == kNanKey) ? 1 : 0;
      srt[i] = k;
      plc[i] = c0 + i;       // the padding sorts behind every (key, place) of the chunk: no key is kBehind
    }
    __syncthreads();
    sort_pairs<kOrdThreads>(srt, plc, cpad, tid);
    for (int32_t i = tid; i < M; i += kOrdThreads) {
      const int32_t below = pairs_below(srt, plc, len, key[i], i);
      pos[i] = c0 == 0 ? below : pos[i] + below;
    }
    __syncthreads();   // the next chunk overwrites srt
  }
  if (__syncthreads_or(nan_here)) {
    double *w = w_out + (size_t)blockIdx.x * M;
    for (int32_t i = tid; i < M; i += kOrdThreads) {
      pos[i] = -1;
      w[i] = quiet_nan();
    }
  }
}

// ---- the score --------------------------------------------------------------------------------------------------------------------------
// ES and its peak of the members among the len entries (p = pos, a = weight, ascending p): every entry (rho null), or those with
// rho[e] < m.  m = the number of members.  One lane walks; the statement of include/gssgcn.h, operation by operation
__device__ __forceinline__ void es_walk(const uint64_t *p, const double *a, const int32_t *rho, int32_t len, int32_t m, int32_t M, double &es,
                                        int32_t &peak) {
#pragma clang fp contract(off)
  double N = 0.0;
  for (int32_t e = 0; e < len; ++e)
    if (!rho || rho[e] < m) N = N + a[e];
  if (N == 0.0) {
    es = quiet_nan();
    peak = -1;
    return;
  }
  const double den = (double)(M - m);
  double c = 0.0, hi = -__builtin_inf(), lo = __builtin_inf();
  int32_t khi = -1, klo = -1, k = 0;
  for (int32_t e = 0; e < len; ++e) {
    if (rho && rho[e] >= m) continue;
    const double miss = (double)((int32_t)p[e] - k) / den;
    const double l = c / N - miss;
    c = c + a[e];
    const double h = c / N - miss;
    if (h > hi) {
      hi = h;
      khi = k;
    }
    if (l < lo) {
      lo = l;
      klo = k;
    }
    ++k;
  }
  if (hi >= -lo) {
    es = hi;
    peak = khi;
  } else {
    es = lo;
    peak = klo;
  }
}

// ---- gss_enrich_lists -------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long pack_refusal(int32_t list, int kind, int32_t at) {
  return ((unsigned long long)list << 32) | ((unsigned long long)kind << 16) | (unsigned long long)at;
}

// one workgroup per list (lengths in [1, kEsMaxSet], checked on the host): *status = the least (list, kind, position) of a place outside
// [0, M) (kind 0, the first such position) or repeated within its list (kind 1: the second position of the least repeated place)
__global__ __launch_bounds__(kEsThreads) void es_check_kernel(int32_t M, const int32_t *__restrict__ ptr, const int32_t *__restrict__ idx,
                                                               unsigned long long *__restrict__ status) {
  __shared__ uint32_t seen[kOrdMaxM / 32];
  __shared__ int32_t bad_range, rep_place, first, second;
  const int32_t c = blockIdx.x, tid = threadIdx.x;
  const int32_t b = ptr[c], s = ptr[c + 1] - b;
  if (tid == 0) bad_range = rep_place = first = second = INT32_MAX;
  for (int32_t i = tid; i < (M + 31) / 32; i += kEsThreads) seen[i] = 0u;
  __syncthreads();
  for (int32_t k = tid; k < s; k += kEsThreads) {
    const int32_t u = idx[b + k];
    if (u < 0 || u >= M) {
      atomicMin(&bad_range, k);
      continue;
    }
    const uint32_t bit = 1u << (u & 31);
    if (atomicOr(&seen[u >> 5], bit) & bit) atomicMin(&rep_place, u);
  }
  __syncthreads();
  if (bad_range != INT32_MAX) {
    if (tid == 0) atomicMin(status, pack_refusal(c, 0, bad_range));
    return;
  }
  if (rep_place == INT32_MAX) return;   // uniform
  for (int32_t k = tid; k < s; k += kEsThreads)
    if (idx[b + k] == rep_place) atomicMin(&first, k);
  __syncthreads();
  for (int32_t k = tid; k < s; k += kEsThreads)
    if (idx[b + k] == rep_place && k != first) atomicMin(&second, k);
  __syncthreads();
  if (tid == 0) atomicMin(status, pack_refusal(c, 1, second));
}

// workgroup = (list blockIdx.x, column blockIdx.y)
__global__ __launch_bounds__(kEsThreads) void es_lists_kernel(int32_t M, const int32_t *__restrict__ pos, const double *__restrict__ w, int weighted,
                                                               int32_t C, const int32_t *__restrict__ ptr, const int32_t *__restrict__ idx,
                                                               double *__restrict__ es_out, int32_t *__restrict__ peak_out) {
  __shared__ uint64_t key[kEsMaxSet];
  __shared__ int32_t plc[kEsMaxSet];
  __shared__ double a[kEsMaxSet];
  const int32_t c = blockIdx.x, j = blockIdx.y, tid = threadIdx.x;
  const int32_t b = ptr[c], s = ptr[c + 1] - b;
  const int32_t *__restrict__ pj = pos + (size_t)j * M;
  const double *__restrict__ wj = w + (size_t)j * M;
  const size_t out = (size_t)j * C + c;
  if (pj[0] < 0) {   // a flagged column holds -1 at every place: uniform
    if (tid == 0) {
      es_out[out] = quiet_nan();
      peak_out[out] = -1;
    }
    return;
  }
  const int32_t cpad = pow2_at_least(s);
  for (int32_t i = tid; i < cpad; i += kEsThreads) {
    const int32_t u = i < s ? idx[b + i] : 0;
    key[i] = i < s ? (uint64_t)pj[u] : kBehind;
    plc[i] = i < s ? u : M + i;
  }
  __syncthreads();
  sort_pairs<kEsThreads>(key, plc, cpad, tid);
  for (int32_t i = tid; i < s; i += kEsThreads) a[i] = weighted ? wj[plc[i]] : 1.0;
  __syncthreads();
  if (tid == 0) {
    double es;
    int32_t peak;
    es_walk(key, a, nullptr, s, s, M, es, peak);
    es_out[out] = es;
    peak_out[out] = peak;
  }
}

// ---- gss_enrich_random ------------------------------------------------------------------------------------------------------------------
// sample s0 + blockIdx.x.  t0: the first threshold (all ones where M <= kSelCap: every key is collected)
__global__ __launch_bounds__(kEsThreads) void es_random_kernel(int32_t M, int32_t nc, const int32_t *__restrict__ pos, const double *__restrict__ w,
                                                                int weighted, uint64_t seed, int64_t s0, int32_t P, uint64_t t0, int32_t n_sizes,
                                                                const int32_t *__restrict__ sizes, int32_t kmax, double *__restrict__ es_out,
                                                                int32_t *__restrict__ perm_out) {
  __shared__ uint64_t sel_key[kSelCap];
  __shared__ int32_t sel_idx[kSelCap];
  __shared__ int32_t rho[kEsMaxSet];
  __shared__ int32_t count;
  const int32_t tid = threadIdx.x;
  const uint64_t s = (uint64_t)(s0 + blockIdx.x);
  // the kmax smallest keys: collect the keys <= T; too few (tlo = T) or more than the buffer holds (thi = T) bisects T.  The keys of a
  // sample are distinct (mix64 is a bijection and i enters one word), so a T between the kmax-th and the kSelCap-th smallest key exists
  uint64_t T = t0, tlo = 0, thi = ~0ull;
  int32_t got = -1;
  for (int round = 0; round < kSelRounds; ++round) {
    if (tid == 0) count = 0;
    __syncthreads();
    for (int32_t i = tid; i < M; i += kEsThreads) {
      const uint64_t k = perm_key(seed, kRngEnrichPerm, s, i);
      if (k <= T) {
        const int32_t slot = atomicAdd(&count, 1);
        if (slot < kSelCap) {
          sel_key[slot] = k;
          sel_idx[slot] = i;
        }
      }
    }
    __syncthreads();
    const int32_t n = count;
    __syncthreads();   // every thread has read count before the next round resets it
    if (n >= kmax && n <= kSelCap) {
      got = n;
      break;
    }
    if (n < kmax) tlo = T;
    else thi = T;
    T = tlo + (thi - tlo) / 2;
  }
  if (got < 0) {   // not reached (see above); a sample that did would read as missing, not as a score
    for (int64_t i = tid; i < (int64_t)nc * n_sizes; i += kEsThreads)
      es_out[((i / n_sizes) * P + blockIdx.x) * n_sizes + i % n_sizes] = quiet_nan();
    if (perm_out)
      for (int32_t i = tid; i < kmax; i += kEsThreads) perm_out[(int64_t)blockIdx.x * kmax + i] = -1;
    return;
  }
  const int32_t spad = pow2_at_least(got);
  for (int32_t i = got + tid; i < spad; i += kEsThreads) {
    sel_key[i] = kBehind;
    sel_idx[i] = M + i;    // perm_null.h's padding: an index >= M sorts behind a place whose key is all ones
  }
  __syncthreads();
  sort_pairs<kEsThreads>(sel_key, sel_idx, spad, tid);   // the order it leaves does not depend on the slots the keys came in: (key, i) is total
  if (perm_out)
    for (int32_t i = tid; i < kmax; i += kEsThreads) perm_out[(int64_t)blockIdx.x * kmax + i] = sel_idx[i];
  // the keys have done their work: their LDS holds a column's sorted positions and, behind them, the members' weights
  uint64_t *pk = sel_key;
  double *pa = reinterpret_cast<double *>(sel_key + kEsMaxSet);
  const int32_t cpad = pow2_at_least(kmax);
  for (int32_t j = 0; j < nc; ++j) {
    const int32_t *__restrict__ pj = pos + (size_t)j * M;
    const double *__restrict__ wj = w + (size_t)j * M;
    double *__restrict__ out = es_out + ((size_t)j * P + blockIdx.x) * n_sizes;
    if (pj[0] < 0) {   // a flagged column: uniform
      for (int32_t k = tid; k < n_sizes; k += kEsThreads) out[k] = quiet_nan();
      continue;
    }
    __syncthreads();   // the lanes of the column before have left pk, pa and rho
    for (int32_t i = tid; i < cpad; i += kEsThreads) {
      pk[i] = i < kmax ? (uint64_t)pj[sel_idx[i]] : kBehind;
      rho[i] = i;
    }
    __syncthreads();
    sort_pairs<kEsThreads>(pk, rho, cpad, tid);
    for (int32_t i = tid; i < kmax; i += kEsThreads) pa[i] = weighted ? wj[sel_idx[rho[i]]] : 1.0;
    __syncthreads();
    for (int32_t k = tid; k < n_sizes; k += kEsThreads) {
      double es;
      int32_t peak;
      es_walk(pk, pa, rho, kmax, sizes[k], M, es, peak);
      out[k] = es;
    }
  }
}

int check_order(const char *who, int32_t M, int32_t nc) {
  GSS_REQUIRE(M >= 2 && M <= kOrdMaxM, "%s: M=%d places is outside [2, %d]", who, M, kOrdMaxM);
  GSS_REQUIRE(nc >= 0, "%s: nc=%d columns must be >= 0", who, nc);
  return GSS_OK;
}

inline int32_t max_set(int32_t M) { return M - 1 < kEsMaxSet ? M - 1 : kEsMaxSet; }

}  // namespace
}  // namespace gss

using namespace gss;

extern "C" {

// status words, then per listed column M keys of 8 bytes
size_t gss_profile_order_workspace_bytes(int32_t M, int32_t nc) {
  if (M < 2 || M > kOrdMaxM || nc < 0) return 0;
  return kStatusBytes + (size_t)nc * (size_t)M * 8;
}

int gss_profile_order(int32_t n, const double *x, int64_t ld, int32_t nc, const int32_t *cols, int32_t M, const int32_t *universe, int32_t *pos_out,
                      double *w_out, void *workspace, size_t workspace_bytes, void *stream) {
  GSS_REQUIRE(n >= 1 && n <= kKeyMaxRows, "profile_order: n=%d rows is outside [1, %d]", n, kKeyMaxRows);
  const int32_t m_max = n < kOrdMaxM ? n : kOrdMaxM;
  GSS_REQUIRE(M >= 2 && M <= m_max, "profile_order: M=%d places is outside [2, min(n, %d) = %d] (the counting scheme is quadratic in M / chunk: "
              "every place searches every sorted chunk of %d pairs)", M, kOrdMaxM, m_max, kOrdChunk);
  GSS_REQUIRE(nc >= 0 && nc <= kEsMaxCols, "profile_order: nc=%d columns is outside [0, %d]", nc, kEsMaxCols);
  GSS_REQUIRE(ld >= 1, "profile_order: ld=%lld must be >= 1", (long long)ld);
  GSS_REQUIRE(universe != nullptr, "profile_order: universe is null");
  GSS_REQUIRE(workspace != nullptr, "profile_order: workspace is null");
  GSS_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "profile_order: workspace is not 8-byte aligned");
  const size_t want = gss_profile_order_workspace_bytes(M, nc);
  GSS_REQUIRE(workspace_bytes >= want, "profile_order: workspace of %zu bytes is below the %zu that M=%d, nc=%d need", workspace_bytes, want, M, nc);
  if (nc > 0) {
    GSS_REQUIRE(x != nullptr, "profile_order: x is null");
    GSS_REQUIRE(pos_out != nullptr, "profile_order: pos_out is null");
    GSS_REQUIRE(w_out != nullptr, "profile_order: w_out is null");
    GSS_REQUIRE((reinterpret_cast<uintptr_t>(pos_out) & 3) == 0, "profile_order: pos_out is not 4-byte aligned");
    GSS_REQUIRE((reinterpret_cast<uintptr_t>(w_out) & 7) == 0, "profile_order: w_out is not 8-byte aligned");
    GSS_REQUIRE(cols || nc <= ld, "profile_order: ld=%lld is below nc=%d (cols is null: columns 0 .. nc - 1)", (long long)ld, nc);
  }
  hipStream_t st = as_stream(stream);
  uint32_t *status = static_cast<uint32_t *>(workspace);
  // nothing reads x through a list before every entry of it is known to be a row or a column of x
  GSS_HIP(hipMemsetAsync(status + 2, 0xff, 4, st));
  hipLaunchKernelGGL(ord_universe_kernel, dim3(ceil_div(M, kListThreads)), dim3(kListThreads), 0, st, n, M, universe, status);
  GSS_LAUNCH_CHECK("ord_universe_kernel");
  uint32_t at = kListNone;
  if (int rc = read_back(&at, status + 2, 4, st)) return rc;
  if (at != kListNone) {
    int32_t e[2] = {0, 0};
    GSS_HIP(hipMemcpy(e, universe + (at > 0 ? at - 1 : 0), at > 0 ? 8 : 4, hipMemcpyDeviceToHost));
    const int32_t here = at > 0 ? e[1] : e[0];
    if (here < 0 || here >= n) return fail(GSS_EINVAL, "profile_order: universe[%u] = %d is outside [0, n=%d)", at, here, n);
    return fail(GSS_EINVAL, "profile_order: universe[%u] = %d is not above universe[%u] = %d (strictly ascending)", at, here, at - 1, e[0]);
  }
  if (nc == 0) return GSS_OK;
  if (cols) {
    const CheckedList a{cols, nc, 0, ld, "cols", "ld"}, none{nullptr, 0, 0, 0, "", ""};
    if (int rc = check_lists("profile_order", a, none, status, st)) return rc;
  }
  uint64_t *keys = reinterpret_cast<uint64_t *>(static_cast<char *>(workspace) + kStatusBytes);
  hipLaunchKernelGGL(ord_keys_kernel, dim3(ceil_div(M, kListThreads), nc), dim3(kListThreads), 0, st, M, x, ld, cols, universe, keys, w_out);
  GSS_LAUNCH_CHECK("ord_keys_kernel");
  hipLaunchKernelGGL(ord_rank_kernel, dim3(nc), dim3(kOrdThreads), 0, st, M, keys, pos_out, w_out);
  GSS_LAUNCH_CHECK("ord_rank_kernel");
  return GSS_OK;
}

int gss_enrich_lists(int32_t M, int32_t nc, const int32_t *pos, const double *w, int32_t weighted, int32_t C, const int32_t *ptr, const int32_t *idx,
                     double *es_out, int32_t *peak_out, void *stream) {
  if (int rc = check_order("enrich_lists", M, nc)) return rc;
  GSS_REQUIRE(nc <= kEsMaxCols, "enrich_lists: nc=%d columns is above %d", nc, kEsMaxCols);
  GSS_REQUIRE(weighted == 0 || weighted == 1, "enrich_lists: weighted=%d must be 0 or 1", weighted);
  GSS_REQUIRE(C >= 0, "enrich_lists: C=%d lists must be >= 0", C);
  if (C == 0 || nc == 0) return GSS_OK;
  GSS_REQUIRE(pos != nullptr, "enrich_lists: pos is null");
  GSS_REQUIRE(w != nullptr, "enrich_lists: w is null");
  GSS_REQUIRE(ptr != nullptr, "enrich_lists: ptr is null");
  GSS_REQUIRE(idx != nullptr, "enrich_lists: idx is null");
  GSS_REQUIRE(es_out != nullptr, "enrich_lists: es_out is null");
  GSS_REQUIRE(peak_out != nullptr, "enrich_lists: peak_out is null");
  hipStream_t st = as_stream(stream);
  std::unique_ptr<int32_t[]> h;
  if (int rc = check_list_offsets("enrich_lists", ptr, C, st, h)) return rc;
  const int32_t s_max = max_set(M);
  for (int32_t c = 0; c < C; ++c) {
    const int32_t s = h[c + 1] - h[c];
    GSS_REQUIRE(s >= 1 && s <= s_max, "enrich_lists: list %d has %d places, outside [1, min(%d, M - 1) = %d]", c, s, kEsMaxSet, s_max);
  }
  {   // nothing reads pos or w through a list before every entry of it is known to be a place, once; the status word is freed before the launch
    DeviceBuf<unsigned long long> status;
    if (int rc = status.alloc("enrich_lists", 8)) return rc;
    GSS_HIP(hipMemsetAsync(status.p, 0xff, 8, st));
    hipLaunchKernelGGL(es_check_kernel, dim3(C), dim3(kEsThreads), 0, st, M, ptr, idx, status.p);
    GSS_LAUNCH_CHECK("es_check_kernel");
    unsigned long long word = ~0ull;
    if (int rc = read_back(&word, status.p, 8, st)) return rc;
    if (word != ~0ull) {
      const int32_t c = (int32_t)(word >> 32), kind = (int32_t)((word >> 16) & 0xffff), at = (int32_t)(word & 0xffff);
      int32_t e = 0;
      GSS_HIP(hipMemcpy(&e, idx + h[c] + at, 4, hipMemcpyDeviceToHost));
      if (kind == 0) return fail(GSS_EINVAL, "enrich_lists: list %d: idx[%d] = %d is outside [0, M=%d)", c, at, e, M);
      return fail(GSS_EINVAL, "enrich_lists: list %d: idx[%d] = %d repeats a place of the list", c, at, e);
    }
  }
  hipLaunchKernelGGL(es_lists_kernel, dim3(C, nc), dim3(kEsThreads), 0, st, M, pos, w, (int)weighted, C, ptr, idx, es_out, peak_out);
  GSS_LAUNCH_CHECK("es_lists_kernel");
  return GSS_OK;
}

int gss_enrich_random(int32_t M, int32_t nc, const int32_t *pos, const double *w, int32_t weighted, uint64_t seed, int64_t s0, int32_t P,
                      int32_t n_sizes, const int32_t *sizes, double *es_out, int32_t *perm_out, void *stream) {
  if (int rc = check_order("enrich_random", M, nc)) return rc;
  GSS_REQUIRE(weighted == 0 || weighted == 1, "enrich_random: weighted=%d must be 0 or 1", weighted);
  GSS_REQUIRE(P >= 1, "enrich_random: P=%d samples must be >= 1", P);
  if (int rc = check_sample_window("enrich_random", s0, P)) return rc;
  const int32_t s_max = max_set(M);
  GSS_REQUIRE(n_sizes >= 1 && n_sizes <= s_max, "enrich_random: n_sizes=%d is outside [1, min(%d, M - 1) = %d]", n_sizes, kEsMaxSet, s_max);
  GSS_REQUIRE(sizes != nullptr, "enrich_random: sizes is null");
  if (nc > 0) {
    GSS_REQUIRE(pos != nullptr, "enrich_random: pos is null");
    GSS_REQUIRE(w != nullptr, "enrich_random: w is null");
    GSS_REQUIRE(es_out != nullptr, "enrich_random: es_out is null");
  }
  hipStream_t st = as_stream(stream);
  std::unique_ptr<int32_t[]> h;
  char hi_words[48];
  snprintf(hi_words, sizeof(hi_words), "min(%d, M - 1) = %d", kEsMaxSet, s_max);
  if (int rc = check_sizes("enrich_random", sizes, n_sizes, 1, s_max, hi_words, st, h)) return rc;
  if (nc == 0 && !perm_out) return GSS_OK;
  const int32_t kmax = h[n_sizes - 1];
  // the first threshold expects kmax + kmax / 4 + 8 of the M keys under it (include/gssgcn.h states it: a test replays a sample that it fails)
  const uint64_t t0 = M <= kSelCap ? ~0ull : (uint64_t)((((unsigned __int128)(kmax + kmax / 4 + 8)) << 64) / (unsigned __int128)M);
  hipLaunchKernelGGL(es_random_kernel, dim3(P), dim3(kEsThreads), 0, st, M, nc, pos, w, (int)weighted, seed, s0, P, t0, n_sizes, sizes, kmax, es_out,
                     perm_out);
  GSS_LAUNCH_CHECK("es_random_kernel");
  return GSS_OK;
}

}  // extern "C"

// class_cohesion.hip -- sums of a distance matrix over the pairs of a drug set: of listed sets (gss_pair_sums_lists, the observed statistic of
// an ATC class) and of the prefixes of seeded random permutations (gss_pair_sums_random, the null of every class size at once).
//
// include/gssgcn.h has the contract, DESIGN.md section 9.12 the definitions, the cost model and the measurements.  One statement of the sum
// serves both entry points (pair_prefix_sums): for an ordered list a[0 .. m) of rows of the symmetric fp64 matrix d,
//   r_j  = sum over i < j of d[a[j]][a[i]]    one wave per row j, in perm_null.h's fixed order (wave_ordered_sum): it depends on j alone;
//   T(m) = r_1 + r_2 + ... + r_{m-1}          added in that order by one thread that walks j and writes T at each requested size.
// So T(m) is a function of the ordered list and d: its bits do not depend on the grid, on the other lists or samples of the call, on the
// other sizes asked for, or on the chunks the rows are taken in.  Nothing is accumulated with atomics.
//   cc_lists_kernel    one workgroup per list; the list is read from global memory, r_j goes through an LDS buffer of kCcRowChunk rows;
//   cc_random_kernel   one workgroup per sample s: perm_null.h's permutation under the tag kRngClassPerm, sorted in LDS; its first
//                      sizes[n_sizes - 1] places are the list, every shorter prefix a smaller set, and r_j reuses the keys' LDS.
#include "profile_front.h"

#include "perm_null.h"

namespace gss {
namespace {

constexpr int kCcThreads = 256;
constexpr int kCcWaves = kCcThreads / kWave;
constexpr int kCcMaxN = 4096;       // the permutation of a sample is sorted in LDS: 4,096 x 12 B
constexpr int kCcRowChunk = 1024;   // rows of a list whose sums wait in LDS for the walking thread

// T(sizes[k]) of the list a[0 .. m) -> out[k] for the n_sizes sizes (strictly ascending, in [2, m]); r: LDS, cap doubles.  Rows are taken cap
// at a time; thread 0 carries T across the chunks.  Made of barriers: EVERY thread of the workgroup must reach the call, with the same m
__device__ __forceinline__ void pair_prefix_sums(const double *__restrict__ d, int64_t ld, const int32_t *a, int32_t m, const int32_t *sizes,
                                                 int32_t n_sizes, double *__restrict__ out, double *r, int32_t cap, int32_t tid) {
  const int wave = tid / kWave, lane = tid % kWave;
  double T = 0.0;
  int32_t k = 0;
  for (int32_t j0 = 1; j0 < m; j0 += cap) {
    const int32_t j1 = j0 + cap < m ? j0 + cap : m;
    for (int32_t j = j0 + wave; j < j1; j += kCcWaves) {
      const double *__restrict__ row = d + (int64_t)a[j] * ld;
      const double v = wave_ordered_sum<1>(j, lane, [&](int32_t i) { return row[a[i]]; });   // r_j; a: global memory or LDS
      if (lane == 0) r[j - j0] = v;
    }
    __syncthreads();
    if (tid == 0) {
      for (int32_t j = j0; j < j1; ++j) {
        T = j == 1 ? r[0] : T + r[j - j0];
        if (k < n_sizes && sizes[k] == j + 1) out[k++] = T;
      }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kCcThreads) void cc_lists_kernel(const double *__restrict__ d, int64_t ld, const int32_t *__restrict__ ptr,
                                                               const int32_t *__restrict__ idx, double *__restrict__ sum_out) {
  __shared__ double r[kCcRowChunk];
  __shared__ int32_t len;
  const int32_t c = blockIdx.x, tid = threadIdx.x;
  const int32_t b = ptr[c], m = ptr[c + 1] - b;   // uniform over the workgroup
  if (m < 2) {
    if (tid == 0) sum_out[c] = 0.0;
    return;
  }
  if (tid == 0) len = m;
  __syncthreads();
  pair_prefix_sums(d, ld, idx + b, m, &len, 1, sum_out + c, r, kCcRowChunk, tid);
}

// sample s0 + blockIdx.x.  LDS: key [cpad] then idx [cpad]
__global__ __launch_bounds__(kCcThreads) void cc_random_kernel(int32_t n, const double *__restrict__ d, int64_t ld, uint64_t seed, int64_t s0,
                                                                int32_t cpad, int32_t n_sizes, const int32_t *__restrict__ sizes, int32_t m_max,
                                                                double *__restrict__ sums_out, int32_t *__restrict__ perm_out) {
  extern __shared__ uint64_t cc_lds[];
  uint64_t *key = cc_lds;
  int32_t *idx = reinterpret_cast<int32_t *>(key + cpad);
  const int32_t tid = threadIdx.x;
  const uint64_t s = (uint64_t)(s0 + blockIdx.x);
  for (int32_t i = tid; i < cpad; i += kCcThreads) {
    key[i] = i < n ? perm_key(seed, kRngClassPerm, s, i) : kBehind;
    idx[i] = i;
  }
  __syncthreads();
  sort_pairs<kCcThreads>(key, idx, cpad, tid);
  if (perm_out)
    for (int32_t i = tid; i < m_max; i += kCcThreads) perm_out[(int64_t)blockIdx.x * m_max + i] = idx[i];
  // the keys have done their work: their LDS holds the row sums (m_max - 1 <= cpad of them, one chunk)
  pair_prefix_sums(d, ld, idx, m_max, sizes, n_sizes, sums_out + (int64_t)blockIdx.x * n_sizes, reinterpret_cast<double *>(key), cpad, tid);
}

int check_matrix(const char *who, int32_t n, const double *d, int64_t ld) {
  GSS_REQUIRE(d != nullptr, "%s: d is null", who);
  GSS_REQUIRE(ld >= n, "%s: ld=%lld is below n=%d", who, (long long)ld, n);
  return GSS_OK;
}

}  // namespace
}  // namespace gss

using namespace gss;

extern "C" {

int gss_pair_sums_lists(int32_t n, const double *d, int64_t ld, int32_t C, const int32_t *ptr, const int32_t *idx, double *sum_out, void *stream) {
  GSS_REQUIRE(n >= 1, "pair_sums_lists: n=%d must be >= 1", n);
  if (int rc = check_matrix("pair_sums_lists", n, d, ld)) return rc;
  GSS_REQUIRE(C >= 0, "pair_sums_lists: C=%d lists must be >= 0", C);
  if (C == 0) return GSS_OK;
  GSS_REQUIRE(ptr != nullptr, "pair_sums_lists: ptr is null");
  GSS_REQUIRE(sum_out != nullptr, "pair_sums_lists: sum_out is null");
  hipStream_t st = as_stream(stream);
  std::unique_ptr<int32_t[]> h;
  if (int rc = check_list_offsets("pair_sums_lists", ptr, C, st, h)) return rc;
  const int32_t total = h[C];
  if (total > 0) {   // nothing reads d through a list before every entry of it is known to be a row; the status words are freed before the launch
    GSS_REQUIRE(idx != nullptr, "pair_sums_lists: idx is null");
    DeviceBuf<uint32_t> status;
    if (int rc = status.alloc("pair_sums_lists", 8)) return rc;
    const CheckedList la{idx, total, 0, n, "idx", "n"}, none{nullptr, 0, 0, 0, "", ""};
    if (int rc = check_lists("pair_sums_lists", la, none, status.p, st)) return rc;
  }
  hipLaunchKernelGGL(cc_lists_kernel, dim3(C), dim3(kCcThreads), 0, st, d, ld, ptr, idx, sum_out);
  GSS_LAUNCH_CHECK("cc_lists_kernel");
  return GSS_OK;
}

int gss_pair_sums_random(int32_t n, const double *d, int64_t ld, uint64_t seed, int64_t s0, int32_t P, int32_t n_sizes, const int32_t *sizes,
                         double *sums_out, int32_t *perm_out, void *stream) {
  GSS_REQUIRE(n >= 2 && n <= kCcMaxN, "pair_sums_random: n=%d is outside [2, %d] (a sample's permutation is sorted in LDS)", n, kCcMaxN);
  if (int rc = check_matrix("pair_sums_random", n, d, ld)) return rc;
  GSS_REQUIRE(P >= 1, "pair_sums_random: P=%d samples must be >= 1", P);
  if (int rc = check_sample_window("pair_sums_random", s0, P)) return rc;
  GSS_REQUIRE(n_sizes >= 1 && n_sizes <= n - 1, "pair_sums_random: n_sizes=%d is outside [1, n - 1 = %d]", n_sizes, n - 1);
  GSS_REQUIRE(sizes != nullptr, "pair_sums_random: sizes is null");
  GSS_REQUIRE(sums_out != nullptr, "pair_sums_random: sums_out is null");
  hipStream_t st = as_stream(stream);
  std::unique_ptr<int32_t[]> h;
  char hi_words[32];
  snprintf(hi_words, sizeof(hi_words), "n=%d", n);
  if (int rc = check_sizes("pair_sums_random", sizes, n_sizes, 2, n, hi_words, st, h)) return rc;
  const int32_t cpad = pow2_at_least(n);
  hipLaunchKernelGGL(cc_random_kernel, dim3(P), dim3(kCcThreads), (size_t)cpad * 12, st, n, d, ld, seed, s0, cpad, n_sizes, sizes, h[n_sizes - 1],
                     sums_out, perm_out);
  GSS_LAUNCH_CHECK("cc_random_kernel");
  return GSS_OK;
}

}  // extern "C"

// matrix_mantel.hip -- the cross-product sum of two symmetric matrices under seeded relabellings of one of them (gss_matrix_cross_sums): the
// statistic and the permutation null of Mantel's test between two drug x drug matrices (mantel.py, drug_signatures.py).
//
// include/gssgcn.h has the contract, DESIGN.md section 9.14 the definitions, the cost model and the measurements.  For replicate s and the
// fp64 matrices a, b [n][n]:
//   out[s] = sum over 0 <= i < j < n of a[j][i] * b[pi_s(j)][pi_s(i)]
//   mode 0  plain   pi = the identity: the observed statistic, with the arithmetic of the null (one replicate);
//   mode 1  null    pi_s = perm_null.h's permutation under the tag kRngMantelPerm, sorted in LDS.
// The order of the additions is fixed:
//   r_j = sum over i < j of a[j][i] * b[pi(j)][pi(i)]   one wave per row j = 1 .. n - 1, in perm_null.h's fixed order (wave_ordered_sum),
//                                                        every product rounded on its own (the file is compiled with contraction off: no
//                                                        fused multiply-add);
//   T   = r_1 + r_2 + ... + r_{n-1}                     added in that order by one thread.
// So a replicate's bits are a function of (n, a, b, seed, s) alone: not of first / count, the grid or the other replicates of the call, and a
// numpy statement of the same additions reproduces them (tests/mantel_mirror.py).  Nothing is accumulated with atomics.
// One workgroup per replicate.  a is read along its rows (coalesced); b is gathered inside one row, pi(j), per wave, kMtAhead strides ahead
// of the additions.
#include "perm_null.h"

#pragma clang fp contract(off)   // the products of the row sum's terms

namespace gss {
namespace {

constexpr int kMtThreads = 256;
constexpr int kMtWaves = kMtThreads / kWave;
constexpr int kMtMaxN = 4096;         // pi is sorted in LDS: 4,096 x 12 B
constexpr int kMtAhead = 4;           // strides of a row whose loads are in flight before the first of their additions
constexpr int kMtMaxGrid = 1 << 20;   // replicates per launch

// replicate first + blockIdx.x.  LDS: key [cpad] then pi [cpad].  After the sort the keys' LDS holds the row sums: n - 1 <= cpad of them
__global__ __launch_bounds__(kMtThreads) void mantel_cross_kernel(int32_t n, const double *__restrict__ a, int64_t lda, const double *__restrict__ b,
                                                                   int64_t ldb, int32_t mode, uint64_t seed, int64_t first, int32_t cpad,
                                                                   double *__restrict__ out, int32_t *__restrict__ perm_out) {
  extern __shared__ uint64_t mt_lds[];
  uint64_t *key = mt_lds;
  int32_t *pi = reinterpret_cast<int32_t *>(key + cpad);
  const int32_t tid = threadIdx.x;
  const int wave = tid / kWave, lane = tid % kWave;
  const uint64_t s = (uint64_t)(first + blockIdx.x);
  for (int32_t i = tid; i < cpad; i += kMtThreads) {   // mode 0: every pair is padding and stays where it is
    key[i] = mode == 1 && i < n ? perm_key(seed, kRngMantelPerm, s, i) : kBehind;
    pi[i] = i;
  }
  __syncthreads();
  if (mode == 1) sort_pairs<kMtThreads>(key, pi, cpad, tid);   // uniform over the grid
  if (perm_out)
    for (int32_t i = tid; i < n; i += kMtThreads) perm_out[(int64_t)blockIdx.x * n + i] = pi[i];
  double *r = reinterpret_cast<double *>(key);
  for (int32_t j = 1 + wave; j < n; j += kMtWaves) {
    const double *__restrict__ arow = a + (int64_t)j * lda, *__restrict__ brow = b + (int64_t)pi[j] * ldb;
    const double v = wave_ordered_sum<kMtAhead>(j, lane, [&](int32_t i) { return arow[i] * brow[pi[i]]; });   // r_j
    if (lane == 0) r[j] = v;
  }
  __syncthreads();
  if (tid == 0) {
    double T = r[1];
#pragma unroll 8
    for (int32_t j = 2; j < n; ++j) T = T + r[j];
    out[blockIdx.x] = T;
  }
}

}  // namespace
}  // namespace gss

using namespace gss;

extern "C" {

int gss_matrix_cross_sums(int32_t n, const double *a, int64_t lda, const double *b, int64_t ldb, int32_t mode, uint64_t seed, int64_t first,
                          int64_t count, double *out, int32_t *perm_out, void *stream) {
  GSS_REQUIRE(n >= 2 && n <= kMtMaxN, "matrix_cross_sums: n=%d is outside [2, %d] (a replicate's permutation is sorted in LDS)", n, kMtMaxN);
  GSS_REQUIRE(lda >= n, "matrix_cross_sums: lda=%lld is below n=%d", (long long)lda, n);
  GSS_REQUIRE(ldb >= n, "matrix_cross_sums: ldb=%lld is below n=%d", (long long)ldb, n);
  GSS_REQUIRE(mode >= 0 && mode <= 1, "matrix_cross_sums: mode=%d is unknown (0 = plain, 1 = permuted)", mode);
  GSS_REQUIRE(count >= 0, "matrix_cross_sums: count=%lld replicates must be >= 0", (long long)count);
  GSS_REQUIRE(mode != 0 || (first == 0 && count == 1), "matrix_cross_sums: mode 0 (plain) has one replicate: first=%lld, count=%lld must be 0, 1",
              (long long)first, (long long)count);
  GSS_REQUIRE(first >= 0 && first <= ((int64_t)1 << 31) && count <= ((int64_t)1 << 31) - first,
              "matrix_cross_sums: replicates first=%lld, count=%lld reach outside [0, 2^31]", (long long)first, (long long)count);
  if (count == 0) return GSS_OK;
  GSS_REQUIRE(a != nullptr, "matrix_cross_sums: a is null");
  GSS_REQUIRE(b != nullptr, "matrix_cross_sums: b is null");
  GSS_REQUIRE(out != nullptr, "matrix_cross_sums: out is null");
  hipStream_t st = as_stream(stream);
  const int32_t cpad = pow2_at_least(n);
  for (int64_t r0 = 0; r0 < count; r0 += kMtMaxGrid) {
    const unsigned g = (unsigned)(count - r0 < kMtMaxGrid ? count - r0 : kMtMaxGrid);
    hipLaunchKernelGGL(mantel_cross_kernel, dim3(g), dim3(kMtThreads), (size_t)cpad * 12, st, n, a, lda, b, ldb, mode, seed, first + r0, cpad,
                       out + r0, perm_out ? perm_out + r0 * n : nullptr);
    GSS_LAUNCH_CHECK("mantel_cross_kernel");
  }
  return GSS_OK;
}

}  // extern "C"

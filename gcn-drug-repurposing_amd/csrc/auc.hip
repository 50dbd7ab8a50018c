// auc.hip -- batched ROC-AUC, one query per row (evaluate_auc.py:156-170: sklearn.metrics.roc_auc_score per indication over all drugs).
//
// One workgroup per row (include/gssgcn.h has the contract; DESIGN.md section 9.4 the cost model and the measured stage times of evaluate_auc.py).  The row's
// positives are marked in an LDS bitmap (an LDS atomicOr per entry also finds a repeated column); every score becomes an order-preserving
// uint64 key (-0.0 folded into +0.0 first), the negatives' keys are sorted in LDS (bitonic; the positives get the all-ones key and sort
// behind them), and each positive counts the negatives below it and tied with it by two binary searches:
//   2 U = sum over positives of (lower_bound + upper_bound) = sum of (2 * below + tied),   AUC = 2 U / (2 P N)
// which is the average-rank (Mann-Whitney) form of roc_auc_score.  The counts are integers, so the result depends only on the multiset
// of (score, label) pairs; every output word is written by the one thread that owns it (no atomics on results: bitwise deterministic).
#include <new>

#include "common.h"

namespace gss {
namespace {

constexpr int kAucThreads = 256;
constexpr int kMaxCols = 16384;                 // the sort buffer: pow2ceil(C) keys of 8 bytes in LDS (128 KiB at the limit)
constexpr uint64_t kBehind = ~0ull;             // the key of positives and padding: above every finite score's key

// per-row refusal, written to n_pos[r] as -code with the offending column in n_neg[r]
enum AucRefusal { kBadPtr = 1, kColRange = 2, kColRepeat = 3, kNonFinite = 4 };

__host__ __device__ inline int64_t pow2_at_least(int64_t c) {
  int64_t p = 64;
  while (p < c) p <<= 1;
  return p;
}

__device__ __forceinline__ bool finite_bits(uint64_t b) { return (b & 0x7ff0000000000000ull) != 0x7ff0000000000000ull; }

// order-preserving key of a finite double; +0.0 and -0.0 are one value
__device__ __forceinline__ uint64_t score_key(double x) {
  const uint64_t b = (uint64_t)__double_as_longlong(x == 0.0 ? 0.0 : x);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

// first index in [0, n) whose key is >= k (strict = false) or > k (strict = true)
__device__ __forceinline__ int32_t search(const uint64_t *key, int32_t n, uint64_t k, bool strict) {
  int32_t lo = 0, hi = n;
  while (lo < hi) {
    const int32_t mid = (lo + hi) >> 1;
    const uint64_t m = key[mid];
    if (strict ? m <= k : m < k) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(kAucThreads) void auc_rows_kernel(int32_t C, int32_t cpad, const double *__restrict__ scores, int64_t ld,
                                                               const int32_t *__restrict__ pos_ptr, const int32_t *__restrict__ pos_col,
                                                               double *__restrict__ auc, int32_t *__restrict__ n_pos,
                                                               int32_t *__restrict__ n_neg) {
  extern __shared__ __align__(16) unsigned char lds[];
  uint64_t *key = reinterpret_cast<uint64_t *>(lds);                     // [cpad]
  uint32_t *is_pos = reinterpret_cast<uint32_t *>(lds + (size_t)cpad * 8);  // [cpad / 32] bitmap
  __shared__ int32_t bad_range, bad_repeat, bad_finite;
  __shared__ unsigned long long partial[kAucThreads / kWave];
  const int32_t r = blockIdx.x, tid = threadIdx.x;
  const double *row = scores + (int64_t)r * ld;
  const int32_t b = pos_ptr[r], e = pos_ptr[r + 1];
  const int32_t P = e - b;
  if (b < 0 || P < 0 || P > C || (r == 0 && b != 0)) {   // uniform: every thread read the same two words
    if (tid == 0) {
      auc[r] = __longlong_as_double(0x7ff8000000000000ll);
      n_pos[r] = -kBadPtr;
      n_neg[r] = P;
    }
    return;
  }
  if (tid == 0) {
    bad_range = INT32_MAX;
    bad_repeat = INT32_MAX;
    bad_finite = INT32_MAX;
  }
  for (int32_t w = tid; w < cpad / 32; w += kAucThreads) is_pos[w] = 0u;
  __syncthreads();
  for (int32_t k = tid; k < P; k += kAucThreads) {
    const int32_t c = pos_col[b + k];
    if (c < 0 || c >= C) {
      atomicMin(&bad_range, k);     // the first offending entry in list order
      continue;
    }
    const uint32_t bit = 1u << (c & 31);
    if (atomicOr(&is_pos[c >> 5], bit) & bit) atomicMin(&bad_repeat, c);
  }
  __syncthreads();
  for (int32_t c = tid; c < cpad; c += kAucThreads) {
    uint64_t k = kBehind;
    if (c < C) {
      const double x = row[c];
      if (!finite_bits((uint64_t)__double_as_longlong(x))) atomicMin(&bad_finite, c);
      else if (!((is_pos[c >> 5] >> (c & 31)) & 1u)) k = score_key(x);
    }
    key[c] = k;
  }
  __syncthreads();
  const int32_t N = C - P;
  if (bad_range != INT32_MAX || bad_repeat != INT32_MAX || bad_finite != INT32_MAX || P == 0 || N == 0) {
    if (tid == 0) {
      auc[r] = __longlong_as_double(0x7ff8000000000000ll);
      if (bad_range != INT32_MAX) {
        n_pos[r] = -kColRange;
        n_neg[r] = pos_col[b + bad_range];
      } else if (bad_repeat != INT32_MAX) {
        n_pos[r] = -kColRepeat;
        n_neg[r] = bad_repeat;
      } else if (bad_finite != INT32_MAX) {
        n_pos[r] = -kNonFinite;
        n_neg[r] = bad_finite;
      } else {
        n_pos[r] = P;
        n_neg[r] = N;
      }
    }
    return;
  }
  // bitonic sort of the cpad keys, ascending: the N negatives' keys come first
  for (int32_t k = 2; k <= cpad; k <<= 1) {
    for (int32_t j = k >> 1; j > 0; j >>= 1) {
      for (int32_t i = tid; i < cpad / 2; i += kAucThreads) {
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
  unsigned long long twice_u = 0;
  for (int32_t k = tid; k < P; k += kAucThreads) {
    const uint64_t kp = score_key(row[pos_col[b + k]]);
    twice_u += (unsigned long long)search(key, N, kp, false) + (unsigned long long)search(key, N, kp, true);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) twice_u += __shfl_xor(twice_u, o, kWave);
  if ((tid & (kWave - 1)) == 0) partial[tid / kWave] = twice_u;
  __syncthreads();
  if (tid == 0) {
    unsigned long long s = 0;
    for (int w = 0; w < kAucThreads / kWave; ++w) s += partial[w];
    auc[r] = (double)s / (2.0 * (double)P * (double)N);   // s < 2^53 and 2 P N < 2^53: exact operands, one rounding
    n_pos[r] = P;
    n_neg[r] = N;
  }
}

}  // namespace
}  // namespace gss

using namespace gss;

extern "C" {

int gss_auc_rows(int32_t R, int32_t C, const double *scores, int64_t ld, const int32_t *pos_ptr, const int32_t *pos_col, double *auc,
                 int32_t *n_pos, int32_t *n_neg, void *stream) {
  GSS_REQUIRE(R >= 0, "auc_rows: R=%d rows must be >= 0", R);
  GSS_REQUIRE(C >= 1, "auc_rows: C=%d candidates must be >= 1", C);
  GSS_REQUIRE(C <= kMaxCols, "auc_rows: C=%d candidates is above the limit of %d per row (one workgroup sorts a row in LDS)", C, kMaxCols);
  GSS_REQUIRE(ld >= C, "auc_rows: ld=%lld is below C=%d", (long long)ld, C);
  if (R == 0) return GSS_OK;
  GSS_REQUIRE(scores && pos_ptr && pos_col && auc && n_pos && n_neg, "auc_rows: null argument");
  hipStream_t st = as_stream(stream);
  const int32_t cpad = (int32_t)pow2_at_least(C);
  const size_t lds = (size_t)cpad * 8 + (size_t)cpad / 8;
  hipLaunchKernelGGL(auc_rows_kernel, dim3(R), dim3(kAucThreads), lds_request(auc_rows_kernel, lds), st, C, cpad, scores, ld, pos_ptr,
                     pos_col, auc, n_pos, n_neg);
  GSS_LAUNCH_CHECK("auc_rows_kernel");
  // the refusals come back in the count words: -code in n_pos, the column in n_neg
  int32_t *h = new (std::nothrow) int32_t[(size_t)2 * R];
  if (!h) return fail(GSS_ENOMEM, "auc_rows: host status buffer of %d rows", R);
  hipError_t e1 = hipMemcpyAsync(h, n_pos, (size_t)R * 4, hipMemcpyDeviceToHost, st);
  hipError_t e2 = e1 == hipSuccess ? hipMemcpyAsync(h + R, n_neg, (size_t)R * 4, hipMemcpyDeviceToHost, st) : e1;
  hipError_t e3 = e2 == hipSuccess ? hipStreamSynchronize(st) : e2;
  int rc = GSS_OK;
  if (e3 != hipSuccess) rc = fail(GSS_EHIP, "auc_rows: reading the row status failed: %s", hipGetErrorString(e3));
  for (int32_t r = 0; rc == GSS_OK && r < R; ++r) {
    const int32_t code = -h[r], col = h[R + r];
    if (code == kBadPtr)
      rc = fail(GSS_EINVAL, "auc_rows: row %d: pos_ptr is not a CSR row pointer (0 first, non-decreasing, at most C=%d per row; %d here)", r, C, col);
    else if (code == kColRange)
      rc = fail(GSS_EINVAL, "auc_rows: row %d: pos_col %d is outside [0, %d)", r, col, C);
    else if (code == kColRepeat)
      rc = fail(GSS_EINVAL, "auc_rows: row %d: pos_col %d is repeated", r, col);
    else if (code == kNonFinite)
      rc = fail(GSS_EINVAL, "auc_rows: row %d, column %d: the score is NaN or infinite (roc_auc_score refuses it)", r, col);
  }
  delete[] h;
  return rc;
}

}  // extern "C"

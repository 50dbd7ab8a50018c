// resample.hip -- the mean and the median of resampled series (gss_resample_stats): the bootstrap replicates and the sign-flip null behind
// the intervals and the paired tests of the per-indication metrics (resample.py, compare_methods.py, evaluate_auc.py --bootstrap).
//
// include/gssgcn.h has the contract, DESIGN.md section 9.13 the definitions, the cost model and the measurements.  Replicate b of series s
// is a multiset of n values of the series (counter_rng.h gives the randomness: nothing is stored between draws):
//   mode 0  plain       v[s][j], j < n                                                  -- the observed statistic, with the arithmetic of the nulls
//   mode 1  bootstrap   v[s][idx(b, j)], idx(b, j) = ((rng_key(seed, kRngBootDraw, b, j, 0) >> 32) * n) >> 32   (64-bit integers; in [0, n))
//   mode 2  sign flip   -v[s][j] if the top bit of rng_key(seed, kRngSignFlip, b, j, 0) is set, else v[s][j]
// idx and the sign do not depend on s: one replicate draws the same places, or flips the same places, in every series of the call.
// One workgroup per replicate walks the S series: the multiset becomes order_keys (rank_keys.h), padded with kBehind to a power of two,
// sorted ascending in LDS by rank_keys.h's network, and read back as the sorted values x_0 <= ... <= x_{n-1}.
//   median = x_{(n-1)/2} for odd n, (x_{n/2-1} + x_{n/2}) * 0.5 for even n                                        (np.median's arithmetic)
//   mean   = T / n, T added in an order that is a function of the sorted values alone:
//            p_t = x_t + x_{t+256} + x_{t+512} + ... in ascending order from +0.0, t = 0 .. 255     (thread t of the first four waves)
//            W_w = the butterfly of wave_sum_d over p_{64 w} .. p_{64 w + 63} (p_l += p_{l ^ o}, o = 32, 16, 8, 4, 2, 1), w = 0 .. 3
//            T   = ((W_0 + W_1) + W_2) + W_3                                                          (one thread walks the waves)
// So a replicate's bits depend on (seed, mode, b, n, the series' values) and on nothing else: not on first / count, not on S or the other
// series, not on the grid or the workgroup's size.  Nothing is accumulated with atomics.  order_key folds -0.0 into +0.0, so the sorted
// values hold no -0.0: results are defined up to the sign of a zero (a mean can still round to -0.0 from a negative denormal sum).
// A value that is not finite is found by a pass of its own before anything is resampled (rs_check_kernel: the least offending place, by
// an atomicMin on a status word that no result is made of), so a refused call writes nothing.
#include "rank_keys.h"

#include "counter_rng.h"

namespace gss {
namespace {

constexpr int kRsMaxN = 16384;           // the keys of one series sorted in LDS: 128 KiB, the chunk of profile_rank.hip
constexpr int kRsSmallThreads = 256;     // up to kRsSmallPad keys: 16 KiB of LDS at most, several workgroups per CU
constexpr int kRsSmallPad = 2048;
constexpr int kRsBigThreads = 1024;      // above: 16 waves, one workgroup per CU at 128 KiB
constexpr int kRsSumThreads = 256;       // the mean's partial sums: the first four waves, whatever the workgroup's size
constexpr int kRsSumWaves = kRsSumThreads / kWave;
constexpr int kRsMaxGrid = 1 << 20;      // replicates per launch (workgroups x threads stays below 2^32)
constexpr int kRsCheckThreads = 256;
constexpr int kRsCheckBlocks = 1024;

// order_key's inverse on the keys of finite values
__device__ __forceinline__ double key_value(uint64_t k) {
  return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

// the least e = s * n + j whose value v[s][j] is not finite -> *status (~0 before: none)
__global__ __launch_bounds__(kRsCheckThreads) void rs_check_kernel(const double *__restrict__ v, int64_t ld, int64_t total, int32_t n,
                                                                   unsigned long long *__restrict__ status) {
  for (int64_t e = (int64_t)blockIdx.x * kRsCheckThreads + threadIdx.x; e < total; e += (int64_t)gridDim.x * kRsCheckThreads) {
    const int64_t s = e / n, j = e - s * n;
    if (!finite_bits((uint64_t)__double_as_longlong(v[s * ld + j]))) atomicMin(status, (unsigned long long)e);
  }
}

// replicate first + blockIdx.x of every series.  LDS: key [cpad]
template <int THREADS>
__global__ __launch_bounds__(THREADS) void rs_stats_kernel(const double *__restrict__ v, int64_t ld, int32_t S, int32_t n, int32_t mode,
                                                           uint64_t seed, int64_t first, int32_t cpad, double *__restrict__ out) {
  extern __shared__ uint64_t rs_key[];
  __shared__ double wave_total[kRsSumWaves];
  uint64_t *key = rs_key;
  const int32_t tid = threadIdx.x;
  const uint64_t b = (uint64_t)(first + blockIdx.x);
  double *__restrict__ o = out + (int64_t)blockIdx.x * S * 2;
  for (int32_t s = 0; s < S; ++s) {   // S, n and cpad are uniform: every thread reaches every barrier
    const double *__restrict__ row = v + (int64_t)s * ld;
    for (int32_t i = tid; i < cpad; i += THREADS) {
      uint64_t k = kBehind;
      if (i < n) {
        double x;
        if (mode == 1) {
          const uint64_t h = rng_key(seed, kRngBootDraw, b, (uint64_t)i, 0);
          x = row[((h >> 32) * (uint64_t)n) >> 32];
        } else {
          x = row[i];
          if (mode == 2 && (rng_key(seed, kRngSignFlip, b, (uint64_t)i, 0) >> 63)) x = -x;
        }
        k = order_key(x);
      }
      key[i] = k;
    }
    __syncthreads();
    sort_keys<THREADS>(key, cpad, tid);
    if (tid < kRsSumThreads) {   // whole waves: THREADS is a multiple of kRsSumThreads
      double p = 0.0;
      for (int32_t i = tid; i < n; i += kRsSumThreads) p += key_value(key[i]);
      p = wave_sum_d(p);
      if ((tid & (kWave - 1)) == 0) wave_total[tid / kWave] = p;
    }
    __syncthreads();
    if (tid == 0) {
      double T = wave_total[0];
#pragma unroll
      for (int w = 1; w < kRsSumWaves; ++w) T += wave_total[w];
      o[2 * s] = __ddiv_rn(T, (double)n);
      o[2 * s + 1] = (n & 1) ? key_value(key[n >> 1]) : (key_value(key[(n >> 1) - 1]) + key_value(key[n >> 1])) * 0.5;
    }
    __syncthreads();   // the next series overwrites the keys and the waves' sums
  }
}

}  // namespace
}  // namespace gss

using namespace gss;

extern "C" {

int gss_resample_stats(const double *v, int64_t ld, int32_t S, int32_t n, int32_t mode, uint64_t seed, int64_t first, int64_t count, double *out,
                       void *stream) {
  static_assert(kRsSmallThreads % kRsSumThreads == 0 && kRsBigThreads % kRsSumThreads == 0, "the mean's four waves are whole waves of every workgroup");
  GSS_REQUIRE(n >= 1 && n <= kRsMaxN, "resample_stats: n=%d is outside [1, %d] (a series is sorted in LDS)", n, kRsMaxN);
  GSS_REQUIRE(S >= 1, "resample_stats: S=%d series must be >= 1", S);
  GSS_REQUIRE(ld >= n, "resample_stats: ld=%lld is below n=%d", (long long)ld, n);
  GSS_REQUIRE(mode >= 0 && mode <= 2, "resample_stats: mode=%d is unknown (0 = plain, 1 = bootstrap, 2 = sign flip)", mode);
  GSS_REQUIRE(count >= 0, "resample_stats: count=%lld replicates must be >= 0", (long long)count);
  GSS_REQUIRE(mode != 0 || (first == 0 && count == 1), "resample_stats: mode 0 (plain) has one replicate: first=%lld, count=%lld must be 0, 1",
              (long long)first, (long long)count);
  GSS_REQUIRE(first >= 0 && first <= ((int64_t)1 << 31) && count <= ((int64_t)1 << 31) - first,
              "resample_stats: replicates first=%lld, count=%lld reach outside [0, 2^31]", (long long)first, (long long)count);
  if (count == 0) return GSS_OK;
  GSS_REQUIRE(v != nullptr, "resample_stats: v is null");
  GSS_REQUIRE(out != nullptr, "resample_stats: out is null");
  hipStream_t st = as_stream(stream);
  {   // nothing is resampled, and nothing written, before every value is known to be finite
    DeviceBuf<unsigned long long> status;
    unsigned long long h = 0;
    const int64_t total = (int64_t)S * n;
    const int64_t blocks = (total + kRsCheckThreads - 1) / kRsCheckThreads;
    if (int rc = status.alloc("resample_stats", 8)) return rc;
    GSS_HIP(hipMemsetAsync(status.p, 0xff, 8, st));
    hipLaunchKernelGGL(rs_check_kernel, dim3((unsigned)(blocks < kRsCheckBlocks ? blocks : kRsCheckBlocks)), dim3(kRsCheckThreads), 0, st, v, ld,
                       total, n, status.p);
    GSS_LAUNCH_CHECK("rs_check_kernel");
    if (int rc = read_back(&h, status.p, 8, st)) return rc;
    GSS_REQUIRE(h == ~0ull, "resample_stats: series %lld, position %lld: the value is NaN or infinite", (long long)(h / (uint64_t)n),
                (long long)(h % (uint64_t)n));
  }
  const int32_t cpad = pow2_at_least(n);
  const size_t lds = (size_t)cpad * 8;
  const size_t lds_big = lds_request(rs_stats_kernel<kRsBigThreads>, lds);
  for (int64_t r0 = 0; r0 < count; r0 += kRsMaxGrid) {
    const unsigned g = (unsigned)(count - r0 < kRsMaxGrid ? count - r0 : kRsMaxGrid);
    double *o = out + r0 * S * 2;
    if (cpad <= kRsSmallPad)
      hipLaunchKernelGGL(rs_stats_kernel<kRsSmallThreads>, dim3(g), dim3(kRsSmallThreads), lds, st, v, ld, S, n, mode, seed, first + r0, cpad, o);
    else
      hipLaunchKernelGGL(rs_stats_kernel<kRsBigThreads>, dim3(g), dim3(kRsBigThreads), lds_big, st, v, ld, S, n, mode, seed, first + r0, cpad, o);
    GSS_LAUNCH_CHECK("rs_stats_kernel");
  }
  return GSS_OK;
}

}  // extern "C"

// profile_dist.hip -- pairwise distances between diffusion profiles (columns of the fp64 matrix gss_ppr_run leaves on the device).
//
// "By comparing the diffusion profiles of a drug and a disease, the multiscale interactome predicts whether the drug treats the disease"
// (multiscale/README.md, overview (c)); the reference never compares two profiles.  include/gssgcn.h has the contract, DESIGN.md section 9.6 the
// cost model and the measurements.  Five metrics with scipy.spatial.distance.cdist's definitions, two kernel classes:
//
//   difference class (cityblock, euclidean, canberra): no product form exists.  A workgroup owns a 64 x 64 tile of outputs and walks the N rows in
//   slabs of 32: the slab of both column panels is staged in LDS (the next one is already in flight in registers), every thread keeps a 4 x 4 block
//   of accumulators and adds its 16 terms row by row.
//   dot class (cosine, correlation): the Gram product of the two panels on the fp64 matrix cores (v_mfma_f64_16x16x4_f64; a wave owns 32 x 32 outputs
//   as 2 x 2 MFMA blocks and reads its operands straight from the matrix, 16 adjacent columns of 4 rows per load), after a pass of its own that
//   gives every listed column its mean (correlation; 0 for cosine) and the norm of the centred column.  The mean is subtracted as the operand is
//   read: true two-pass centring.
//
// Order: every output sums the rows 0, 1, ... N - 1 in that order (the MFMA takes them four at a time, always the same four), whatever na, nb, the
// grid or the pair's place in its tile; the row range is never split across workgroups and nothing is accumulated with atomics.  So two runs are
// bit-equal, out(a, b) == out(b, a) bit for bit (|a - b|, (a - b)^2, |a| + |b| and a * b do not depend on the order of their operands), a pair has the
// same bits alone and inside a large call, and dist(c, c) of the difference class is exactly 0.0.
//
// Column lists: a thread that stages or reads column cols[i] adds that offset to a row pointer once; the loads of adjacent lanes coalesce by
// address, so an ascending contiguous list costs what the null list (0 .. n - 1) costs, and a scattered one pays only for the lines it touches.
#include "common.h"

namespace gss {
namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int kPdTile = 64;       // outputs per workgroup: 64 x 64
constexpr int kPdSlab = 32;       // rows per staged slab (difference class): 2 panels x 32 x 64 x 8 bytes = 32 KiB of LDS
constexpr int kPdThreads = 256;
constexpr uint32_t kNoBad = 0xffffffffu;
constexpr int kPdMaxList = 1 << 21;   // 32,768 tiles per grid dimension

__device__ __forceinline__ int32_t col_at(const int32_t *cols, int32_t i) { return cols ? cols[i] : i; }

// status[0] / status[1]: the first entry of cols_a / cols_b outside [0, ld) (kNoBad = none); the host set both words to kNoBad
__global__ __launch_bounds__(kPdThreads) void pd_check_cols_kernel(int32_t na, const int32_t *__restrict__ cols_a, int32_t nb,
                                                                    const int32_t *__restrict__ cols_b, int64_t ld, uint32_t *__restrict__ status) {
  const int32_t t = blockIdx.x * kPdThreads + threadIdx.x;
  if (cols_a && t < na) {
    const int32_t c = cols_a[t];
    if (c < 0 || c >= ld) atomicMin(&status[0], (uint32_t)t);
  }
  if (cols_b && t < nb) {
    const int32_t c = cols_b[t];
    if (c < 0 || c >= ld) atomicMin(&status[1], (uint32_t)t);
  }
}

// one thread per list entry (a's entries, then b's): mean[e] (0 unless centre) and norm[e] = sqrt(sum_k (x[k][c] - mean)^2), rows in order
__global__ __launch_bounds__(kPdThreads) void pd_stats_kernel(int32_t n, const double *__restrict__ x, int64_t ld, int32_t na,
                                                               const int32_t *__restrict__ cols_a, int32_t nb, const int32_t *__restrict__ cols_b,
                                                               int centre, double *__restrict__ mean, double *__restrict__ norm) {
  const int32_t e = blockIdx.x * kPdThreads + threadIdx.x;
  if (e >= na + nb) return;
  const double *p = x + (e < na ? col_at(cols_a, e) : col_at(cols_b, e - na));
  double m = 0.0;
  if (centre) {
    double s = 0.0;
#pragma unroll 8
    for (int32_t k = 0; k < n; ++k) s += p[(int64_t)k * ld];
    m = s / (double)n;
  }
  double ss = 0.0;
#pragma unroll 8
  for (int32_t k = 0; k < n; ++k) {
    const double d = p[(int64_t)k * ld] - m;
    ss += d * d;
  }
  mean[e] = m;
  norm[e] = sqrt(ss);
}

// ---- dot class --------------------------------------------------------------------------------------------------------------------------------
// wave w of a workgroup: outputs [i0, i0 + 32) x [j0, j0 + 32) as acc[s][t], s / t = 16-wide block of a / b columns.  Lane (c = lane & 15, q = lane >> 4)
// supplies row k + q of column block entry c for both operands (A[i = c][k = q], B[k = q][j = c]); D: col = c, row = q + 4 * reg.
__global__ __launch_bounds__(kPdThreads) void pd_dot_kernel(int32_t n, const double *__restrict__ x, int64_t ld, int32_t na,
                                                             const int32_t *__restrict__ cols_a, int32_t nb, const int32_t *__restrict__ cols_b,
                                                             const double *__restrict__ mean, const double *__restrict__ norm,
                                                             double *__restrict__ out, int64_t ld_out) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int c = lane & 15, q = lane >> 4;
  const int32_t i0 = blockIdx.y * kPdTile + (w >> 1) * 32, j0 = blockIdx.x * kPdTile + (w & 1) * 32;
  if (i0 >= na || j0 >= nb) return;   // wave-uniform; the kernel has no barrier
  const double *pa[2], *pb[2];
  double ma[2], mb[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int32_t ia = min(na - 1, i0 + 16 * t + c), jb = min(nb - 1, j0 + 16 * t + c);   // a tail block reads the last column again and stores nothing
    pa[t] = x + col_at(cols_a, ia);
    pb[t] = x + col_at(cols_b, jb);
    ma[t] = mean[ia];
    mb[t] = mean[na + jb];
  }
  f64x4 acc[2][2];
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int t = 0; t < 2; ++t) acc[s][t] = (f64x4){0.0, 0.0, 0.0, 0.0};
  int32_t k = 0;
#pragma unroll 4
  for (; k + 4 <= n; k += 4) {
    const int64_t ro = (int64_t)(k + q) * ld;
    const double a0 = pa[0][ro] - ma[0], a1 = pa[1][ro] - ma[1];
    const double b0 = pb[0][ro] - mb[0], b1 = pb[1][ro] - mb[1];
    acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
    acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
    acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
    acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
  }
  if (k < n) {   // the last 1..3 rows: the rows past N enter as 0 * 0 (the same for every pair, so the order still depends on N alone)
    const bool live = k + q < n;
    const int64_t ro = (int64_t)(live ? k + q : 0) * ld;
    const double a0 = live ? pa[0][ro] - ma[0] : 0.0, a1 = live ? pa[1][ro] - ma[1] : 0.0;
    const double b0 = live ? pb[0][ro] - mb[0] : 0.0, b1 = live ? pb[1][ro] - mb[1] : 0.0;
    acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
    acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
    acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
    acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
  }
  // scipy's cosine: 1 - clip(u.v / (|u| |v|), -1, 1); a zero norm gives 0 / 0 = NaN, which the clip passes on
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int32_t j = j0 + 16 * t + c;
    if (j >= nb) continue;
    const double nj = norm[na + j];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int32_t i = i0 + 16 * s + q + 4 * r;
        if (i >= na) continue;
        double cs = acc[s][t][r] / (norm[i] * nj);
        if (fabs(cs) > 1.0) cs = copysign(1.0, cs);
        out[(int64_t)i * ld_out + j] = 1.0 - cs;
      }
  }
}

// ---- difference class -------------------------------------------------------------------------------------------------------------------------
template <int kMetric>
__device__ __forceinline__ double pd_term(double a, double b) {
  if (kMetric == GSS_DIST_CITYBLOCK) return fabs(a - b);
  if (kMetric == GSS_DIST_EUCLIDEAN) {
    const double d = a - b;
    return d * d;
  }
  const double den = fabs(a) + fabs(b);          // canberra: a term with a = b = 0 contributes 0 (scipy's rule)
  const double t = fabs(a - b) / den;
  return den > 0.0 ? t : 0.0;
}

// thread (ty = tid >> 4, tx = tid & 15): outputs (i0 + 4 ty + u, j0 + 4 tx + v).  Staging: thread tid loads column tid & 63 of both panels for the
// slab's rows (tid >> 6) + 4 m.
template <int kMetric>
__global__ __launch_bounds__(kPdThreads) void pd_diff_kernel(int32_t n, const double *__restrict__ x, int64_t ld, int32_t na,
                                                              const int32_t *__restrict__ cols_a, int32_t nb, const int32_t *__restrict__ cols_b,
                                                              double *__restrict__ out, int64_t ld_out) {
  __shared__ __align__(16) double sa[kPdSlab][kPdTile];
  __shared__ __align__(16) double sb[kPdSlab][kPdTile];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4, lc = tid & 63, lr = tid >> 6;
  const int32_t i0 = blockIdx.y * kPdTile, j0 = blockIdx.x * kPdTile;
  const double *ga = x + col_at(cols_a, min(na - 1, i0 + lc));   // a tail tile stages the last column again and stores nothing for it
  const double *gb = x + col_at(cols_b, min(nb - 1, j0 + lc));
  constexpr int kPer = kPdSlab / 4;   // slab rows per staging thread
  double ra[kPer], rb[kPer];
  auto fetch = [&](int32_t k0) {
#pragma unroll
    for (int m = 0; m < kPer; ++m) {
      const int32_t k = k0 + lr + 4 * m;
      const bool live = k < n;
      ra[m] = live ? ga[(int64_t)k * ld] : 0.0;
      rb[m] = live ? gb[(int64_t)k * ld] : 0.0;
    }
  };
  double acc[4][4];
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int v = 0; v < 4; ++v) acc[u][v] = 0.0;
  fetch(0);
  for (int32_t k0 = 0; k0 < n; k0 += kPdSlab) {
#pragma unroll
    for (int m = 0; m < kPer; ++m) {
      sa[lr + 4 * m][lc] = ra[m];
      sb[lr + 4 * m][lc] = rb[m];
    }
    __syncthreads();
    if (k0 + kPdSlab < n) fetch(k0 + kPdSlab);   // in flight while this slab is summed
    const int rows = min(kPdSlab, n - k0);        // uniform; rows past N are never added
    if (rows == kPdSlab) {
#pragma unroll 8
      for (int r = 0; r < kPdSlab; ++r) {
        double a[4], b[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) a[u] = sa[r][4 * ty + u];
#pragma unroll
        for (int v = 0; v < 4; ++v) b[v] = sb[r][4 * tx + v];
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int v = 0; v < 4; ++v) acc[u][v] += pd_term<kMetric>(a[u], b[v]);
      }
    } else {
      for (int r = 0; r < rows; ++r) {
        double a[4], b[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) a[u] = sa[r][4 * ty + u];
#pragma unroll
        for (int v = 0; v < 4; ++v) b[v] = sb[r][4 * tx + v];
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int v = 0; v < 4; ++v) acc[u][v] += pd_term<kMetric>(a[u], b[v]);
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int32_t i = i0 + 4 * ty + u;
    if (i >= na) continue;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int32_t j = j0 + 4 * tx + v;
      if (j < nb) out[(int64_t)i * ld_out + j] = kMetric == GSS_DIST_EUCLIDEAN ? sqrt(acc[u][v]) : acc[u][v];
    }
  }
}

struct DeviceScratch {   // freed on every way out of the call
  void *p = nullptr;
  ~DeviceScratch() {
    if (p) (void)hipFree(p);
  }
};

}  // namespace
}  // namespace gss

using namespace gss;

extern "C" {

int gss_profile_dist(int32_t n, const double *x, int64_t ld, int32_t na, const int32_t *cols_a, int32_t nb, const int32_t *cols_b,
                     int32_t metric, double *out, int64_t ld_out, void *stream) {
  GSS_REQUIRE(x != nullptr, "profile_dist: x is null");
  GSS_REQUIRE(out != nullptr, "profile_dist: out is null");
  GSS_REQUIRE(n >= 1, "profile_dist: n=%d rows must be >= 1", n);
  GSS_REQUIRE(na >= 0 && nb >= 0, "profile_dist: na=%d, nb=%d must be >= 0", na, nb);
  GSS_REQUIRE(na <= kPdMaxList && nb <= kPdMaxList, "profile_dist: na=%d, nb=%d is above the limit of %d columns per list", na, nb, kPdMaxList);
  GSS_REQUIRE(metric >= GSS_DIST_CITYBLOCK && metric <= GSS_DIST_CORRELATION,
              "profile_dist: metric %d is unknown (0 cityblock, 1 euclidean, 2 canberra, 3 cosine, 4 correlation)", metric);
  GSS_REQUIRE(ld >= 1, "profile_dist: ld=%lld must be >= 1", (long long)ld);
  GSS_REQUIRE(cols_a || na <= ld, "profile_dist: ld=%lld is below na=%d (cols_a is null: columns 0 .. na - 1)", (long long)ld, na);
  GSS_REQUIRE(cols_b || nb <= ld, "profile_dist: ld=%lld is below nb=%d (cols_b is null: columns 0 .. nb - 1)", (long long)ld, nb);
  GSS_REQUIRE(ld_out >= nb, "profile_dist: ld_out=%lld is below nb=%d", (long long)ld_out, nb);
  if (na == 0 || nb == 0) return GSS_OK;
  hipStream_t st = as_stream(stream);
  const bool dot = metric == GSS_DIST_COSINE || metric == GSS_DIST_CORRELATION;
  const bool lists = cols_a || cols_b;
  // scratch: the two status words of the column check (16 bytes), then mean and norm of every listed column (dot class)
  const size_t entries = (size_t)na + (size_t)nb;
  const size_t want = 16 + (dot ? 2 * entries * sizeof(double) : 0);
  DeviceScratch ws;
  if (lists || dot) {
    if (hipMalloc(&ws.p, want) != hipSuccess) {
      (void)hipGetLastError();
      ws.p = nullptr;
      return fail(GSS_ENOMEM, "profile_dist: hipMalloc of %zu bytes failed", want);
    }
  }
  if (lists) {   // nothing reads x through a list before every entry of it is known to be a column of x
    uint32_t *status = static_cast<uint32_t *>(ws.p);
    GSS_HIP(hipMemsetAsync(status, 0xff, 8, st));
    hipLaunchKernelGGL(pd_check_cols_kernel, dim3(ceil_div(na > nb ? na : nb, kPdThreads)), dim3(kPdThreads), 0, st, na, cols_a, nb, cols_b, ld,
                       status);
    GSS_LAUNCH_CHECK("pd_check_cols_kernel");
    uint32_t h[2] = {kNoBad, kNoBad};
    GSS_HIP(hipMemcpyAsync(h, status, 8, hipMemcpyDeviceToHost, st));
    GSS_HIP(hipStreamSynchronize(st));
    for (int s = 0; s < 2; ++s) {
      if (h[s] == kNoBad) continue;
      int32_t c = 0;
      GSS_HIP(hipMemcpy(&c, (s == 0 ? cols_a : cols_b) + h[s], 4, hipMemcpyDeviceToHost));
      return fail(GSS_EINVAL, "profile_dist: cols_%c[%u] = %d is outside [0, ld=%lld)", s == 0 ? 'a' : 'b', h[s], c, (long long)ld);
    }
  }
  const dim3 grid(ceil_div(nb, kPdTile), ceil_div(na, kPdTile)), block(kPdThreads);
  if (dot) {
    double *mean = reinterpret_cast<double *>(static_cast<char *>(ws.p) + 16), *norm = mean + entries;
    hipLaunchKernelGGL(pd_stats_kernel, dim3(ceil_div((int64_t)entries, kPdThreads)), block, 0, st, n, x, ld, na, cols_a, nb, cols_b,
                       metric == GSS_DIST_CORRELATION ? 1 : 0, mean, norm);
    GSS_LAUNCH_CHECK("pd_stats_kernel");
    hipLaunchKernelGGL(pd_dot_kernel, grid, block, 0, st, n, x, ld, na, cols_a, nb, cols_b, mean, norm, out, ld_out);
    GSS_LAUNCH_CHECK("pd_dot_kernel");
  } else if (metric == GSS_DIST_CITYBLOCK) {
    hipLaunchKernelGGL(pd_diff_kernel<GSS_DIST_CITYBLOCK>, grid, block, 0, st, n, x, ld, na, cols_a, nb, cols_b, out, ld_out);
    GSS_LAUNCH_CHECK("pd_diff_kernel<cityblock>");
  } else if (metric == GSS_DIST_EUCLIDEAN) {
    hipLaunchKernelGGL(pd_diff_kernel<GSS_DIST_EUCLIDEAN>, grid, block, 0, st, n, x, ld, na, cols_a, nb, cols_b, out, ld_out);
    GSS_LAUNCH_CHECK("pd_diff_kernel<euclidean>");
  } else {
    hipLaunchKernelGGL(pd_diff_kernel<GSS_DIST_CANBERRA>, grid, block, 0, st, n, x, ld, na, cols_a, nb, cols_b, out, ld_out);
    GSS_LAUNCH_CHECK("pd_diff_kernel<canberra>");
  }
  if (ws.p) GSS_HIP(hipStreamSynchronize(st));   // the scratch is freed on return: its readers have to be done
  return GSS_OK;
}

}  // extern "C"

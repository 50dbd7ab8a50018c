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
#include "profile_front.h"

namespace gss {
namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int kPdTile = 64;       // outputs per workgroup: 64 x 64
constexpr int kPdSlab = 32;       // rows per staged slab (difference class): 2 panels x 32 x 64 x 8 bytes = 32 KiB of LDS
constexpr int kPdThreads = 256;
constexpr int kPdMaxList = 1 << 21;   // 32,768 tiles per grid dimension

__device__ __forceinline__ int32_t col_at(const int32_t *cols, int32_t i) { return cols ? cols[i] : i; }

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

// ---- listed pairs (gss_profile_dist_pairs) ----------------------------------------------------------------------------------------------------
// T distances, not T x T: a bandwidth kernel.  A list may name a column many times (a screen's baselines are in three of a gene's four pairs);
// those rereads are of the row block's own 32 rows, which stay in cache while the wave sweeps the list, so nothing is staged in LDS.
// A wave owns the kPpRows rows of row block rb and sweeps the pair list, lane = pair: at one row the 64 lanes read 64 pairs' entries, which
// sit next to each other in that row of x when the listed columns do (x is row-major: down a column nothing coalesces, across the list it
// does).  A pair whose two columns are neighbours in an aligned 16 bytes takes both with one load.  Every lane adds its block's rows in order
// and writes one partial per sum to part[sum][rb][t]; pp_finish_kernel adds the blocks 0, 1, ... in order.  The order of every sum therefore
// depends on n alone: a pair's bits do not depend on its place in the list or on the list's length, and the terms do not depend on the
// order of a and b.
constexpr int kPpRows = 32;       // rows per row block
constexpr int kPpWaves = 4;       // row blocks per workgroup
enum { kPpSums = 5, kPpDot = 6 };   // modes beside the three difference metrics: column sums (for the means), centred dot and norms

template <int kMode>
__global__ __launch_bounds__(64 * kPpWaves) void pp_partial_kernel(int32_t n, const double *__restrict__ x, int64_t ld, int32_t T,
                                                                    const int32_t *__restrict__ col_a, const int32_t *__restrict__ col_b,
                                                                    const double *__restrict__ mean, int32_t n_blk, int vec_ok,
                                                                    double *__restrict__ part) {
  const int lane = threadIdx.x & 63;
  const int32_t rb = blockIdx.x * kPpWaves + (threadIdx.x >> 6);
  if (rb >= n_blk) return;   // wave-uniform; the kernel has no barrier
  const int32_t r0 = rb * kPpRows, rows = min(kPpRows, n - r0);
  const size_t plane = (size_t)n_blk * T;
  for (int32_t t = lane; t < T; t += 64) {
    const int32_t ca = col_a[t], cb = col_b[t], lo = min(ca, cb);
    const bool both = vec_ok && (lo & 1) == 0 && (ca - cb == 1 || cb - ca == 1);   // the two columns share an aligned 16 bytes of every row
    const bool a_first = ca < cb;
    const double *pa = x + (int64_t)r0 * ld + ca, *pb = x + (int64_t)r0 * ld + cb, *pl = x + (int64_t)r0 * ld + lo;
    double ma = 0.0, mb = 0.0;
    if (kMode == kPpDot && mean) {
      ma = mean[t];
      mb = mean[T + t];
    }
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    auto add = [&](double a, double b) {
      if (kMode == kPpSums) {
        s0 += a;
        s1 += b;
      } else if (kMode == kPpDot) {
        const double da = a - ma, db = b - mb;
        s0 += da * db;
        s1 += da * da;
        s2 += db * db;
      } else {
        s0 += pd_term<kMode>(a, b);
      }
    };
    auto sweep = [&](int cnt) {
      if (both) {
#pragma unroll 8
        for (int r = 0; r < cnt; ++r) {
          const double2 v = *reinterpret_cast<const double2 *>(pl + (int64_t)r * ld);
          add(a_first ? v.x : v.y, a_first ? v.y : v.x);
        }
      } else {
#pragma unroll 8
        for (int r = 0; r < cnt; ++r) add(pa[(int64_t)r * ld], pb[(int64_t)r * ld]);
      }
    };
    if (rows == kPpRows) sweep(kPpRows);
    else sweep(rows);
    const size_t at = (size_t)rb * T + t;
    part[at] = s0;
    if (kMode == kPpSums || kMode == kPpDot) part[plane + at] = s1;
    if (kMode == kPpDot) part[2 * plane + at] = s2;
  }
}

// one thread per pair: the blocks' partials in block order, then the metric's last step (kPpSums: the two means into mean[t], mean[T + t])
template <int kMode>
__global__ __launch_bounds__(kPdThreads) void pp_finish_kernel(int32_t n, int32_t T, int32_t n_blk, const double *__restrict__ part,
                                                                double *__restrict__ mean, double *__restrict__ out) {
  const int32_t t = blockIdx.x * kPdThreads + threadIdx.x;
  if (t >= T) return;
  const size_t plane = (size_t)n_blk * T;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  for (int32_t b = 0; b < n_blk; ++b) {
    const size_t at = (size_t)b * T + t;
    s0 += part[at];
    if (kMode == kPpSums || kMode == kPpDot) s1 += part[plane + at];
    if (kMode == kPpDot) s2 += part[2 * plane + at];
  }
  if (kMode == kPpSums) {
    mean[t] = s0 / (double)n;
    mean[T + t] = s1 / (double)n;
  } else if (kMode == kPpDot) {   // as pd_dot_kernel: 0 / 0 = NaN for a zero (constant) vector, which the clip passes on
    double cs = s0 / (sqrt(s1) * sqrt(s2));
    if (fabs(cs) > 1.0) cs = copysign(1.0, cs);
    out[t] = 1.0 - cs;
  } else {
    out[t] = kMode == GSS_DIST_EUCLIDEAN ? sqrt(s0) : s0;
  }
}

template <int kMode>
int pp_run(int32_t n, const double *x, int64_t ld, int32_t T, const int32_t *col_a, const int32_t *col_b, const double *mean_in, double *mean_out,
           int32_t n_blk, int vec_ok, double *part, double *out, hipStream_t st) {
  hipLaunchKernelGGL(pp_partial_kernel<kMode>, dim3(ceil_div(n_blk, kPpWaves)), dim3(64 * kPpWaves), 0, st, n, x, ld, T, col_a, col_b, mean_in,
                     n_blk, vec_ok, part);
  GSS_LAUNCH_CHECK("pp_partial_kernel");
  hipLaunchKernelGGL(pp_finish_kernel<kMode>, dim3(ceil_div(T, kPdThreads)), dim3(kPdThreads), 0, st, n, T, n_blk, part, mean_out, out);
  GSS_LAUNCH_CHECK("pp_finish_kernel");
  return GSS_OK;
}

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
  DeviceBuf<char> ws;
  if (lists || dot)
    if (int rc = ws.alloc("profile_dist", want)) return rc;
  if (lists) {   // nothing reads x through a list before every entry of it is known to be a column of x
    const CheckedList a{cols_a, na, 0, ld, "cols_a", "ld"}, b{cols_b, nb, 0, ld, "cols_b", "ld"};
    if (int rc = check_lists("profile_dist", a, b, reinterpret_cast<uint32_t *>(ws.p), st)) return rc;
  }
  const dim3 grid(ceil_div(nb, kPdTile), ceil_div(na, kPdTile)), block(kPdThreads);
  if (dot) {
    double *mean = reinterpret_cast<double *>(ws.p + 16), *norm = mean + entries;
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
  if (ws.p) GSS_HIP(hipStreamSynchronize(st));   // not for the free (device_scope.h): a call with scratch has always returned with its work done
  return GSS_OK;
}

// workspace: the status words of the column check, the two means of every pair (correlation), three planes of [row blocks][T] partial sums
size_t gss_profile_dist_pairs_workspace_bytes(int32_t n, int32_t T) {
  if (n < 1 || T < 0) return 0;
  const size_t n_blk = (size_t)ceil_div(n, kPpRows);
  return kStatusBytes + sizeof(double) * (2 * (size_t)T + 3 * n_blk * (size_t)T);
}

int gss_profile_dist_pairs(int32_t n, const double *x, int64_t ld, int32_t T, const int32_t *col_a, const int32_t *col_b, int32_t metric,
                           double *out, void *workspace, size_t workspace_bytes, void *stream) {
  GSS_REQUIRE(n >= 1, "profile_dist_pairs: n=%d rows must be >= 1", n);
  GSS_REQUIRE(T >= 0 && T <= kPdMaxList, "profile_dist_pairs: T=%d pairs must be in [0, %d]", T, kPdMaxList);
  GSS_REQUIRE(metric >= GSS_DIST_CITYBLOCK && metric <= GSS_DIST_CORRELATION,
              "profile_dist_pairs: metric %d is unknown (0 cityblock, 1 euclidean, 2 canberra, 3 cosine, 4 correlation)", metric);
  GSS_REQUIRE(ld >= 1, "profile_dist_pairs: ld=%lld must be >= 1", (long long)ld);
  if (T == 0) return GSS_OK;
  GSS_REQUIRE(x != nullptr, "profile_dist_pairs: x is null");
  GSS_REQUIRE(col_a != nullptr, "profile_dist_pairs: col_a is null");
  GSS_REQUIRE(col_b != nullptr, "profile_dist_pairs: col_b is null");
  GSS_REQUIRE(out != nullptr, "profile_dist_pairs: out is null");
  GSS_REQUIRE(workspace != nullptr, "profile_dist_pairs: workspace is null");
  GSS_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "profile_dist_pairs: workspace is not 8-byte aligned");
  const size_t want = gss_profile_dist_pairs_workspace_bytes(n, T);
  GSS_REQUIRE(workspace_bytes >= want, "profile_dist_pairs: workspace of %zu bytes is below the %zu that n=%d, T=%d need", workspace_bytes, want,
              n, T);
  hipStream_t st = as_stream(stream);
  // nothing reads x through a list before every entry of it is known to be a column of x
  const CheckedList a{col_a, T, 0, ld, "col_a", "ld"}, b{col_b, T, 0, ld, "col_b", "ld"};
  if (int rc = check_lists("profile_dist_pairs", a, b, static_cast<uint32_t *>(workspace), st)) return rc;
  const int32_t n_blk = ceil_div(n, kPpRows);
  double *mean = reinterpret_cast<double *>(static_cast<char *>(workspace) + kStatusBytes), *part = mean + 2 * (size_t)T;
  const int vec_ok = (ld & 1) == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0;
  switch (metric) {
    case GSS_DIST_CITYBLOCK:
      return pp_run<GSS_DIST_CITYBLOCK>(n, x, ld, T, col_a, col_b, nullptr, nullptr, n_blk, vec_ok, part, out, st);
    case GSS_DIST_EUCLIDEAN:
      return pp_run<GSS_DIST_EUCLIDEAN>(n, x, ld, T, col_a, col_b, nullptr, nullptr, n_blk, vec_ok, part, out, st);
    case GSS_DIST_CANBERRA:
      return pp_run<GSS_DIST_CANBERRA>(n, x, ld, T, col_a, col_b, nullptr, nullptr, n_blk, vec_ok, part, out, st);
    case GSS_DIST_COSINE:
      return pp_run<kPpDot>(n, x, ld, T, col_a, col_b, nullptr, nullptr, n_blk, vec_ok, part, out, st);
    default: {
      const int rc = pp_run<kPpSums>(n, x, ld, T, col_a, col_b, nullptr, mean, n_blk, vec_ok, part, out, st);
      return rc != GSS_OK ? rc : pp_run<kPpDot>(n, x, ld, T, col_a, col_b, mean, nullptr, n_blk, vec_ok, part, out, st);
    }
  }
}

}  // extern "C"

// scores.hip -- the indication x drug score matrix straight from the embedding tensor a plan holds on the device: fp64 inner products of
// listed fp32 rows, raw (the node2vec branch, predict_drug.py:55) or after sklearn.preprocessing.normalize's row L2 normalisation (the GCN
// branch, predict_drug.py:52-66).  evaluate.DeviceEvaluator feeds the result to gss_auc_rows where it lies, so a trainer can score every
// epoch without writing a text file (include/gssgcn.h has the contract, DESIGN.md section 9.7 the cost model and the measurements).
//
// Two launches.  scores_prepare_kernel: one wave per list entry (the rows' entries, then the columns') checks the entry's index and its
// row's values, takes the row's norm and writes the row widened to fp64 and divided by the norm into a scratch panel xn [nr + nc][d].
// scores_dot_kernel: a workgroup owns a 64 x 64 tile of outputs and walks d in slabs of 32: the slab of both panels is staged in LDS (the
// next one is already in flight in registers), every thread keeps a 4 x 4 block of fp64 accumulators -- sixteen independent chains, which
// is all the instruction-level parallelism the fp64 pipe needs.
//
// Order (it depends on d alone):
//   norm   lane l of the wave sums the squares of the row's values l, l + 64, l + 128 ... in that order, starting from +0.0 (the square of
//          a widened fp32 is exact in fp64, so each step rounds once); the 64 lane sums are then combined by the butterfly
//          s[l] = s[l] + s[l ^ m] for m = 32, 16, 8, 4, 2, 1 (a + b = b + a, so every lane ends with the same bits); norm = sqrt of that,
//          correctly rounded, and a norm of 0 is replaced by 1.  With normalize = 0 the norm is 1.
//   value  (double)x / norm: one correctly rounded division per value (not a multiplication by a reciprocal).
//   dot    acc = +0.0, then acc = acc + a[k] * b[k] for k = 0, 1 ... d - 1: the product rounded to fp64, then the sum rounded to fp64.
//          No fused multiply-add (the file is compiled with contraction off), so a numpy mirror reproduces every bit.
// a[k] * b[k] does not depend on the order of its operands and no entry's sum is split between threads, so an entry has the same bits run
// to run, under any other choice of rows and cols, and with rows and columns swapped.  Every output word is written by the one thread that
// owns it; the only atomic is the status word.
#include <math.h>

#include "device_scope.h"

#pragma clang fp contract(off)

namespace gss {
namespace {

constexpr int kScTile = 64;       // outputs per workgroup: 64 x 64
constexpr int kScSlab = 32;       // values of d per staged slab
constexpr int kScPitch = kScTile + 2;   // fp64 per LDS slab row: 16-byte aligned rows, the staging stores of a wave spread over the banks
constexpr int kScThreads = 256;
constexpr int kScMaxList = 1 << 21;   // 32,768 tiles per grid dimension
constexpr unsigned long long kScClean = ~0ull;

enum : int { kScErrIndex = 1, kScErrValue = 2 };

// one rounding each.  Written as plain operators under this file's `fp contract(off)`: the __dmul_rn / __dadd_rn of the HIP headers are
// inline functions compiled under the headers' own contraction setting, and a product feeding a sum through them becomes v_fma_f64
__device__ __forceinline__ double sc_mul(double a, double b) { return a * b; }
__device__ __forceinline__ double sc_add(double a, double b) { return a + b; }

// the smallest (code, list, position) wins, so the word does not depend on the order in which the waves report: a bad index before a bad
// value, rows before cols, the first position of the list / the lowest embedding row
__device__ __forceinline__ void sc_report(unsigned long long *status, int code, int list, int32_t at) {
  atomicMin(status, ((unsigned long long)code << 56) | ((unsigned long long)list << 48) | (uint32_t)at);
}

// wave e of the grid: list entry e (rows first).  A bad index reads nothing and leaves a zero row, so the tile kernel stays inside xn.
__global__ __launch_bounds__(kScThreads) void scores_prepare_kernel(int32_t n, int32_t d, const float *__restrict__ emb, int64_t ld, int32_t nr,
                                                                    const int32_t *__restrict__ rows, int32_t nc,
                                                                    const int32_t *__restrict__ cols, int normalize, double *__restrict__ xn,
                                                                    unsigned long long *__restrict__ status) {
  const int lane = threadIdx.x & (kWave - 1);
  const int32_t e = blockIdx.x * (kScThreads / kWave) + threadIdx.x / kWave;
  if (e >= nr + nc) return;   // wave-uniform
  const int list = e < nr ? 0 : 1;
  const int32_t at = list ? e - nr : e;
  const int32_t v = list ? cols[at] : rows[at];
  double *out = xn + (int64_t)e * d;
  if (v < 0 || v >= n) {
    if (lane == 0) sc_report(status, kScErrIndex, list, at);
    for (int32_t k = lane; k < d; k += kWave) out[k] = 0.0;
    return;
  }
  const float *row = emb + (int64_t)v * ld;
  double s = 0.0;
  bool bad = false;
  for (int32_t k = lane; k < d; k += kWave) {
    const float x = row[k];
    bad |= !isfinite(x);
    const double w = (double)x;
    s = sc_add(s, sc_mul(w, w));
  }
  if (__ballot(bad) != 0) {
    if (lane == 0) sc_report(status, kScErrValue, 0, v);
    for (int32_t k = lane; k < d; k += kWave) out[k] = 0.0;
    return;
  }
  double nrm = 1.0;
  if (normalize) {
#pragma unroll
    for (int m = kWave / 2; m > 0; m >>= 1) s = sc_add(s, __shfl_xor(s, m, kWave));
    nrm = __dsqrt_rn(s);
    if (nrm == 0.0) nrm = 1.0;
  }
  for (int32_t k = lane; k < d; k += kWave) out[k] = __ddiv_rn((double)row[k], nrm);
}

// thread (ty = tid >> 4, tx = tid & 15): outputs (i0 + 4 ty + u, j0 + 4 tx + v).  Staging: thread tid loads value k0 + (tid & 31) of the panel
// rows (tid >> 5) + 8 m, so a wave reads two runs of 256 contiguous bytes per load.
__global__ __launch_bounds__(kScThreads) void scores_dot_kernel(int32_t d, const double *__restrict__ xn, int32_t nr, int32_t nc,
                                                                double *__restrict__ out, int64_t ld_out) {
  __shared__ __align__(16) double sa[kScSlab][kScPitch];
  __shared__ __align__(16) double sb[kScSlab][kScPitch];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4, lk = tid & 31, lr = tid >> 5;
  const int32_t i0 = blockIdx.y * kScTile, j0 = blockIdx.x * kScTile;
  constexpr int kPer = kScTile / 8;   // panel rows per staging thread
  const double *ga[kPer], *gb[kPer];
#pragma unroll
  for (int m = 0; m < kPer; ++m) {   // a tail tile stages the last row again and stores nothing for it
    ga[m] = xn + (int64_t)min(nr - 1, i0 + lr + 8 * m) * d;
    gb[m] = xn + (int64_t)(nr + min(nc - 1, j0 + lr + 8 * m)) * d;
  }
  double ra[kPer], rb[kPer];
  auto fetch = [&](int32_t k0) {
    const int32_t k = k0 + lk;
    const bool live = k < d;
#pragma unroll
    for (int m = 0; m < kPer; ++m) {
      ra[m] = live ? ga[m][k] : 0.0;
      rb[m] = live ? gb[m][k] : 0.0;
    }
  };
  double acc[4][4];
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int v = 0; v < 4; ++v) acc[u][v] = 0.0;
  fetch(0);
  for (int32_t k0 = 0; k0 < d; k0 += kScSlab) {
#pragma unroll
    for (int m = 0; m < kPer; ++m) {
      sa[lk][lr + 8 * m] = ra[m];
      sb[lk][lr + 8 * m] = rb[m];
    }
    __syncthreads();
    if (k0 + kScSlab < d) fetch(k0 + kScSlab);   // in flight while this slab is summed
    const int len = min(kScSlab, d - k0);          // uniform; values past d are never added
    if (len == kScSlab) {
#pragma unroll 8
      for (int k = 0; k < kScSlab; ++k) {
        double a[4], b[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) a[u] = sa[k][4 * ty + u];
#pragma unroll
        for (int v = 0; v < 4; ++v) b[v] = sb[k][4 * tx + v];
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int v = 0; v < 4; ++v) acc[u][v] = sc_add(acc[u][v], sc_mul(a[u], b[v]));
      }
    } else {
      for (int k = 0; k < len; ++k) {
        double a[4], b[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) a[u] = sa[k][4 * ty + u];
#pragma unroll
        for (int v = 0; v < 4; ++v) b[v] = sb[k][4 * tx + v];
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int v = 0; v < 4; ++v) acc[u][v] = sc_add(acc[u][v], sc_mul(a[u], b[v]));
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int32_t i = i0 + 4 * ty + u;
    if (i >= nr) continue;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int32_t j = j0 + 4 * tx + v;
      if (j < nc) out[(int64_t)i * ld_out + j] = acc[u][v];
    }
  }
}

}  // namespace
}  // namespace gss

using namespace gss;

extern "C" {

int gss_embedding_scores(int32_t n, int32_t d, const float *emb, int64_t ld, int32_t nr, const int32_t *rows, int32_t nc, const int32_t *cols,
                         int32_t normalize, double *out, int64_t ld_out, void *stream) {
  GSS_REQUIRE(emb != nullptr, "embedding_scores: emb is null");
  GSS_REQUIRE(rows != nullptr, "embedding_scores: rows is null");
  GSS_REQUIRE(cols != nullptr, "embedding_scores: cols is null");
  GSS_REQUIRE(out != nullptr, "embedding_scores: out is null");
  GSS_REQUIRE(n >= 1, "embedding_scores: n=%d rows must be >= 1", n);
  GSS_REQUIRE(d >= 1, "embedding_scores: d=%d must be >= 1", d);
  GSS_REQUIRE(ld >= d, "embedding_scores: ld=%lld is below d=%d", (long long)ld, d);
  GSS_REQUIRE(nr >= 1, "embedding_scores: nr=%d rows must be >= 1", nr);
  GSS_REQUIRE(nc >= 1, "embedding_scores: nc=%d cols must be >= 1", nc);
  GSS_REQUIRE(nr <= kScMaxList && nc <= kScMaxList, "embedding_scores: nr=%d, nc=%d is above the limit of %d entries per list", nr, nc, kScMaxList);
  GSS_REQUIRE(ld_out >= nc, "embedding_scores: ld_out=%lld is below nc=%d", (long long)ld_out, nc);
  GSS_REQUIRE(normalize == 0 || normalize == 1, "embedding_scores: normalize=%d must be 0 or 1", normalize);
  hipStream_t st = as_stream(stream);
  // scratch: the status word (16 bytes), then the listed rows as fp64, normalised
  const size_t entries = (size_t)nr + (size_t)nc;
  const size_t want = 16 + entries * (size_t)d * sizeof(double);
  DeviceBuf<char> ws;
  if (int rc = ws.alloc("embedding_scores", want)) return rc;
  unsigned long long *status = reinterpret_cast<unsigned long long *>(ws.p);
  double *xn = reinterpret_cast<double *>(ws.p + 16);
  unsigned long long h = kScClean;
  GSS_HIP(hipMemsetAsync(status, 0xff, sizeof(unsigned long long), st));
  hipLaunchKernelGGL(scores_prepare_kernel, dim3(ceil_div((int64_t)entries, kScThreads / kWave)), dim3(kScThreads), 0, st, n, d, emb, ld, nr, rows, nc,
                     cols, (int)normalize, xn, status);
  GSS_LAUNCH_CHECK("scores_prepare_kernel");
  hipLaunchKernelGGL(scores_dot_kernel, dim3(ceil_div(nc, kScTile), ceil_div(nr, kScTile)), dim3(kScThreads), 0, st, d, xn, nr, nc, out, ld_out);
  GSS_LAUNCH_CHECK("scores_dot_kernel");
  if (int rc = read_back(&h, status, sizeof(h), st)) return rc;
  if (h == kScClean) return GSS_OK;
  const int code = (int)(h >> 56), list = (int)((h >> 48) & 0xff);
  const int32_t at = (int32_t)(h & 0xffffffffu);
  if (code == kScErrIndex) {
    int32_t v = 0;
    GSS_HIP(hipMemcpy(&v, (list ? cols : rows) + at, 4, hipMemcpyDeviceToHost));
    return fail(GSS_EINVAL, "embedding_scores: %s[%d] = %d is not a row index in [0, %d)", list ? "cols" : "rows", at, v, n);
  }
  if (code == kScErrValue) return fail(GSS_EINVAL, "embedding_scores: row %d of emb holds a NaN or infinite value", at);
  return fail(GSS_EHIP, "embedding_scores: unknown status word %llx", h);
}

}  // extern "C"

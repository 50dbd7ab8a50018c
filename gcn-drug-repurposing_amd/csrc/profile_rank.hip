// profile_rank.hip -- exact average-tie ranks of listed profile columns (scipy.stats.rankdata(x[:, c], method="average") per column), the
// transform behind the "spearman" profile distance: Spearman's rho is the Pearson correlation of these ranks, so diffusion.py ranks the
// referenced columns once and hands the rank matrix to gss_profile_dist with GSS_DIST_CORRELATION.
//
// include/gssgcn.h has the contract, DESIGN.md section 9.10 the cost model and the measurements.  A rank needs no sorted payload, only counts:
//   rank(i) = (2 below(i) + tied(i) + 1) / 2,   below(i) = sum over chunks of lower_bound(chunk, key_i),
//                                               tied(i)  = sum over chunks of upper_bound(chunk, key_i) - lower_bound(chunk, key_i)
// so 2 below + tied = sum over chunks of (lower_bound + upper_bound), an integer <= 2 n.  Three launches per panel of kKeyPanel listed columns:
//   keys_kernel      (profile_front.h, shared with gss_profile_topk) reads the panel's columns of x by rows (adjacent lanes = adjacent listed
//                    columns: coalesced when the list is) and writes order-preserving uint64 keys [panel][n] into the workspace through a
//                    64 x 64 LDS tile; -0.0 folds into +0.0, a NaN becomes the all-ones key (above +inf's key, which no other value maps to)
//   rk_rank_kernel   one workgroup per column: per chunk of kRkChunk keys, load the chunk into LDS (padded to a power of two with the all-ones
//                    key), bitonic-sort it there, then every key of the column does its two binary searches in LDS and its owner thread adds
//                    lower + upper to the key's int32 word of the workspace (the first chunk stores).  A column that holds a NaN is flagged
//   rk_write_kernel  (acc + 1) / 2 into r through a 64 x 64 LDS tile, coalesced along r's rows; a flagged column is written as NaN
// The counts are integers and every word (key, accumulator, flag, output) has one owner thread: no atomics, and a column's output depends
// on nothing but its values.  The key, the sort and the search are rank_keys.h's, the ones gss_auc_rows and gss_rank_metrics_rows count
// ties with: a rank here and a U statistic there order the same doubles the same way.  The check of the column list and the key pass are
// profile_front.h's.
#include "profile_front.h"

namespace gss {
namespace {

constexpr int kRkThreads = 1024;       // the rank kernel: 16 waves, four per SIMD, to keep the LDS busy (one workgroup per CU at 128 KiB)
constexpr int kRkChunk = 16384;        // keys sorted in LDS at a time: 128 KiB

inline size_t rk_round8(size_t b) { return (b + 7) & ~(size_t)7; }

// workgroup = panel column blockIdx.x; key i of the column belongs to thread i mod kRkThreads in every chunk round
__global__ __launch_bounds__(kRkThreads) void rk_rank_kernel(int32_t n, const uint64_t *__restrict__ keys, int32_t *__restrict__ acc,
                                                              int32_t *__restrict__ has_nan) {
  extern __shared__ __align__(16) unsigned char rk_lds[];
  uint64_t *srt = reinterpret_cast<uint64_t *>(rk_lds);   // [min(kRkChunk, pow2 >= n)]
  const int tid = threadIdx.x;
  const uint64_t *key = keys + (size_t)blockIdx.x * n;
  int32_t *a = acc + (size_t)blockIdx.x * n;
  int nan_here = 0;
  for (int32_t c0 = 0; c0 < n; c0 += kRkChunk) {
    const int32_t len = min(kRkChunk, n - c0), cpad = pow2_at_least(len);
    for (int32_t i = tid; i < cpad; i += kRkThreads) {
      const uint64_t k = i < len ? key[c0 + i] : kBehind;
      nan_here |= (i < len && k == kBehind) ? 1 : 0;
      srt[i] = k;
    }
    __syncthreads();
    sort_keys<kRkThreads>(srt, cpad, tid);
    for (int32_t i = tid; i < n; i += kRkThreads) {
      const uint64_t k = key[i];
      const int32_t both = search(srt, 0, len, k, false) + search(srt, 0, len, k, true);
      a[i] = c0 == 0 ? both : a[i] + both;
    }
    __syncthreads();   // the next chunk overwrites srt
  }
  const int any = __syncthreads_or(nan_here);
  if (tid == 0) has_nan[blockIdx.x] = any;
}

// panel columns [j0, j0 + 64) x rows [r0, r0 + 64): load phase lane = row, store phase lane = column.  r points at the panel's first column
__global__ __launch_bounds__(kKeyTileThreads) void rk_write_kernel(int32_t n, int32_t pw, const int32_t *__restrict__ acc,
                                                                   const int32_t *__restrict__ has_nan, double *__restrict__ r, int64_t ld_r) {
  __shared__ int32_t tile[kKeyTile][kKeyTile + 1];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int32_t r0 = blockIdx.x * kKeyTile, j0 = blockIdx.y * kKeyTile;
  if (r0 + tx < n) {
#pragma unroll 4
    for (int m = 0; m < kKeyTile / 4; ++m) {
      const int32_t j = j0 + ty + 4 * m;
      if (j < pw) tile[ty + 4 * m][tx] = acc[(size_t)j * n + r0 + tx];
    }
  }
  __syncthreads();
  const int32_t j = j0 + tx;
  if (j >= pw) return;
  const bool nan_col = has_nan[j] != 0;
#pragma unroll 4
  for (int m = 0; m < kKeyTile / 4; ++m) {
    const int32_t row = r0 + ty + 4 * m;
    if (row < n)   // acc = 2 below + tied <= 2 n: the sum and the halving are exact
      r[(int64_t)row * ld_r + j] = nan_col ? __longlong_as_double(0x7ff8000000000000ll) : (double)(tile[tx][ty + 4 * m] + 1) * 0.5;
  }
}

}  // namespace
}  // namespace gss

using namespace gss;

extern "C" {

// status words, then per panel column: n keys of 8 bytes, n accumulators of 4 bytes, one NaN flag
size_t gss_profile_rank_workspace_bytes(int32_t n, int32_t nc) {
  if (n < 1 || nc < 0) return 0;
  const size_t p = (size_t)(nc < kKeyPanel ? nc : kKeyPanel);
  return kStatusBytes + p * (size_t)n * 8 + rk_round8(p * (size_t)n * 4) + rk_round8(p * 4);
}

int gss_profile_rank(int32_t n, const double *x, int64_t ld, int32_t nc, const int32_t *cols, double *r, int64_t ld_r, void *workspace,
                     size_t workspace_bytes, void *stream) {
  GSS_REQUIRE(n >= 1, "profile_rank: n=%d rows must be >= 1", n);
  GSS_REQUIRE(n <= kKeyMaxRows, "profile_rank: n=%d rows is above the limit of %d (the counting scheme is quadratic in n / chunk: every key "
              "searches every sorted chunk of %d keys)", n, kKeyMaxRows, kRkChunk);
  GSS_REQUIRE(nc >= 0, "profile_rank: nc=%d columns must be >= 0", nc);
  GSS_REQUIRE(ld >= 1, "profile_rank: ld=%lld must be >= 1", (long long)ld);
  GSS_REQUIRE(ld_r >= nc, "profile_rank: ld_r=%lld is below nc=%d", (long long)ld_r, nc);
  if (nc == 0) return GSS_OK;
  GSS_REQUIRE(x != nullptr, "profile_rank: x is null");
  GSS_REQUIRE(r != nullptr, "profile_rank: r is null");
  GSS_REQUIRE(workspace != nullptr, "profile_rank: workspace is null");
  GSS_REQUIRE(cols || nc <= ld, "profile_rank: ld=%lld is below nc=%d (cols is null: columns 0 .. nc - 1)", (long long)ld, nc);
  GSS_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "profile_rank: workspace is not 8-byte aligned");
  const size_t want = gss_profile_rank_workspace_bytes(n, nc);
  GSS_REQUIRE(workspace_bytes >= want, "profile_rank: workspace of %zu bytes is below the %zu that n=%d, nc=%d need", workspace_bytes, want, n,
              nc);
  hipStream_t st = as_stream(stream);
  if (cols) {   // nothing reads x through the list before every entry of it is known to be a column of x
    const CheckedList a{cols, nc, 0, ld, "cols", "ld"}, none{nullptr, 0, 0, 0, "", ""};
    if (int rc = check_lists("profile_rank", a, none, static_cast<uint32_t *>(workspace), st)) return rc;
  }
  const size_t p = (size_t)(nc < kKeyPanel ? nc : kKeyPanel);
  char *base = static_cast<char *>(workspace) + kStatusBytes;
  uint64_t *keys = reinterpret_cast<uint64_t *>(base);
  int32_t *acc = reinterpret_cast<int32_t *>(base + p * (size_t)n * 8);
  int32_t *has_nan = reinterpret_cast<int32_t *>(base + p * (size_t)n * 8 + rk_round8(p * (size_t)n * 4));
  const size_t lds = (size_t)(n < kRkChunk ? pow2_at_least(n) : kRkChunk) * 8;
  const size_t lds_arg = lds_request(rk_rank_kernel, lds);
  for (int32_t first = 0; first < nc; first += kKeyPanel) {   // the stream orders a panel's three launches and the panels after one another
    const int32_t pw = nc - first < kKeyPanel ? nc - first : kKeyPanel;
    const dim3 tiles(ceil_div(n, kKeyTile), ceil_div(pw, kKeyTile));
    if (int rc = launch_keys(n, x, ld, pw, first, cols, keys, st)) return rc;
    hipLaunchKernelGGL(rk_rank_kernel, dim3(pw), dim3(kRkThreads), lds_arg, st, n, keys, acc, has_nan);
    GSS_LAUNCH_CHECK("rk_rank_kernel");
    hipLaunchKernelGGL(rk_write_kernel, tiles, dim3(kKeyTileThreads), 0, st, n, pw, acc, has_nan, r + first, ld_r);
    GSS_LAUNCH_CHECK("rk_write_kernel");
  }
  return GSS_OK;
}

}  // extern "C"

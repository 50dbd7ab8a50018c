// profile_front.h -- the front end the profile entry points share: gss_profile_dist and gss_profile_dist_pairs (profile_dist.hip),
// gss_profile_rank (profile_rank.hip), gss_profile_topk and gss_topk_overlap (profile_topk.hip).  Two things, each stated once:
//   the list check   a caller's int32 lists (columns of x, node groups, selection numbers) are checked against their half-open range
//                    before any kernel indexes x, a histogram or idx through them; the first offending entry comes back by name;
//   the key pass     the listed columns of x, a panel at a time, transposed into rank_keys.h's order-preserving keys [panel][n].
// Everything is in an unnamed namespace: a file that includes this has its own copy of the kernels and of the host code that launches them
// (so profile_dist.hip carries a key kernel that it never launches, about a kilobyte of code), and the library exports nothing from here.
#pragma once
#include "rank_keys.h"

namespace gss {
namespace {

constexpr int kListThreads = 256;             // the list check: one thread per list position
constexpr uint32_t kListNone = 0xffffffffu;   // a status word that no offending position has lowered
constexpr int kStatusBytes = 256;             // the status words of the list check, in front of a caller's workspace
constexpr int kKeyTile = 64;                  // the transposing kernels move 64 rows x 64 listed columns per workgroup
constexpr int kKeyTileThreads = 256;
constexpr int kKeyPanel = 512;                // listed columns per pass through the workspace: two workgroups per CU on 256 CUs
constexpr int kKeyMaxRows = 1 << 24;          // rows of a key pass; a node index is three 8-bit digits

// one list of a call: v[0 .. len) must lie in [lo, hi); v null = no list, nothing to check.  `name` and `bound` are the refusal's words
// for the list and for hi ("cols", "ld")
struct CheckedList {
  const int32_t *v;
  int32_t len;
  int64_t lo, hi;
  const char *name, *bound;
};

__device__ __forceinline__ void check_entry(const int32_t *__restrict__ v, int32_t len, int64_t lo, int64_t hi, int32_t t, uint32_t *word) {
  if (!v || t >= len) return;
  const int32_t e = v[t];
  if (e < lo || e >= hi) atomicMin(word, (uint32_t)t);
}

// status[s]: the first position of list s whose entry is outside [lo_s, hi_s) (kListNone = none; the host set both words to kListNone)
__global__ __launch_bounds__(kListThreads) void check_lists_kernel(const int32_t *__restrict__ v0, int32_t len0, int64_t lo0, int64_t hi0,
                                                                    const int32_t *__restrict__ v1, int32_t len1, int64_t lo1, int64_t hi1,
                                                                    uint32_t *__restrict__ status) {
  const int32_t t = blockIdx.x * kListThreads + threadIdx.x;
  check_entry(v0, len0, lo0, hi0, t, &status[0]);
  check_entry(v1, len1, lo1, hi1, t, &status[1]);
}

// Checks the two lists of entry point `who` in one launch (the grid covers the longer length) with the two status words at `status`
// (device, 8 bytes, set here on every call), waits for the stream and refuses the first offending entry by name, list a's before list
// b's: "<who>: <name>[<position>] = <entry> is outside [<lo>, <bound>=<hi>)".  Call it only with a list to check
inline int check_lists(const char *who, const CheckedList &a, const CheckedList &b, uint32_t *status, hipStream_t st) {
  GSS_HIP(hipMemsetAsync(status, 0xff, 8, st));
  hipLaunchKernelGGL(check_lists_kernel, dim3(ceil_div(a.len > b.len ? a.len : b.len, kListThreads)), dim3(kListThreads), 0, st, a.v, a.len, a.lo,
                     a.hi, b.v, b.len, b.lo, b.hi, status);
  GSS_LAUNCH_CHECK("check_lists_kernel");
  uint32_t h[2] = {kListNone, kListNone};
  if (int rc = read_back(h, status, 8, st)) return rc;
  for (int s = 0; s < 2; ++s) {
    if (h[s] == kListNone) continue;
    const CheckedList &l = s == 0 ? a : b;
    int32_t e = 0;
    GSS_HIP(hipMemcpy(&e, l.v + h[s], 4, hipMemcpyDeviceToHost));
    return fail(GSS_EINVAL, "%s: %s[%u] = %d is outside [%lld, %s=%lld)", who, l.name, h[s], e, (long long)l.lo, l.bound, (long long)l.hi);
  }
  return GSS_OK;
}

// panel columns [j0, j0 + 64) x rows [r0, r0 + 64): load phase lane = column, store phase lane = row.  `first` = the panel's first list
// position; cols null = columns first, first + 1, ...  keys [pw][n]: -0.0 folds into +0.0, a NaN becomes the all-ones key
__global__ __launch_bounds__(kKeyTileThreads) void keys_kernel(int32_t n, const double *__restrict__ x, int64_t ld, int32_t pw, int32_t first,
                                                                const int32_t *__restrict__ cols, uint64_t *__restrict__ keys) {
  __shared__ uint64_t tile[kKeyTile][kKeyTile + 1];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int32_t r0 = blockIdx.x * kKeyTile, j0 = blockIdx.y * kKeyTile;
  if (j0 + tx < pw) {
    const int32_t c = cols ? cols[first + j0 + tx] : first + j0 + tx;
    const double *p = x + c;
#pragma unroll 4
    for (int m = 0; m < kKeyTile / 4; ++m) {
      const int32_t row = r0 + ty + 4 * m;
      if (row < n) tile[ty + 4 * m][tx] = order_key_nan_behind(p[(int64_t)row * ld]);
    }
  }
  __syncthreads();
  const int32_t row = r0 + tx;
  if (row >= n) return;
#pragma unroll 4
  for (int m = 0; m < kKeyTile / 4; ++m) {
    const int32_t j = j0 + ty + 4 * m;
    if (j < pw) keys[(size_t)j * n + row] = tile[tx][ty + 4 * m];
  }
}

// the key pass of one panel: list positions [first, first + pw) of cols -> keys [pw][n]
inline int launch_keys(int32_t n, const double *x, int64_t ld, int32_t pw, int32_t first, const int32_t *cols, uint64_t *keys, hipStream_t st) {
  hipLaunchKernelGGL(keys_kernel, dim3(ceil_div(n, kKeyTile), ceil_div(pw, kKeyTile)), dim3(kKeyTileThreads), 0, st, n, x, ld, pw, first, cols, keys);
  GSS_LAUNCH_CHECK("keys_kernel");
  return GSS_OK;
}

}  // namespace
}  // namespace gss

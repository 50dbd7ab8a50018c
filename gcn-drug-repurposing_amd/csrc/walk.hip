// walk.hip -- node2vec's second-order biased random walks (multiscale/openne/walker.py:58-207) on the device.
//
// The reference builds one alias table per node and one per directed edge (preprocess_transition_probs, O(sum deg^2)
// memory) and draws from them.  Here every step is exact rejection sampling on the raw weighted CSR:
//   - draw x first-order: u * (row total) located by binary search in the row's inclusive fp64 prefix sums (gss_walk_prefix);
//   - step 1 (from the start node) takes x as it is (alias_nodes);
//   - later steps accept x with probability b(x) / max(1/p, 1, 1/q), b = 1/p if x == prev, else 1 if the edge x -> prev
//     exists (binary search in x's sorted row), else 1/q -- the order of get_alias_edge (walker.py:113-131);
//   - after kRejectTries refused candidates the step draws directly from the full row: sum_x w(cur, x) b(x) in row order,
//     u * sum located by a sequential scan.  Both branches sample the same distribution, so the mixture is exact, and a
//     step's cost is bounded whatever p and q are.
// One thread per walk.  All draws come from counter_rng.h keyed by (seed, walk, step, attempt): candidate 2a, acceptance
// 2a + 1, the direct draw 2 kRejectTries.  fp64 products and sums use the _rn intrinsics (no contraction), so a numpy
// statement of the same steps (tests/node2vec_mirror.py) reproduces the walks bit for bit.
#include <float.h>

#include "device_scope.h"

#include "counter_rng.h"

namespace gss {
namespace {

constexpr int kRejectTries = 64;

__global__ void row_prefix_kernel(int32_t n, const int32_t *__restrict__ rowptr, const double *__restrict__ val, double *__restrict__ cum,
                                  unsigned long long *__restrict__ first_bad) {
  const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  double s = 0.0;
  for (int32_t e = rowptr[r]; e < rowptr[r + 1]; ++e) {
    const double w = val[e];
    if (!(w > 0.0 && w <= DBL_MAX)) atomicMin(first_bad, (unsigned long long)e);
    s = __dadd_rn(s, w);
    cum[e] = s;
  }
}

// first entry of [b, e) whose inclusive prefix sum exceeds t (the last one if none does: t can round up to the total)
__device__ __forceinline__ int32_t pick_edge(const double *__restrict__ cum, int32_t b, int32_t e, double t) {
  int32_t lo = b, hi = e - 1;
  while (lo < hi) {
    const int32_t mid = (lo + hi) >> 1;
    if (cum[mid] > t) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

__device__ __forceinline__ bool has_edge(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, int32_t u, int32_t v) {
  int32_t lo = rowptr[u], hi = rowptr[u + 1];
  while (lo < hi) {
    const int32_t mid = (lo + hi) >> 1;
    const int32_t c = col[mid];
    if (c == v) return true;
    if (c < v) lo = mid + 1;
    else hi = mid;
  }
  return false;
}

struct WalkArgs {
  int64_t n_walks;
  int32_t walk_length;
  const int32_t *rowptr, *col, *starts;
  const double *val, *cum;
  double inv_p, inv_q, acc_p, acc_1, acc_q;
  uint64_t seed;
  int32_t *walks, *lengths;
};

__global__ __launch_bounds__(256) void node2vec_walk_kernel(WalkArgs a) {
  const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= a.n_walks) return;
  const int32_t L = a.walk_length;
  int32_t *out = a.walks + w * L;
  int32_t cur = a.starts[w], prev = -1, len = 1;
  out[0] = cur;
  while (len < L) {
    const int32_t b = a.rowptr[cur], e = a.rowptr[cur + 1];
    if (b == e) break;  // no out-edges: the walk ends here (walker.py:85-86)
    const double total = a.cum[e - 1];
    int32_t nxt = -1;
    if (len == 1) {
      const double u = rng_unit_f64(rng_key(a.seed, kRngWalk, (uint64_t)w, (uint64_t)len, 0));
      nxt = a.col[pick_edge(a.cum, b, e, __dmul_rn(u, total))];
    } else {
      for (int t = 0; t < kRejectTries; ++t) {
        const double u = rng_unit_f64(rng_key(a.seed, kRngWalk, (uint64_t)w, (uint64_t)len, (uint64_t)(2 * t)));
        const int32_t x = a.col[pick_edge(a.cum, b, e, __dmul_rn(u, total))];
        const double acc = x == prev ? a.acc_p : (has_edge(a.rowptr, a.col, x, prev) ? a.acc_1 : a.acc_q);
        const double v = rng_unit_f64(rng_key(a.seed, kRngWalk, (uint64_t)w, (uint64_t)len, (uint64_t)(2 * t + 1)));
        if (v < acc) {
          nxt = x;
          break;
        }
      }
      if (nxt < 0) {  // direct draw from the biased row
        double sum = 0.0;
        for (int32_t k = b; k < e; ++k) {
          const int32_t x = a.col[k];
          const double bias = x == prev ? a.inv_p : (has_edge(a.rowptr, a.col, x, prev) ? 1.0 : a.inv_q);
          sum = __dadd_rn(sum, __dmul_rn(a.val[k], bias));
        }
        const double u = rng_unit_f64(rng_key(a.seed, kRngWalk, (uint64_t)w, (uint64_t)len, (uint64_t)(2 * kRejectTries)));
        const double t = __dmul_rn(u, sum);
        double run = 0.0;
        nxt = a.col[e - 1];
        for (int32_t k = b; k < e; ++k) {
          const int32_t x = a.col[k];
          const double bias = x == prev ? a.inv_p : (has_edge(a.rowptr, a.col, x, prev) ? 1.0 : a.inv_q);
          run = __dadd_rn(run, __dmul_rn(a.val[k], bias));
          if (run > t) {
            nxt = x;
            break;
          }
        }
      }
    }
    out[len] = nxt;
    prev = cur;
    cur = nxt;
    ++len;
  }
  for (int32_t k = len; k < L; ++k) out[k] = -1;
  a.lengths[w] = len;
}

}  // namespace

extern "C" {

int gss_walk_prefix(int32_t n, const int32_t *rowptr, const double *val, double *cum, void *stream) {
  GSS_REQUIRE(n >= 1, "walk_prefix: n=%d must be >= 1", n);
  GSS_REQUIRE(rowptr && val && cum, "walk_prefix: null pointer");
  hipStream_t st = as_stream(stream);
  DeviceBuf<unsigned long long> bad;
  if (int rc = bad.alloc("walk_prefix", sizeof(unsigned long long))) return rc;
  unsigned long long h_bad = ~0ull;
  GSS_HIP(hipMemcpyAsync(bad.p, &h_bad, sizeof(h_bad), hipMemcpyHostToDevice, st));
  row_prefix_kernel<<<ceil_div(n, 256), 256, 0, st>>>(n, rowptr, val, cum, bad.p);
  GSS_LAUNCH_CHECK("row_prefix_kernel");
  if (int rc = read_back(&h_bad, bad.p, sizeof(h_bad), st)) return rc;
  GSS_REQUIRE(h_bad == ~0ull, "walk_prefix: edge weight of CSR entry %llu is not positive and finite (node2vec needs weights > 0)", h_bad);
  return GSS_OK;
}

int gss_node2vec_walks(int32_t n, const int32_t *rowptr, const int32_t *col, const double *val, const double *cum, int64_t n_walks,
                       const int32_t *starts, int32_t walk_length, double p, double q, uint64_t seed, int32_t *walks, int32_t *lengths,
                       void *stream) {
  GSS_REQUIRE(n >= 1, "node2vec_walks: n=%d must be >= 1", n);
  GSS_REQUIRE(p > 0.0 && p <= DBL_MAX, "node2vec_walks: p=%g must be positive and finite", p);
  GSS_REQUIRE(q > 0.0 && q <= DBL_MAX, "node2vec_walks: q=%g must be positive and finite", q);
  GSS_REQUIRE(walk_length >= 1, "node2vec_walks: walk_length=%d must be >= 1", walk_length);
  GSS_REQUIRE(n_walks >= 0, "node2vec_walks: n_walks=%lld must be >= 0", (long long)n_walks);
  GSS_REQUIRE(rowptr && col && val && cum && starts && walks && lengths, "node2vec_walks: null pointer");
  if (n_walks == 0) return GSS_OK;
  WalkArgs a;
  a.n_walks = n_walks;
  a.walk_length = walk_length;
  a.rowptr = rowptr;
  a.col = col;
  a.starts = starts;
  a.val = val;
  a.cum = cum;
  a.inv_p = 1.0 / p;
  a.inv_q = 1.0 / q;
  const double bmax = fmax(fmax(a.inv_p, 1.0), a.inv_q);
  a.acc_p = a.inv_p / bmax;
  a.acc_1 = 1.0 / bmax;
  a.acc_q = a.inv_q / bmax;
  a.seed = seed;
  a.walks = walks;
  a.lengths = lengths;
  const int64_t blocks = (n_walks + 255) / 256;
  GSS_REQUIRE(blocks <= 0x7fffffff, "node2vec_walks: %lld walks are too many for one launch", (long long)n_walks);
  node2vec_walk_kernel<<<(unsigned)blocks, 256, 0, as_stream(stream)>>>(a);
  GSS_LAUNCH_CHECK("node2vec_walk_kernel");
  return GSS_OK;
}

}  // extern "C"
}  // namespace gss

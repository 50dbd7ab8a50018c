// trace.hip -- what lies between a source and a target besides one shortest path: the number of shortest paths toward up to 64 targets per
// pass, the best shortest path under a node weight, and for (source, target) pairs the nodes on their shortest paths with the share of
// the paths that pass through each (interpret.py; include/gssgcn.h has the contract, DESIGN.md section 9.5 the cost model).
//
// Count pass: the distances of a gss_paths_run pass are given, so the levels are known before the first launch: level L = 1 .. levels is
// one launch in which every (target q, node v) with dist[q][v] = L reads v's row and sums sigma over the successors with dist = L - 1,
// which the launch before wrote.  No read-back between the levels; one status word is read after the last.  A lane owns one (q, v): the
// lanes of a wave are 64 consecutive nodes of one target, so dist and the results are read and written in whole lines.  A row of more
// than kShortRow entries is read by the whole wave, 64 entries at a time, and reduced across the lanes: the counts are exact integers
// (a sum above 2^53 is refused), so the order of the sum does not matter; the best successor is the larger value, on equal values the
// smaller index, which is order-free as well.  Every result word is written by the one lane that owns it; the only atomic is the status.
//
// Between pass: a lane owns one (target t, node v) and walks the pass's sources in list order, so the mediator sums have the list's order
// however the list is cut into passes.  The pair counts take one workgroup per pair, the node lists of chosen pairs one workgroup per pair
// that compacts in node order (ballot + prefix over the workgroup's waves).
#include <math.h>

#include "device_scope.h"
#include "ops.h"

namespace gss {
namespace {

constexpr int kMaxPass = 64;
constexpr int kMaxLevel = 254;
constexpr int kShortRow = 32;
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr double kMaxCount = 9007199254740992.0;   // 2^53: every integer up to it is an fp64

enum : int { kErrDuplicate = 1, kErrTargetDist = 2, kErrLevels = 3, kErrWeight = 4, kErrCount = 5 };

// the largest (code, target, node) wins, so the word does not depend on the order in which the lanes report
__device__ __forceinline__ void report(unsigned long long *status, int code, int q, int32_t v) {
  atomicMax(status, ((unsigned long long)code << 56) | ((unsigned long long)q << 32) | (uint32_t)v);
}

// a + b of two counts; over = the exact sum is above 2^53.  Both are integers <= 2^53, so a sum <= 2^53 is exact; the first inexact sum is
// 2^53 + 1 rounded to 2^53, which the subtraction (exact here) tells from a true 2^53
__device__ __forceinline__ double add_count(double a, double b, bool &over) {
  const double s = __dadd_rn(a, b);
  if (s > kMaxCount || (s == kMaxCount && __dsub_rn(s, a) != b)) over = true;
  return s;
}

__device__ __forceinline__ double shfl_xor_d(double x, int m) { return __shfl_xor(x, m, kWave); }

// an entry equal to the one before it in the same row: candidates are rare, only they search the row pointer
__global__ __launch_bounds__(kThreads) void trace_duplicate_kernel(int32_t n, int64_t nnz, const int32_t *__restrict__ rowptr,
                                                                   const int32_t *__restrict__ col, unsigned long long *__restrict__ status) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < 1 || i >= nnz || col[i] != col[i - 1]) return;
  int32_t lo = 0, hi = n;   // the row of entry i: the last v with rowptr[v] <= i
  while (hi - lo > 1) {
    const int32_t mid = lo + (hi - lo) / 2;
    if ((int64_t)rowptr[mid] <= i) lo = mid;
    else hi = mid;
  }
  if ((int64_t)rowptr[lo] < i) report(status, kErrDuplicate, 0, lo);
}

struct CountArgs {
  int32_t n, level, levels;
  const int32_t *rowptr, *col, *targets;
  const uint8_t *dist;
  const double *w;
  double *sigma, *best;
  int32_t *best_next;
  unsigned long long *status;
};

// checks dist and w of the pass and writes the values of level 0 and of the unreachable nodes
__global__ __launch_bounds__(kThreads) void trace_init_kernel(CountArgs a) {
  const int32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  const int q = blockIdx.y;
  if (v >= a.n) return;
  const int64_t i = (int64_t)q * a.n + v;
  const int d = a.dist[i];
  if ((d == 0) != (v == a.targets[q])) report(a.status, kErrTargetDist, q, v);
  else if (d != 255 && d > a.levels) report(a.status, kErrLevels, q, v);
  a.sigma[i] = d == 0 ? 1.0 : 0.0;
  if (a.w) {
    if (!isfinite(a.w[i])) report(a.status, kErrWeight, q, v);
    a.best[i] = 0.0;
    a.best_next[i] = -1;
  }
}

// (x, u) beats (y, t): the larger value, the smaller index on equal values; t < 0 = nothing yet
__device__ __forceinline__ bool beats(double x, int32_t u, double y, int32_t t) { return u >= 0 && (t < 0 || x > y || (x == y && u < t)); }

__global__ __launch_bounds__(kThreads) void trace_level_kernel(CountArgs a) {
  const int32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  const int q = blockIdx.y;
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t off = (int64_t)q * a.n;
  const uint8_t *__restrict__ dq = a.dist + off;
  const double *sq = a.sigma + off;   // level L - 1 is read, level L written: not restrict
  const double *bq = a.w ? a.best + off : nullptr;
  const int below = a.level - 1;
  const bool mine = v < a.n && dq[v] == a.level;
  int32_t b = 0, e = 0;
  if (mine) {
    b = a.rowptr[v];
    e = a.rowptr[v + 1];
  }
  const bool lng = mine && e - b > kShortRow;
  double s = 0.0, bb = 0.0;
  int32_t bu = -1;
  bool over = false;
  if (mine && !lng) {
    for (int32_t i = b; i < e; ++i) {
      const int32_t u = a.col[i];
      if (dq[u] != below) continue;
      s = add_count(s, sq[u], over);
      if (bq) {
        const double x = bq[u];
        if (beats(x, u, bb, bu)) {
          bb = x;
          bu = u;
        }
      }
    }
  }
  uint64_t todo = __ballot(lng);
  while (todo) {
    const int owner = __builtin_ctzll(todo);
    todo &= todo - 1;
    const int32_t rb = __shfl(b, owner), re = __shfl(e, owner);
    double rs = 0.0, rbb = 0.0;
    int32_t rbu = -1;
    bool rover = false;
    for (int32_t i = rb + lane; i < re; i += kWave) {
      const int32_t u = a.col[i];
      if (dq[u] != below) continue;
      rs = add_count(rs, sq[u], rover);
      if (bq) {
        const double x = bq[u];
        if (beats(x, u, rbb, rbu)) {
          rbb = x;
          rbu = u;
        }
      }
    }
#pragma unroll
    for (int m = kWave / 2; m > 0; m >>= 1) {
      rs = add_count(rs, shfl_xor_d(rs, m), rover);
      const double ob = shfl_xor_d(rbb, m);
      const int32_t ou = __shfl_xor(rbu, m, kWave);
      if (beats(ob, ou, rbb, rbu)) {
        rbb = ob;
        rbu = ou;
      }
    }
    const bool any_over = __ballot(rover) != 0;
    if (lane == owner) {
      s = rs;
      bb = rbb;
      bu = rbu;
      over = any_over;
    }
  }
  if (mine) {
    a.sigma[off + v] = s;
    if (over) report(a.status, kErrCount, q, v);
    if (bq) {
      a.best[off + v] = __dadd_rn(a.w[off + v], bb);
      a.best_next[off + v] = bu;
    }
  }
}

struct BetweenArgs {
  int32_t n, ns, nt;
  const uint8_t *ds, *dt;
  const double *sig_s, *sig_t;
  int32_t src[kMaxPass];   // the sources' node indices (the kernels need a target only as a row of dt / sig_t)
};

// mediators: lane = (target t, node v), sources in list order
__global__ __launch_bounds__(kThreads) void trace_mediator_kernel(BetweenArgs a, double *__restrict__ med_sum, int32_t *__restrict__ med_cnt) {
  __shared__ int32_t len[kMaxPass];
  __shared__ double paths[kMaxPass];
  const int t = blockIdx.y;
  const int64_t toff = (int64_t)t * a.n;
  if (threadIdx.x < a.ns) {
    const int32_t s = a.src[threadIdx.x];
    len[threadIdx.x] = a.dt[toff + s];
    paths[threadIdx.x] = a.sig_t[toff + s];
  }
  __syncthreads();
  const int32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= a.n) return;
  const int dtv = a.dt[toff + v];
  if (dtv == 255 || dtv == 0) return;   // not on any path toward t, or t itself
  const double stv = a.sig_t[toff + v];
  double m = 0.0;
  int32_t c = 0;
  bool first = true;
  for (int s = 0; s < a.ns; ++s) {
    const int d = len[s];
    if (d == 255) continue;
    const int dsv = a.ds[(int64_t)s * a.n + v];
    if (dsv == 255 || dsv == 0 || dsv + dtv != d) continue;
    if (first) {
      m = med_sum[toff + v];
      c = med_cnt[toff + v];
      first = false;
    }
    const double through = __dmul_rn(a.sig_s[(int64_t)s * a.n + v], stv);
    m = __dadd_rn(m, __ddiv_rn(through, paths[s]));
    ++c;
  }
  if (!first) {
    med_sum[toff + v] = m;
    med_cnt[toff + v] = c;
  }
}

__device__ __forceinline__ bool on_path(const BetweenArgs &a, int s, int t, int32_t v, int d) {
  const int dsv = a.ds[(int64_t)s * a.n + v], dtv = a.dt[(int64_t)t * a.n + v];
  return dsv != 255 && dtv != 255 && dsv + dtv == d;
}

// one workgroup per pair: its length, its number of shortest paths and the number of nodes on them (the end points included)
__global__ __launch_bounds__(kThreads) void trace_pair_kernel(BetweenArgs a, int32_t *__restrict__ pair_len, double *__restrict__ pair_paths,
                                                              int32_t *__restrict__ pair_nodes) {
  __shared__ int32_t part[kWaves];
  const int t = blockIdx.x, s = blockIdx.y;
  const int32_t src = a.src[s];
  const int d = a.dt[(int64_t)t * a.n + src];
  int32_t cnt = 0;
  if (d != 255)
    for (int32_t v = threadIdx.x; v < a.n; v += kThreads) cnt += on_path(a, s, t, v, d);
#pragma unroll
  for (int m = kWave / 2; m > 0; m >>= 1) cnt += __shfl_xor(cnt, m, kWave);
  if ((threadIdx.x & (kWave - 1)) == 0) part[threadIdx.x / kWave] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    int32_t total = 0;
    for (int w = 0; w < kWaves; ++w) total += part[w];
    const int64_t i = (int64_t)s * a.nt + t;
    pair_len[i] = d == 255 ? -1 : d;
    pair_paths[i] = d == 255 ? 0.0 : a.sig_t[(int64_t)t * a.n + src];
    pair_nodes[i] = total;
  }
}

struct FillArgs {
  int64_t cap;
  const int32_t *pairs;     // [n_pairs][2]: source and target position in the pass
  const int64_t *offset;    // [n_pairs + 1]
  int32_t *node;
  uint8_t *hops_from, *hops_to;
  double *paths_from, *through, *share;
};

// one workgroup per chosen pair: the nodes on its shortest paths in ascending node index
__global__ __launch_bounds__(kThreads) void trace_fill_kernel(BetweenArgs a, FillArgs f) {
  __shared__ int32_t part[kWaves];
  const int p = blockIdx.x;
  const int s = f.pairs[2 * p], t = f.pairs[2 * p + 1];
  if ((uint32_t)s >= (uint32_t)a.ns || (uint32_t)t >= (uint32_t)a.nt) return;
  const int32_t src = a.src[s];
  const int d = a.dt[(int64_t)t * a.n + src];
  if (d == 255) return;
  const double total = a.sig_t[(int64_t)t * a.n + src];
  const int64_t end = f.offset[p + 1] < f.cap ? f.offset[p + 1] : f.cap;
  int64_t base = f.offset[p];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  for (int32_t v0 = 0; v0 < a.n; v0 += kThreads) {
    const int32_t v = v0 + threadIdx.x;
    const bool on = v < a.n && on_path(a, s, t, v, d);
    const uint64_t mask = __ballot(on);
    if (lane == 0) part[wave] = __builtin_popcountll(mask);
    __syncthreads();
    int32_t before = 0, all = 0;
    for (int w = 0; w < kWaves; ++w) {
      before += w < wave ? part[w] : 0;
      all += part[w];
    }
    const int64_t at = base + before + __builtin_popcountll(mask & ((1ull << lane) - 1));
    if (on && at >= 0 && at < end) {
      const double sv = a.sig_s[(int64_t)s * a.n + v], tv = a.sig_t[(int64_t)t * a.n + v];
      const double th = __dmul_rn(sv, tv);
      f.node[at] = v;
      f.hops_from[at] = a.ds[(int64_t)s * a.n + v];
      f.hops_to[at] = a.dt[(int64_t)t * a.n + v];
      f.paths_from[at] = sv;
      f.through[at] = th;
      f.share[at] = __ddiv_rn(th, total);
    }
    base += all;
    __syncthreads();
  }
}

int between_args(const char *what, BetweenArgs *a, int32_t n, int32_t ns, const int32_t *sources, const uint8_t *ds, const double *sig_s, int32_t nt,
                 const int32_t *targets, const uint8_t *dt, const double *sig_t) {
  GSS_REQUIRE(sources && ds && sig_s && targets && dt && sig_t, "%s: null argument", what);
  GSS_REQUIRE(n >= 1, "%s: n=%d must be >= 1", what, n);
  GSS_REQUIRE(ns >= 1 && ns <= kMaxPass, "%s: S=%d sources; a pass takes 1 to %d", what, ns, kMaxPass);
  GSS_REQUIRE(nt >= 1 && nt <= kMaxPass, "%s: T=%d targets; a pass takes 1 to %d", what, nt, kMaxPass);
  for (int32_t i = 0; i < ns; ++i)
    GSS_REQUIRE(sources[i] >= 0 && sources[i] < n, "%s: source %d = %d is not a node index in [0, %d)", what, i, sources[i], n);
  for (int32_t i = 0; i < nt; ++i)
    GSS_REQUIRE(targets[i] >= 0 && targets[i] < n, "%s: target %d = %d is not a node index in [0, %d)", what, i, targets[i], n);
  a->n = n;
  a->ns = ns;
  a->nt = nt;
  a->ds = ds;
  a->dt = dt;
  a->sig_s = sig_s;
  a->sig_t = sig_t;
  memset(a->src, 0, sizeof(a->src));
  memcpy(a->src, sources, (size_t)ns * sizeof(int32_t));
  return GSS_OK;
}

}  // namespace
}  // namespace gss

using namespace gss;

extern "C" {

int gss_paths_count(gss_paths *p, int32_t q, const int32_t *targets, const uint8_t *dist, int32_t levels, const double *w, double *sigma,
                    double *best, int32_t *best_next, void *stream) {
  GSS_REQUIRE(p && targets && dist && sigma, "paths_count: null argument");
  GSS_REQUIRE(!w == !best && !w == !best_next, "paths_count: w, best and best_next are given together or not at all");
  GSS_REQUIRE(q >= 1 && q <= kMaxPass, "paths_count: Q=%d targets; a pass takes 1 to %d", q, kMaxPass);
  GSS_REQUIRE(levels >= 0 && levels <= kMaxLevel, "paths_count: levels=%d is outside 0..%d", levels, kMaxLevel);
  PathsView g;
  if (int rc = paths_view(p, &g)) return rc;
  for (int32_t i = 0; i < q; ++i)
    GSS_REQUIRE(targets[i] >= 0 && targets[i] < g.n, "paths_count: target %d = %d is not a node index in [0, %d)", i, targets[i], g.n);
  const int per = w ? 1 + 4 + 8 + 8 + 4 + 8 : 1 + 4 + 8;
  const int64_t need = (int64_t)per * q * g.n + (int64_t)24 * g.n;
  GSS_REQUIRE(need <= g.max_bytes,
              "paths_count: the pass needs %lld bytes (%d Q N: dist 1 + next 4%s + sigma 8%s, + 24 N of state, Q=%d N=%d), above the budget "
              "max_bytes=%lld",
              (long long)need, per, w ? " + w 8" : "", w ? " + best_next 4 + best 8" : "", q, g.n, (long long)g.max_bytes);
  hipStream_t st = as_stream(stream);
  GSS_HIP(hipMemcpyAsync(g.targets, targets, (size_t)q * 4, hipMemcpyHostToDevice, st));
  GSS_HIP(hipMemsetAsync(g.status, 0, sizeof(unsigned long long), st));
  if (g.nnz > 1) {
    trace_duplicate_kernel<<<ceil_div(g.nnz, kThreads), kThreads, 0, st>>>(g.n, g.nnz, g.rowptr, g.col, g.status);
    GSS_LAUNCH_CHECK("trace_duplicate_kernel");
  }
  CountArgs a;
  a.n = g.n;
  a.level = 0;
  a.levels = levels;
  a.rowptr = g.rowptr;
  a.col = g.col;
  a.targets = g.targets;
  a.dist = dist;
  a.w = w;
  a.sigma = sigma;
  a.best = best;
  a.best_next = best_next;
  a.status = g.status;
  const dim3 grid(ceil_div(g.n, kThreads), q);
  trace_init_kernel<<<grid, kThreads, 0, st>>>(a);
  GSS_LAUNCH_CHECK("trace_init_kernel");
  // the level launches back to back: nothing is read back between them
  for (int32_t L = 1; L <= levels; ++L) {
    a.level = L;
    trace_level_kernel<<<grid, kThreads, 0, st>>>(a);
    GSS_LAUNCH_CHECK("trace_level_kernel");
  }
  if (int rc = read_back(g.h_status, g.status, sizeof(unsigned long long), st)) return rc;
  const unsigned long long status = *g.h_status;
  if (status) {
    const int code = (int)(status >> 56), tq = (int)((status >> 32) & 0xff);
    const int32_t v = (int32_t)(status & 0xffffffffu);
    const int32_t t = tq < q ? targets[tq] : -1;
    switch (code) {
      case kErrDuplicate:
        return fail(GSS_EINVAL, "paths_count: row %d of the graph holds a column twice; the counts need every edge once", v);
      case kErrTargetDist:
        return fail(GSS_EINVAL, "paths_count: dist of target %d (node %d) at node %d is not 0 exactly at the target: not the dist of a gss_paths_run "
                                "pass with these targets", tq, t, v);
      case kErrLevels:
        return fail(GSS_EINVAL, "paths_count: levels=%d is smaller than the distance of node %d from target %d (node %d)", levels, v, tq, t);
      case kErrWeight:
        return fail(GSS_EINVAL, "paths_count: the weight of node %d for target %d (node %d) is not finite", v, tq, t);
      case kErrCount:
        return fail(GSS_EINVAL, "paths_count: node %d has more than 2^53 shortest paths to target %d (node %d); the counts are exact integers "
                                "in fp64 and are not rounded", v, tq, t);
      default:
        return fail(GSS_EHIP, "paths_count: unknown status word %llx", status);
    }
  }
  return GSS_OK;
}

int gss_paths_between(int32_t n, int32_t ns, const int32_t *sources, const uint8_t *dist_s, const double *sigma_s, int32_t nt,
                      const int32_t *targets, const uint8_t *dist_t, const double *sigma_t, int32_t *pair_len, double *pair_paths,
                      int32_t *pair_nodes, double *med_sum, int32_t *med_count, void *stream) {
  BetweenArgs a;
  if (int rc = between_args("paths_between", &a, n, ns, sources, dist_s, sigma_s, nt, targets, dist_t, sigma_t)) return rc;
  GSS_REQUIRE(pair_len && pair_paths && pair_nodes, "paths_between: null pair output");
  GSS_REQUIRE(!med_sum == !med_count, "paths_between: med_sum and med_count are given together or not at all");
  hipStream_t st = as_stream(stream);
  trace_pair_kernel<<<dim3(nt, ns), kThreads, 0, st>>>(a, pair_len, pair_paths, pair_nodes);
  GSS_LAUNCH_CHECK("trace_pair_kernel");
  if (med_sum) {
    trace_mediator_kernel<<<dim3(ceil_div(n, kThreads), nt), kThreads, 0, st>>>(a, med_sum, med_count);
    GSS_LAUNCH_CHECK("trace_mediator_kernel");
  }
  return GSS_OK;
}

int gss_paths_between_fill(int32_t n, int32_t ns, const int32_t *sources, const uint8_t *dist_s, const double *sigma_s, int32_t nt,
                           const int32_t *targets, const uint8_t *dist_t, const double *sigma_t, int32_t n_pairs, const int32_t *pairs,
                           const int64_t *offset, int64_t capacity, int32_t *node, uint8_t *hops_from, uint8_t *hops_to, double *paths_from,
                           double *through, double *share, void *stream) {
  BetweenArgs a;
  if (int rc = between_args("paths_between_fill", &a, n, ns, sources, dist_s, sigma_s, nt, targets, dist_t, sigma_t)) return rc;
  GSS_REQUIRE(n_pairs >= 0 && n_pairs <= kMaxPass * kMaxPass, "paths_between_fill: %d pairs; a pass has at most %d", n_pairs, kMaxPass * kMaxPass);
  GSS_REQUIRE(capacity >= 0, "paths_between_fill: capacity=%lld is negative", (long long)capacity);
  if (n_pairs == 0 || capacity == 0) return GSS_OK;
  GSS_REQUIRE(pairs && offset && node && hops_from && hops_to && paths_from && through && share, "paths_between_fill: null argument");
  FillArgs f;
  f.cap = capacity;
  f.pairs = pairs;
  f.offset = offset;
  f.node = node;
  f.hops_from = hops_from;
  f.hops_to = hops_to;
  f.paths_from = paths_from;
  f.through = through;
  f.share = share;
  trace_fill_kernel<<<n_pairs, kThreads, 0, as_stream(stream)>>>(a, f);
  GSS_LAUNCH_CHECK("trace_fill_kernel");
  return GSS_OK;
}

}  // extern "C"

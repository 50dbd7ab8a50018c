// paths.hip -- shortest-path trees toward up to 64 targets per pass (predict_drug.py:268-273 / run_covid.py:310-319 ran one
// networkx bidirectional BFS per table row; one search toward the query node answers every row).
//
// Level-synchronous, bottom-up over the forward CSR, so no transpose is needed (include/gssgcn.h has the contract, DESIGN.md
// section 9.3 the cost model and the measurements).  Bit q of a uint64 stands for target q:
//   seen[v]        targets whose distance from v is known;
//   front_cur[u]   targets at distance L - 1 from u (the frontier of the previous level), front_next[v] the same for level L.
// At level L every node v with need = valid & ~seen[v] != 0 reads its own row in column order; successor u claims
// front_cur[u] & need & ~claimed, so a bit goes to the first (smallest-index) successor that is one hop closer -- the tie rule.
// A row of more than kShortRow entries is read by the whole wave, 64 entries at a time, and the first-claim rule becomes an
// exclusive prefix-OR of the lanes' masks in lane order.  Every result word is written by the one lane that owns it (no atomics
// on results: bitwise deterministic); the only atomic is the per-level "something changed" flag the host reads.
#include <algorithm>

#include "device_scope.h"
#include "ops.h"

struct PathsWords {            // what the kernels report through, on the device and as a pinned host copy
  int32_t flag;                // a level's word: 1 changed, 2 a node 255+ hops away, 4 a bad column
  unsigned long long status;   // the status of a count pass (trace.hip)
};

struct __attribute__((visibility("hidden"))) gss_paths {
  int32_t n;
  int64_t nnz;
  int64_t max_bytes;
  const int32_t *rowptr, *col;   // device CSR (owned when uploaded)
  gss::DeviceBuf<int32_t> own_rowptr, own_col;
  gss::DeviceBuf<uint64_t> seen, front[2];   // [n] each: 24 n bytes of state
  gss::DeviceBuf<PathsWords> words;
  gss::DeviceBuf<PathsWords, true> h_words;
  gss::DeviceBuf<int32_t> targets;   // [kMaxTargets] device
};

namespace gss {
namespace {

constexpr int kMaxTargets = 64;
constexpr int kMaxLevel = 254;    // dist is one byte and 255 means unreachable
constexpr int kShortRow = 32;     // rows up to this many entries are read by one lane
constexpr int kLevelThreads = 256;

__global__ __launch_bounds__(256) void paths_check_kernel(int32_t n, int64_t nnz, const int32_t *__restrict__ rowptr,
                                                          const int32_t *__restrict__ col, int32_t *__restrict__ flag) {
  const int32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n) return;
  const int32_t b = rowptr[v], e = rowptr[v + 1];
  if (b < 0 || e < b || (int64_t)e > nnz || (v == 0 && b != 0)) {
    atomicOr(flag, 1);
    return;
  }
  for (int32_t i = b; i < e; ++i) {
    const int32_t u = col[i];
    if (u < 0 || u >= n) atomicOr(flag, 2);
    else if (i > b && u < col[i - 1]) atomicOr(flag, 4);
  }
}

__global__ __launch_bounds__(256) void paths_init_kernel(int32_t n, int32_t q, const int32_t *__restrict__ targets,
                                                         uint64_t *__restrict__ seen, uint64_t *__restrict__ front, uint8_t *__restrict__ dist,
                                                         int32_t *__restrict__ next) {
  __shared__ int32_t t[kMaxTargets];
  if (threadIdx.x < q) t[threadIdx.x] = targets[threadIdx.x];
  __syncthreads();
  const int32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n) return;
  uint64_t m = 0;
  for (int32_t i = 0; i < q; ++i) {
    const bool hit = t[i] == v;
    m |= (uint64_t)hit << i;
    dist[(int64_t)i * n + v] = hit ? 0 : 255;
    next[(int64_t)i * n + v] = -1;
  }
  seen[v] = m;
  front[v] = m;
}

__device__ __forceinline__ uint64_t shfl_up_u64(uint64_t x, int d) {
  const uint32_t lo = __shfl_up((uint32_t)x, d), hi = __shfl_up((uint32_t)(x >> 32), d);
  return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t shfl_u64(uint64_t x, int src) {
  const uint32_t lo = __shfl((uint32_t)x, src), hi = __shfl((uint32_t)(x >> 32), src);
  return ((uint64_t)hi << 32) | lo;
}

struct LevelArgs {
  int32_t n, level;
  uint64_t valid;
  const int32_t *rowptr, *col;
  const uint64_t *front_cur;
  uint64_t *front_next, *seen;
  uint8_t *dist;
  int32_t *next, *flag;
};

__device__ __forceinline__ void write_bits(const LevelArgs &a, int32_t v, int32_t u, uint64_t bits) {
  while (bits) {
    const int q = __builtin_ctzll(bits);
    bits &= bits - 1;
    a.next[(int64_t)q * a.n + v] = u;
    a.dist[(int64_t)q * a.n + v] = (uint8_t)a.level;
  }
}

// one lane per node; the lanes whose row is long hand it to the whole wave afterwards, one row at a time (ballot loop)
__global__ __launch_bounds__(kLevelThreads) void paths_level_kernel(LevelArgs a) {
  const int32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & (kWave - 1);
  const bool probe = a.level > kMaxLevel;   // a level past 254 only asks whether anything would still be found
  uint64_t need = 0, claimed = 0;
  int32_t b = 0, e = 0;
  bool changed = false, bad = false;
  if (v < a.n) {
    need = a.valid & ~a.seen[v];
    if (need) {
      b = a.rowptr[v];
      e = a.rowptr[v + 1];
    }
  }
  const bool lng = need && e - b > kShortRow;
  if (need && !lng) {
    for (int32_t i = b; i < e; ++i) {
      const int32_t u = a.col[i];
      if ((uint32_t)u >= (uint32_t)a.n) {
        bad = true;
        continue;
      }
      const uint64_t m = a.front_cur[u] & need & ~claimed;
      if (m) {
        claimed |= m;
        if (!probe) write_bits(a, v, u, m);
        if (claimed == need) break;
      }
    }
  }
  // long rows: the wave reads each one 64 entries at a time; lane order is row order, so the first claim of a bit is the lowest lane
  // that carries it: new = m & ~(OR of the masks of the lanes below)
  uint64_t todo = __ballot(lng);
  while (todo) {
    const int owner = __builtin_ctzll(todo);
    todo &= todo - 1;
    const int32_t rv = __shfl(v, owner), rb = __shfl(b, owner), re = __shfl(e, owner);
    const uint64_t rneed = shfl_u64(need, owner);
    uint64_t rclaimed = 0;
    for (int32_t base = rb; base < re && rclaimed != rneed; base += kWave) {
      const int32_t i = base + lane;
      int32_t u = -1;
      uint64_t m = 0;
      if (i < re) {
        u = a.col[i];
        if ((uint32_t)u >= (uint32_t)a.n) bad = true;
        else m = a.front_cur[u] & rneed & ~rclaimed;
      }
      uint64_t incl = m;
      for (int d = 1; d < kWave; d <<= 1) {
        const uint64_t y = shfl_up_u64(incl, d);
        if (lane >= d) incl |= y;
      }
      uint64_t excl = shfl_up_u64(incl, 1);
      if (lane == 0) excl = 0;
      const uint64_t mine = m & ~excl;
      if (mine && !probe) write_bits(a, rv, u, mine);
      rclaimed |= shfl_u64(incl, kWave - 1);
    }
    if (lane == owner) claimed = rclaimed;
  }
  if (v < a.n) {
    if (claimed) {
      changed = true;
      if (!probe) a.seen[v] |= claimed;
    }
    if (!probe) a.front_next[v] = claimed;
  }
  const uint64_t any_changed = __ballot(changed), any_bad = __ballot(bad);
  if (lane == 0 && (any_changed || any_bad)) atomicOr(a.flag, (any_changed ? (probe ? 2 : 1) : 0) | (any_bad ? 4 : 0));
}

}  // namespace

// what a count pass (trace.hip) needs of a handle
int paths_view(const gss_paths *p, PathsView *out) {
  out->n = p->n;
  out->nnz = p->nnz;
  out->max_bytes = p->max_bytes;
  out->rowptr = p->rowptr;
  out->col = p->col;
  out->targets = p->targets.p;
  out->status = &p->words.p->status;
  out->h_status = &p->h_words.p->status;
  return GSS_OK;
}

}  // namespace gss

using namespace gss;

extern "C" {

int gss_paths_create(gss_paths **out, int32_t n, int64_t nnz, const int32_t *rowptr, const int32_t *col, int32_t on_device,
                     int64_t max_bytes, void *stream) {
  GSS_REQUIRE(out, "paths_create: null handle pointer");
  *out = nullptr;
  GSS_REQUIRE(n >= 1 && nnz >= 0, "paths_create: n=%d must be >= 1 and nnz=%lld >= 0", n, (long long)nnz);
  GSS_REQUIRE(nnz <= INT32_MAX, "paths_create: nnz=%lld does not fit the int32 row pointers", (long long)nnz);
  GSS_REQUIRE(rowptr && (col || nnz == 0), "paths_create: null rowptr / col");
  const int64_t state = (int64_t)24 * n;
  GSS_REQUIRE(state + (int64_t)5 * n <= max_bytes,
              "paths_create: one target needs %lld bytes (24 N of state + 5 N of output, N=%d), above the budget max_bytes=%lld",
              (long long)(state + (int64_t)5 * n), n, (long long)max_bytes);
  hipStream_t st = as_stream(stream);
  std::unique_ptr<gss_paths> p(new gss_paths());
  p->n = n;
  p->nnz = nnz;
  p->max_bytes = max_bytes;
  const char *who = "paths_create";
  if (p->seen.alloc(who, (size_t)n * 8) || p->front[0].alloc(who, (size_t)n * 8) || p->front[1].alloc(who, (size_t)n * 8) ||
      p->words.alloc(who, sizeof(PathsWords)) || p->targets.alloc(who, kMaxTargets * sizeof(int32_t)) || p->h_words.alloc(who, sizeof(PathsWords)) ||
      (!on_device && (p->own_rowptr.alloc(who, (size_t)(n + 1) * 4) || p->own_col.alloc(who, (size_t)std::max<int64_t>(nnz, 1) * 4))))
    return fail(GSS_ENOMEM, "paths_create: device allocation failed (N=%d, nnz=%lld)", n, (long long)nnz);
  if (!on_device) {
    GSS_HIP(hipMemcpyAsync(p->own_rowptr.p, rowptr, (size_t)(n + 1) * 4, hipMemcpyHostToDevice, st));
    if (nnz) GSS_HIP(hipMemcpyAsync(p->own_col.p, col, (size_t)nnz * 4, hipMemcpyHostToDevice, st));
    p->rowptr = p->own_rowptr.p;
    p->col = p->own_col.p;
  } else {
    p->rowptr = rowptr;
    p->col = col;
  }
  int32_t *flag = &p->words.p->flag, *h_flag = &p->h_words.p->flag;
  GSS_HIP(hipMemsetAsync(flag, 0, sizeof(int32_t), st));
  paths_check_kernel<<<ceil_div(n, 256), 256, 0, st>>>(n, nnz, p->rowptr, p->col, flag);
  GSS_LAUNCH_CHECK("paths_check_kernel");
  if (int rc = read_back(h_flag, flag, sizeof(int32_t), st)) return rc;
  GSS_REQUIRE(!(*h_flag & 1), "paths_create: rowptr is not a CSR row pointer (0 first, non-decreasing, <= nnz=%lld)", (long long)nnz);
  GSS_REQUIRE(!(*h_flag & 2), "paths_create: a column index is outside [0, %d)", n);
  GSS_REQUIRE(!(*h_flag & 4), "paths_create: the columns of a row are not ascending (the tie rule needs row order = index order)");
  *out = p.release();
  return GSS_OK;
}

void gss_paths_destroy(gss_paths *p) { delete p; }

int gss_paths_run(gss_paths *p, int32_t q, const int32_t *targets, uint8_t *dist, int32_t *next, int32_t *levels, void *stream) {
  GSS_REQUIRE(p && targets && dist && next, "paths_run: null argument");
  GSS_REQUIRE(q >= 1 && q <= kMaxTargets, "paths_run: Q=%d targets; a pass takes 1 to %d", q, kMaxTargets);
  for (int32_t i = 0; i < q; ++i)
    GSS_REQUIRE(targets[i] >= 0 && targets[i] < p->n, "paths_run: target %d = %d is not a node index in [0, %d)", i, targets[i], p->n);
  const int64_t need = (int64_t)q * p->n * 5 + (int64_t)24 * p->n;
  GSS_REQUIRE(need <= p->max_bytes, "paths_run: the pass needs %lld bytes (5 Q N of output + 24 N of state, Q=%d N=%d), above the budget max_bytes=%lld",
              (long long)need, q, p->n, (long long)p->max_bytes);
  hipStream_t st = as_stream(stream);
  GSS_HIP(hipMemcpyAsync(p->targets.p, targets, (size_t)q * 4, hipMemcpyHostToDevice, st));
  paths_init_kernel<<<ceil_div(p->n, 256), 256, 0, st>>>(p->n, q, p->targets.p, p->seen.p, p->front[0].p, dist, next);
  GSS_LAUNCH_CHECK("paths_init_kernel");
  LevelArgs a;
  a.n = p->n;
  a.valid = q == 64 ? ~0ull : ((1ull << q) - 1);
  a.rowptr = p->rowptr;
  a.col = p->col;
  a.seen = p->seen.p;
  a.dist = dist;
  a.next = next;
  a.flag = &p->words.p->flag;
  int32_t *h_flag = &p->h_words.p->flag;
  int32_t level = 0;
  for (int32_t L = 1;; ++L) {
    a.level = L;
    a.front_cur = p->front[(L - 1) & 1].p;
    a.front_next = p->front[L & 1].p;
    GSS_HIP(hipMemsetAsync(a.flag, 0, sizeof(int32_t), st));
    paths_level_kernel<<<ceil_div(p->n, kLevelThreads), kLevelThreads, 0, st>>>(a);
    GSS_LAUNCH_CHECK("paths_level_kernel");
    if (int rc = read_back(h_flag, a.flag, sizeof(int32_t), st)) return rc;
    const int32_t flag = *h_flag;
    GSS_REQUIRE(!(flag & 4), "paths_run: a column index is outside [0, %d)", p->n);
    GSS_REQUIRE(!(flag & 2), "paths_run: a node lies 255 or more hops from a target; hop counts are stored in one byte (depth <= %d)",
                kMaxLevel);
    if (!(flag & 1)) break;
    level = L;
  }
  if (levels) *levels = level;
  return GSS_OK;
}

}  // extern "C"

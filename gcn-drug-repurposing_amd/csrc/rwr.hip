// rwr.hip -- random walk with restart (network propagation) from seed sets, and its null against degree-matched random seed sets.
// include/gssgcn.h has the contract, the statistic and the summation order; DESIGN.md section 9.21 the LDS budget and the cost model.
//
// gss_rwr_rank: one kernel, one unit (one row of a seed table, admitted as seed_units.h states) per workgroup at a time.  Node i belongs
// to thread i % 1024, which keeps p[i] in register i / 1024 for all iterations; q[j] = p[j] / deg[j] of every node lives in LDS, so an
// iteration reads the column index (from L2) and q (from LDS) and nothing else.  The wave that owns a row sums it: a row of up to 32
// entries by its owner's lane alone, a longer row by the 64 lanes of the owner's wave -- the owner keeps the butterfly's result, so no
// sum ever leaves its wave.  The order of every sum is fixed by (n, CSR) alone: the same bits on every run, at every table position.
// gss_rwr_null_stats: a thread per (set, node) walks the samples in ascending order; then one workgroup per set ranks.
// Both end in the same selection (TopSelect): 4,096 (key, key, node) triples in LDS, the best 1,024 so far in front, 3,072 nodes fed
// per round, rank_keys.h's order-preserving keys under a bitonic sort whose order is total.  The only global atomics are the status
// word's atomicOr and the integer count of the units that did not converge.
#include <algorithm>
#include <cmath>

#include "rank_keys.h"
#include "seed_units.h"

// the contract's p', err, mean and sd are sequences of single IEEE operations: no multiply-add may be formed of them
#pragma clang fp contract(off)

namespace gss {
namespace {

constexpr int kThreads = 1024;           // one workgroup per CU (the LDS decides that)
constexpr int kWaves = kThreads / 64;
constexpr int32_t kLdsBudget = 163840;   // what a workgroup may declare
constexpr int32_t kStatic = 3840;        // kept for the static words (the error's 16 partial sums, the barrier's vote)
constexpr int32_t kMaxN = (kLdsBudget - kStatic) / (int32_t)sizeof(double);   // 20,000: q is 8 n bytes
constexpr int kPer = (kMaxN + kThreads - 1) / kThreads;                       // 20 nodes per thread at the most
constexpr int32_t kLongRow = 32;         // a row of more entries than this is summed by its owner's wave, not by one lane
constexpr int32_t kMaxAdd = 1024;        // the selection's head (profile_topk.hip's cap)
constexpr int32_t kSel = 4096;           // triples the selection sorts at a time
constexpr int32_t kFeed = kSel - kMaxAdd;   // nodes fed per round: three per thread
constexpr int kFeedPer = kFeed / kThreads;
constexpr int kRounds = (kPer + kFeedPer - 1) / kFeedPer;
constexpr int32_t kSelBytes = kSel * (2 * (int32_t)sizeof(uint64_t) + (int32_t)sizeof(int32_t));   // 81,920
constexpr int32_t kMaxSeeds = 4096;      // the seed table's row length, as gss_diamond_grow's
constexpr int kMaxBlocks = 2048;         // workgroups walk the units with this stride
constexpr int kRowEmpty = 16;            // beside seed_units.h's bits: a row of the CSR has no entry
static_assert(kThreads == kMaxAdd, "TopSelect::begin: a thread per slot of the head");
static_assert(kMaxN == 20000 && kPer == 20 && kFeedPer == 3 && kRounds == 7, "the budget of DESIGN.md section 9.21");
static_assert(kSelBytes + kMaxN / 8 + 4 <= kLdsBudget - kStatic, "gss_rwr_null_stats: the selection beside a membership bit per node");

// bitonic sort of cpad (key, key, node) triples, ascending by the first key, then the second, then the node: rank_keys.h's sort_pairs
// with one more key.  Made of barriers: every thread of the workgroup must reach the call
template <int THREADS>
__device__ __forceinline__ void sort_triples(uint64_t *k1, uint64_t *k2, int32_t *idx, int32_t cpad, int32_t tid) {
  for (int32_t k = 2; k <= cpad; k <<= 1) {
    for (int32_t j = k >> 1; j > 0; j >>= 1) {
      for (int32_t i = tid; i < cpad / 2; i += THREADS) {
        const int32_t lo = ((i & ~(j - 1)) << 1) | (i & (j - 1)), hi = lo + j;
        const uint64_t x = k1[lo], y = k1[hi], x2 = k2[lo], y2 = k2[hi];
        const int32_t ix = idx[lo], iy = idx[hi];
        const bool above = x > y || (x == y && (x2 > y2 || (x2 == y2 && ix > iy)));
        if (above == ((lo & k) == 0)) {
          k1[lo] = y;
          k1[hi] = x;
          k2[lo] = y2;
          k2[hi] = x2;
          idx[lo] = iy;
          idx[hi] = ix;
        }
      }
      __syncthreads();
    }
  }
}

// The selection both ops end in.  The first kMaxAdd triples are the best seen so far; a round feeds kFeed more behind them and sorts.
// A node that is no candidate is fed as (kBehind, kBehind, INT32_MAX) and sorts behind every candidate.
struct TopSelect {
  uint64_t *k1, *k2;
  int32_t *idx;
  __device__ __forceinline__ explicit TopSelect(void *lds)
      : k1(static_cast<uint64_t *>(lds)), k2(k1 + kSel), idx(reinterpret_cast<int32_t *>(k2 + kSel)) {}
  __device__ __forceinline__ void put(int32_t slot, uint64_t a, uint64_t b, int32_t v) {
    k1[slot] = a;
    k2[slot] = b;
    idx[slot] = v;
  }
  __device__ __forceinline__ void none(int32_t slot) { put(slot, kBehind, kBehind, INT32_MAX); }
  // a key that sorts the larger value first
  static __device__ __forceinline__ uint64_t falling(double x) { return ~order_key(x); }
  __device__ __forceinline__ void begin(int32_t tid) { none(tid); }                    // tid in [0, kMaxAdd); the first round's barrier follows
  __device__ __forceinline__ void round(int32_t tid) {
    __syncthreads();
    sort_triples<kThreads>(k1, k2, idx, kSel, tid);
  }
  // the node at rank r in [0, kMaxAdd), -1 past the candidates; after a round
  __device__ __forceinline__ int32_t at(int32_t r) const { return idx[r] == INT32_MAX ? -1 : idx[r]; }
};

struct RankArgs {
  int32_t n, max_deg, max_size, n_add, max_iter;
  int64_t n_units;
  const int32_t *rowptr, *col, *nodes, *sizes;
  double restart, tol;
  int32_t *node, *iters, *flag, *notconv;
  double *score, *p_out;
};

// q of a column; a column that is no node (the caller's CSR is not the one the contract asks for) adds nothing and reads nothing
__device__ __forceinline__ double q_at(const double *q, int32_t c, int32_t n) { return (uint32_t)c < (uint32_t)n ? q[c] : 0.0; }

// The thread's index as a value the compiler knows nothing about.  Each phase of the rank kernel takes it anew: what twenty unrolled
// nodes per thread derive from it (indices, addresses, bounds) is then computed where it is used, not kept in registers over the whole
// kernel, where it would push p into scratch
__device__ __forceinline__ int32_t anew(int32_t tid) {
  asm volatile("" : "+v"(tid));
  return tid;
}

__device__ __forceinline__ double wave_sum(double x) {      // the butterfly: partners at distance 32, 16, 8, 4, 2, 1; every lane ends with the sum
  for (int o = 32; o > 0; o >>= 1) x = x + __shfl_xor(x, o);
  return x;
}

__global__ __launch_bounds__(kThreads) void rwr_rank_kernel(RankArgs a) {
  extern __shared__ double dyn[];
  double *q = dyn;
  uint32_t *bits = reinterpret_cast<uint32_t *>(dyn);      // the unit's membership, until every thread has its own bits in a register
  __shared__ double red[kWaves];
  const int32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int32_t n = a.n, words = (n + 31) >> 5;
  const double restart = a.restart, keep = 1.0 - a.restart, nan = __longlong_as_double(0x7ff8000000000000ll);
  for (int64_t u = blockIdx.x; u < a.n_units; u += gridDim.x) {
    const int32_t m = unit_size(a.sizes, u, a.max_size, a.flag);
    if (m < 0) continue;
    const int32_t *x = a.nodes + u * a.max_size;
    int bad = 0;
    for (int32_t v = tid; v < n; v += kThreads) {
      bad |= unit_row_bits(a.rowptr, v, a.max_deg);
      if (a.rowptr[v + 1] == a.rowptr[v]) bad |= kRowEmpty;
    }
    for (int32_t i = tid; i < m; i += kThreads) bad |= unit_member_bits(x, i, n);
    for (int32_t i = tid; i < words; i += kThreads) bits[i] = 0;
    if (unit_refused(bad, a.flag)) continue;             // no row of a refused unit is walked; a barrier
    const int64_t out = u * a.n_add;
    if (m == 0) {                                        // an empty unit: nothing to walk from
      if (tid == 0) a.iters[u] = 0;
      if (a.node)
        for (int32_t i = tid; i < a.n_add; i += kThreads) {
          a.node[out + i] = -1;
          a.score[out + i] = nan;
        }
      if (a.p_out)
        for (int32_t v = tid; v < n; v += kThreads) a.p_out[u * n + v] = nan;
      continue;
    }
    for (int32_t i = tid; i < m; i += kThreads) atomicOr(&bits[x[i] >> 5], 1u << (x[i] & 31));
    __syncthreads();
    uint32_t mine = 0;                                   // bit k: node k * 1024 + tid is a seed
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
      const int32_t v = k * kThreads + anew(tid);
      if (v < n && ((bits[v >> 5] >> (v & 31)) & 1)) mine |= 1u << k;
    }
    __syncthreads();                                     // bits is read: q may take its place
    const double p0 = 1.0 / (double)m;
    double p[kPer];
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
      const int32_t v = k * kThreads + anew(tid);
      p[k] = (mine >> k) & 1 ? p0 : 0.0;
      if (v < n) q[v] = p[k] / (double)(a.rowptr[v + 1] - a.rowptr[v]);
      __builtin_amdgcn_sched_barrier(0);                 // one division at a time: twenty in flight would not fit the registers
    }
    __syncthreads();
    int32_t it = 0;
    bool done = false;
    while (it < a.max_iter && !done) {
      ++it;
      // the row pointers are read anew in every iteration: kept over the loop, two words and a divisor per node would not fit the registers
      const int32_t *rowptr = a.rowptr;
      asm volatile("" : "+s"(rowptr));
      double err = 0.0;
#pragma unroll
      for (int k = 0; k < kPer; ++k) {
        const int32_t v = k * kThreads + anew(tid);
        if (k * kThreads < n) {                          // the same for every thread of the workgroup
          int32_t lo = 0, hi = 0;
          if (v < n) {
            lo = rowptr[v];
            hi = rowptr[v + 1];
          }
          double s = 0.0;
          if (hi - lo <= kLongRow)                       // the lane's own row, entry by entry
            for (int32_t e = lo; e < hi; ++e) s = s + q_at(q, a.col[e], n);
          unsigned long long wide = __ballot(hi - lo > kLongRow);
          while (wide) {                                 // the wave's long rows, in ascending node order
            const int b = __ffsll((long long)wide) - 1;
            wide &= wide - 1;
            const int32_t rhi = __shfl(hi, b);
            double part = 0.0;
            for (int32_t e = __shfl(lo, b) + lane; e < rhi; e += 64) part = part + q_at(q, a.col[e], n);
            part = wave_sum(part);
            if (lane == b) s = part;
          }
          if (v < n) {
            const double walk = keep * s, back = restart * ((mine >> k) & 1 ? p0 : 0.0);
            const double next = walk + back;
            err = err + fabs(next - p[k]);
            p[k] = next;
          }
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      err = wave_sum(err);
      if (lane == 0) red[w] = err;
      __syncthreads();                                   // every row is summed: q may be written
      err = red[0];
      for (int i = 1; i < kWaves; ++i) err = err + red[i];
      done = err < a.tol;
      asm volatile("" : "+s"(rowptr));                   // and once more: the lengths read above are not kept for the divisions either
#pragma unroll
      for (int k = 0; k < kPer; ++k) {
        const int32_t v = k * kThreads + anew(tid);
        if (v < n) q[v] = p[k] / (double)(rowptr[v + 1] - rowptr[v]);
        __builtin_amdgcn_sched_barrier(0);
      }
      __syncthreads();                                   // and red is free
    }
    if (tid == 0) {
      a.iters[u] = it;
      if (!done && a.tol > 0.0) atomicAdd(a.notconv, 1);
    }
    if (a.p_out) {
#pragma unroll
      for (int k = 0; k < kPer; ++k) {
        const int32_t v = k * kThreads + anew(tid);
        if (v < n) a.p_out[u * n + v] = p[k];
      }
    }
    if (!a.node) continue;                               // the loop's last barrier stands between this unit's q and the next one's bits
    TopSelect sel(dyn);
    sel.begin(tid);
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
      if (r * kFeed < n) {                               // the same for every thread
#pragma unroll
        for (int c = 0; c < kFeedPer; ++c) {
          const int k = r * kFeedPer + c;
          const int32_t t = anew(tid), v = k * kThreads + t, slot = kMaxAdd + c * kThreads + t;
          if (k < kPer && v < n && !((mine >> k) & 1)) sel.put(slot, TopSelect::falling(p[k < kPer ? k : 0]), 0, v);
          else sel.none(slot);
        }
        sel.round(tid);
      }
    }
    for (int32_t i = tid; i < a.n_add; i += kThreads) {
      const int32_t v = sel.at(i);
      a.node[out + i] = v;
      // the key holds the score's bits: p >= 0, so its key is the bits with the sign set, and falling() is their complement
      a.score[out + i] = v < 0 ? nan : __longlong_as_double((long long)(~sel.k1[i] & 0x7fffffffffffffffull));
    }
    __syncthreads();                                     // the selection is read before the next unit writes bits
  }
}

struct NullArgs {
  int32_t n, R, max_size, n_add, by_z, n_sets;
  const double *p;
  const int32_t *nodes, *sizes;
  double *mean, *sd, *z;
  int32_t *ge, *node, *flag;
};

// mean, sd, z and ge of every (set, node): a thread per node walks the samples 1 .. R - 1 in ascending order
__global__ __launch_bounds__(256) void rwr_null_stats_kernel(NullArgs a) {
  const int32_t s = blockIdx.y, v = blockIdx.x * 256 + threadIdx.x, n = a.n, R = a.R;
  if (v >= n) return;
  const double nan = __longlong_as_double(0x7ff8000000000000ll), count = (double)(R - 1);
  const double *obs = a.p + (int64_t)s * R * n;
  double mean = nan, sd = nan, z = nan;
  int32_t ge = -1;
  if (a.sizes[(int64_t)s * R] != 0) {                    // an empty set has no walk
    const double o = obs[v];
    double sum = 0.0;
    ge = 0;
    for (int32_t k = 1; k < R; ++k) {
      const double y = obs[(int64_t)k * n + v];
      sum = sum + y;
      ge += y >= o;
    }
    mean = sum / count;
    double sq = 0.0;
    for (int32_t k = 1; k < R; ++k) {
      const double d = obs[(int64_t)k * n + v] - mean;
      const double dd = d * d;
      sq = sq + dd;
    }
    sd = sqrt(sq / count);
    z = sd > 0.0 ? (o - mean) / sd : 0.0;
  }
  const int64_t at = (int64_t)s * n + v;
  a.mean[at] = mean;
  a.sd[at] = sd;
  a.z[at] = z;
  a.ge[at] = ge;
}

// after it, on the same stream: a workgroup per set admits the set itself (sample 0), gives its seeds z = NaN and ranks the rest
__global__ __launch_bounds__(kThreads) void rwr_null_select_kernel(NullArgs a) {
  extern __shared__ double dyn[];
  uint32_t *bits = reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(dyn) + kSelBytes);
  const int32_t tid = threadIdx.x, n = a.n, words = (n + 31) >> 5;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  for (int32_t s = blockIdx.x; s < a.n_sets; s += gridDim.x) {
    const int64_t unit = (int64_t)s * a.R;               // sample 0: the set itself
    const int32_t m = unit_size(a.sizes, unit, a.max_size, a.flag);
    if (m < 0) continue;
    const int32_t *x = a.nodes + unit * a.max_size;
    int bad = 0;
    for (int32_t i = tid; i < m; i += kThreads) bad |= unit_member_bits(x, i, n);
    for (int32_t i = tid; i < words; i += kThreads) bits[i] = 0;
    if (unit_refused(bad, a.flag)) continue;
    const double *obs = a.p + unit * n;
    const int64_t row = (int64_t)s * n, out = (int64_t)s * a.n_add;
    for (int32_t i = tid; i < m; i += kThreads) {
      atomicOr(&bits[x[i] >> 5], 1u << (x[i] & 31));
      a.z[row + x[i]] = nan;
    }
    TopSelect sel(dyn);
    sel.begin(tid);
    __syncthreads();
    if (m > 0) {
      for (int32_t base = 0; base < n; base += kFeed) {
        for (int c = 0; c < kFeedPer; ++c) {
          const int32_t v = base + c * kThreads + tid, slot = kMaxAdd + c * kThreads + tid;
          if (v < n && !((bits[v >> 5] >> (v & 31)) & 1)) {
            const uint64_t kp = TopSelect::falling(obs[v]);
            if (a.by_z) sel.put(slot, TopSelect::falling(a.z[row + v]), kp, v);
            else sel.put(slot, kp, 0, v);
          } else {
            sel.none(slot);
          }
        }
        sel.round(tid);
      }
    }
    for (int32_t i = tid; i < a.n_add; i += kThreads) a.node[out + i] = sel.at(i);
    __syncthreads();                                     // the selection and bits are read before the next set writes them
  }
}

}  // namespace

extern "C" {

int gss_rwr_rank(int32_t n, const int32_t *rowptr, const int32_t *col, int32_t max_deg, int64_t n_units, int32_t max_size,
                 const int32_t *nodes, const int32_t *sizes, double restart, double tol, int32_t max_iter, int32_t n_add, int32_t *node_out,
                 double *score_out, int32_t *iters_out, double *p_out, void *stream) {
  GSS_REQUIRE(rowptr && col && nodes && sizes && iters_out, "rwr_rank: null pointer");
  GSS_REQUIRE((node_out == nullptr) == (score_out == nullptr), "rwr_rank: node_out and score_out are given together or not at all");
  GSS_REQUIRE(node_out || p_out, "rwr_rank: neither a ranking nor p_out is asked for");
  GSS_REQUIRE(n >= 2 && n <= kMaxN, "rwr_rank: n=%d must be in [2, %d] (q of every node lives in LDS)", n, kMaxN);
  GSS_REQUIRE(n_units >= 1, "rwr_rank: n_units=%lld must be >= 1", (long long)n_units);
  GSS_REQUIRE(max_size >= 1 && max_size <= kMaxSeeds, "rwr_rank: max_size=%d must be in [1, %d]", max_size, kMaxSeeds);
  GSS_REQUIRE(max_deg >= 1, "rwr_rank: max_deg=%d must be >= 1", max_deg);
  GSS_REQUIRE(restart > 0.0 && restart < 1.0, "rwr_rank: restart=%g must be in (0, 1)", restart);
  GSS_REQUIRE(tol >= 0.0, "rwr_rank: tol=%g must be >= 0", tol);
  GSS_REQUIRE(max_iter >= 1, "rwr_rank: max_iter=%d must be >= 1", max_iter);
  GSS_REQUIRE(n_add >= 1 && n_add <= kMaxAdd, "rwr_rank: n_add=%d must be in [1, %d]", n_add, kMaxAdd);
  GSS_REQUIRE(n_units <= ((int64_t(1) << 40) - 1) / std::max(std::max(max_size, n_add), n),
              "rwr_rank: the tables are too large (n_units=%lld x max_size=%d, n_add=%d, n=%d)", (long long)n_units, max_size, n_add, n);
  hipStream_t st = as_stream(stream);
  UnitStatus status;
  if (int rc = status.begin("rwr_rank", st)) return rc;
  DeviceBuf<int32_t> notconv;
  if (int rc = notconv.alloc("rwr_rank", sizeof(int32_t))) return rc;
  GSS_HIP(hipMemsetAsync(notconv.p, 0, sizeof(int32_t), st));
  RankArgs a;
  a.n = n;
  a.max_deg = max_deg;
  a.max_size = max_size;
  a.n_add = n_add;
  a.max_iter = max_iter;
  a.n_units = n_units;
  a.rowptr = rowptr;
  a.col = col;
  a.nodes = nodes;
  a.sizes = sizes;
  a.restart = restart;
  a.tol = tol;
  a.node = node_out;
  a.iters = iters_out;
  a.flag = status.flag.p;
  a.notconv = notconv.p;
  a.score = score_out;
  a.p_out = p_out;
  const size_t lds = std::max<size_t>((size_t)n * sizeof(double), (size_t)kSelBytes);
  const int blocks = (int)std::min<int64_t>(n_units, kMaxBlocks);
  rwr_rank_kernel<<<blocks, kThreads, lds_request(rwr_rank_kernel, lds), st>>>(a);
  GSS_LAUNCH_CHECK("rwr_rank_kernel");
  if (int rc = status.end("rwr_rank", "seed", n, max_size, max_deg, st)) return rc;
  int32_t h[2] = {0, 0};
  if (int rc = read_back(&h[0], status.flag.p, sizeof(int32_t), st)) return rc;
  GSS_REQUIRE(!(h[0] & kRowEmpty), "rwr_rank: a row of the CSR is empty (a walk cannot leave a node without a neighbour)");
  if (int rc = read_back(&h[1], notconv.p, sizeof(int32_t), st)) return rc;
  if (h[1] > 0)
    return fail(GSS_ENOTCONV, "rwr_rank: %d of %lld units did not reach err < tol=%g within max_iter=%d iterations (the outputs hold the last iterates)",
                h[1], (long long)n_units, tol, max_iter);
  return GSS_OK;
}

int gss_rwr_null_stats(int32_t n, int32_t n_sets, int32_t R, const double *p, int32_t max_size, const int32_t *nodes, const int32_t *sizes,
                       int32_t n_add, int32_t rank_by, double *mean, double *sd, double *z, int32_t *ge, int32_t *node_out, void *stream) {
  GSS_REQUIRE(p && nodes && sizes && mean && sd && z && ge && node_out, "rwr_null_stats: null pointer");
  GSS_REQUIRE(n >= 2 && n <= kMaxN, "rwr_null_stats: n=%d must be in [2, %d]", n, kMaxN);
  GSS_REQUIRE(n_sets >= 1 && n_sets <= 65535, "rwr_null_stats: n_sets=%d must be in [1, 65535]", n_sets);
  GSS_REQUIRE(R >= 3 && R <= (1 << 20), "rwr_null_stats: R=%d must be in [3, %d] (the set and at least two random samples)", R, 1 << 20);
  GSS_REQUIRE(max_size >= 1 && max_size <= kMaxSeeds, "rwr_null_stats: max_size=%d must be in [1, %d]", max_size, kMaxSeeds);
  GSS_REQUIRE(n_add >= 1 && n_add <= kMaxAdd, "rwr_null_stats: n_add=%d must be in [1, %d]", n_add, kMaxAdd);
  GSS_REQUIRE(rank_by == 0 || rank_by == 1, "rwr_null_stats: rank_by=%d must be 0 (p) or 1 (z)", rank_by);
  GSS_REQUIRE((int64_t)n_sets * R <= ((int64_t(1) << 40) - 1) / std::max(max_size, n),
              "rwr_null_stats: the tables are too large (n_sets=%d x R=%d x max_size=%d, n=%d)", n_sets, R, max_size, n);
  hipStream_t st = as_stream(stream);
  UnitStatus status;
  if (int rc = status.begin("rwr_null_stats", st)) return rc;
  NullArgs a;
  a.n = n;
  a.R = R;
  a.max_size = max_size;
  a.n_add = n_add;
  a.by_z = rank_by;
  a.n_sets = n_sets;
  a.p = p;
  a.nodes = nodes;
  a.sizes = sizes;
  a.mean = mean;
  a.sd = sd;
  a.z = z;
  a.ge = ge;
  a.node = node_out;
  a.flag = status.flag.p;
  const size_t lds = (size_t)kSelBytes + (size_t)((n + 31) >> 5) * sizeof(uint32_t);
  rwr_null_stats_kernel<<<dim3((unsigned)((n + 255) / 256), (unsigned)n_sets), 256, 0, st>>>(a);
  GSS_LAUNCH_CHECK("rwr_null_stats_kernel");
  const int blocks = std::min(n_sets, kMaxBlocks);
  rwr_null_select_kernel<<<blocks, kThreads, lds_request(rwr_null_select_kernel, lds), st>>>(a);
  GSS_LAUNCH_CHECK("rwr_null_select_kernel");
  return status.end("rwr_null_stats", "seed", n, max_size, 0, st);
}

}  // extern "C"
}  // namespace gss

// steiner.hip -- approximate Steiner trees of seed sets: Mehlhorn's 1988 form of the Kou-Markowsky-Berman 2(1 - 1/l) approximation, on
// unit edge weights.  include/gssgcn.h has the definition (nearest terminal, bridges, paths) and the tie rules, DESIGN.md section 9.20
// the cost model.
//
// One kernel, one unit (one row of a seed table, admitted as seed_units.h states) per workgroup at a time.  The unit's state lives in
// dynamic LDS, 4 n + 16 max_size bytes (plus under 512 bytes of static LDS; a call that needs more than 160 KiB is refused by name):
//   best[i]   64 bits per terminal position: the smallest key (w << 30 | u << 15 | v) of a bridge that leaves the component whose root
//             is i, in one Boruvka round;
//   key[v]    32 bits per node: dist(v) << 12 | src(v), 0xffffffff while no terminal has reached v; bit 27 marks a tree node later on;
//   par[i]    32 bits per terminal position: the union-find of lds_union_find.h (a root is its component's smallest position);
//   chosen[j] 32 bits per chosen bridge, u << 15 | v (at most max_size - 1 of them).
// 1. A level-synchronous search from all terminals: the nodes at distance L push (L + 1) << 12 | src to their neighbours with an LDS
//    atomicMin, which leaves in every word the minimum of (dist, src) over the neighbours whatever the schedule.
// 2. Boruvka rounds: every edge u < v with src(u) != src(v) offers its key to the two components it joins (an LDS atomicMin behind a
//    plain compare); every root takes its minimum, the two ends are united, the union-find is flattened.  The order on the keys is strict,
//    so the rounds end in the one minimum spanning forest that Kruskal finds.
// 3. A wave walks the parent chain from each end of each chosen bridge and marks its nodes until it meets a marked node or a terminal.
//    parent(x) is the first entry of x's ascending row with key = key(x) - (1 << 12): found by the wave, 64 entries at a time.
// Rows are walked by walk_rows: a lane walks a row of up to kLane entries itself, kBatch loads in flight; a longer row is handed to the
// lane's wave.  A hub row is never walked by one lane.
// All integers: the outputs do not depend on the schedule.  The only global atomic is the status word's atomicOr.
#include <algorithm>

#include "lds_union_find.h"
#include "seed_units.h"

namespace gss {
namespace {

constexpr int32_t kMaxN = 30720;             // a node index fits 15 bits of a bridge's key
constexpr int32_t kMaxSeeds = 4096;          // src fits 12 bits of a node's word
constexpr int32_t kMaxDeg = (1 << 20) - 1;
constexpr size_t kLdsBudget = 160 * 1024 - 512;   // the CU's LDS less the static words below
constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxBlocks = 1024;             // workgroups walk the units with this stride
constexpr int kLane = 32;                    // a row longer than this is walked by a wave
constexpr int kBatch = 8;                    // entries of a row a lane has in flight
constexpr int kWaveBatch = 4;                // ... and a lane of a wave on a long row
constexpr uint32_t kUnreached = 0xffffffffu, kSrc = 0xfffu, kWord = 0x07ffffffu, kMark = 0x08000000u;
constexpr int kDist = 12;
constexpr uint32_t kNode = 0x7fffu;
constexpr unsigned long long kNone = ~0ull;

struct SteinerArgs {
  int32_t n, max_deg, max_size, max_add;
  int64_t n_units;
  const int32_t *rowptr, *col, *seeds, *sizes;
  int32_t *n_comp, *length, *n_steiner, *n_edges, *max_w, *steiner, *parent, *bridge, *flag;
};

// Every row v with ctx = pred(v) >= 0: body(v, ctx, c) for every entry c of the row (c < 0 never; c >= n is the body's to refuse).
// Called by the whole workgroup; no barrier inside.
template <typename Pred, typename Body>
__device__ __forceinline__ void walk_rows(const SteinerArgs &a, int32_t tid, int32_t lane, Pred pred, Body body) {
  for (int32_t base = 0; base < a.n; base += kThreads) {   // the same trips for every lane of a wave
    const int32_t v = base + tid;
    int32_t lo = 0, hi = 0, ctx = -1;
    if (v < a.n) ctx = pred(v);
    if (ctx >= 0) {
      lo = a.rowptr[v];
      hi = a.rowptr[v + 1];
    }
    const bool wide = hi - lo > kLane;
    for (unsigned long long m = __ballot(wide); m; m &= m - 1) {   // the wave on each long row in turn
      const int from = __ffsll((long long)m) - 1;
      const int32_t wv = __shfl(v, from), wctx = __shfl(ctx, from), whi = __shfl(hi, from);
      for (int32_t e = __shfl(lo, from) + lane; e < whi; e += 64 * kWaveBatch) {
        int32_t c[kWaveBatch];
#pragma unroll
        for (int b = 0; b < kWaveBatch; ++b) c[b] = e + 64 * b < whi ? a.col[e + 64 * b] : -1;
#pragma unroll
        for (int b = 0; b < kWaveBatch; ++b)
          if (c[b] >= 0) body(wv, wctx, c[b]);
      }
    }
    for (int32_t e = lo; e < hi && !wide; e += kBatch) {
      int32_t c[kBatch];
#pragma unroll
      for (int b = 0; b < kBatch; ++b) c[b] = e + b < hi ? a.col[e + b] : -1;
#pragma unroll
      for (int b = 0; b < kBatch; ++b)
        if (c[b] >= 0) body(v, ctx, c[b]);
    }
  }
}

// The whole wave on row x, whose word (without the mark) is kx, dist > 0: the smallest neighbour one level nearer to the same terminal,
// to every lane; -1 when the row holds none (a CSR that is not symmetric)
__device__ __forceinline__ int32_t parent_of(const SteinerArgs &a, const uint32_t *key, int32_t x, uint32_t kx, int32_t lane) {
  const uint32_t want = kx - (1u << kDist);
  const int32_t hi = a.rowptr[x + 1];
  for (int32_t e = a.rowptr[x]; e < hi; e += 64) {
    const int32_t c = e + lane < hi ? a.col[e + lane] : -1;
    const bool node = (uint32_t)c < (uint32_t)a.n;
    const unsigned long long hit = __ballot(node && (key[node ? c : 0] & kWord) == want);
    if (hit) return __shfl(c, __ffsll((long long)hit) - 1);
  }
  return -1;
}

__global__ __launch_bounds__(kThreads) void steiner_kernel(SteinerArgs a) {
  extern __shared__ unsigned long long dyn[];
  unsigned long long *best = dyn;
  uint32_t *key = reinterpret_cast<uint32_t *>(best + a.max_size);
  int32_t *par = reinterpret_cast<int32_t *>(key + a.n);
  uint32_t *chosen = reinterpret_cast<uint32_t *>(par + a.max_size);
  __shared__ int32_t wsum[kWaves];
  __shared__ int32_t n_chosen, length, max_w;
  const int32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int32_t n = a.n;
  for (int64_t u = blockIdx.x; u < a.n_units; u += gridDim.x) {
    const int32_t m = unit_size(a.sizes, u, a.max_size, a.flag);
    if (m < 0) continue;
    const int32_t *x = a.seeds + u * a.max_size;
    int bad = 0;
    for (int32_t v = tid; v < n; v += kThreads) {
      key[v] = kUnreached;
      bad |= unit_row_bits(a.rowptr, v, a.max_deg);
    }
    for (int32_t i = tid; i < m; i += kThreads) bad |= unit_member_bits(x, i, n);
    if (unit_refused(bad, a.flag)) continue;             // no row of a refused unit is walked
    for (int32_t i = tid; i < m; i += kThreads) {
      key[x[i]] = (uint32_t)i;                           // dist 0, src = the position
      par[i] = i;
    }
    if (tid == 0) n_chosen = length = max_w = 0;
    __syncthreads();

    // 1. the nearest terminal of every node
    for (int32_t L = 0;; ++L) {
      int grew = 0;
      walk_rows(
          a, tid, lane,
          [&](int32_t v) -> int32_t {
            const uint32_t k = key[v];
            return (k >> kDist) == (uint32_t)L ? (int32_t)(k + (1u << kDist)) : -1;
          },
          [&](int32_t, int32_t nk, int32_t c) {
            if ((uint32_t)c < (uint32_t)n && key[c] > (uint32_t)nk) {
              atomicMin(&key[c], (uint32_t)nk);
              grew = 1;
            }
          });
      if (!__syncthreads_or(grew)) break;                // a level that reached nothing new: L <= n - 1 < 2^15
    }

    // 2. the minimum spanning forest of the terminals over the bridges
    for (;;) {
      for (int32_t i = tid; i < m; i += kThreads) best[i] = kNone;
      __syncthreads();
      walk_rows(
          a, tid, lane,
          [&](int32_t v) -> int32_t {
            const uint32_t k = key[v];
            return k == kUnreached ? -1 : (int32_t)k;
          },
          [&](int32_t v, int32_t kv, int32_t c) {
            if (c <= v || c >= n) return;
            const uint32_t kc = key[c];
            if (kc == kUnreached || ((kc ^ (uint32_t)kv) & kSrc) == 0) return;
            const int32_t rv = par[(uint32_t)kv & kSrc], rc = par[kc & kSrc];
            if (rv == rc) return;
            const unsigned long long wt = ((uint32_t)kv >> kDist) + (kc >> kDist) + 1u;
            const unsigned long long k64 = (wt << 30) | ((unsigned long long)v << 15) | (unsigned long long)c;
            if (k64 < best[rv]) atomicMin(&best[rv], k64);
            if (k64 < best[rc]) atomicMin(&best[rc], k64);
          });
      __syncthreads();
      int any = 0;
      for (int32_t i = tid; i < m; i += kThreads) {
        const unsigned long long k64 = best[i];
        if (k64 == kNone) continue;                      // no root, or a root whose component is complete
        any = 1;
        const int32_t ra = par[key[(k64 >> 15) & kNode] & kSrc], rb = par[key[k64 & kNode] & kSrc];
        const int32_t other = ra == i ? rb : ra;
        if (i < other || best[other] != k64) {           // chosen from both sides: the smaller root records it
          chosen[atomicAdd(&n_chosen, 1)] = (uint32_t)(k64 & 0x3fffffffull);
          atomicAdd(&length, (int32_t)(k64 >> 30));
          atomicMax(&max_w, (int32_t)(k64 >> 30));
        }
      }
      if (!__syncthreads_or(any)) break;
      for (int32_t i = tid; i < m; i += kThreads) {
        const unsigned long long k64 = best[i];
        if (k64 != kNone) uf_union(par, (int32_t)(key[(k64 >> 15) & kNode] & kSrc), (int32_t)(key[k64 & kNode] & kSrc));
      }
      __syncthreads();
      uf_flatten(par, m, tid, kThreads);
    }
    const int32_t nb = n_chosen;                         // at most m - 1: every bridge chosen joins two components

    // 3. the paths: a wave per end of a chosen bridge
    for (int32_t j = w; j < 2 * nb; j += kWaves) {
      const uint32_t word = chosen[j >> 1];
      int32_t v = (int32_t)((j & 1) ? word & kNode : word >> 15);
      while (v >= 0) {
        const uint32_t k = key[v] & kWord;
        if ((k >> kDist) == 0) break;                    // a terminal
        uint32_t old = 0;
        if (lane == 0) old = atomicOr(&key[v], kMark);
        if (__shfl(old, 0) & kMark) break;               // another chain went up from here
        v = parent_of(a, key, v, k, lane);
      }
    }
    __syncthreads();

    // the Steiner nodes, counted and listed in ascending order
    int32_t count = 0;
    for (int32_t base = 0; base < n; base += kThreads) {
      const int32_t v = base + tid;
      const uint32_t k = v < n ? key[v] : kUnreached;
      const bool is = k != kUnreached && (k & kMark);
      const unsigned long long mask = __ballot(is);
      if (lane == 0) wsum[w] = __popcll(mask);
      __syncthreads();
      int32_t before = 0, total = 0;
      for (int i = 0; i < kWaves; ++i) {
        const int32_t s = wsum[i];
        total += s;
        before += i < w ? s : 0;
      }
      if (a.steiner) {
        const int32_t pos = count + before + __popcll(mask & ((1ull << lane) - 1ull));
        const bool listed = is && pos < a.max_add;
        if (listed) a.steiner[u * a.max_add + pos] = v;
        for (unsigned long long todo = __ballot(listed); todo; todo &= todo - 1) {   // the wave on each listed node's row in turn
          const int from = __ffsll((long long)todo) - 1;
          const int32_t p = parent_of(a, key, __shfl(v, from), __shfl(k, from) & kWord, lane);
          if (lane == from) a.parent[u * a.max_add + pos] = p;
        }
      }
      count += total;
      __syncthreads();                                   // wsum is free for the next tile
    }

    // the bridges in ascending (u, v): the words are distinct, so the number of smaller words is a bridge's place
    if (a.bridge) {
      for (int32_t j = tid; j < nb; j += kThreads) {
        const uint32_t word = chosen[j];
        int32_t rank = 0;
        for (int32_t i = 0; i < nb; ++i) rank += chosen[i] < word;
        int32_t *out = a.bridge + (u * (a.max_size - 1) + rank) * 2;
        out[0] = (int32_t)(word >> 15);
        out[1] = (int32_t)(word & kNode);
      }
    }
    if (tid == 0) {
      a.n_comp[u] = m - nb;
      a.length[u] = length;
      a.n_steiner[u] = count;
      a.n_edges[u] = count + nb;                         // m + n_steiner - n_comp
      a.max_w[u] = max_w;
    }
    __syncthreads();                                     // the LDS arrays and counters are free for the next unit
  }
}

}  // namespace

extern "C" {

int gss_steiner_trees(int32_t n, const int32_t *rowptr, const int32_t *col, int32_t max_deg, int64_t n_units, int32_t max_size,
                      const int32_t *seeds, const int32_t *sizes, int32_t max_add, int32_t *n_comp, int32_t *length, int32_t *n_steiner,
                      int32_t *n_edges, int32_t *max_w, int32_t *steiner, int32_t *parent, int32_t *bridge, void *stream) {
  GSS_REQUIRE(rowptr && col && seeds && sizes && n_comp && length && n_steiner && n_edges && max_w, "steiner_trees: null pointer");
  GSS_REQUIRE(!steiner == !parent, "steiner_trees: steiner and parent must both be given or both be NULL");
  GSS_REQUIRE(n >= 1 && n_units >= 1, "steiner_trees: n=%d n_units=%lld must be >= 1", n, (long long)n_units);
  GSS_REQUIRE(n <= kMaxN, "steiner_trees: n=%d is over the limit of %d nodes (a bridge's key holds a node in 15 bits)", n, kMaxN);
  GSS_REQUIRE(max_size >= 1 && max_size <= kMaxSeeds, "steiner_trees: max_size=%d must be in [1, %d]", max_size, kMaxSeeds);
  GSS_REQUIRE(max_add >= 0, "steiner_trees: max_add=%d must be >= 0", max_add);
  GSS_REQUIRE(max_deg >= 0 && max_deg <= kMaxDeg, "steiner_trees: max_deg=%d must be in [0, %d]", max_deg, kMaxDeg);
  const size_t lds = 4 * (size_t)n + 16 * (size_t)max_size;
  GSS_REQUIRE(lds <= kLdsBudget, "steiner_trees: 4 n + 16 max_size = %zu bytes of LDS for n=%d, max_size=%d is over the budget of %zu (160 KiB less 512)",
              lds, n, max_size, kLdsBudget);
  GSS_REQUIRE(n_units <= ((int64_t(1) << 40) - 1) / std::max(max_size, std::max(max_add, 1)),
              "steiner_trees: the tables are too large (n_units=%lld x max(max_size=%d, max_add=%d))", (long long)n_units, max_size, max_add);
  hipStream_t st = as_stream(stream);
  UnitStatus status;
  if (int rc = status.begin("steiner_trees", st)) return rc;
  SteinerArgs a;
  a.n = n;
  a.max_deg = max_deg;
  a.max_size = max_size;
  a.max_add = max_add;
  a.n_units = n_units;
  a.rowptr = rowptr;
  a.col = col;
  a.seeds = seeds;
  a.sizes = sizes;
  a.n_comp = n_comp;
  a.length = length;
  a.n_steiner = n_steiner;
  a.n_edges = n_edges;
  a.max_w = max_w;
  a.steiner = steiner;
  a.parent = parent;
  a.bridge = bridge;
  a.flag = status.flag.p;
  const int blocks = (int)std::min<int64_t>(n_units, kMaxBlocks);
  steiner_kernel<<<blocks, kThreads, lds_request(steiner_kernel, lds), st>>>(a);
  GSS_LAUNCH_CHECK("steiner_kernel");
  return status.end("steiner_trees", "seed", n, max_size, max_deg, st);
}

}  // extern "C"
}  // namespace gss

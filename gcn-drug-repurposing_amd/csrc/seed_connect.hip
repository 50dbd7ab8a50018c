// seed_connect.hip -- the seed connector algorithm (Wang and Loscalzo 2018): join the fragments of a seed set, one node per step, each
// step the node outside the module that most enlarges the largest connected component of the subgraph the module induces.
// include/gssgcn.h has the contract and the tie rule, DESIGN.md section 9.19 the LDS budget and the cost model.
//
// One kernel, one unit (one row of a seed table, admitted as seed_units.h states) per workgroup at a time.  The unit's state lives in LDS
// for all its steps:
//   lab[v]   one 32-bit word per node: for a member of the module kMember | its position in the module (seeds in their order, then
//            the added nodes in the order added); otherwise kTouch when a neighbour is a member (a candidate), 0 when none is;
//   ps[i]    one 32-bit word per member position: the position of its component's root in the low 15 bits (always the root itself:
//            the components are kept flat), bit 15 a mark while a row's distinct components are summed, and in a root's word the
//            component's size in the high half.  A root is the smallest position of its component;
//   list     the candidates of one tile of the scan that go down the exact slow path.
// The seeds' components come from the lock-free union-find of lds_union_find.h over seed rows walked by a wave each.  A step: every lane
// walks the rows of its candidates and sums the sizes of the distinct components next to each, holding up to kRoots roots in registers;
// a candidate next to more, or with a row longer than the workgroup, is summed by the whole workgroup over marks on the roots' words
// (exact for any number of components; a hub row is never walked by one lane).  A block reduction over the key
// (largest new LCC, smaller degree, smaller node) -- a total order -- picks the winner; the whole workgroup walks its row, marks the
// components it joins, and one pass over the member positions points them at the smallest root among them.
// All integers: the outputs do not depend on the schedule.  The only global atomic is the status word's atomicOr.
#include <algorithm>

#include "lds_union_find.h"
#include "seed_units.h"

namespace gss {
namespace {

constexpr int32_t kMaxN = 30720;         // 4 n (lab) + 4 x 8,192 (ps) + 4 KiB (list) = 156 KiB at this n, of the CU's 160 KiB
constexpr int32_t kMaxSeeds = 4096;      // the seed table's row length, as gss_set_components'
constexpr int32_t kMaxMembers = 8192;    // max_size + n_add: member positions (15 bits of a ps word hold more; the LDS does not)
constexpr int32_t kMaxDeg = (1 << 20) - 1;   // the key holds a degree and a node in 20 bits each
constexpr int kRoots = 8;                // distinct components a lane holds in registers for one candidate; more take the slow path
constexpr int kBatch = 8;                // entries of a candidate's row a lane has in flight
constexpr int kThreads = 1024;           // a row longer than this is walked by the whole workgroup
constexpr int kWaves = kThreads / 64;
constexpr int kMaxBlocks = 1024;         // workgroups walk the units with this stride
constexpr uint32_t kMember = 0x80000000u, kTouch = 1u, kSlow = 2u, kSlotMask = 0x7fffu;
constexpr uint32_t kParent = 0x7fffu, kMark = 0x8000u;
constexpr unsigned long long kNone = ~0ull;
constexpr unsigned long long kField = 0xfffffull;

struct ConnectArgs {
  int32_t n, max_deg, max_size, n_add;
  int64_t n_units;
  const int32_t *rowptr, *col, *seeds, *sizes;
  int32_t *node, *lcc, *merged, *deg, *steps, *first_lcc, *final_lcc, *seeds_in, *added_in, *label, *flag;
};

// smaller is better: the larger new LCC, then the smaller degree, then the smaller node
__device__ __forceinline__ unsigned long long make_key(int32_t lcc, int32_t deg, int32_t v) {
  return ((kField - (unsigned long long)lcc) << 40) | ((unsigned long long)deg << 20) | (unsigned long long)v;
}

// the smallest k of the workgroup, to every lane; two barriers, red is free again afterwards
__device__ __forceinline__ unsigned long long block_min(unsigned long long k, unsigned long long *red, int32_t lane, int32_t w) {
  for (int o = 32; o > 0; o >>= 1) k = min(k, (unsigned long long)__shfl_xor(k, o));
  if (lane == 0) red[w] = k;
  __syncthreads();
  k = red[0];
  for (int i = 1; i < kWaves; ++i) k = min(k, red[i]);
  __syncthreads();
  return k;
}

// The whole workgroup on row v: marks the root of every component with a member in the row and leaves in acc[0] 1 + the sum of their
// sizes, in acc[1] their number, in acc[2] the smallest root.  With `touch` the row's other nodes become candidates.  Ends in a barrier.
__device__ __forceinline__ void mark_row(const ConnectArgs &a, uint32_t *lab, uint32_t *ps, int32_t *acc, int32_t v, bool touch, int32_t tid) {
  if (tid == 0) {
    acc[0] = 1;
    acc[1] = 0;
    acc[2] = 0x7fffffff;
  }
  __syncthreads();
  const int32_t hi = a.rowptr[v + 1];
  for (int32_t e = a.rowptr[v] + tid; e < hi; e += kThreads) {
    const int32_t c = a.col[e];
    if ((uint32_t)c >= (uint32_t)a.n || c == v) continue;
    const uint32_t y = lab[c];
    if (y & kMember) {
      const int32_t r = (int32_t)(ps[y & kSlotMask] & kParent);
      const uint32_t old = atomicOr(&ps[r], kMark);
      if (!(old & kMark)) {                              // the first lane to reach this component counts it
        atomicAdd(&acc[0], (int32_t)(old >> 16));
        atomicAdd(&acc[1], 1);
        atomicMin(&acc[2], r);
      }
    } else if (touch) {
      lab[c] = kTouch;
    }
  }
  __syncthreads();
}

__global__ __launch_bounds__(kThreads) void seed_connect_kernel(ConnectArgs a) {
  extern __shared__ uint32_t dyn[];
  uint32_t *lab = dyn, *ps = dyn + a.n;
  int32_t *list = reinterpret_cast<int32_t *>(ps + a.max_size + a.n_add);
  __shared__ unsigned long long red[kWaves];
  __shared__ int32_t acc[3], n_slow, n_list;
  const int32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int32_t n = a.n, width = a.max_size + a.n_add;
  for (int64_t u = blockIdx.x; u < a.n_units; u += gridDim.x) {
    const int32_t m = unit_size(a.sizes, u, a.max_size, a.flag);
    if (m < 0) continue;
    const int32_t *x = a.seeds + u * a.max_size;
    int bad = 0;
    for (int32_t v = tid; v < n; v += kThreads) {
      lab[v] = 0;
      bad |= unit_row_bits(a.rowptr, v, a.max_deg);
    }
    for (int32_t i = tid; i < m; i += kThreads) bad |= unit_member_bits(x, i, n);
    if (unit_refused(bad, a.flag)) continue;             // no row of a refused unit is walked
    for (int32_t i = tid; i < m; i += kThreads) {
      lab[x[i]] = kMember | (uint32_t)i;
      ps[i] = (uint32_t)i;
    }
    if (tid == 0) n_slow = 0;
    __syncthreads();
    for (int32_t i = w; i < m; i += kWaves) {            // a wave per seed row: the seeds' components and the first candidates
      const int32_t v = x[i], hi = a.rowptr[v + 1];
      for (int32_t e = a.rowptr[v] + lane; e < hi; e += 64) {
        const int32_t c = a.col[e];
        if ((uint32_t)c >= (uint32_t)n) continue;
        const uint32_t y = lab[c];
        if (!(y & kMember)) lab[c] = kTouch;
        else if ((int32_t)(y & kSlotMask) != i) uf_union(reinterpret_cast<int32_t *>(ps), i, (int32_t)(y & kSlotMask));
      }
    }
    __syncthreads();
    uf_flatten(reinterpret_cast<int32_t *>(ps), m, tid, kThreads);
    for (int32_t i = tid; i < m; i += kThreads) atomicAdd(&ps[ps[i] & kParent], 1u << 16);   // sizes onto the roots' high halves
    __syncthreads();
    int32_t big = 0;
    for (int32_t i = tid; i < m; i += kThreads) big = max(big, (int32_t)(ps[i] >> 16));
    int32_t L = (int32_t)(kField - block_min(kField - (unsigned long long)big, red, lane, w));
    const int64_t out = u * a.n_add;
    if (tid == 0) a.first_lcc[u] = L;
    int32_t t = 0;
    for (; t < a.n_add; ++t) {
      unsigned long long best = kNone;
      int slow = 0;
      for (int32_t v = tid; v < n; v += kThreads) {      // a lane per candidate
        if (lab[v] != kTouch) continue;
        const int32_t lo = a.rowptr[v], hi = a.rowptr[v + 1];
        bool over = hi - lo > kThreads;
        int32_t roots[kRoots], cnt = 0, tot = 1;
        for (int32_t e = lo; e < hi && !over; e += kBatch) {   // kBatch entries' loads and label reads in flight, then in order
          int32_t c[kBatch];
          uint32_t y[kBatch];
#pragma unroll
          for (int b = 0; b < kBatch; ++b) c[b] = e + b < hi ? a.col[e + b] : -1;
#pragma unroll
          for (int b = 0; b < kBatch; ++b) y[b] = (uint32_t)c[b] < (uint32_t)n ? lab[c[b]] : 0u;
#pragma unroll
          for (int b = 0; b < kBatch; ++b) {
            if (!(y[b] & kMember) || over) continue;
            const int32_t r = (int32_t)(ps[y[b] & kSlotMask] & kParent);
            bool seen = false;
#pragma unroll
            for (int j = 0; j < kRoots; ++j) seen |= j < cnt && roots[j] == r;
            if (seen) continue;
            if (cnt == kRoots) {
              over = true;
              continue;
            }
#pragma unroll
            for (int j = 0; j < kRoots; ++j)
              if (j == cnt) roots[j] = r;
            ++cnt;
            tot += (int32_t)(ps[r] >> 16);
          }
        }
        if (over) {
          lab[v] = kTouch | kSlow;
          slow = 1;
        } else {
          best = min(best, make_key(max(L, tot), hi - lo, v));
        }
      }
      if (slow) n_slow = 1;
      __syncthreads();
      if (n_slow) {                                      // the same word for every thread
        for (int32_t base = 0; base < n; base += kThreads) {   // a tile holds at most one slow candidate per lane: the list cannot overflow
          const int32_t v = base + tid;
          const bool mine = v < n && lab[v] == (kTouch | kSlow);
          if (tid == 0) n_list = 0;
          if (!__syncthreads_or(mine)) continue;
          if (mine) {
            list[atomicAdd(&n_list, 1)] = v;
            lab[v] = kTouch;
          }
          __syncthreads();
          const int32_t listed = n_list;
          for (int32_t j = 0; j < listed; ++j) {         // one at a time, the whole workgroup on its row
            const int32_t c = list[j], hi = a.rowptr[c + 1];
            mark_row(a, lab, ps, acc, c, false, tid);
            if (tid == 0) best = min(best, make_key(max(L, acc[0]), hi - a.rowptr[c], c));
            for (int32_t e = a.rowptr[c] + tid; e < hi; e += kThreads) {   // the marks come off again
              const int32_t d = a.col[e];
              if ((uint32_t)d >= (uint32_t)n || d == c) continue;
              const uint32_t y = lab[d];
              if (y & kMember) atomicAnd(&ps[ps[y & kSlotMask] & kParent], ~kMark);
            }
            __syncthreads();
          }
        }
      }
      best = block_min(best, red, lane, w);
      if (tid == 0) n_slow = 0;
      if (best == kNone) break;                          // no candidate: the same for every lane
      const int32_t Lp = (int32_t)(kField - (best >> 40));
      if (Lp - L < 2) break;                             // the best candidate joins nothing to the largest component
      const int32_t win = (int32_t)(best & kField), cur = m + t;
      mark_row(a, lab, ps, acc, win, true, tid);
      const int32_t root = acc[2], merged = acc[1];
      // One pass points every member of a marked component at the smallest marked root.  A root that stops being one keeps its mark (a
      // lane may still be looking at it through a member's word); no later step reads the mark of a word that is no root's.
      for (int32_t i = tid; i < cur; i += kThreads) {
        const uint32_t word = ps[i];
        const int32_t r = (int32_t)(word & kParent);
        if (r == i) {
          if ((word & kMark) && i != root) ps[i] = (uint32_t)root | kMark;
        } else if (ps[r] & kMark) {
          ps[i] = (uint32_t)root;
        }
      }
      __syncthreads();
      if (tid == 0) {
        ps[root] = (uint32_t)root | ((uint32_t)Lp << 16);
        ps[cur] = (uint32_t)root;
        lab[win] = kMember | (uint32_t)cur;
        a.node[out + t] = win;
        a.lcc[out + t] = Lp;
        a.merged[out + t] = merged;
        a.deg[out + t] = (int32_t)((best >> 20) & kField);
      }
      L = Lp;
      __syncthreads();                                   // lab, ps and acc free for the next step
    }
    for (int32_t i = t + tid; i < a.n_add; i += kThreads) {
      a.node[out + i] = -1;
      a.lcc[out + i] = 0;
      a.merged[out + i] = 0;
      a.deg[out + i] = 0;
    }
    // the final largest component: of two as large the one with the smaller root, which is gss_set_components' smaller label
    const int32_t cur = m + t;
    unsigned long long mine = kNone;
    for (int32_t i = tid; i < cur; i += kThreads)
      if ((int32_t)(ps[i] & kParent) == i && (int32_t)(ps[i] >> 16) == L) mine = min(mine, (unsigned long long)i);
    if (tid == 0) acc[0] = 0;
    const unsigned long long top = block_min(mine, red, lane, w);
    int32_t in = 0;
    for (int32_t i = tid; i < cur; i += kThreads) {
      const int32_t r = (int32_t)(ps[i] & kParent);
      in += i < m && (unsigned long long)r == top;
      if (a.label) a.label[u * width + i] = r;
    }
    for (int o = 32; o > 0; o >>= 1) in += __shfl_xor(in, o);
    if (lane == 0 && in) atomicAdd(&acc[0], in);
    __syncthreads();
    if (tid == 0) {
      a.steps[u] = t;
      a.final_lcc[u] = L;
      a.seeds_in[u] = acc[0];
      a.added_in[u] = L - acc[0];
    }
    __syncthreads();                                     // acc and the LDS arrays are free for the next unit
  }
}

}  // namespace

extern "C" {

int gss_seed_connectors(int32_t n, const int32_t *rowptr, const int32_t *col, int32_t max_deg, int64_t n_units, int32_t max_size,
                        const int32_t *seeds, const int32_t *sizes, int32_t n_add, int32_t *node, int32_t *lcc, int32_t *merged,
                        int32_t *deg, int32_t *steps, int32_t *first_lcc, int32_t *final_lcc, int32_t *seeds_in, int32_t *added_in,
                        int32_t *label, void *stream) {
  GSS_REQUIRE(rowptr && col && seeds && sizes && node && lcc && merged && deg && steps && first_lcc && final_lcc && seeds_in && added_in,
              "seed_connectors: null pointer");
  GSS_REQUIRE(n >= 1 && n_units >= 1, "seed_connectors: n=%d n_units=%lld must be >= 1", n, (long long)n_units);
  GSS_REQUIRE(n <= kMaxN, "seed_connectors: n=%d is over the limit of %d nodes (a unit's node labels live in LDS)", n, kMaxN);
  GSS_REQUIRE(n_add >= 1, "seed_connectors: n_add=%d must be >= 1", n_add);
  GSS_REQUIRE(max_size >= 1 && max_size <= kMaxSeeds, "seed_connectors: max_size=%d must be in [1, %d]", max_size, kMaxSeeds);
  GSS_REQUIRE((int64_t)max_size + n_add <= kMaxMembers, "seed_connectors: max_size=%d + n_add=%d is over %d (a unit's components live in LDS)",
              max_size, n_add, kMaxMembers);
  GSS_REQUIRE(max_deg >= 0 && max_deg <= kMaxDeg, "seed_connectors: max_deg=%d must be in [0, %d]", max_deg, kMaxDeg);
  GSS_REQUIRE(n_units <= ((int64_t(1) << 40) - 1) / (max_size + n_add),
              "seed_connectors: the tables are too large (n_units=%lld x (max_size=%d + n_add=%d))", (long long)n_units, max_size, n_add);
  hipStream_t st = as_stream(stream);
  UnitStatus status;
  if (int rc = status.begin("seed_connectors", st)) return rc;
  ConnectArgs a;
  a.n = n;
  a.max_deg = max_deg;
  a.max_size = max_size;
  a.n_add = n_add;
  a.n_units = n_units;
  a.rowptr = rowptr;
  a.col = col;
  a.seeds = seeds;
  a.sizes = sizes;
  a.node = node;
  a.lcc = lcc;
  a.merged = merged;
  a.deg = deg;
  a.steps = steps;
  a.first_lcc = first_lcc;
  a.final_lcc = final_lcc;
  a.seeds_in = seeds_in;
  a.added_in = added_in;
  a.label = label;
  a.flag = status.flag.p;
  const size_t lds = ((size_t)n + (size_t)max_size + (size_t)n_add + (size_t)kThreads) * sizeof(uint32_t);
  const int blocks = (int)std::min<int64_t>(n_units, kMaxBlocks);
  seed_connect_kernel<<<blocks, kThreads, lds_request(seed_connect_kernel, lds), st>>>(a);
  GSS_LAUNCH_CHECK("seed_connect_kernel");
  return status.end("seed_connectors", "seed", n, max_size, max_deg, st);
}

}  // extern "C"
}  // namespace gss

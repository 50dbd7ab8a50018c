// set_modules.hip -- connected components of the subgraphs that node sets induce (Menche et al. 2015: does a disease's gene set form a
// module on the interactome?) on the device.  include/gssgcn.h has the contract, DESIGN.md section 9.17 the cost model and the measurements.
//
// One kernel, one unit (one row of a set table, the layout gss_prox_random_sets writes) per workgroup at a time:
//   1. the member list goes into LDS, checked on the way as seed_units.h states; parent[i] = i beside it;
//   2. a wave per member probes the member's CSR row against the list in the cheaper direction -- lanes over the row's entries, each a
//      binary search of the LDS list (deg * log2 m), or lanes over the members, each a binary search of the row (m * log2 deg) -- so a hub
//      row is never walked by one lane.  Every hit (i, j) is a union in a lock-free union-find in LDS: the larger root is hooked under
//      the smaller with a compare-and-swap, finds halve their path.  A hit with j > i counts as an edge;
//   3. pointer jumping until no parent changes: every parent is then its component's root, the smallest position of the component;
//   4. component sizes by LDS integer adds onto the roots; the largest, the number of roots and the edge count are reduced over the block.
// Every loop ends on the data (a union when the roots meet or its hook lands, the jumping when nothing moved), none on a round count.
// All integers: the outputs do not depend on the schedule.  The only global atomic is the status word's atomicOr.
#include <algorithm>

#include "lds_union_find.h"
#include "seed_units.h"

namespace gss {
namespace {

constexpr int32_t kMaxSet = 4096;        // the member list and the parents of one unit live in LDS (2 x 16 KB): proximity.hip's kMaxTo
constexpr int kSmallSet = 64;            // tables of at most this many members per unit run one wave per workgroup, larger ones four
constexpr int kMaxBlocks = 32768;        // workgroups walk the units with this stride

struct CompArgs {
  int32_t n, max_size;
  int64_t n_units;
  const int32_t *rowptr, *col, *nodes, *sizes;
  int32_t *lcc, *n_comp, *n_edges, *label, *flag;
};

__device__ __forceinline__ int ilog2_ceil(int32_t x) { return x <= 1 ? 1 : 32 - __clz(x - 1); }

// position of v in the ascending list a[0 .. cnt), or -1
template <typename P>
__device__ __forceinline__ int32_t find_sorted(P a, int32_t cnt, int32_t v) {
  int32_t lo = 0, hi = cnt;
  while (lo < hi) {
    const int32_t mid = (lo + hi) >> 1;
    if (a[mid] < v) lo = mid + 1;
    else hi = mid;
  }
  return lo < cnt && a[lo] == v ? lo : -1;
}

__device__ __forceinline__ int wave_sum_i(int v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ int wave_max_i(int v) {
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
  return v;
}

__global__ __launch_bounds__(256) void set_components_kernel(CompArgs a) {
  extern __shared__ int32_t lds[];
  int32_t *mem = lds, *parent = lds + a.max_size;        // mem: the members, later the component sizes
  __shared__ int32_t red[3][4];
  const int32_t tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, w = tid >> 6, nw = nt >> 6;
  for (int64_t u = blockIdx.x; u < a.n_units; u += gridDim.x) {
    const int32_t m = unit_size(a.sizes, u, a.max_size, a.flag);
    if (m < 0) continue;
    const int32_t *x = a.nodes + u * a.max_size;
    int bad = 0;
    for (int32_t i = tid; i < m; i += nt) {
      mem[i] = x[i];
      parent[i] = i;
      bad |= unit_member_bits(x, i, a.n);
    }
    if (unit_refused(bad, a.flag)) continue;             // the barrier after the copy; no row of a refused unit is read
    int edges = 0;
    for (int32_t i = w; i < m; i += nw) {                // a wave per member
      const int32_t v = mem[i], lo = a.rowptr[v], deg = a.rowptr[v + 1] - lo;
      if (deg <= 0) continue;
      const int32_t *row = a.col + lo;
      if ((int64_t)deg * ilog2_ceil(m) <= (int64_t)m * ilog2_ceil(deg)) {
        for (int32_t e = lane; e < deg; e += 64) {       // lanes over the row, the list searched in LDS
          const int32_t j = find_sorted(mem, m, row[e]);
          if (j >= 0 && j != i) {                        // j == i: a stored self loop
            uf_union(parent, i, j);
            edges += j > i;
          }
        }
      } else {
        for (int32_t j = lane; j < m; j += 64) {         // lanes over the members, the row searched in global memory
          if (j != i && find_sorted(row, deg, mem[j]) >= 0) {
            uf_union(parent, i, j);
            edges += j > i;
          }
        }
      }
    }
    __syncthreads();
    uf_flatten(parent, m, tid, nt);
    for (int32_t i = tid; i < m; i += nt) mem[i] = 0;    // the members are not needed any more
    __syncthreads();
    int roots = 0;
    int32_t *lab = a.label ? a.label + u * a.max_size : nullptr;
    for (int32_t i = tid; i < m; i += nt) {
      const int32_t r = parent[i];
      atomicAdd(&mem[r], 1);
      roots += r == i;
      if (lab) lab[i] = r;
    }
    __syncthreads();
    int big = 0;
    for (int32_t i = tid; i < m; i += nt) big = max(big, mem[i]);
    big = wave_max_i(big);
    roots = wave_sum_i(roots);
    edges = wave_sum_i(edges);
    if (lane == 0) {
      red[0][w] = big;
      red[1][w] = roots;
      red[2][w] = edges;
    }
    __syncthreads();
    if (tid == 0) {
      for (int32_t k = 1; k < nw; ++k) {
        big = max(big, red[0][k]);
        roots += red[1][k];
        edges += red[2][k];
      }
      a.lcc[u] = big;
      a.n_comp[u] = roots;
      a.n_edges[u] = edges;
    }
    __syncthreads();                                     // red and the LDS arrays are free for the next unit
  }
}

}  // namespace

extern "C" {

int gss_set_components(int32_t n, const int32_t *rowptr, const int32_t *col, int64_t n_units, int32_t max_size, const int32_t *nodes,
                       const int32_t *sizes, int32_t *lcc, int32_t *n_comp, int32_t *n_edges, int32_t *label, void *stream) {
  GSS_REQUIRE(rowptr && col && nodes && sizes && lcc && n_comp && n_edges, "set_components: null pointer");
  GSS_REQUIRE(n >= 1 && n_units >= 1, "set_components: n=%d n_units=%lld must be >= 1", n, (long long)n_units);
  GSS_REQUIRE(max_size >= 1 && max_size <= kMaxSet, "set_components: max_size=%d must be in [1, %d] (one unit's members live in LDS)",
              max_size, kMaxSet);
  GSS_REQUIRE(n_units <= ((int64_t(1) << 40) - 1) / max_size, "set_components: the set table is too large (n_units=%lld x max_size=%d)",
              (long long)n_units, max_size);
  hipStream_t st = as_stream(stream);
  UnitStatus status;
  if (int rc = status.begin("set_components", st)) return rc;
  CompArgs a;
  a.n = n;
  a.max_size = max_size;
  a.n_units = n_units;
  a.rowptr = rowptr;
  a.col = col;
  a.nodes = nodes;
  a.sizes = sizes;
  a.lcc = lcc;
  a.n_comp = n_comp;
  a.n_edges = n_edges;
  a.label = label;
  a.flag = status.flag.p;
  const int threads = max_size <= kSmallSet ? 64 : 256;
  const int blocks = (int)std::min<int64_t>(n_units, kMaxBlocks);
  set_components_kernel<<<blocks, threads, 2 * (size_t)max_size * sizeof(int32_t), st>>>(a);
  GSS_LAUNCH_CHECK("set_components_kernel");
  return status.end("set_components", "member", n, max_size, 0, st);   // max_deg: this kernel checks no row
}

}  // extern "C"
}  // namespace gss

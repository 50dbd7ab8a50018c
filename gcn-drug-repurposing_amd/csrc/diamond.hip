// diamond.hip -- DIAMOnD (Ghiassian, Menche and Barabasi 2015): grow a module from seed nodes, one node per step, each step the node whose
// links into the module are the most significant under the hypergeometric null.  include/gssgcn.h has the contract and the statistic,
// DESIGN.md section 9.18 the LDS budget and the cost model.
//
// One kernel, one unit (one row of a seed table, admitted as seed_units.h states) per workgroup at a time.  The unit's state lives in LDS
// for all its steps:
//   cnt[v]   one 32-bit word per node: ks (neighbours among the seeds) in the low half, ka (neighbours among the added nodes) in the high
//            half, kept by LDS integer adds while a row is walked (a wave per seed row, the whole workgroup on a winner's row: a hub row
//            is never walked by one lane);
//   in       a bit per node: in the module (seed or added);
//   slot[kb] stage 1 of the choice: the smallest key (k' << 32 | v) of the candidates with kb' = kb, by LDS atomic-min in one scan of cnt.
// A step: clear the slots a step can reach, scan, one lane per occupied slot evaluates the tail (the sequential sum of the contract),
// a block reduction by (logp, -kb') -- a total order, kb' being the slot -- picks the winner, its row bumps ka.
// Integers and a fixed order of fp64 operations per slot: the outputs do not depend on the schedule.  The only global atomic is the
// status word's atomicOr.
#include <algorithm>

#include "seed_units.h"

// the contract's S and lt0 are sequences of single IEEE operations: no multiply-add may be formed of term * q and S + term
#pragma clang fp contract(off)

namespace gss {
namespace {

constexpr int32_t kMaxN = 30720;         // 4 n (cnt) + n / 8 (in) + 32 KiB (slot) = 156 KiB at this n, of the CU's 160 KiB
constexpr int32_t kSlots = 4096;         // stage 1's table: kb' in [0, kSlots)
constexpr int32_t kMaxSeeds = 4096;      // the seed table's row length, as gss_set_components'
constexpr int32_t kMaxCount = 65535;     // ks, ka and kb' are 16 bits
constexpr int kThreads = 1024;           // one workgroup per CU (the LDS decides that): all its lanes scan
constexpr int kWaves = kThreads / 64;
constexpr int kMaxBlocks = 1024;         // workgroups walk the units with this stride
constexpr unsigned long long kEmpty = ~0ull;

struct GrowArgs {
  int32_t n, max_deg, max_size, n_add, alpha;
  int64_t n_units;
  const int32_t *rowptr, *col, *seeds, *sizes;
  const double *lg;
  int32_t *node, *k, *kb, *flag;
  double *lt0, *S, *logp;
};

// log C(a, b) from the table lg[i] = lgamma(i), in the contract's order
__device__ __forceinline__ double log_choose(const double *lg, int64_t a, int64_t b) { return lg[a + 1] - (lg[a - b + 1] + lg[b + 1]); }

__device__ __forceinline__ bool better(double p, int32_t kb, double than_p, int32_t than_kb) {
  return p < than_p || (p == than_p && kb > than_kb);
}

__global__ __launch_bounds__(kThreads) void diamond_grow_kernel(GrowArgs a) {
  extern __shared__ unsigned long long dyn[];
  unsigned long long *slot = dyn;
  uint32_t *cnt = reinterpret_cast<uint32_t *>(dyn + kSlots);
  uint32_t *in = cnt + a.n;
  __shared__ double red_p[kWaves];
  __shared__ int32_t red_kb[kWaves];
  const int32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int32_t n = a.n, alpha = a.alpha, words = (n + 31) >> 5;
  for (int64_t u = blockIdx.x; u < a.n_units; u += gridDim.x) {
    const int32_t m = unit_size(a.sizes, u, a.max_size, a.flag);
    if (m < 0) continue;
    const int32_t *x = a.seeds + u * a.max_size;
    int bad = 0;
    for (int32_t v = tid; v < n; v += kThreads) {
      cnt[v] = 0;
      bad |= unit_row_bits(a.rowptr, v, a.max_deg);
    }
    for (int32_t i = tid; i < words; i += kThreads) in[i] = 0;
    for (int32_t i = tid; i < m; i += kThreads) bad |= unit_member_bits(x, i, n);
    if (unit_refused(bad, a.flag)) continue;             // no row of a refused unit is walked
    for (int32_t i = tid; i < m; i += kThreads) atomicOr(&in[x[i] >> 5], 1u << (x[i] & 31));
    for (int32_t i = w; i < m; i += kWaves) {            // a wave per seed row
      const int32_t v = x[i], hi = a.rowptr[v + 1];
      for (int32_t e = a.rowptr[v] + lane; e < hi; e += 64) {
        const int32_t c = a.col[e];
        if ((uint32_t)c < (uint32_t)n) atomicAdd(&cnt[c], 1u);
      }
    }
    __syncthreads();
    const int64_t Np = n + (int64_t)(alpha - 1) * m;
    const int64_t out = u * a.n_add;
    int32_t t = 0;
    for (; t < a.n_add; ++t) {
      const int64_t sp = (int64_t)alpha * m + t;
      // kb' = alpha ks + ka <= alpha deg and <= alpha |S| + |A|; the host refuses a call in which this exceeds the table
      const int32_t top = (int32_t)std::min<int64_t>((int64_t)alpha * a.max_deg, sp);
      for (int32_t i = tid; i <= top; i += kThreads) slot[i] = kEmpty;
      __syncthreads();
      for (int32_t v = tid; v < n; v += kThreads) {
        const uint32_t c = cnt[v];
        if (c == 0 || ((in[v >> 5] >> (v & 31)) & 1)) continue;
        const int32_t ks = c & 0xffff, kb = alpha * ks + (int32_t)(c >> 16);
        const int32_t kp = a.rowptr[v + 1] - a.rowptr[v] + (alpha - 1) * ks;
        if (kb <= top) atomicMin(&slot[kb], ((unsigned long long)(uint32_t)kp << 32) | (uint32_t)v);
      }
      __syncthreads();
      double my_p = INFINITY, my_lt0 = 0.0, my_S = 0.0;   // this lane's best slot; kb' = 0 is no slot
      int32_t my_kb = 0, my_kp = 0;
      for (int32_t kb = 1 + tid; kb <= top; kb += kThreads) {
        const unsigned long long key = slot[kb];
        if (key == kEmpty) continue;
        const int64_t kp = (int64_t)(key >> 32);
        if (kp < kb || kp - kb > Np - sp) continue;      // only a CSR that is not symmetric gets here: no table entry of its is read
        const double lt0 = (log_choose(a.lg, sp, kb) + log_choose(a.lg, Np - sp, kp - kb)) - log_choose(a.lg, Np, kp);
        double term = 1.0, S = 1.0;
        const int64_t end = std::min<int64_t>(kp, sp), base = Np - sp - kp + 1;
        for (int64_t i = kb; i < end; ++i) {
          const double q = (double)((sp - i) * (kp - i)) / (double)((i + 1) * (base + i));
          term = term * q;
          S = S + term;
        }
        const double p = lt0 + log(S);
        if (better(p, kb, my_p, my_kb)) {
          my_p = p;
          my_kb = kb;
          my_kp = (int32_t)kp;
          my_lt0 = lt0;
          my_S = S;
        }
      }
      double p = my_p;
      int32_t kb = my_kb;
      for (int o = 32; o > 0; o >>= 1) {
        const double p2 = __shfl_xor(p, o);
        const int32_t kb2 = __shfl_xor(kb, o);
        if (better(p2, kb2, p, kb)) {
          p = p2;
          kb = kb2;
        }
      }
      if (lane == 0) {
        red_p[w] = p;
        red_kb[w] = kb;
      }
      __syncthreads();
      p = red_p[0];
      kb = red_kb[0];
      for (int i = 1; i < kWaves; ++i)                   // every lane reads the same winner
        if (better(red_p[i], red_kb[i], p, kb)) {
          p = red_p[i];
          kb = red_kb[i];
        }
      if (kb == 0) break;                                // no candidate left: the same for every lane
      const int32_t win = (int32_t)(uint32_t)slot[kb];
      if (my_kb == kb) {                                 // one lane: a slot is evaluated by one lane
        a.node[out + t] = win;
        a.k[out + t] = my_kp;
        a.kb[out + t] = kb;
        a.lt0[out + t] = my_lt0;
        a.S[out + t] = my_S;
        a.logp[out + t] = my_p;
      }
      if (tid == 0) in[win >> 5] |= 1u << (win & 31);
      const int32_t hi = a.rowptr[win + 1];
      for (int32_t e = a.rowptr[win] + tid; e < hi; e += kThreads) {   // the whole workgroup on the winner's row
        const int32_t c = a.col[e];
        if ((uint32_t)c < (uint32_t)n) atomicAdd(&cnt[c], 0x10000u);
      }
      __syncthreads();                                   // cnt, in, and slot and red free for the next step
    }
    for (int32_t i = t + tid; i < a.n_add; i += kThreads) {
      a.node[out + i] = -1;
      a.k[out + i] = 0;
      a.kb[out + i] = 0;
      a.lt0[out + i] = 0.0;
      a.S[out + i] = 0.0;
      a.logp[out + i] = 0.0;
    }
    __syncthreads();                                     // after a break: red is read before the next unit writes it
  }
}

}  // namespace

extern "C" {

int gss_diamond_grow(int32_t n, const int32_t *rowptr, const int32_t *col, int32_t max_deg, const double *lg, int64_t n_lg, int64_t n_units,
                     int32_t max_size, const int32_t *seeds, const int32_t *sizes, int32_t n_add, int32_t alpha, int32_t *node, int32_t *k,
                     int32_t *kb, double *lt0, double *S, double *logp, void *stream) {
  GSS_REQUIRE(rowptr && col && lg && seeds && sizes && node && k && kb && lt0 && S && logp, "diamond_grow: null pointer");
  GSS_REQUIRE(n >= 1 && n_units >= 1, "diamond_grow: n=%d n_units=%lld must be >= 1", n, (long long)n_units);
  GSS_REQUIRE(n <= kMaxN, "diamond_grow: n=%d is over the limit of %d nodes (a unit's link counts and membership live in LDS)", n, kMaxN);
  GSS_REQUIRE(alpha >= 1, "diamond_grow: alpha=%d must be >= 1", alpha);
  GSS_REQUIRE(n_add >= 1, "diamond_grow: n_add=%d must be >= 1", n_add);
  GSS_REQUIRE(max_size >= 1 && max_size <= kMaxSeeds, "diamond_grow: max_size=%d must be in [1, %d]", max_size, kMaxSeeds);
  GSS_REQUIRE(max_deg >= 0, "diamond_grow: max_deg=%d must be >= 0", max_deg);
  GSS_REQUIRE((int64_t)alpha * max_deg <= kMaxCount, "diamond_grow: alpha=%d x max_deg=%d is over %d (the link counts are 16 bits)", alpha,
              max_deg, kMaxCount);
  const int64_t top = std::min<int64_t>((int64_t)alpha * max_deg, (int64_t)alpha * max_size + n_add - 1);
  GSS_REQUIRE(top < kSlots, "diamond_grow: a node can have %lld weighted links into the module (alpha=%d, max_deg=%d, max_size=%d, n_add=%d); "
              "the table holds %d", (long long)top, alpha, max_deg, max_size, n_add, kSlots);
  GSS_REQUIRE(n_lg >= n + (int64_t)(alpha - 1) * max_size + 2, "diamond_grow: n_lg=%lld, the lgamma table needs %lld entries",
              (long long)n_lg, (long long)(n + (int64_t)(alpha - 1) * max_size + 2));
  GSS_REQUIRE(n_units <= ((int64_t(1) << 40) - 1) / std::max(max_size, n_add),
              "diamond_grow: the tables are too large (n_units=%lld x max_size=%d, n_add=%d)", (long long)n_units, max_size, n_add);
  hipStream_t st = as_stream(stream);
  UnitStatus status;
  if (int rc = status.begin("diamond_grow", st)) return rc;
  GrowArgs a;
  a.n = n;
  a.max_deg = max_deg;
  a.max_size = max_size;
  a.n_add = n_add;
  a.alpha = alpha;
  a.n_units = n_units;
  a.rowptr = rowptr;
  a.col = col;
  a.seeds = seeds;
  a.sizes = sizes;
  a.lg = lg;
  a.node = node;
  a.k = k;
  a.kb = kb;
  a.flag = status.flag.p;
  a.lt0 = lt0;
  a.S = S;
  a.logp = logp;
  const size_t lds = (size_t)kSlots * sizeof(unsigned long long) + ((size_t)n + (size_t)((n + 31) >> 5)) * sizeof(uint32_t);
  const int blocks = (int)std::min<int64_t>(n_units, kMaxBlocks);
  diamond_grow_kernel<<<blocks, kThreads, lds_request(diamond_grow_kernel, lds), st>>>(a);
  GSS_LAUNCH_CHECK("diamond_grow_kernel");
  return status.end("diamond_grow", "seed", n, max_size, max_deg, st);
}

}  // extern "C"
}  // namespace gss

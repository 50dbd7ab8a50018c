// proximity.hip -- drug-disease network proximity (Guney et al. 2016; method/test_proximity.py + the toolbox it calls) on the device.
//
// Four kernels (include/gssgcn.h has the contract, DESIGN.md section 9.2 the cost model and the measurements):
//   apsp_kernel       all-pairs hop distances as a uint8 N x N matrix: one workgroup per source, the source's level bytes in
//                     LDS, level-synchronous top-down BFS over the symmetric CSR (each frontier node's row is read once);
//   random_sets       one thread per (set, sample): the degree-matched random set of the toolbox (a draw from each member's
//                     degree bin, up to 20 redraws while the draw is already taken), compacted and sorted ascending; behind
//                     gss_prox_random_sets and, without a handle, gss_random_sets (set_modules.py draws the same sets from it);
//   set_stats         one wave per (set, sample): the inner closest mean (separation's d_AA) and the tied centres (center);
//   score_kernel      one wave per (pair, sample): all five measures from one pass over the T' x S' block of D;
//   stats_kernel      one thread per (pair, measure): mean / population sd over the samples in ascending order, z, pval.
// Sample 0 of every set is the set itself, samples 1..n_random the random sets k = 0..n_random-1.  All draws come from
// counter_rng.h keyed by (seed, kRngProxFrom / kRngProxTo, set, k, member * 32 + attempt), so tests/proximity_mirror.py replays them.
#include <math.h>

#include <algorithm>

#include "device_scope.h"

#include "counter_rng.h"

struct __attribute__((visibility("hidden"))) gss_prox {
  int32_t n;
  int32_t diameter;                 // max finite eccentricity
  gss::DeviceBuf<uint8_t> dist;     // [n][n]
  gss::DeviceBuf<double> vals;      // scoring scratch: [batch pairs][kProxMeasures][n_samples]
  gss::DeviceBuf<int32_t> flag;     // two device words for error reports
};

namespace gss {
namespace {

constexpr int kApspThreads = 512;
constexpr int32_t kApspMaxN = 65536;       // the level bytes of one source live in LDS
constexpr int kMeasures = 5;                // closest, shortest, kernel, center, separation
constexpr int kRedraws = 20;
constexpr int kScoreWaves = 4;
constexpr int32_t kMaxTo = 4096;            // per-wave LDS column minima of the to-set (uint8)
constexpr size_t kScratchBytes = size_t(256) << 20;

__global__ __launch_bounds__(kApspThreads) void apsp_kernel(int32_t n, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                            uint8_t *__restrict__ dist, int32_t *__restrict__ ecc_max,
                                                            int32_t *__restrict__ too_deep) {
  extern __shared__ uint8_t lvl[];
  const int32_t src = blockIdx.x;
  for (int32_t i = threadIdx.x; i < n; i += blockDim.x) lvl[i] = 255;
  __syncthreads();
  if (threadIdx.x == 0) lvl[src] = 0;
  __syncthreads();
  int cur = 0;
  for (;;) {
    int grew = 0, deep = 0;
    for (int32_t v = threadIdx.x; v < n; v += blockDim.x) {
      if (lvl[v] != cur) continue;
      for (int32_t e = rowptr[v], end = rowptr[v + 1]; e < end; ++e) {
        const int32_t u = col[e];
        if (lvl[u] == 255) {
          if (cur == 254) deep = 1;          // distance 255 would read as "unreachable"
          else { lvl[u] = (uint8_t)(cur + 1); grew = 1; }
        }
      }
    }
    if (__syncthreads_or(deep)) {
      if (threadIdx.x == 0) atomicOr(too_deep, 1);
      break;
    }
    if (!__syncthreads_or(grew)) break;
    ++cur;
  }
  uint8_t *row = dist + (int64_t)src * n;
  for (int32_t i = threadIdx.x; i < n; i += blockDim.x) row[i] = lvl[i];
  if (threadIdx.x == 0) atomicMax(ecc_max, cur);
}

struct RandArgs {
  int32_t n, n_sets, n_samples, max_size;
  const int32_t *set_ptr, *set_nodes, *node_bin, *bin_ptr, *bin_nodes;
  uint64_t seed, tag;
  int32_t *out_nodes, *out_size, *flag;
};

__device__ __forceinline__ bool taken(const int32_t *s, int32_t cnt, int32_t v) {
  for (int32_t i = 0; i < cnt; ++i)
    if (s[i] == v) return true;
  return false;
}

__global__ __launch_bounds__(256) void random_sets_kernel(RandArgs a) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)a.n_sets * a.n_samples) return;
  const int32_t s = (int32_t)(t / a.n_samples), r = (int32_t)(t % a.n_samples);
  const int32_t b0 = a.set_ptr[s], m = a.set_ptr[s + 1] - b0;
  int32_t *out = a.out_nodes + t * a.max_size;
  int32_t cnt = 0;
  if (m > a.max_size) {  // the host sizes max_size; never write past the row
    atomicOr(a.flag, 2);
    a.out_size[t] = 0;
    return;
  }
  for (int32_t i = 0; i < m; ++i) {
    const int32_t v = a.set_nodes[b0 + i];
    if (v < 0 || v >= a.n) {
      atomicOr(a.flag, 1);
      continue;
    }
    if (r == 0) {
      out[cnt++] = v;  // the set itself (sorted and unique on the host)
      continue;
    }
    const int32_t bin = a.node_bin[v], lo = a.bin_ptr[bin];
    const uint64_t sz = (uint64_t)(a.bin_ptr[bin + 1] - lo);
    const uint64_t k = (uint64_t)(r - 1);
    int32_t pick = a.bin_nodes[lo + (int32_t)(((uint64_t)rng_u32(rng_key(a.seed, a.tag, s, k, (uint64_t)i * 32)) * sz) >> 32)];
    for (int at = 1; at <= kRedraws && taken(out, cnt, pick); ++at)
      pick = a.bin_nodes[lo + (int32_t)(((uint64_t)rng_u32(rng_key(a.seed, a.tag, s, k, (uint64_t)i * 32 + at)) * sz) >> 32)];
    if (!taken(out, cnt, pick)) out[cnt++] = pick;
  }
  for (int32_t i = 1; i < cnt; ++i) {  // insertion sort: the compacted set ascending
    const int32_t v = out[i];
    int32_t j = i - 1;
    while (j >= 0 && out[j] > v) {
      out[j + 1] = out[j];
      --j;
    }
    out[j + 1] = v;
  }
  a.out_size[t] = cnt;
}

__device__ __forceinline__ int wave_min_i(int v) {
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ long long wave_sum_ll(long long v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

struct StatArgs {
  int32_t n, n_samples, max_size;
  int64_t n_units;
  const uint8_t *dist;
  const int32_t *nodes, *sizes;
  double *inner;
  int32_t *centres, *n_centres;
};

__global__ __launch_bounds__(256) void set_stats_kernel(StatArgs a) {
  const int32_t lane = threadIdx.x & 63;
  const int64_t unit = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (unit >= a.n_units) return;
  const int32_t cnt = a.sizes[unit];
  const int32_t *x = a.nodes + unit * a.max_size;
  long long inner = 0;
  int best = 0x7fffffff;
  for (int32_t i = lane; i < cnt; i += 64) {
    const uint8_t *row = a.dist + (int64_t)x[i] * a.n;
    int mn = 0x7fffffff, tot = 0;
    for (int32_t j = 0; j < cnt; ++j) {
      const int v = row[x[j]];
      tot += v;
      if (j != i) mn = min(mn, v);
    }
    if (cnt > 1) inner += mn;
    best = min(best, tot);
  }
  inner = wave_sum_ll(inner);
  best = wave_min_i(best);
  if (lane == 0) a.inner[unit] = cnt > 1 ? (double)inner / cnt : 0.0;
  if (!a.centres) return;
  int32_t *c = a.centres + unit * a.max_size;
  int32_t nc = 0;
  for (int32_t i0 = 0; i0 < cnt; i0 += 64) {  // every node of the set whose summed distance is minimal, ascending
    const int32_t i = i0 + lane;
    bool is_c = false;
    if (i < cnt) {
      const uint8_t *row = a.dist + (int64_t)x[i] * a.n;
      int tot = 0;
      for (int32_t j = 0; j < cnt; ++j) tot += row[x[j]];
      is_c = tot == best;
    }
    const uint64_t mask = __ballot(is_c);
    if (is_c) c[nc + __popcll(mask & ((1ull << lane) - 1))] = x[i];
    nc += __popcll(mask);
  }
  if (lane == 0) a.n_centres[unit] = nc;
}

struct ScoreArgs {
  int32_t n, n_samples, measures;
  int64_t p0, n_units, n_to_all;
  const uint8_t *dist;
  gss_prox_sets from, to;
  const int32_t *pair_from, *pair_to;
  double *vals;
};

__global__ __launch_bounds__(64 * kScoreWaves) void score_kernel(ScoreArgs a) {
  __shared__ double etab[256];
  __shared__ uint8_t colmin_all[kScoreWaves][kMaxTo];
  for (int v = threadIdx.x; v < 256; v += blockDim.x) etab[v] = exp(-(double)(v + 1));
  __syncthreads();
  const int32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t unit = (int64_t)blockIdx.x * kScoreWaves + w;
  if (unit >= a.n_units) return;
  const int64_t pl = unit / a.n_samples, p = a.p0 + pl;
  const int32_t r = (int32_t)(unit % a.n_samples);
  const int32_t i = a.pair_from ? a.pair_from[p] : (int32_t)(p / a.n_to_all);
  const int32_t j = a.pair_from ? a.pair_to[p] : (int32_t)(p % a.n_to_all);
  const int64_t fu = (int64_t)i * a.n_samples + r, tu = (int64_t)j * a.n_samples + r;
  const int32_t nt = a.from.sizes[fu], ns = a.to.sizes[tu];
  const int32_t *T = a.from.nodes + fu * a.from.max_size, *S = a.to.nodes + tu * a.to.max_size;
  double *out = a.vals + pl * kMeasures * a.n_samples + r;
  if (nt == 0 || ns == 0) {
    if (lane == 0)
      for (int m = 0; m < kMeasures; ++m) out[(int64_t)m * a.n_samples] = __builtin_nan("");
    return;
  }
  uint8_t *colmin = colmin_all[w];
  for (int32_t s = lane; s < ns; s += 64) colmin[s] = 255;
  long long closest = 0, shortest = 0;
  double kern = 0.0;
  for (int32_t t = 0; t < nt; ++t) {
    const uint8_t *row = a.dist + (int64_t)T[t] * a.n;
    int mn = 255;
    double ex = 0.0;
    for (int32_t s = lane; s < ns; s += 64) {
      const int v = row[S[s]];
      mn = min(mn, v);
      shortest += v;
      ex += etab[v];
      if (v < colmin[s]) colmin[s] = (uint8_t)v;
    }
    closest += wave_min_i(mn);
    if (a.measures & 4) kern += log(wave_sum_d(ex) / ns);
  }
  shortest = wave_sum_ll(shortest);
  double centre = 0.0, sep = 0.0;
  if (a.measures & 8) {
    const int32_t nc = a.to.n_centres[tu];
    const int32_t *C = a.to.centres + tu * a.to.max_size;
    long long cs = 0;
    for (int32_t t = 0; t < nt; ++t) {
      const uint8_t *row = a.dist + (int64_t)T[t] * a.n;
      for (int32_t c = lane; c < nc; c += 64) cs += row[C[c]];
    }
    centre = (double)wave_sum_ll(cs) / ((double)nt * nc);
  }
  if (a.measures & 16) {
    long long cm = 0;
    for (int32_t s = lane; s < ns; s += 64) cm += colmin[s];
    cm = wave_sum_ll(cm);
    sep = (double)(closest + cm) / (nt + ns) - (a.from.inner[fu] + a.to.inner[tu]) / 2.0;
  }
  if (lane == 0) {
    const int64_t st = a.n_samples;
    out[0] = (double)closest / nt;
    out[st] = (double)shortest / ((double)nt * ns);
    out[2 * st] = -kern / nt;
    out[3 * st] = centre;
    out[4 * st] = sep;
  }
}

__global__ __launch_bounds__(256) void stats_kernel(int64_t n_items, int32_t n_samples, int64_t p0, const double *__restrict__ vals,
                                                    double *__restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_items) return;
  const double *x = vals + t * n_samples;
  double *o = out + (p0 * kMeasures + t) * 5;
  const double d = x[0];
  const int32_t k = n_samples - 1;
  if (isnan(d)) {
    for (int q = 0; q < 5; ++q) o[q] = d;
    return;
  }
  double sum = 0.0;
  for (int32_t i = 1; i <= k; ++i) sum += x[i];
  const double m = sum / k;
  double ss = 0.0;
  for (int32_t i = 1; i <= k; ++i) ss += (x[i] - m) * (x[i] - m);
  const double s = sqrt(ss / k);
  const double z = s == 0.0 ? 0.0 : (d - m) / s;
  o[0] = d;
  o[1] = m;
  o[2] = s;
  o[3] = z;
  o[4] = 0.5 * erfc(-z * M_SQRT1_2);
}

int check_sets(const char *what, const gss_prox_sets *s, int32_t n_samples) {
  GSS_REQUIRE(s, "prox_score: %s sets missing", what);
  GSS_REQUIRE(s->n_sets >= 1 && s->max_size >= 1, "prox_score: %s: n_sets=%d max_size=%d must be >= 1", what, s->n_sets, s->max_size);
  GSS_REQUIRE(s->nodes && s->sizes && s->inner, "prox_score: %s: null nodes / sizes / inner", what);
  GSS_REQUIRE((int64_t)s->n_sets * n_samples * s->max_size < (int64_t(1) << 40), "prox_score: %s sets too large", what);
  return GSS_OK;
}

// gss_prox_random_sets and gss_random_sets: the checks, the launch and the read-back of the status word `flag` (device), in `who`'s name
int random_sets(const char *who, int32_t n, int32_t *flag, int32_t side, int32_t n_sets, const int32_t *set_ptr, const int32_t *set_nodes,
                int32_t max_size, const int32_t *node_bin, const int32_t *bin_ptr, const int32_t *bin_nodes, int32_t n_random, uint64_t seed,
                int32_t *out_nodes, int32_t *out_size, void *stream) {
  GSS_REQUIRE(side == 0 || side == 1, "%s: side=%d must be 0 (from) or 1 (to)", who, side);
  GSS_REQUIRE(n_sets >= 1 && max_size >= 1 && n_random >= 0, "%s: n_sets=%d max_size=%d n_random=%d", who, n_sets, max_size, n_random);
  GSS_REQUIRE(set_ptr && set_nodes && node_bin && bin_ptr && bin_nodes && out_nodes && out_size, "%s: null pointer", who);
  hipStream_t st = as_stream(stream);
  RandArgs a;
  a.n = n;
  a.n_sets = n_sets;
  a.n_samples = n_random + 1;
  a.max_size = max_size;
  a.set_ptr = set_ptr;
  a.set_nodes = set_nodes;
  a.node_bin = node_bin;
  a.bin_ptr = bin_ptr;
  a.bin_nodes = bin_nodes;
  a.seed = seed;
  a.tag = side == 0 ? kRngProxFrom : kRngProxTo;
  a.out_nodes = out_nodes;
  a.out_size = out_size;
  a.flag = flag;
  GSS_HIP(hipMemsetAsync(a.flag, 0, sizeof(int32_t), st));
  const int64_t units = (int64_t)n_sets * a.n_samples;
  random_sets_kernel<<<ceil_div(units, 256), 256, 0, st>>>(a);
  GSS_LAUNCH_CHECK("random_sets_kernel");
  int32_t h = 0;
  if (int rc = read_back(&h, a.flag, sizeof(int32_t), st)) return rc;
  GSS_REQUIRE(!(h & 1), "%s: a set member is not a node index in [0, %d)", who, n);
  GSS_REQUIRE(!(h & 2), "%s: a set has more than max_size=%d members", who, max_size);
  return GSS_OK;
}

}  // namespace

extern "C" {

int gss_prox_create(gss_prox **out, int32_t n, const int32_t *rowptr, const int32_t *col, int64_t max_bytes, void *stream) {
  GSS_REQUIRE(out && rowptr && col, "prox_create: null argument");
  *out = nullptr;
  GSS_REQUIRE(n >= 1 && n <= kApspMaxN, "prox_create: n=%d must be in [1, %d] (one source's levels live in LDS)", n, kApspMaxN);
  const int64_t bytes = (int64_t)n * n;
  GSS_REQUIRE(bytes <= max_bytes, "prox_create: the distance matrix needs %lld bytes (N=%d), above the budget max_bytes=%lld",
              (long long)bytes, n, (long long)max_bytes);
  hipStream_t st = as_stream(stream);
  std::unique_ptr<gss_prox> p(new gss_prox());
  p->n = n;
  if (p->dist.alloc("prox_create", (size_t)bytes) || p->flag.alloc("prox_create", 2 * sizeof(int32_t)))
    return fail(GSS_ENOMEM, "prox_create: hipMalloc of %lld bytes failed", (long long)bytes);
  int32_t *dev = p->flag.p, h[2] = {0, 0};
  GSS_HIP(hipMemsetAsync(dev, 0, 2 * sizeof(int32_t), st));
  apsp_kernel<<<n, kApspThreads, (size_t)n, st>>>(n, rowptr, col, p->dist.p, dev, dev + 1);
  GSS_LAUNCH_CHECK("apsp_kernel");
  if (int rc = read_back(h, dev, sizeof(h), st)) return rc;
  GSS_REQUIRE(!h[1], "prox_create: a node lies 255 or more hops from another; distances are stored in one byte (eccentricity <= 254)");
  p->diameter = h[0];
  *out = p.release();
  return GSS_OK;
}

void gss_prox_destroy(gss_prox *p) { delete p; }

const uint8_t *gss_prox_distances(const gss_prox *p) { return p ? p->dist.p : nullptr; }

int32_t gss_prox_diameter(const gss_prox *p) { return p ? p->diameter : -1; }

int gss_prox_random_sets(gss_prox *p, int32_t side, int32_t n_sets, const int32_t *set_ptr, const int32_t *set_nodes, int32_t max_size,
                         const int32_t *node_bin, const int32_t *bin_ptr, const int32_t *bin_nodes, int32_t n_random, uint64_t seed,
                         int32_t *out_nodes, int32_t *out_size, void *stream) {
  GSS_REQUIRE(p, "prox_random_sets: null handle");
  return random_sets("prox_random_sets", p->n, p->flag.p, side, n_sets, set_ptr, set_nodes, max_size, node_bin, bin_ptr, bin_nodes, n_random,
                     seed, out_nodes, out_size, stream);
}

int gss_random_sets(int32_t n, int32_t side, int32_t n_sets, const int32_t *set_ptr, const int32_t *set_nodes, int32_t max_size,
                    const int32_t *node_bin, const int32_t *bin_ptr, const int32_t *bin_nodes, int32_t n_random, uint64_t seed,
                    int32_t *out_nodes, int32_t *out_size, void *stream) {
  GSS_REQUIRE(n >= 1, "random_sets: n=%d must be >= 1", n);
  DeviceBuf<int32_t> flag;
  if (int rc = flag.alloc("random_sets", sizeof(int32_t))) return rc;
  return random_sets("random_sets", n, flag.p, side, n_sets, set_ptr, set_nodes, max_size, node_bin, bin_ptr, bin_nodes, n_random, seed,
                     out_nodes, out_size, stream);
}

int gss_prox_set_stats(gss_prox *p, int32_t n_sets, int32_t n_samples, int32_t max_size, const int32_t *nodes, const int32_t *sizes,
                       double *inner, int32_t *centres, int32_t *n_centres, void *stream) {
  GSS_REQUIRE(p && nodes && sizes && inner, "prox_set_stats: null argument");
  GSS_REQUIRE(!centres == !n_centres, "prox_set_stats: centres and n_centres go together");
  GSS_REQUIRE(n_sets >= 1 && n_samples >= 1 && max_size >= 1, "prox_set_stats: n_sets=%d n_samples=%d max_size=%d", n_sets, n_samples,
              max_size);
  StatArgs a;
  a.n = p->n;
  a.n_units = (int64_t)n_sets * n_samples;
  a.n_samples = n_samples;
  a.max_size = max_size;
  a.dist = p->dist.p;
  a.nodes = nodes;
  a.sizes = sizes;
  a.inner = inner;
  a.centres = centres;
  a.n_centres = n_centres;
  set_stats_kernel<<<ceil_div((int64_t)a.n_units * 64, 256), 256, 0, as_stream(stream)>>>(a);
  GSS_LAUNCH_CHECK("set_stats_kernel");
  return GSS_OK;
}

int gss_prox_score(gss_prox *p, const gss_prox_sets *from, const gss_prox_sets *to, int32_t n_samples, int64_t n_pairs,
                   const int32_t *pair_from, const int32_t *pair_to, int32_t measures, double *out, void *stream) {
  GSS_REQUIRE(p && out, "prox_score: null argument");
  GSS_REQUIRE(n_samples >= 3, "prox_score: n_samples=%d: need the set itself and n_random >= 2 random samples", n_samples);
  if (int rc = check_sets("from", from, n_samples)) return rc;
  if (int rc = check_sets("to", to, n_samples)) return rc;
  GSS_REQUIRE(to->max_size <= kMaxTo, "prox_score: to-sets of up to %d nodes are supported (max_size=%d)", kMaxTo, to->max_size);
  GSS_REQUIRE(measures > 0 && measures < 32, "prox_score: measures=%d must be a non-empty mask of the 5 measure bits", measures);
  GSS_REQUIRE(!(measures & 8) || (to->centres && to->n_centres), "prox_score: center needs the to-sets' centres");
  GSS_REQUIRE(!pair_from == !pair_to, "prox_score: pair_from and pair_to go together");
  const int64_t all = (int64_t)from->n_sets * to->n_sets;
  GSS_REQUIRE(n_pairs >= 0 && (pair_from || n_pairs == all), "prox_score: without pair lists n_pairs must be n_from * n_to = %lld",
              (long long)all);
  if (n_pairs == 0) return GSS_OK;
  hipStream_t st = as_stream(stream);
  const size_t per_pair = (size_t)kMeasures * n_samples * sizeof(double);
  int64_t batch = std::max<int64_t>(1, (int64_t)(kScratchBytes / per_pair));
  batch = std::min(batch, n_pairs);
  if (K().prox_batch_pairs > 0) batch = std::min<int64_t>(batch, K().prox_batch_pairs);   // knob: a few pairs take several trips
  const size_t want = (size_t)batch * per_pair;
  if (p->vals.bytes < want)
    if (int rc = p->vals.alloc("prox_score", want)) return rc;
  ScoreArgs a;
  a.n = p->n;
  a.n_samples = n_samples;
  a.measures = measures;
  a.n_to_all = to->n_sets;
  a.dist = p->dist.p;
  a.from = *from;
  a.to = *to;
  a.pair_from = pair_from;
  a.pair_to = pair_to;
  a.vals = p->vals.p;
  for (int64_t p0 = 0; p0 < n_pairs; p0 += batch) {
    const int64_t nb = std::min(batch, n_pairs - p0);
    a.p0 = p0;
    a.n_units = nb * n_samples;
    score_kernel<<<ceil_div(a.n_units, kScoreWaves), 64 * kScoreWaves, 0, st>>>(a);
    GSS_LAUNCH_CHECK("score_kernel");
    stats_kernel<<<ceil_div(nb * kMeasures, 256), 256, 0, st>>>(nb * kMeasures, n_samples, p0, p->vals.p, out);
    GSS_LAUNCH_CHECK("stats_kernel");
  }
  return GSS_OK;
}

}  // extern "C"
}  // namespace gss

// profile_topk.hip -- the k highest nodes of listed profile columns, per node group (gss_profile_topk), and how many nodes two such selections
// share (gss_topk_overlap): "the proteins and biological functions" a treatment's diffusion profile runs through.
//
// include/gssgcn.h has the contract, DESIGN.md section 9.11 the cost model and the measurements.  A column of 29,960 keys is 240 KB and does not
// fit the LDS, and k <= 1024 of them are wanted: the column is not sorted, the k-th key is SELECTED.  Per panel of kKeyPanel listed columns:
//   keys_kernel       (profile_front.h, shared with gss_profile_rank) reads the panel's columns of x by rows (adjacent lanes = adjacent listed
//                     columns) and writes rank_keys.h's order-preserving uint64 keys [panel][n] into the workspace through a 64 x 64 LDS tile
//                     (-0.0 folded into +0.0, NaN -> the all-ones key)
//   tk_select_kernel  one workgroup per column, all G groups at once (node i's group is read beside its key):
//                       sweep 0    counts every group's members and notes a NaN among them;
//                       sweeps     a radix select, 8-bit digits from the top: every key that still matches its group's prefix adds one to
//                                  hist[group][digit] in LDS; wave g then scans group g's 256 bins from the top and extends the prefix by the
//                                  digit that holds the group's `need`-th key.  A group whose bucket is taken whole (need == its count) is
//                                  done -- with distinct keys after two or three sweeps; a group with more ties at the k-th key than places
//                                  left goes on with up to three sweeps over the digits of the NODE INDEX among the tied keys (ascending), so
//                                  that its threshold (key T, index I) admits exactly min(k, members) nodes: key > T, or key == T and i <= I;
//                       collect    one more sweep appends the admitted (key, index) pairs to the group's LDS list (an integer slot counter);
//                       sort       the list is bitonic-sorted by (key descending, index ascending) -- a total order, so the slot order of
//                                  the collection does not show -- and written out; val is read back from x, bit for bit.
// Groups are in different phases in one sweep, and a finished group's keys are not read again.  The only atomics are integer counters in LDS.
// The checks of the column, group and selection lists are profile_front.h's.
#include "profile_front.h"

namespace gss {
namespace {

constexpr int kTkThreads = 512;        // the select kernel: 8 waves, wave g scans group g's histogram
constexpr int kTkMaxK = 1024;
constexpr int kTkMaxGroups = 8;
constexpr int kTkBins = 256;
constexpr int kTkKeyPhases = 8, kTkIdxPhases = 3, kTkDone = kTkKeyPhases + kTkIdxPhases;
constexpr int kToThreads = 256;        // the overlap kernel
static_assert(kTkThreads / kWave >= kTkMaxGroups, "one wave per group scans its histogram");

// hist[bin] += 1 for every active lane.  The lanes that share the first active lane's bin add once, together: a column's keys share their
// leading digits, and 64 additions to one LDS word would queue.  EVERY lane of the wave must reach the call
__device__ __forceinline__ void hist_add(int32_t *hist, int32_t bin, bool active) {
  const uint64_t act = __ballot(active);
  if (act == 0) return;   // uniform over the wave
  const int leader = __ffsll((unsigned long long)act) - 1;
  const int32_t lb = __shfl(bin, leader);
  const uint64_t same = __ballot(active && bin == lb);
  if (!active) return;
  if (bin != lb) atomicAdd(&hist[bin], 1);
  else if ((int)(threadIdx.x & 63) == leader) atomicAdd(&hist[lb], (int32_t)__popcll((unsigned long long)same));
}

// what a group's select has decided so far
struct TkState {
  uint64_t T[kTkMaxGroups];        // key phases: the decided leading digits, zeros below; then the k-th key
  int32_t I[kTkMaxGroups];         // index phases: the decided leading digits of the last admitted tied index, zeros below; then that index
  int32_t phase[kTkMaxGroups];     // 0 .. 7 key digit, 8 .. 10 index digit, kTkDone
  int32_t need[kTkMaxGroups];      // places left for the keys that match the prefix
  int32_t take[kTkMaxGroups];      // min(k, members); -1 = a NaN among the members
  int32_t size[kTkMaxGroups];
  int32_t nan[kTkMaxGroups];
  int32_t fill[kTkMaxGroups];
};

// workgroup = panel column blockIdx.x (list position first + blockIdx.x)
__global__ __launch_bounds__(kTkThreads) void tk_select_kernel(int32_t n, const uint64_t *__restrict__ keys, const int32_t *__restrict__ group,
                                                                int32_t G, int32_t k, int32_t cp, const double *__restrict__ x, int64_t ld,
                                                                int32_t first, const int32_t *__restrict__ cols, int32_t *__restrict__ idx,
                                                                double *__restrict__ val, int32_t *__restrict__ cnt) {
  extern __shared__ __align__(16) unsigned char tk_lds[];
  uint64_t *ck = reinterpret_cast<uint64_t *>(tk_lds);                 // [G][cp] the admitted keys
  int32_t *ci = reinterpret_cast<int32_t *>(ck + (size_t)G * cp);       // [G][cp] and their node indices
  int32_t *hist = ci + (size_t)G * cp;                                  // [G][kTkBins]
  __shared__ TkState s;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint64_t *key = keys + (size_t)blockIdx.x * n;

  for (int32_t q = tid; q < G * kTkBins; q += kTkThreads) hist[q] = 0;
  if (tid < kTkMaxGroups) {
    s.size[tid] = 0;
    s.nan[tid] = 0;
    s.fill[tid] = 0;
  }
  __syncthreads();
  // sweep 0: members and NaNs per group
  for (int32_t base = 0; base < n; base += kTkThreads) {
    const int32_t i = base + tid;
    int32_t g = -1;
    if (i < n) g = group ? group[i] : 0;
    const bool member = g >= 0 && g < G;
    hist_add(s.size, member ? g : 0, member);
    if (member && key[i] == kBehind) s.nan[g] = 1;
  }
  __syncthreads();
  if (tid < G) {
    const int32_t size = s.size[tid];
    const bool all = size <= k;                       // everything is admitted: key > 0 holds for every key
    s.take[tid] = s.nan[tid] ? -1 : (all ? size : k);
    s.phase[tid] = (s.nan[tid] || all) ? kTkDone : 0;
    s.need[tid] = k;
    s.T[tid] = 0;
    s.I[tid] = INT32_MAX;
  }
  __syncthreads();

  for (int sweep = 0; sweep < kTkDone; ++sweep) {   // a busy group's phase grows with every sweep: kTkDone sweeps finish every group
    bool busy = false;
    for (int32_t g = 0; g < G; ++g) busy |= s.phase[g] != kTkDone;
    if (!busy) break;   // uniform: everyone read the same words behind a barrier
    for (int32_t base = 0; base < n; base += kTkThreads) {
      const int32_t i = base + tid;
      int32_t g = -1;
      if (i < n) g = group ? group[i] : 0;
      bool active = false;
      int32_t bin = 0;
      if (g >= 0 && g < G) {
        const int32_t ph = s.phase[g];
        if (ph != kTkDone) {
          const uint64_t key_i = key[i];
          if (ph < kTkKeyPhases) {
            const int shift = 56 - 8 * ph;
            active = ph == 0 || ((key_i ^ s.T[g]) >> (shift + 8)) == 0;
            bin = g * kTkBins + (int32_t)((key_i >> shift) & 255u);
          } else {
            const int shift = 16 - 8 * (ph - kTkKeyPhases);
            active = key_i == s.T[g] && (ph == kTkKeyPhases || ((i ^ s.I[g]) >> (shift + 8)) == 0);
            bin = g * kTkBins + ((i >> shift) & 255);
          }
        }
      }
      hist_add(hist, bin, active);
    }
    __syncthreads();
    // wave g extends group g's prefix: lane l holds bins 4 l .. 4 l + 3
    if (wave < G && s.phase[wave] != kTkDone) {
      const int32_t g = wave, ph = s.phase[g], need = s.need[g];
      const bool by_key = ph < kTkKeyPhases;            // keys: from the top bin down; indices: from the bottom bin up
      int32_t h[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) h[e] = hist[g * kTkBins + 4 * lane + e];
      const int32_t mine = h[0] + h[1] + h[2] + h[3];
      int32_t run = mine;                               // inclusive scan toward this lane: from lane 63 down (keys) or from lane 0 up
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int32_t v = by_key ? __shfl_down(run, o) : __shfl_up(run, o);
        if (by_key ? lane + o < 64 : lane >= o) run += v;
      }
      int32_t before = run - mine;                      // what the bins ahead of this lane's hold
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int b = by_key ? 3 - e : e;
        const int32_t hb = by_key ? h[3 - e] : h[e];    // static register indices either way
        if (before < need && need <= before + hb) {     // one (lane, bin) of the wave: 1 <= need <= the sum of the bins
          const int32_t digit = 4 * lane + b, left = need - before;
          const bool whole = hb == left;                // the bucket is taken whole: nothing below this digit matters
          if (by_key) {
            const uint64_t T = s.T[g] | ((uint64_t)digit << (56 - 8 * ph));
            s.T[g] = T;
            s.need[g] = left;
            s.phase[g] = whole ? kTkDone : ph + 1;       // after the last key digit: ties at the k-th key, on to the index digits
          } else {
            const int shift = 16 - 8 * (ph - kTkKeyPhases);
            const int32_t I = (ph == kTkKeyPhases ? 0 : s.I[g]) | (digit << shift);
            s.I[g] = whole ? (I | ((1 << shift) - 1)) : I;
            s.need[g] = left;
            s.phase[g] = (whole || ph + 1 == kTkDone) ? kTkDone : ph + 1;
          }
        }
        before += hb;
      }
    }
    __syncthreads();
    for (int32_t q = tid; q < G * kTkBins; q += kTkThreads) hist[q] = 0;
    __syncthreads();
  }

  // collect: exactly take[g] pairs per group
  for (int32_t i = tid; i < n; i += kTkThreads) {
    const int32_t g = group ? group[i] : 0;
    if (g < 0 || g >= G || s.take[g] <= 0) continue;
    const uint64_t key_i = key[i], T = s.T[g];
    if (key_i > T || (key_i == T && (s.I[g] == INT32_MAX || i <= s.I[g]))) {
      const int32_t slot = atomicAdd(&s.fill[g], 1);
      if (slot < cp) {
        ck[(size_t)g * cp + slot] = key_i;
        ci[(size_t)g * cp + slot] = i;
      }
    }
  }
  __syncthreads();
  const int32_t j = first + blockIdx.x;
  const int32_t c = cols ? cols[j] : j;
  for (int32_t g = 0; g < G; ++g) {
    const int32_t take = s.take[g];
    uint64_t *gk = ck + (size_t)g * cp;
    int32_t *gi = ci + (size_t)g * cp;
    if (take > 0) {   // uniform
      for (int32_t q = min(s.fill[g], take) + tid; q < cp; q += kTkThreads) {   // the padding sorts behind every pair: no key is 0
        gk[q] = 0;
        gi[q] = INT32_MAX;
      }
      __syncthreads();
      for (int32_t kk = 2; kk <= cp; kk <<= 1) {
        for (int32_t jj = kk >> 1; jj > 0; jj >>= 1) {
          for (int32_t q = tid; q < cp / 2; q += kTkThreads) {
            const int32_t lo = ((q & ~(jj - 1)) << 1) | (q & (jj - 1)), hi = lo + jj;
            const uint64_t ka = gk[lo], kb = gk[hi];
            const int32_t ia = gi[lo], ib = gi[hi];
            const bool b_first = kb > ka || (kb == ka && ib < ia);   // the pair at hi belongs in front of the pair at lo
            if (b_first == ((lo & kk) == 0)) {
              gk[lo] = kb;
              gk[hi] = ka;
              gi[lo] = ib;
              gi[hi] = ia;
            }
          }
          __syncthreads();
        }
      }
    }
    const size_t out = ((size_t)j * G + g) * k;
    for (int32_t q = tid; q < k; q += kTkThreads) {
      const int32_t node = (q < take && gi[q] < n) ? gi[q] : -1;   // (never the padding: the collection filled take slots)
      idx[out + q] = node;
      val[out + q] = node >= 0 ? x[(int64_t)node * ld + c] : __longlong_as_double(0x7ff8000000000000ll);
    }
    if (tid == 0) cnt[(size_t)j * G + g] = take;
  }
}

// workgroup = (pair blockIdx.x, group blockIdx.y): side a sorted in LDS, every entry of side b searched in it
__global__ __launch_bounds__(kToThreads) void to_overlap_kernel(int32_t G, int32_t k, int32_t cp, const int32_t *__restrict__ idx,
                                                                 const int32_t *__restrict__ cnt, const int32_t *__restrict__ a,
                                                                 const int32_t *__restrict__ b, int32_t *__restrict__ shared) {
  extern __shared__ __align__(16) unsigned char to_lds[];
  uint64_t *srt = reinterpret_cast<uint64_t *>(to_lds);   // [cp]
  __shared__ int32_t hits;
  const int tid = threadIdx.x;
  const int32_t t = blockIdx.x, g = blockIdx.y;
  const size_t sa = (size_t)a[t] * G + g, sb = (size_t)b[t] * G + g;
  const int32_t ca = cnt[sa], cb = cnt[sb];
  if (ca < 0 || cb < 0) {   // uniform
    if (tid == 0) shared[(size_t)t * G + g] = -1;
    return;
  }
  const int32_t la = min(ca, k), lb = min(cb, k);
  if (tid == 0) hits = 0;
  for (int32_t q = tid; q < cp; q += kToThreads) srt[q] = q < la ? (uint64_t)(uint32_t)idx[sa * k + q] : kBehind;
  __syncthreads();
  sort_keys<kToThreads>(srt, cp, tid);
  int32_t found = 0;
  for (int32_t q = tid; q < lb; q += kToThreads) {
    const uint64_t want = (uint64_t)(uint32_t)idx[sb * k + q];
    const int32_t at = search(srt, 0, la, want, false);
    found += (at < la && srt[at] == want) ? 1 : 0;
  }
  if (found) atomicAdd(&hits, found);
  __syncthreads();
  if (tid == 0) shared[(size_t)t * G + g] = hits;
}

}  // namespace
}  // namespace gss

using namespace gss;

extern "C" {

// status words, then the keys of a panel
size_t gss_profile_topk_workspace_bytes(int32_t n, int32_t nc, int32_t G, int32_t k) {
  if (n < 1 || n > kKeyMaxRows || nc < 0 || G < 1 || G > kTkMaxGroups || k < 1 || k > kTkMaxK) return 0;
  const size_t p = (size_t)(nc < kKeyPanel ? nc : kKeyPanel);
  return kStatusBytes + p * (size_t)n * 8;
}

int gss_profile_topk(int32_t n, const double *x, int64_t ld, int32_t nc, const int32_t *cols, int32_t G, const int32_t *group, int32_t k,
                     int32_t *idx, double *val, int32_t *cnt, void *workspace, size_t workspace_bytes, void *stream) {
  GSS_REQUIRE(n >= 1, "profile_topk: n=%d rows must be >= 1", n);
  GSS_REQUIRE(n <= kKeyMaxRows, "profile_topk: n=%d rows is above the limit of %d (ties are resolved over three 8-bit digits of the node index)", n,
              kKeyMaxRows);
  GSS_REQUIRE(k >= 1 && k <= kTkMaxK, "profile_topk: k=%d is outside [1, %d]", k, kTkMaxK);
  GSS_REQUIRE(G >= 1 && G <= kTkMaxGroups, "profile_topk: G=%d groups is outside [1, %d]", G, kTkMaxGroups);
  GSS_REQUIRE(nc >= 0, "profile_topk: nc=%d columns must be >= 0", nc);
  GSS_REQUIRE(ld >= 1, "profile_topk: ld=%lld must be >= 1", (long long)ld);
  if (nc == 0) return GSS_OK;
  GSS_REQUIRE(x != nullptr, "profile_topk: x is null");
  GSS_REQUIRE(idx != nullptr, "profile_topk: idx is null");
  GSS_REQUIRE(val != nullptr, "profile_topk: val is null");
  GSS_REQUIRE(cnt != nullptr, "profile_topk: cnt is null");
  GSS_REQUIRE(workspace != nullptr, "profile_topk: workspace is null");
  GSS_REQUIRE(group || G == 1, "profile_topk: group is null (every node in group 0) and G=%d is not 1", G);
  GSS_REQUIRE(cols || nc <= ld, "profile_topk: ld=%lld is below nc=%d (cols is null: columns 0 .. nc - 1)", (long long)ld, nc);
  GSS_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "profile_topk: workspace is not 8-byte aligned");
  const size_t want = gss_profile_topk_workspace_bytes(n, nc, G, k);
  GSS_REQUIRE(workspace_bytes >= want, "profile_topk: workspace of %zu bytes is below the %zu that n=%d, nc=%d need", workspace_bytes, want, n, nc);
  hipStream_t st = as_stream(stream);
  if (cols || group) {   // nothing reads x through the list, or a histogram through a group, before every entry is known to be in range
    const CheckedList a{cols, nc, 0, ld, "cols", "ld"}, b{group, group ? n : 0, -1, G, "group", "G"};
    if (int rc = check_lists("profile_topk", a, b, static_cast<uint32_t *>(workspace), st)) return rc;
  }
  uint64_t *keys = reinterpret_cast<uint64_t *>(static_cast<char *>(workspace) + kStatusBytes);
  const int32_t cp = pow2_at_least(k);
  const size_t lds = (size_t)G * cp * 12 + (size_t)G * kTkBins * 4;
  const size_t lds_arg = lds_request(tk_select_kernel, lds);
  for (int32_t first = 0; first < nc; first += kKeyPanel) {   // the stream orders a panel's two launches and the panels after one another
    const int32_t pw = nc - first < kKeyPanel ? nc - first : kKeyPanel;
    if (int rc = launch_keys(n, x, ld, pw, first, cols, keys, st)) return rc;
    hipLaunchKernelGGL(tk_select_kernel, dim3(pw), dim3(kTkThreads), lds_arg, st, n, keys, group, G, k, cp, x, ld, first, cols, idx, val, cnt);
    GSS_LAUNCH_CHECK("tk_select_kernel");
  }
  return GSS_OK;
}

int gss_topk_overlap(int32_t S, int32_t G, int32_t k, const int32_t *idx, const int32_t *cnt, int32_t T, const int32_t *a, const int32_t *b,
                     int32_t *shared, void *stream) {
  GSS_REQUIRE(S >= 1, "topk_overlap: S=%d selections must be >= 1", S);
  GSS_REQUIRE(k >= 1 && k <= kTkMaxK, "topk_overlap: k=%d is outside [1, %d]", k, kTkMaxK);
  GSS_REQUIRE(G >= 1 && G <= kTkMaxGroups, "topk_overlap: G=%d groups is outside [1, %d]", G, kTkMaxGroups);
  GSS_REQUIRE(T >= 0, "topk_overlap: T=%d pairs must be >= 0", T);
  if (T == 0) return GSS_OK;
  GSS_REQUIRE(idx != nullptr, "topk_overlap: idx is null");
  GSS_REQUIRE(cnt != nullptr, "topk_overlap: cnt is null");
  GSS_REQUIRE(a != nullptr, "topk_overlap: a is null");
  GSS_REQUIRE(b != nullptr, "topk_overlap: b is null");
  GSS_REQUIRE(shared != nullptr, "topk_overlap: shared is null");
  hipStream_t st = as_stream(stream);
  {   // nothing reads idx or cnt through a list before every entry of it is known to be a selection; the status words are freed before the launch
    DeviceBuf<uint32_t> status;
    if (int rc = status.alloc("topk_overlap", 8)) return rc;
    const CheckedList la{a, T, 0, S, "a", "S"}, lb{b, T, 0, S, "b", "S"};
    if (int rc = check_lists("topk_overlap", la, lb, status.p, st)) return rc;
  }
  const int32_t cp = pow2_at_least(k);
  hipLaunchKernelGGL(to_overlap_kernel, dim3(T, G), dim3(kToThreads), (size_t)cp * 8, st, G, k, cp, idx, cnt, a, b, shared);
  GSS_LAUNCH_CHECK("to_overlap_kernel");
  return GSS_OK;
}

}  // extern "C"

// rank_metrics.hip -- batched ROC-AUC, average precision and hits@k, one query per row (the three ranking statistics the
// multiscale-interactome work reports for drug-indication prediction; include/gssgcn.h has the contract, DESIGN.md section 9.8 the
// definitions, the cost model and the measurement).
//
// One workgroup per row, as auc.hip; the key, the sort, the search and the check of the row's positives are rank_keys.h's, which both
// files use.  160 KiB of LDS hold the 16,384 keys of one sorted array, not two, so the row is sorted twice in the same LDS buffer:
//   1. the positives' keys (negatives and padding get the all-ones key and sort behind them); the P sorted keys are parked in the row's
//      slice of the caller's workspace, ws[r * C .. r * C + P);
//   2. the negatives' keys, as auc.hip does; they stay in LDS.
// Sorted positive i (key k) then takes four counts by binary search, negL / negU in LDS and posL / posU in its parked slice (the number
// of keys below k, and of keys not above k, among the negatives and among the positives), and everything follows from those integers:
//   AUC   2 U = sum over positives of (negL + negU), one division: the integers and the expression of auc.hip, so the same bits;
//   AP    the first positive of a tie group (i == posL) adds pos_g TP_g / (TP_g + FP_g) with pos_g = posU - posL, TP_g = P - posL,
//         FP_g = N - negL: an exact integer product and one division per group.  Thread t adds the groups of sorted positives
//         P-1-t, P-1-t-256, ... (descending threshold) serially, then a butterfly over the wave and the four waves in order: the order
//         comes from the sorted keys alone, never from the pos_col list;
//   hits  the item of rank k' (descending) has ascending index m = C - k' in the merged order.  With lt = posL + negL and le = posU + negU
//         a positive's tie group holds that item iff lt <= m < le, and lies strictly above it iff lt > m.  The first positive of the one
//         group that holds it writes that group's counts; every positive counts itself into `above` where lt > m (integer sums).  If no
//         positive's group holds the item its group has no positive and hits = above.
// Every output word is written by one thread and no result goes through an atomic: bitwise reproducible, and a function of the row's
// multiset of (score, label) pairs alone.
#include "rank_keys.h"

namespace gss {
namespace {

constexpr int kRmThreads = 256;
constexpr int kRmWaves = kRmThreads / kWave;
constexpr int kRmMaxCols = 16384;               // the sort buffer: pow2ceil(C) keys of 8 bytes in LDS (128 KiB at the limit)
constexpr int kRmMaxCuts = 8;

struct Cuts {
  int32_t nk;
  int32_t m[kRmMaxCuts];   // ascending index of the item of rank min(k, C): C - min(k, C)
};

__global__ __launch_bounds__(kRmThreads) void rank_metrics_kernel(int32_t C, int32_t cpad, const double *__restrict__ scores, int64_t ld,
                                                                  const int32_t *__restrict__ pos_ptr, const int32_t *__restrict__ pos_col,
                                                                  Cuts cuts, double *__restrict__ auc, double *__restrict__ ap,
                                                                  double *__restrict__ hits, int32_t *__restrict__ n_pos,
                                                                  int32_t *__restrict__ n_neg, uint64_t *ws) {
  extern __shared__ __align__(16) unsigned char lds[];
  uint64_t *key = reinterpret_cast<uint64_t *>(lds);                        // [cpad]
  uint32_t *is_pos = reinterpret_cast<uint32_t *>(lds + (size_t)cpad * 8);  // [cpad / 32] bitmap
  __shared__ unsigned long long part_u[kRmWaves];
  __shared__ double part_ap[kRmWaves];
  __shared__ int32_t part_above[kRmWaves][kRmMaxCuts];
  __shared__ int32_t grp[kRmMaxCuts][4];   // the tie group that holds cut j's item, if it has a positive: posL, posU, negL, negU
  const int32_t r = blockIdx.x, tid = threadIdx.x;
  const double qnan = __longlong_as_double(0x7ff8000000000000ll);
  const double *row = scores + (int64_t)r * ld;
  uint64_t *park = ws + (int64_t)r * C;                                     // [P] of the row's C words
  if (tid < kRmMaxCuts) grp[tid][0] = -1;
  int32_t b, P;
  // first sort: the positives' keys
  const bool has_list = row_positives(pos_ptr, r, C, tid, n_pos, n_neg, b, P);
  if (!has_list || !mark_and_fill<kRmThreads, true>(C, cpad, row, pos_col + b, P, tid, key, is_pos, &n_pos[r], &n_neg[r])) {
    if (tid == 0) {                 // refused, or one class
      auc[r] = qnan;
      ap[r] = qnan;
    }
    if (has_list && tid < cuts.nk) hits[(int64_t)r * cuts.nk + tid] = qnan;
    return;                         // uniform: both answers are the workgroup's
  }
  const int32_t N = C - P;
  sort_keys<kRmThreads>(key, cpad, tid);
  for (int32_t i = tid; i < P; i += kRmThreads) park[i] = key[i];
  __syncthreads();                  // the keys are read out of LDS before the second fill overwrites them
  // second sort: the negatives' keys, which stay in LDS
  for (int32_t c = tid; c < cpad; c += kRmThreads) {
    uint64_t k = kBehind;
    if (c < C && !((is_pos[c >> 5] >> (c & 31)) & 1u)) k = order_key(row[c]);
    key[c] = k;
  }
  __syncthreads();
  sort_keys<kRmThreads>(key, cpad, tid);        // its barriers also make the parked keys visible to the whole workgroup

  unsigned long long twice_u = 0;
  double ap_sum = 0.0;
  int32_t above[kRmMaxCuts];
#pragma unroll
  for (int j = 0; j < kRmMaxCuts; ++j) above[j] = 0;
  for (int32_t i = P - 1 - tid; i >= 0; i -= kRmThreads) {   // descending threshold
    const uint64_t kp = park[i];
    const int32_t negL = search(key, 0, N, kp, false), negU = search(key, negL, N, kp, true);
    // most positives are alone at their score: look at the neighbours before searching
    const int32_t posL = (i == 0 || park[i - 1] < kp) ? i : search(park, 0, i - 1, kp, false);
    const int32_t posU = (i == P - 1 || park[i + 1] > kp) ? i + 1 : search(park, i + 2, P, kp, true);
    twice_u += (unsigned long long)negL + (unsigned long long)negU;
    const bool first = i == posL;
    if (first) {
      const long long tp = P - posL, fp = N - negL;
      ap_sum += (double)((long long)(posU - posL) * tp) / (double)(tp + fp);   // exact operands (< 2^53), one rounding
    }
    const int32_t lt = posL + negL, le = posU + negU;
#pragma unroll
    for (int j = 0; j < kRmMaxCuts; ++j) {
      if (j < cuts.nk) {
        const int32_t m = cuts.m[j];
        if (lt > m) above[j] += 1;
        else if (le > m && first) {       // one group holds the item and it has one first positive: one writer
          grp[j][1] = posU;
          grp[j][2] = negL;
          grp[j][3] = negU;
          grp[j][0] = posL;
        }
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    twice_u += __shfl_xor(twice_u, o, kWave);
    ap_sum += __shfl_xor(ap_sum, o, kWave);
#pragma unroll
    for (int j = 0; j < kRmMaxCuts; ++j) above[j] += __shfl_xor(above[j], o, kWave);
  }
  if ((tid & (kWave - 1)) == 0) {
    part_u[tid / kWave] = twice_u;
    part_ap[tid / kWave] = ap_sum;
#pragma unroll
    for (int j = 0; j < kRmMaxCuts; ++j) part_above[tid / kWave][j] = above[j];
  }
  __syncthreads();
  if (tid == 0) {
    unsigned long long s = 0;
    double a = 0.0;
    for (int w = 0; w < kRmWaves; ++w) {
      s += part_u[w];
      a += part_ap[w];
    }
    auc[r] = (double)s / (2.0 * (double)P * (double)N);   // s < 2^53 and 2 P N < 2^53: exact operands, one rounding
    ap[r] = a / (double)P;
    n_pos[r] = P;
    n_neg[r] = N;
  }
  if (tid < cuts.nk) {
    const int32_t m = cuts.m[tid];
    double h;
    if (grp[tid][0] >= 0) {
      const int32_t posL = grp[tid][0], posU = grp[tid][1], negL = grp[tid][2], negU = grp[tid][3];
      const long long g = (long long)(posU - posL) + (negU - negL), pos_g = posU - posL;
      const long long slots = (long long)(posU + negU) - m;   // k' - (C - le): 1 .. g
      const double A = (double)(P - posU);
      h = slots == g ? A + (double)pos_g : A + (double)(pos_g * slots) / (double)g;
    } else {
      int32_t n = 0;
      for (int w = 0; w < kRmWaves; ++w) n += part_above[w][tid];
      h = (double)n;                                          // the item's group holds no positive
    }
    hits[(int64_t)r * cuts.nk + tid] = h;
  }
}

}  // namespace
}  // namespace gss

using namespace gss;

extern "C" {

size_t gss_rank_metrics_workspace_bytes(int32_t R, int32_t C) {
  if (R <= 0 || C <= 0) return 0;
  return (size_t)R * (size_t)C * sizeof(uint64_t);
}

int gss_rank_metrics_rows(int32_t R, int32_t C, const double *scores, int64_t ld, const int32_t *pos_ptr, const int32_t *pos_col, int32_t nk,
                          const int32_t *ks, double *auc, double *ap, double *hits, int32_t *n_pos, int32_t *n_neg, void *workspace,
                          size_t workspace_bytes, void *stream) {
  GSS_REQUIRE(R >= 0, "rank_metrics_rows: R=%d rows must be >= 0", R);
  GSS_REQUIRE(C >= 1, "rank_metrics_rows: C=%d candidates must be >= 1", C);
  GSS_REQUIRE(C <= kRmMaxCols, "rank_metrics_rows: C=%d candidates is above the limit of %d per row (one workgroup sorts a row in LDS)", C,
              kRmMaxCols);
  GSS_REQUIRE(ld >= C, "rank_metrics_rows: ld=%lld is below C=%d", (long long)ld, C);
  GSS_REQUIRE(nk >= 0 && nk <= kRmMaxCuts, "rank_metrics_rows: nk=%d cut-offs is outside 0..%d", nk, kRmMaxCuts);
  GSS_REQUIRE(nk == 0 || ks, "rank_metrics_rows: null argument");
  Cuts cuts;
  cuts.nk = nk;
  for (int j = 0; j < kRmMaxCuts; ++j) cuts.m[j] = 0;
  for (int j = 0; j < nk; ++j) {
    GSS_REQUIRE(ks[j] >= 1, "rank_metrics_rows: cut-off %d is k=%d; a cut-off must be >= 1", j, ks[j]);
    cuts.m[j] = C - (ks[j] < C ? ks[j] : C);
  }
  if (R == 0) return GSS_OK;
  GSS_REQUIRE(scores && pos_ptr && pos_col && auc && ap && n_pos && n_neg && (nk == 0 || hits) && workspace,
              "rank_metrics_rows: null argument");
  GSS_REQUIRE(workspace_bytes >= gss_rank_metrics_workspace_bytes(R, C),
              "rank_metrics_rows: the workspace has %zu bytes, gss_rank_metrics_workspace_bytes(%d, %d) = %zu", workspace_bytes, R, C,
              gss_rank_metrics_workspace_bytes(R, C));
  GSS_REQUIRE(((uintptr_t)workspace & 7) == 0, "rank_metrics_rows: the workspace must be 8-byte aligned");
  hipStream_t st = as_stream(stream);
  const int32_t cpad = pow2_at_least(C);
  const size_t lds = (size_t)cpad * 8 + (size_t)cpad / 8;
  hipLaunchKernelGGL(rank_metrics_kernel, dim3(R), dim3(kRmThreads), lds_request(rank_metrics_kernel, lds), st, C, cpad, scores, ld, pos_ptr,
                     pos_col, cuts, auc, ap, hits, n_pos, n_neg, reinterpret_cast<uint64_t *>(workspace));
  GSS_LAUNCH_CHECK("rank_metrics_kernel");
  return read_refusals("rank_metrics_rows", R, C, n_pos, n_neg, st);
}

}  // extern "C"

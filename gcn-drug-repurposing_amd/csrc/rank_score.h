// rank_score.h -- the one scoring body behind gss_rank_metrics_rows (rank_metrics.hip) and gss_rank_metrics_strata (rank_strata.hip), and
// what the three row-ranking entry points (those two and gss_auc_rows, auc.hip) share on the host: the limits, the cut-offs, the argument
// checks and the refusals' way back.  rank_keys.h below it has the key, the sort, the search and the check of a row's positives.
//
// The contract of gss_rank_metrics_strata is that a stratum has, bit for bit, the words gss_rank_metrics_rows writes for the stratum
// gathered into a row of its own.  It holds because both kernels hand their sorted positives and sorted negatives to score_positives:
// tie handling, the order of the AP additions and the hits formula exist here and nowhere else (DESIGN.md sections 9.8 and 9.15).
// Inline device and host code only.
#pragma once
#include "rank_keys.h"

namespace gss {

constexpr int kRankThreads = 256;               // one workgroup per row; the order of the AP additions is stated for four waves of 64
constexpr int kRankMaxCols = 16384;             // the sort buffer: pow2ceil(C) keys of 8 bytes in LDS (128 KiB at the limit)
constexpr int kRankMaxCuts = 8;

struct RankCuts {
  int32_t nk;
  int32_t k[kRankMaxCuts];   // as given (>= 1); the ascending index of the item of rank min(k, Cs) is taken in score_positives
};

// the negatives' keys of a row whose positives are marked in is_pos: key [cpad] gets them, and kBehind for the positives and the
// padding.  Ends behind a barrier: EVERY thread of the workgroup (of THREADS) must reach the call
template <int THREADS>
__device__ __forceinline__ void fill_negatives(int32_t C, int32_t cpad, const double *__restrict__ row, const uint32_t *is_pos, uint64_t *key,
                                               int32_t tid) {
  for (int32_t c = tid; c < cpad; c += THREADS) {
    uint64_t k = kBehind;
    if (c < C && !((is_pos[c >> 5] >> (c & 31)) & 1u)) k = order_key(row[c]);
    key[c] = k;
  }
  __syncthreads();
}

// AUC, average precision and hits@k of the P positives park[0 .. P) (sorted keys, in global memory) against the N negatives key[0 .. N)
// (sorted keys, in LDS), P >= 1 and N >= 1: *auc_w, *ap_w and hits_w[0 .. cuts.nk) are written, each by one thread, and nothing else.
// Sorted positive i (key k) takes four counts by binary search, negL / negU in key and posL / posU in park (the number of keys below k,
// and of keys not above k, among the negatives and among the positives), and everything follows from those integers:
//   AUC   2 U = sum over positives of (negL + negU), one division: the integers and the expression of auc.hip, so the same bits;
//   AP    the first positive of a tie group (i == posL) adds pos_g TP_g / (TP_g + FP_g) with pos_g = posU - posL, TP_g = P - posL,
//         FP_g = N - negL: an exact integer product and one division per group.  Thread t adds the groups of sorted positives
//         P-1-t, P-1-t-THREADS, ... (descending threshold) serially, then a butterfly over the wave and the waves in order: the order
//         comes from the sorted keys alone;
//   hits  the item of rank k' = min(k, Cs), Cs = P + N, has ascending index m = Cs - k' in the merged order.  With lt = posL + negL and
//         le = posU + negU a positive's tie group holds that item iff lt <= m < le, and lies strictly above it iff lt > m.  The first
//         positive of the one group that holds it writes that group's counts; every positive counts itself into `above` where lt > m
//         (integer sums).  If no positive's group holds the item its group has no positive and hits = above.
// It is made of two barriers: EVERY thread of the workgroup (of THREADS) must reach the call, with the same arguments.  The first also
// orders the previous call's reads of the partial sums before this call's writes, so it may be called in a loop
template <int THREADS>
__device__ __forceinline__ void score_positives(const uint64_t *park, int32_t P, const uint64_t *key, int32_t N, const RankCuts &cuts, int32_t tid,
                                                double *__restrict__ auc_w, double *__restrict__ ap_w, double *__restrict__ hits_w) {
  constexpr int kWaves = THREADS / kWave;
  __shared__ unsigned long long part_u[kWaves];
  __shared__ double part_ap[kWaves];
  __shared__ int32_t part_above[kWaves][kRankMaxCuts];
  __shared__ int32_t grp[kRankMaxCuts][4];   // the tie group that holds cut j's item, if it has a positive: posL, posU, negL, negU
  if (tid < kRankMaxCuts) grp[tid][0] = -1;
  __syncthreads();
  const int32_t Cs = P + N;
  unsigned long long twice_u = 0;
  double ap_sum = 0.0;
  int32_t above[kRankMaxCuts], cut[kRankMaxCuts];
#pragma unroll
  for (int j = 0; j < kRankMaxCuts; ++j) {
    above[j] = 0;
    cut[j] = j < cuts.nk ? Cs - (cuts.k[j] < Cs ? cuts.k[j] : Cs) : 0;   // ascending index of the item of rank min(k, Cs)
  }
  for (int32_t i = P - 1 - tid; i >= 0; i -= THREADS) {   // descending threshold
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
    for (int j = 0; j < kRankMaxCuts; ++j) {
      if (j < cuts.nk) {
        const int32_t m = cut[j];
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
    for (int j = 0; j < kRankMaxCuts; ++j) above[j] += __shfl_xor(above[j], o, kWave);
  }
  if ((tid & (kWave - 1)) == 0) {
    part_u[tid / kWave] = twice_u;
    part_ap[tid / kWave] = ap_sum;
#pragma unroll
    for (int j = 0; j < kRankMaxCuts; ++j) part_above[tid / kWave][j] = above[j];
  }
  __syncthreads();
  if (tid == 0) {
    unsigned long long u = 0;
    double a = 0.0;
    for (int w = 0; w < kWaves; ++w) {
      u += part_u[w];
      a += part_ap[w];
    }
    *auc_w = (double)u / (2.0 * (double)P * (double)N);   // u < 2^53 and 2 P N < 2^53: exact operands, one rounding
    *ap_w = a / (double)P;
  }
  if (tid < cuts.nk) {
    const int32_t m = cut[tid];
    double h;
    if (grp[tid][0] >= 0) {
      const int32_t posL = grp[tid][0], posU = grp[tid][1], negL = grp[tid][2], negU = grp[tid][3];
      const long long g = (long long)(posU - posL) + (negU - negL), pos_g = posU - posL;
      const long long slots = (long long)(posU + negU) - m;   // k' - (Cs - le): 1 .. g
      const double A = (double)(P - posU);
      h = slots == g ? A + (double)pos_g : A + (double)(pos_g * slots) / (double)g;
    } else {
      int32_t n = 0;
      for (int w = 0; w < kWaves; ++w) n += part_above[w][tid];
      h = (double)n;                                          // the item's group holds no positive
    }
    hits_w[tid] = h;
  }
}

// ---- the host side of the three entry points --------------------------------------------------------------------------------------------
// what gss_auc_rows (nk = 0, no cuts), gss_rank_metrics_rows and gss_rank_metrics_strata require of R, C, ld and the nk host cut-offs ks,
// refused in the words of entry point `who`; cuts is filled
inline int check_rank_args(const char *who, int32_t R, int32_t C, int64_t ld, int32_t nk, const int32_t *ks, RankCuts &cuts) {
  GSS_REQUIRE(R >= 0, "%s: R=%d rows must be >= 0", who, R);
  GSS_REQUIRE(C >= 1, "%s: C=%d candidates must be >= 1", who, C);
  GSS_REQUIRE(C <= kRankMaxCols, "%s: C=%d candidates is above the limit of %d per row (one workgroup sorts a row in LDS)", who, C, kRankMaxCols);
  GSS_REQUIRE(ld >= C, "%s: ld=%lld is below C=%d", who, (long long)ld, C);
  GSS_REQUIRE(nk >= 0 && nk <= kRankMaxCuts, "%s: nk=%d cut-offs is outside 0..%d", who, nk, kRankMaxCuts);
  GSS_REQUIRE(nk == 0 || ks, "%s: null argument", who);
  cuts.nk = nk;
  for (int j = 0; j < kRankMaxCuts; ++j) cuts.k[j] = 1;
  for (int j = 0; j < nk; ++j) {
    GSS_REQUIRE(ks[j] >= 1, "%s: cut-off %d is k=%d; a cut-off must be >= 1", who, j, ks[j]);
    cuts.k[j] = ks[j];
  }
  return GSS_OK;
}

// a row's status words (-code of rank_keys.h's RowRefusal in n_pos[r], the offending column or length in n_neg[r]) -> the refusal in the
// words of entry point `who`, GSS_OK for any other code
inline int row_refusal(const char *who, int32_t r, int32_t C, int32_t code, int32_t col) {
  GSS_REQUIRE(code != kBadPtr, "%s: row %d: pos_ptr is not a CSR row pointer (0 first, non-decreasing, at most C=%d per row; %d here)", who, r, C, col);
  GSS_REQUIRE(code != kColRange, "%s: row %d: pos_col %d is outside [0, %d)", who, r, col, C);
  GSS_REQUIRE(code != kColRepeat, "%s: row %d: pos_col %d is repeated", who, r, col);
  GSS_REQUIRE(code != kNonFinite, "%s: row %d, column %d: the score is NaN or infinite (roc_auc_score refuses it)", who, r, col);
  return GSS_OK;
}

// The refusals come back in the count words: -code in n_pos, the column in n_neg.  Reads both arrays of R words back on the stream,
// waits for it, and names the first refused row in the words of entry point `who` ("auc_rows", "rank_metrics_rows")
inline int read_refusals(const char *who, int32_t R, int32_t C, const int32_t *n_pos, const int32_t *n_neg, hipStream_t st) {
  std::unique_ptr<int32_t[]> h(new (std::nothrow) int32_t[(size_t)2 * R]);
  if (!h) return fail(GSS_ENOMEM, "%s: host status buffer of %d rows", who, R);
  GSS_HIP(hipMemcpyAsync(h.get(), n_pos, (size_t)R * 4, hipMemcpyDeviceToHost, st));   // no wait of its own: the stream orders it before n_neg's
  if (int rc = read_back(h.get() + R, n_neg, (size_t)R * 4, st)) return rc;
  for (int32_t r = 0; r < R; ++r)
    if (int rc = row_refusal(who, r, C, -h[r], h[R + r])) return rc;
  return GSS_OK;
}

}  // namespace gss

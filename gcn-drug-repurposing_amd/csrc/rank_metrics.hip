// rank_metrics.hip -- batched ROC-AUC, average precision and hits@k, one query per row (the three ranking statistics the
// multiscale-interactome work reports for drug-indication prediction; include/gssgcn.h has the contract, DESIGN.md section 9.8 the
// definitions, the cost model and the measurement).
//
// One workgroup per row, as auc.hip; the key, the sort, the search and the check of the row's positives are rank_keys.h's.  160 KiB of
// LDS hold the 16,384 keys of one sorted array, not two, so the row is sorted twice in the same LDS buffer:
//   1. the positives' keys (negatives and padding get the all-ones key and sort behind them); the P sorted keys are parked in the row's
//      slice of the caller's workspace, ws[r * C .. r * C + P);
//   2. the negatives' keys, as auc.hip does; they stay in LDS.
// The two sorted arrays go to rank_score.h's score_positives, the scoring body this kernel shares with rank_strata.hip: the four counts
// per positive, the three statistics as functions of those integers and the order of the AP additions are stated there.
// Every output word is written by one thread and no result goes through an atomic: bitwise reproducible, and a function of the row's
// multiset of (score, label) pairs alone.
#include "rank_score.h"

namespace gss {
namespace {

__global__ __launch_bounds__(kRankThreads) void rank_metrics_kernel(int32_t C, int32_t cpad, const double *__restrict__ scores, int64_t ld,
                                                                    const int32_t *__restrict__ pos_ptr, const int32_t *__restrict__ pos_col,
                                                                    RankCuts cuts, double *__restrict__ auc, double *__restrict__ ap,
                                                                    double *__restrict__ hits, int32_t *__restrict__ n_pos,
                                                                    int32_t *__restrict__ n_neg, uint64_t *ws) {
  extern __shared__ __align__(16) unsigned char lds[];
  uint64_t *key = reinterpret_cast<uint64_t *>(lds);                        // [cpad]
  uint32_t *is_pos = reinterpret_cast<uint32_t *>(lds + (size_t)cpad * 8);  // [cpad / 32] bitmap
  const int32_t r = blockIdx.x, tid = threadIdx.x;
  const double qnan = __longlong_as_double(0x7ff8000000000000ll);
  const double *row = scores + (int64_t)r * ld;
  uint64_t *park = ws + (int64_t)r * C;                                     // [P] of the row's C words
  int32_t b, P;
  // first sort: the positives' keys
  const bool has_list = row_positives(pos_ptr, r, C, tid, n_pos, n_neg, b, P);
  if (!has_list || !mark_and_fill<kRankThreads, true>(C, cpad, row, pos_col + b, P, tid, key, is_pos, &n_pos[r], &n_neg[r])) {
    if (tid == 0) {                 // refused, or one class
      auc[r] = qnan;
      ap[r] = qnan;
    }
    if (has_list && tid < cuts.nk) hits[(int64_t)r * cuts.nk + tid] = qnan;
    return;                         // uniform: both answers are the workgroup's
  }
  const int32_t N = C - P;
  sort_keys<kRankThreads>(key, cpad, tid);
  for (int32_t i = tid; i < P; i += kRankThreads) park[i] = key[i];
  __syncthreads();                  // the keys are read out of LDS before the second fill overwrites them
  // second sort: the negatives' keys, which stay in LDS
  fill_negatives<kRankThreads>(C, cpad, row, is_pos, key, tid);
  sort_keys<kRankThreads>(key, cpad, tid);      // its barriers also make the parked keys visible to the whole workgroup
  score_positives<kRankThreads>(park, P, key, N, cuts, tid, &auc[r], &ap[r], hits + (int64_t)r * cuts.nk);
  if (tid == 0) {
    n_pos[r] = P;
    n_neg[r] = N;
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
  RankCuts cuts;
  if (int rc = check_rank_args("rank_metrics_rows", R, C, ld, nk, ks, cuts)) return rc;
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
  hipLaunchKernelGGL(rank_metrics_kernel, dim3(R), dim3(kRankThreads), lds_request(rank_metrics_kernel, lds), st, C, cpad, scores, ld, pos_ptr,
                     pos_col, cuts, auc, ap, hits, n_pos, n_neg, reinterpret_cast<uint64_t *>(workspace));
  GSS_LAUNCH_CHECK("rank_metrics_kernel");
  return read_refusals("rank_metrics_rows", R, C, n_pos, n_neg, st);
}

}  // extern "C"

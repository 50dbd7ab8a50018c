// auc.hip -- batched ROC-AUC, one query per row (evaluate_auc.py:156-170: sklearn.metrics.roc_auc_score per indication over all drugs).
//
// One workgroup per row (include/gssgcn.h has the contract; DESIGN.md section 9.4 the cost model and the measured stage times of evaluate_auc.py).  The
// key, the sort, the search and the check of the row's positives are rank_keys.h's, shared with rank_metrics.hip and profile_rank.hip: the
// positives are marked in an LDS bitmap, every score becomes an order-preserving uint64 key, the negatives' keys are sorted in LDS (the
// positives get the all-ones key and sort behind them), and each positive counts the negatives below it and tied with it by two binary searches:
//   2 U = sum over positives of (lower_bound + upper_bound) = sum of (2 * below + tied),   AUC = 2 U / (2 P N)
// which is the average-rank (Mann-Whitney) form of roc_auc_score.  The counts are integers, so the result depends only on the multiset
// of (score, label) pairs; every output word is written by the one thread that owns it (no atomics on results: bitwise deterministic).
// The limits, the argument checks and the refusals' way back are rank_score.h's, shared with rank_metrics.hip and rank_strata.hip.  Their
// scoring body is not used here: this kernel sorts once and has no workspace to park its positives in, so it keeps its own loop.
#include "rank_score.h"

namespace gss {
namespace {

__global__ __launch_bounds__(kRankThreads) void auc_rows_kernel(int32_t C, int32_t cpad, const double *__restrict__ scores, int64_t ld,
                                                                const int32_t *__restrict__ pos_ptr, const int32_t *__restrict__ pos_col,
                                                                double *__restrict__ auc, int32_t *__restrict__ n_pos,
                                                                int32_t *__restrict__ n_neg) {
  extern __shared__ __align__(16) unsigned char lds[];
  uint64_t *key = reinterpret_cast<uint64_t *>(lds);                     // [cpad]
  uint32_t *is_pos = reinterpret_cast<uint32_t *>(lds + (size_t)cpad * 8);  // [cpad / 32] bitmap
  __shared__ unsigned long long partial[kRankThreads / kWave];
  const int32_t r = blockIdx.x, tid = threadIdx.x;
  const double *row = scores + (int64_t)r * ld;
  int32_t b, P;
  // the negatives' keys: the positives get the all-ones key and sort behind them
  if (!row_positives(pos_ptr, r, C, tid, n_pos, n_neg, b, P) ||
      !mark_and_fill<kRankThreads, false>(C, cpad, row, pos_col + b, P, tid, key, is_pos, &n_pos[r], &n_neg[r])) {
    if (tid == 0) auc[r] = __longlong_as_double(0x7ff8000000000000ll);   // refused, or one class
    return;                                                               // uniform: both answers are the workgroup's
  }
  const int32_t N = C - P;
  sort_keys<kRankThreads>(key, cpad, tid);   // ascending: the N negatives' keys come first
  unsigned long long twice_u = 0;
  for (int32_t k = tid; k < P; k += kRankThreads) {
    const uint64_t kp = order_key(row[pos_col[b + k]]);
    twice_u += (unsigned long long)search(key, 0, N, kp, false) + (unsigned long long)search(key, 0, N, kp, true);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) twice_u += __shfl_xor(twice_u, o, kWave);
  if ((tid & (kWave - 1)) == 0) partial[tid / kWave] = twice_u;
  __syncthreads();
  if (tid == 0) {
    unsigned long long s = 0;
    for (int w = 0; w < kRankThreads / kWave; ++w) s += partial[w];
    auc[r] = (double)s / (2.0 * (double)P * (double)N);   // s < 2^53 and 2 P N < 2^53: exact operands, one rounding
    n_pos[r] = P;
    n_neg[r] = N;
  }
}

}  // namespace
}  // namespace gss

using namespace gss;

extern "C" {

int gss_auc_rows(int32_t R, int32_t C, const double *scores, int64_t ld, const int32_t *pos_ptr, const int32_t *pos_col, double *auc,
                 int32_t *n_pos, int32_t *n_neg, void *stream) {
  RankCuts none;
  if (int rc = check_rank_args("auc_rows", R, C, ld, 0, nullptr, none)) return rc;
  if (R == 0) return GSS_OK;
  GSS_REQUIRE(scores && pos_ptr && pos_col && auc && n_pos && n_neg, "auc_rows: null argument");
  hipStream_t st = as_stream(stream);
  const int32_t cpad = pow2_at_least(C);
  const size_t lds = (size_t)cpad * 8 + (size_t)cpad / 8;
  hipLaunchKernelGGL(auc_rows_kernel, dim3(R), dim3(kRankThreads), lds_request(auc_rows_kernel, lds), st, C, cpad, scores, ld, pos_ptr,
                     pos_col, auc, n_pos, n_neg);
  GSS_LAUNCH_CHECK("auc_rows_kernel");
  return read_refusals("auc_rows", R, C, n_pos, n_neg, st);
}

}  // extern "C"

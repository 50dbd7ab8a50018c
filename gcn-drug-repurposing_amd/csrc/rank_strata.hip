// rank_strata.hip -- ROC-AUC, average precision and hits@k per stratum of a query row: a stratum is a subset Q of the row's positives (the
// drugs of one ATC class among the drugs listed for an indication), ranked against ALL of the row's negatives; the row's other positives
// are neither positive nor negative (include/gssgcn.h has the contract, DESIGN.md section 9.15 the definition, the cost model and the
// measurement).  A stratum is the sub-problem of C_s = N + |Q| columns, and every output word is the word gss_rank_metrics_rows
// (rank_metrics.hip) writes for that sub-problem gathered into a row of its own.
//
// One workgroup per row, as rank_metrics.hip, and rank_keys.h's key, sort, search and check of the row's positives:
//   1. mark_and_fill marks the row's positives in one LDS bitmap and refuses what the row kernels refuse;
//   2. each of the row's strata in turn: its list is checked against that bitmap and, through a second bitmap, for a repeated column;
//      its |Q| keys are sorted in the LDS key buffer at pow2_at_least(|Q|) and parked at ws[sub_ptr[s] ..);
//   3. the row's negatives are sorted ONCE and stay in LDS;
//   4. each stratum in turn hands its parked keys and the negatives to rank_score.h's score_positives, the scoring body
//      rank_metrics_kernel calls for its row, with P = |Q|.  A positive's counts among the negatives do not depend on which other
//      positives are in play, so the integers, and with them the bits, are those of the gathered sub-problem.
// Trip counts of every loop that holds a barrier depend on str_ptr, sub_ptr and refusals found behind a barrier alone: the whole workgroup
// reaches each barrier.  Every output word has one writer and no result goes through an atomic.
#include "rank_score.h"

namespace gss {
namespace {

// what a row can be refused for beside rank_keys.h's RowRefusal (-code in n_pos[r], the offending word in n_neg[r]) ...
enum StrataRowRefusal { kBadStrPtr = 5, kWorkspaceShort = 6 };
// ... and a stratum (-code in s_pos[s], the offending word in s_neg[s])
enum StratumRefusal { kBadSubPtr = 1, kSubNotPositive = 2, kSubRepeat = 3 };

__global__ __launch_bounds__(kRankThreads) void rank_strata_kernel(int32_t R, int32_t C, int32_t cpad, const double *__restrict__ scores, int64_t ld,
                                                                   const int32_t *__restrict__ pos_ptr, const int32_t *__restrict__ pos_col,
                                                                   int32_t S, const int32_t *__restrict__ str_ptr,
                                                                   const int32_t *__restrict__ sub_ptr, const int32_t *__restrict__ sub_col,
                                                                   RankCuts cuts, double *__restrict__ auc, double *__restrict__ ap,
                                                                   double *__restrict__ hits, int32_t *s_pos, int32_t *s_neg,
                                                                   int32_t *__restrict__ n_pos, int32_t *__restrict__ n_neg, uint64_t *ws,
                                                                   int64_t ws_words) {
  extern __shared__ __align__(16) unsigned char lds[];
  uint64_t *key = reinterpret_cast<uint64_t *>(lds);                                        // [cpad]
  uint32_t *is_pos = reinterpret_cast<uint32_t *>(lds + (size_t)cpad * 8);                  // [cpad / 32] the row's positives
  uint32_t *in_sub = reinterpret_cast<uint32_t *>(lds + (size_t)cpad * 8 + (size_t)cpad / 8);   // [cpad / 32] the stratum in hand
  __shared__ int32_t bad_member, bad_again;
  const int32_t r = blockIdx.x, tid = threadIdx.x;
  const double qnan = __longlong_as_double(0x7ff8000000000000ll);
  const double *row = scores + (int64_t)r * ld;

  // the row's strata [s0, s1): uniform, every thread reads the same words
  const int32_t s0 = str_ptr[r], s1 = str_ptr[r + 1];
  if (s0 < 0 || s1 < s0 || s1 > S || (r == 0 && s0 != 0) || (r == R - 1 && s1 != S)) {
    if (tid == 0) {
      n_pos[r] = -kBadStrPtr;
      n_neg[r] = s1;
    }
    return;
  }
  const int32_t n_sub = sub_ptr[S];
  if ((int64_t)n_sub > ws_words) {
    if (tid == 0) {
      n_pos[r] = -kWorkspaceShort;
      n_neg[r] = n_sub;
    }
    return;
  }
  int32_t b, P;
  if (!row_positives(pos_ptr, r, C, tid, n_pos, n_neg, b, P)) return;
  // with its counts or its refusal written where the row does not go on.  A row of one class still has its strata's lists checked
  const bool ranked = mark_and_fill<kRankThreads, true>(C, cpad, row, pos_col + b, P, tid, key, is_pos, &n_pos[r], &n_neg[r]);
  const int32_t N = C - P;

  // every stratum: its list checked, its keys sorted and parked
  for (int32_t s = s0; s < s1; ++s) {
    const int32_t q0 = sub_ptr[s], q1 = sub_ptr[s + 1], Q = q1 - q0;
    if (q0 < 0 || Q < 0 || q1 > n_sub || Q > P || (s == 0 && q0 != 0)) {   // uniform
      if (tid == 0) {
        s_pos[s] = -kBadSubPtr;
        s_neg[s] = Q;
      }
      continue;
    }
    if (tid == 0) {
      bad_member = INT32_MAX;
      bad_again = INT32_MAX;
    }
    for (int32_t w = tid; w < cpad / 32; w += kRankThreads) in_sub[w] = 0u;
    __syncthreads();
    for (int32_t k = tid; k < Q; k += kRankThreads) {
      const int32_t c = sub_col[q0 + k];
      if (c < 0 || c >= C || !((is_pos[c >> 5] >> (c & 31)) & 1u)) {
        atomicMin(&bad_member, k);      // the first offending entry in list order
        continue;
      }
      const uint32_t bit = 1u << (c & 31);
      if (atomicOr(&in_sub[c >> 5], bit) & bit) atomicMin(&bad_again, c);
    }
    __syncthreads();
    const int32_t member = bad_member, again = bad_again;
    const bool sorted = ranked && Q != 0 && member == INT32_MAX && again == INT32_MAX;   // uniform
    if (sorted) {
      const int32_t qpad = pow2_at_least(Q);                                             // <= cpad: Q <= P <= C
      for (int32_t k = tid; k < qpad; k += kRankThreads) key[k] = k < Q ? order_key(row[sub_col[q0 + k]]) : kBehind;
    }
    if (tid == 0) {
      if (member != INT32_MAX) {
        s_pos[s] = -kSubNotPositive;
        s_neg[s] = sub_col[q0 + member];
      } else if (again != INT32_MAX) {
        s_pos[s] = -kSubRepeat;
        s_neg[s] = again;
      } else {
        s_pos[s] = Q;
        s_neg[s] = N;
        if (!sorted) {                  // no positive in the stratum, or a row of one class (or a refused one)
          auc[s] = qnan;
          ap[s] = qnan;
        }
      }
    }
    if (!sorted && member == INT32_MAX && again == INT32_MAX && tid < cuts.nk) hits[(int64_t)s * cuts.nk + tid] = qnan;
    __syncthreads();                    // the two words are read before the next stratum resets them; the keys are filled
    if (sorted) {
      const int32_t qpad = pow2_at_least(Q);
      sort_keys<kRankThreads>(key, qpad, tid);
      for (int32_t i = tid; i < Q; i += kRankThreads) ws[q0 + i] = key[i];
      __syncthreads();                  // read out of LDS before the next fill overwrites them
    }
  }
  if (!ranked || s0 == s1) {
    if (ranked && tid == 0) {
      n_pos[r] = P;
      n_neg[r] = N;
    }
    return;                             // uniform
  }

  // the negatives' keys, sorted once; they stay in LDS
  fill_negatives<kRankThreads>(C, cpad, row, is_pos, key, tid);
  sort_keys<kRankThreads>(key, cpad, tid);          // its barriers also make the parked keys and the s_pos words visible to the whole workgroup

  // The cut-offs are read out of the kernel's argument here, word by word.  Handing `cuts` itself to score_positives takes its address,
  // and the compiler then copies all nine words into SGPRs at the kernel's entry, where they stay live through every loop above: 102
  // SGPRs and 7 waves per SIMD instead of 96 and 8
  RankCuts late;
  late.nk = cuts.nk;
#pragma unroll
  for (int j = 0; j < kRankMaxCuts; ++j) late.k[j] = cuts.k[j];
  for (int32_t s = s0; s < s1; ++s) {
    const int32_t Q = s_pos[s];                   // |Q_s|, or a refusal: written above by this workgroup, uniform
    if (Q <= 0) continue;
    score_positives<kRankThreads>(ws + sub_ptr[s], Q, key, N, late, tid, &auc[s], &ap[s], hits + (int64_t)s * late.nk);
  }
  if (tid == 0) {
    n_pos[r] = P;
    n_neg[r] = N;
  }
}

// the refusals' way back: the rows' words as read_refusals reads them and the strata's, in one wait for the stream.  The row of a refused
// stratum is looked up in str_ptr, which is read back only then
int read_strata_refusals(int32_t R, int32_t C, int32_t S, const int32_t *str_ptr, const int32_t *n_pos, const int32_t *n_neg, const int32_t *s_pos,
                         const int32_t *s_neg, size_t workspace_bytes, hipStream_t st) {
  const char *who = "rank_metrics_strata";
  const size_t words = (size_t)2 * R + (size_t)2 * S;
  std::unique_ptr<int32_t[]> h(new (std::nothrow) int32_t[words]);
  if (!h) return fail(GSS_ENOMEM, "%s: host status buffer of %d rows and %d strata", who, R, S);
  int32_t *h_pos = h.get(), *h_neg = h_pos + R, *hs_pos = h_neg + R, *hs_neg = hs_pos + S;
  GSS_HIP(hipMemcpyAsync(h_pos, n_pos, (size_t)R * 4, hipMemcpyDeviceToHost, st));
  GSS_HIP(hipMemcpyAsync(h_neg, n_neg, (size_t)R * 4, hipMemcpyDeviceToHost, st));
  GSS_HIP(hipMemcpyAsync(hs_pos, s_pos, (size_t)S * 4, hipMemcpyDeviceToHost, st));
  if (int rc = read_back(hs_neg, s_neg, (size_t)S * 4, st)) return rc;
  for (int32_t r = 0; r < R; ++r) {
    const int32_t code = -h_pos[r], col = h_neg[r];
    GSS_REQUIRE(code != kWorkspaceShort, "%s: the workspace has %zu bytes, gss_rank_strata_workspace_bytes(%d) = %zu", who, workspace_bytes, col,
                (size_t)col * 8);
    GSS_REQUIRE(code != kBadStrPtr, "%s: row %d: str_ptr is not a row pointer over [0, %d] (0 first, non-decreasing, %d last; %d here)", who, r, S, S,
                col);
    if (int rc = row_refusal(who, r, C, code, col)) return rc;
  }
  for (int32_t s = 0; s < S; ++s) {
    if (hs_pos[s] >= 0) continue;
    std::unique_ptr<int32_t[]> ptr;
    if (int rc = host_copy(ptr, str_ptr, (size_t)R + 1, st, "%s: host copy of str_ptr, %d rows", who, R)) return rc;
    int32_t r = 0;
    while (r + 1 < R && ptr[r + 1] <= s) ++r;
    const int32_t code = -hs_pos[s], col = hs_neg[s];
    GSS_REQUIRE(code != kBadSubPtr,
                "%s: row %d, stratum %d: sub_ptr is not a row pointer over the strata (0 first, non-decreasing, at most the row's positives "
                "per stratum; %d here)", who, r, s, col);
    GSS_REQUIRE(code != kSubNotPositive, "%s: row %d, stratum %d: sub_col %d is not a positive of the row", who, r, s, col);
    GSS_REQUIRE(code != kSubRepeat, "%s: row %d, stratum %d: sub_col %d is repeated", who, r, s, col);
    return fail(GSS_EINVAL, "%s: row %d, stratum %d: unknown status %d", who, r, s, hs_pos[s]);
  }
  return GSS_OK;
}

}  // namespace
}  // namespace gss

using namespace gss;

extern "C" {

size_t gss_rank_strata_workspace_bytes(int64_t n_sub) { return n_sub <= 0 ? 0 : (size_t)n_sub * sizeof(uint64_t); }

int gss_rank_metrics_strata(int32_t R, int32_t C, const double *scores, int64_t ld, const int32_t *pos_ptr, const int32_t *pos_col, int32_t S,
                            const int32_t *str_ptr, const int32_t *sub_ptr, const int32_t *sub_col, int32_t nk, const int32_t *ks, double *auc,
                            double *ap, double *hits, int32_t *s_pos, int32_t *s_neg, int32_t *n_pos, int32_t *n_neg, void *workspace,
                            size_t workspace_bytes, void *stream) {
  RankCuts cuts;
  if (int rc = check_rank_args("rank_metrics_strata", R, C, ld, nk, ks, cuts)) return rc;
  GSS_REQUIRE(S >= 0, "rank_metrics_strata: S=%d strata must be >= 0", S);
  if (R == 0 || S == 0) return GSS_OK;
  GSS_REQUIRE(scores && pos_ptr && pos_col && str_ptr && sub_ptr && sub_col && auc && ap && (nk == 0 || hits) && s_pos && s_neg && n_pos && n_neg &&
                  workspace,
              "rank_metrics_strata: null argument");
  GSS_REQUIRE(((uintptr_t)workspace & 7) == 0, "rank_metrics_strata: the workspace must be 8-byte aligned");
  hipStream_t st = as_stream(stream);
  const int32_t cpad = pow2_at_least(C);
  const size_t lds = (size_t)cpad * 8 + 2 * ((size_t)cpad / 8);
  hipLaunchKernelGGL(rank_strata_kernel, dim3(R), dim3(kRankThreads), lds_request(rank_strata_kernel, lds), st, R, C, cpad, scores, ld, pos_ptr, pos_col,
                     S, str_ptr, sub_ptr, sub_col, cuts, auc, ap, hits, s_pos, s_neg, n_pos, n_neg, reinterpret_cast<uint64_t *>(workspace),
                     (int64_t)(workspace_bytes / 8));
  GSS_LAUNCH_CHECK("rank_strata_kernel");
  return read_strata_refusals(R, C, S, str_ptr, n_pos, n_neg, s_pos, s_neg, workspace_bytes, st);
}

}  // extern "C"

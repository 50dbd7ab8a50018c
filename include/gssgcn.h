/*
 * gssgcn.h -- C ABI of libgssgcn.so, the MI355X (gfx950) implementation of the GSS-GCN
 * training hot path of bowang-lab/gcn-drug-repurposing.
 *
 * The reference has no native code: its hot path is a sequence of torch calls.  Each entry
 * point below replaces the torch call(s) named in its comment (file:line relative to the
 * reference root).  A reference maintainer binds these with ctypes.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller unless its name starts with h_
 *   - matrices are dense row-major fp32 [rows][d]; CSR uses int32 rowptr/col and fp32 values
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); calls are
 *     asynchronous on it and never synchronise the device
 *   - return 0 on success, a negative GSS_E* code on failure; gss_last_error() gives the text
 *   - d (feature width == --hidden-units, modules/model.py:142) must be a multiple of 16, <= 1024
 */
#ifndef GSSGCN_H
#define GSSGCN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSS_ABI_VERSION 25  /* 25: the mean and the median of bootstrap resamples and sign flips of series, behind intervals and paired tests of the per-indication metrics -- gss_resample_stats; 24: sums of a distance matrix over the pairs of listed sets and of the prefixes of seeded random permutations, the statistic and the null of ATC class coherence -- gss_pair_sums_lists, gss_pair_sums_random; 23: entry points for tests of the halo bookkeeping and the batch preparation of a sharded plan -- gss_pack_rows, gss_unpack_rows, gss_halo_need_mark, gss_send_slot_bits, gss_bits_clear, gss_bits_set_list, gss_bits_compact, gss_bits_compact_scratch_bytes, gss_batch_prepare, gss_scatter_add_rows_ex, gss_spmm_prep_side; 22: two forward products in one launch and layer 1 one pass ahead -- gss_spmm_fwd_pair, gss_plan_l1_ahead, plan option "l1_ahead"; 21: entry points for tests of the dense half of a plan's step -- gss_dense_fwd_rows, gss_dense_fwd_first, gss_dense_fwd_split_available, gss_dense_fwd_norm, gss_rownorm_fwd_rows, gss_wgrad_slices, gss_wgrad_slices_max, gss_wgrad_partial, gss_wgrad_partial_pair, gss_wgrad_reduce, gss_wgrad_reduce_adam, gss_adam_step4, gss_transpose2; 20: entry points for tests of the loss stages of a plan's step -- gss_loss_step, gss_loss_slab_sweep, gss_loss_workspace_bytes_parts, gss_loss_gather_rows, gss_loss_gather_rows_mapped, gss_loss_gather_batch; loss_step refuses input-gradient weights at widths outside {64, 128, 256}; 19: exact typed top-k selection of listed profile columns and set overlap between selections -- gss_profile_topk, gss_profile_topk_workspace_bytes, gss_topk_overlap; 18: exact average-tie ranks of listed profile columns, the transform behind the spearman distance -- gss_profile_rank, gss_profile_rank_workspace_bytes; 17: gene knock-outs per column of the diffusion profiles -- gss_ppr_set_knockout; distances of listed column pairs of the profile matrix -- gss_profile_dist_pairs, gss_profile_dist_pairs_workspace_bytes; 16: ROC-AUC, average precision and hits@k per row in one launch -- gss_rank_metrics_rows, gss_rank_metrics_workspace_bytes; 15: entry points for tests of the row-sparse SpMM modes -- gss_spmm_bwd1_sparse_ex, gss_spmm_bwd2_sparse_res, gss_spmm_filtered, gss_mark_rows_and_neighbours, gss_batch_bits, gss_bits_fill; 14:indication x drug scores from the embedding tensor -- gss_embedding_scores; 13: pairwise distances between diffusion profiles -- gss_profile_dist; 12: shortest-path counts, best paths and the nodes between pairs -- gss_paths_count, gss_paths_between, gss_paths_between_fill; 11: batched ROC-AUC per row -- gss_auc_rows; 10: shortest-path trees toward up to 64 targets per pass -- gss_paths_*; 9: drug-disease network proximity -- gss_prox_*; 8: the debug entry point that set a wall-clock stamp buffer for the projection kernels is gone; 7: node2vec input embeddings -- gss_walk_prefix, gss_node2vec_walks, gss_sgns_*; 6 (round 6): gss_source_hash; the access-shape knobs whose sweeps said "default holds" twice are gone; 5 (round 5): gss_rowsum_check, gss_plan_sync_stats, gss_comm_local_mode / gss_comm_local_log, gss_csr_giant_rows; 4 (round 4): gss_shard_desc gained a_loc_t, gss_plan_comm_stats, gss_knn_topk_rows.  gss_matrix_cross_sums, the permuted cross-product sum of two matrices behind Mantel's test, joined under 25 without a new number: an added export breaks no caller; so did gss_profile_order, gss_enrich_lists and gss_enrich_random, the preranked gene-set enrichment of profile columns; and gss_csr_set_job_cols, gss_csr_job_cols and gss_spmm_auto_slices, the job-wide operand row count behind the SpMM's automatic slice count; and gss_rownorm_elu_bwd_ex, the row-norm backward with its pos_set side write, for tests */

#define GSS_OK 0
#define GSS_EINVAL (-22)   /* bad argument (shape, null pointer, unsupported d) */
#define GSS_ENOMEM (-12)   /* hipMalloc failed */
#define GSS_EHIP (-5)      /* a HIP call or kernel launch failed */
#define GSS_ENOTCONV (-34)  /* gss_ppr_run: max_iter reached */
#define GSS_ECOMM (-104)    /* a collective failed or the communicator was aborted (RCCL error, dead peer) */
#define GSS_ETIMEOUT (-110) /* gss_comm_sync: the stream did not drain before the deadline; the communicator was aborted */

typedef struct gss_csr gss_csr;   /* a CSR operand plus its launch schedule (row bins) */
typedef struct gss_plan gss_plan; /* activations + workspace of one training replica/shard */
typedef struct gss_comm gss_comm; /* the communicator of a node-range sharded job (RCCL over xGMI, or in-process ranks) */

int gss_abi_version(void);
/* sha256 (lower-case hex) of a source file the library was built from -- "spmm.hip", "dense.hip", "common.h", "gssgcn.h" ... --, of all of
 * them concatenated in name order ("*" or NULL), or NULL for any other name.  Evidence under profiles/ records the hashes of the kernels it
 * measured; bench.py drops a counter file whose recorded spmm.hip hash is not this library's, __graft_entry__.build() rebuilds a library
 * whose hashes are not the tree's (a stale .so with fresh timestamps cannot pass for a current one). */
const char *gss_source_hash(const char *file);
/* measurement aid (tools/ab_live.py): changes one KERNEL-SELECTION knob ("gemm_variant", "gemm_ws", "spmm_slices", "spmm_pin", "spmm_list_blocks") in a live
 * plan's snapshot, so that one plan -- the same buffers at the same addresses --
 * can be timed under alternating settings; knobs that size a workspace or steer the plan's bookkeeping are refused (GSS_EINVAL).
 * Not thread-safe against gss_debug_set_option on another thread.
 * One name is a PLAN OPTION and exists here only (it is none of the 20 process-wide knobs): "l1_ahead" = -1 (default: automatic) / 0 / 1.
 * A one-GPU plan with two or more layers and neither cache_layer1 nor pipeline_layer1 computes layer 1's two SpMMs -- functions of
 * A_hat and X alone -- one pass AHEAD: every full forward pass (gss_plan_step, gss_plan_forward) carries them for the next pass as the
 * second halves of layer 2's two SpMM launches (gss_spmm_fwd_pair), into the layer-1 buffers themselves, and a pass that finds them there
 * runs no layer-1 SpMM.  Every step still computes its six products, in ten launches instead of twelve at two layers; same bits.  A lazy
 * step consumes what a full pass left and leaves nothing.  With profiling on, a paired launch counts as two launches of its class that
 * share its time.  As with cache_layer1, X and A_hat must not change under a live plan. */
int gss_plan_debug_set_option(gss_plan *plan, const char *name, int value);
/* 1 while the plan's layer-1 buffers hold layer 1 for the NEXT forward pass (option "l1_ahead"), else 0 */
int gss_plan_l1_ahead(const gss_plan *plan);
const char *gss_last_error(void);

/* ---- K11  preprocess_graph, helpers/helper.py:82-89 (+ fp32 cast helper.py:95) ----------
 * In: CSR of (A + I) with fp64 values (diagonal already inserted, columns sorted).
 * Out: val_out[e] = (float)(dinv[row] * val[e] * dinv[col[e]]), dinv = rowsum^-1/2 in fp64;
 *      rowsum_out (nullable) = fp64 row sums D_ii.  Row sums <= 0 give NaN/inf like the reference. */
int gss_normalize_adj(int32_t n, const int32_t *rowptr, const int32_t *col, const double *val,
                      float *val_out, double *rowsum_out, void *stream);

/* The same for one node-range shard: the shard holds rows [row0, row0 + n) of A + I -- or, transposed != 0, of
 * (A + I)^T -- with GLOBAL column ids.  gss_rowsum_dinv: D_ii and D_ii^-1/2 of the shard's rows of A + I;
 * gss_scale_adj_shard: the normalised values from the all-gathered D^-1/2 of every node, with the rounding sequence of
 * gss_normalize_adj, so a shard's values are bit-identical to the matching entries of the single-GPU A_hat / A_hat^T. */
int gss_rowsum_dinv(int32_t n, const int32_t *rowptr, const double *val, double *dinv_out, double *rowsum_out, void *stream);
int gss_scale_adj_shard(int32_t n, int32_t row0, const int32_t *rowptr, const int32_t *col, const double *val, const double *dinv_global,
                        int32_t transposed, float *val_out, void *stream);
/* The guard the reference lacks (helpers/helper.py:85, SURVEY a3's hazard): counts the rows whose D_ii is not > 0 -- negative
 * similarities in kNN mode can do that -- i.e. the rows whose D_ii^-1/2 is NaN / inf and poisons every entry of their row and column.
 * rowsum = the fp64 row sums gss_normalize_adj / gss_rowsum_dinv wrote (device); *h_count_out and *h_first_out (nullable; the lowest
 * such row, -1 if none) are HOST values: the call waits for the stream.  The normalisation itself stays the reference's arithmetic; what
 * to do about a positive count is the caller's decision (trainer.py refuses to train unless --allow-nan). */
int gss_rowsum_check(int32_t n, const double *rowsum, int64_t *h_count_out, int32_t *h_first_out, void *stream);

/* ---- CSR handle ---------------------------------------------------------------------------
 * Borrows d_rowptr/d_col/d_val (caller keeps them alive).  h_rowptr is a HOST copy of rowptr used
 * once to bin rows by length (long rows get a whole workgroup).  n_cols is the height of the dense
 * operand (== n_rows on one GPU, the global N for a row shard). */
int gss_csr_create(gss_csr **out, int32_t n_rows, int32_t n_cols, int64_t nnz, const int32_t *h_rowptr,
                   const int32_t *d_rowptr, const int32_t *d_col, const float *d_val);
void gss_csr_destroy(gss_csr *a);
/* Optional, for graphs whose nodes were relabelled hub-first (descending degree): declare which rows of the dense operand
 * belong to the hubs -- rows [0, own_hot) and [halo_begin, halo_end) (the second range is for a shard, whose operand holds
 * the other shards' boundary rows behind its own).  Where the operand is far larger than the caches the SpMM then fetches
 * every other row with the non-temporal policy, so that once-read rows do not evict the hubs' rows.  own_hot = -1: no split
 * (the default).  Speed only: results are unchanged. */
int gss_csr_set_hot(gss_csr *a, int32_t own_hot, int32_t halo_begin, int32_t halo_end);
/* The operand rows the JOB multiplies by: the global N for the matrices of a node-range shard, whose own operand (n_cols) holds only
 * its rows and the boundary rows it reads.  Default: the handle's own n_cols, so a handle nobody declares anything on behaves as
 * before.  The balanced SpMM decides its automatic feature-slice count (knob "spmm_slices" = 0) from THIS count, not from n_cols: the
 * slice count sets the lane-group width and so how the segment sums of a row of more than 64 entries are grouped, and a row must be
 * rounded alike on every owner -- a shard's rows are bit-identical to the one-GPU product's rows only when both sides decide from the
 * same count.  Everything that is cache policy (slices pinned to XCDs or time-separated, 32-bit gather offsets, the hot / cold
 * split) changes no bit and still follows n_cols.  cols must be >= n_cols.  The giant-row views of the handle (gss_csr_giant_rows)
 * carry the handle's count, the finish pass included.  gss_plan_create_sharded declares h_bounds[world] on every matrix it is given
 * (a, at and the split halves), so callers of the plan need not; call it yourself for products you run on a shard's handle outside a
 * plan.  gss_csr_job_cols reads the count in force back. */
int gss_csr_set_job_cols(gss_csr *a, int64_t cols);
int gss_csr_job_cols(const gss_csr *a, int64_t *cols_out);
/* The automatic slice policy as a pure function (no handle, no device): what a dense-mode product of width d over a handle whose job
 * count AND own operand are both `cols` rows picks under "spmm_slices" = 0 -- *slices_out feature slices (1 = unsliced), *pinned_out
 * = 1 when they are pinned to XCDs, 0 when time-separated or unsliced.  (N = 29,960, d = 128: 2 slices, pinned.) */
int gss_spmm_auto_slices(int32_t d, int64_t cols, int32_t *slices_out, int32_t *pinned_out);
/* Rows with more stored entries than knob "spmm_giant" (default 32,768; 0 = never) are not one workgroup's job: the dense products cut
 * them into chunks of a quarter of that, sum the chunks in a pass of their own and add a row's chunks in order in a finish pass that runs
 * the product's epilogue (three launches of the same kernel; results agree with the unchunked sum to rounding, rows below the threshold
 * keep their bits).  The hubs of a 10^7-node scale-free graph hold ~3 x 10^5 entries: as one workgroup's job such a row alone outlasts
 * the rest of a shard's launch.  A handle looks at the knob with its first product (or with this call): n_rows_out = its giant rows,
 * n_chunks_out = their chunks. */
int gss_csr_giant_rows(const gss_csr *a, int32_t *n_rows_out, int32_t *n_chunks_out);

/* ---- K1/K2  torch.sparse.mm + torch.mul, modules/model.py:163,168-169 -----------------------
 * y = A x  (x: [n_cols][d], y: [n_rows][d]).  If m != NULL also m = y (.) h, h: [n_rows][d]
 * (the Hadamard of model.py:168 fused into the epilogue of the first SpMM). */
int gss_spmm(const gss_csr *a, int32_t d, const float *x, float *y, const float *h, float *m, void *stream);
/* The second pass of a two-pass product: y = y_in + A x (then m = y (.) h as above).  The entries of the rows may be split over two
 * CSR handles of the same rows (e.g. a shard's own-column and boundary-column entries, gss_shard_desc): gss_spmm with the first,
 * gss_spmm_add with the second.  y_in may be y itself. */
int gss_spmm_add(const gss_csr *a, int32_t d, const float *x, const float *y_in, float *y, const float *h, float *m, void *stream);

/* backward SpMMs (autograd of model.py:163-169 for layers >= 2), A here is CSR(A_hat^T):
 *   gss_spmm_bwd1: dm = A g_am;  u = g_ax + dm (.) x_in;  t = dm (.) ax
 *   gss_spmm_bwd2: gx = t + A u; dp = c * gx (.) elu'(p) (+ res if res != NULL); gx_out nullable */
int gss_spmm_bwd1(const gss_csr *at, int32_t d, const float *g_am, const float *g_ax, const float *x_in,
                  const float *ax, float *u, float *t, void *stream);
int gss_spmm_bwd2(const gss_csr *at, int32_t d, const float *u, const float *t, const float *p, float c,
                  const float *res, float *dp, float *gx_out, void *stream);
/* gss_spmm_bwd1 for row-sparse gradients (the top layer: dLoss/dE is non-zero on the B batch rows only):
 * g_am_b / g_ax_b are compact [B][d]; pos_col[c] is the compact row of column id c (or -1), pos_row[r] the
 * compact row of output row r (or -1).  Neighbours with pos_col < 0 are skipped. */
int gss_spmm_bwd1_sparse(const gss_csr *at, int32_t d, const float *g_am_b, const float *g_ax_b,
                         const int32_t *pos_col, const int32_t *pos_row, const float *x_in, const float *ax,
                         float *u, float *t, void *stream);

/* ---- K3/K4  nn.Linear x2 + add + F.elu + residual, modules/model.py:165,170-173,201-203 -------
 * p = ax W1^T + b1 + am W2^T + b2;  o = elu(p);  x_next = p_prev ? p_prev + decay*o : o.
 * W1, W2: [d][d] row-major ([out][in], the nn.Linear layout).  fp32 MFMA (v_mfma_f32_16x16x4_f32). */
int gss_dense_fwd(int32_t n, int32_t d, const float *ax, const float *am, const float *w1, const float *b1,
                  const float *w2, const float *b2, const float *p_prev, float decay, float *p, float *x_next,
                  void *stream);

/* input gradients of the two Linear layers: g_ax = dp W1, g_am = dp W2 (w1t/w2t are the TRANSPOSED
 * weights, [in][out]).  If rows != NULL, row r of the compact [n][d] input is written to row rows[r]
 * of the outputs (scatter of batch-row gradients into zeroed [N][d] buffers).  rows[0..n) must be UNIQUE,
 * VALID row indices of g_ax / g_am: the kernel uses rows[r] unchecked, and a negative entry is NOT skipped
 * (unlike gss_scatter_add_rows and the forward row lists) -- it would be written in front of the buffers.
 * Rows that are not listed, and rows behind n without a list, are not written. */
int gss_dense_bwd_input(int32_t n, int32_t d, const float *dp, const float *w1t, const float *w2t,
                        const int32_t *rows, float *g_ax, float *g_am, void *stream);

/* weight gradients: gw1 (+)= dp^T ax, gw2 (+)= dp^T am, gb (+)= colsum(dp), fixed-order two-stage
 * reduction (bitwise reproducible).  rows != NULL: dp is compact [n][d] and ax/am rows are gathered
 * at rows[r].  accumulate != 0 adds to the existing gw1/gw2/gb.  ws: workspace of
 * gss_wgrad_workspace_bytes(n, d) bytes. */
size_t gss_wgrad_workspace_bytes(int32_t n, int32_t d);
int gss_dense_bwd_weight(int32_t n, int32_t d, const float *dp, const float *ax, const float *am,
                         const int32_t *rows, float *gw1, float *gw2, float *gb, int accumulate, void *ws,
                         void *stream);

/* ---- K5  F.normalize(x, dim=1), modules/model.py:205 (eps 1e-12) -----------------------------
 * e = x / max(||x||, eps); inv_den[i] = 1 / max(||x_i||, eps) is kept for the backward pass. */
int gss_rownorm_fwd(int32_t n, int32_t d, const float *x, float *e, float *inv_den, void *stream);

/* ---- K6/K7  GSS_loss.gss_loss + its autograd, modules/model.py:214-221 ------------------------
 * E_B = e[idx]; S = E_B E_B^T; loss = mean(-alpha/2 (relu(S) - beta)^2) written to loss_out[0];
 * de_b[b] = dLoss/dE_B[b] = sum_j (G_bj + G_jb) E_B[j], G = -alpha/B^2 (relu(S)-beta) 1[S>0].
 * S is never materialised.  idx: int32[B], unique.  ws: gss_loss_workspace_bytes(B, d) bytes. */
size_t gss_loss_workspace_bytes(int32_t b, int32_t d);
/* The size is NOT monotone in B (fewer row tiles get more column slabs: B = 2032 needs more than B = 2048): a caller that keeps one
 * workspace for batches of up to b_max rows -- e.g. the shorter last batch of an epoch -- sizes it with this. */
size_t gss_loss_workspace_bytes_max(int32_t b_max, int32_t d);
int gss_loss_fwd_bwd(int32_t n, int32_t d, const float *e, const int32_t *idx, int32_t b, float beta,
                     float alpha, float *loss_out, float *de_b, void *ws, void *stream);

/* backward of K5 + K4 on the batch rows: dx_b = (de_b - e_b (e_b . de_b)) * inv_den[idx];
 * dp_b = c * dx_b (.) elu'(p[idx]).  All [B][d] compact.  idx[0..b) must be valid node rows of e / inv_den /
 * p: idx[r] is read unchecked, a negative entry is NOT skipped. */
int gss_rownorm_elu_bwd(int32_t d, const float *de_b, const int32_t *idx, int32_t b, const float *e,
                        const float *inv_den, const float *p, float c, float *dx_b, float *dp_b, void *stream);

/* dst[rows[r]] += src[r] for r < b (rows unique; a negative row is skipped -- a batch row another shard owns) */
int gss_scatter_add_rows(int32_t d, const float *src, const int32_t *rows, int32_t b, float *dst, void *stream);

/* ---- C1-C3  collectives of the node-range sharded trainer (the reference is single-device,
 * train.py:68,118-122, so there is nothing to match -- these are the exchange points 1-D sharding of its step needs).
 * One process per GPU: rank 0 calls gss_comm_unique_id, the host distributes the GSS_COMM_ID_BYTES bytes (torch.distributed
 * store, a file ...), every rank calls gss_comm_create_rccl with its current HIP device set.  gss_comm_create_local makes
 * `world` communicators for ranks that are THREADS of one process (each with its own stream, possibly all on one GPU):
 * device-to-device copies behind a timed host barrier, so that a sharded plan can be run at world 2..8 on a one-GPU box.
 * Collectives are enqueued on `stream` (the local backend also synchronises it); every rank must call them in the same order. */
#define GSS_COMM_ID_BYTES 128
int gss_comm_unique_id(void *id_out);
int gss_comm_create_rccl(gss_comm **out, int32_t world, int32_t rank, const void *id);
int gss_comm_create_local(gss_comm **out /* [world] */, int32_t world);
/* Measurement aid of the in-process backend (tools/shard_emulation.py --serial): rank threads share ONE GPU, so a step timed with all
 * of them running says nothing about one rank's kernels.  mode 1 = record: keep a device copy of what every collective DELIVERS to this
 * rank, in call order; mode 2 = replay: serve those copies again (same call sequence and sizes, checked) by a device-to-device copy --
 * no peers, no barrier, no host wait -- so that one rank's step can run alone on the GPU and be timed; mode 0 (default) = normal, frees
 * the log.  gss_comm_local_log: the delivered bytes of every recorded collective (n_out = how many there are; at most cap are written).
 * Besides the collectives of the steps, gss_plan_create_sharded at world > 1 runs one all-gather (the job-wide knob check), which a log
 * recorded across a plan's creation also holds. */
int gss_comm_local_mode(gss_comm *c, int32_t mode);
int gss_comm_local_log(gss_comm *c, int64_t *bytes_out, int32_t cap, int32_t *n_out);
/* A third backend for boxes where RCCL cannot run the job: one PROCESS per rank as with RCCL, but every collective is staged through
 * pinned host memory and handed to a transport callback of the host language (the Python package passes torch.distributed's gloo;
 * GSS_COMM_BACKEND=host).  RCCL refuses two ranks on one device, so this is how `train.py --ngpus N` / `bench.py --gpus N` run as N
 * real processes on a ONE-GPU test box (all ranks on that GPU).  The callback receives pinned host buffers:
 *   GSS_HOST_ALLGATHER: `count` bytes at send from every rank, rank r's at recv + r * count;
 *   GSS_HOST_ALLTOALLV: bytes [send_off[q], send_off[q+1]) of send go to rank q, the bytes rank q sends land at [recv_off[q], recv_off[q+1])
 *   of recv (byte offsets, world + 1 entries each).
 * (the own range is empty, as in gss_exchange_rows).  It returns 0 on success.  Sums (gss_allreduce_sum) are taken on the host in rank order: the same bits on every rank. */
enum { GSS_HOST_ALLGATHER = 0, GSS_HOST_ALLTOALLV = 1 };
typedef int (*gss_host_xfer_fn)(void *user, int kind, const void *send, const int64_t *send_off, void *recv, const int64_t *recv_off, int64_t count);
int gss_comm_create_host(gss_comm **out, int32_t world, int32_t rank, gss_host_xfer_fn fn, void *user);
void gss_comm_destroy(gss_comm *c);
/* Make every rank that is (or will be) blocked in a collective of this group return an error -- call it from a rank that failed.
 * In-process backend: releases the host barrier (the peers do not wait for its 120 s timeout).  RCCL: ncclCommAbort -- kernels
 * already enqueued stop waiting for the peer, the communicator is unusable afterwards (every later call returns GSS_ECOMM). */
void gss_comm_abort(gss_comm *c);
/* Failure detection (the reference is single-process and has none).  Every collective entry point polls
 * ncclCommGetAsyncError after enqueueing and, on an error, aborts the communicator and returns GSS_ECOMM; gss_comm_check is the same
 * poll on its own.  gss_comm_sync waits until `stream` has drained (hipStreamQuery + the same poll, no busy device wait) and, if
 * that takes longer than timeout_s (> 0) -- a peer that stopped calling, mismatched collectives --, aborts the communicator and
 * returns GSS_ETIMEOUT instead of hanging; callers then exit non-zero.  gss_comm_count: the number of ranks the backend itself
 * reports (ncclCommCount) -- bench.py prints it as `rccl_ranks`. */
int gss_comm_check(gss_comm *c);
int gss_comm_count(gss_comm *c, int32_t *count_out);
int gss_comm_sync(gss_comm *c, void *stream, double timeout_s);
int32_t gss_comm_world(const gss_comm *c);
int32_t gss_comm_rank(const gss_comm *c);
/* C1: src [max_rows][d] (this rank's rows first, the rest don't-care) -> dst_padded [world * max_rows][d], rank r's rows at
 * row r * max_rows.  In place when src == dst_padded + rank * max_rows * d. */
int gss_allgather_rows(gss_comm *c, int32_t d, int32_t max_rows, const float *src, float *dst_padded, void *stream);
int gss_allgather_bytes(gss_comm *c, const void *src, void *dst, size_t bytes_per_rank, void *stream);
/* C2/C3: buf <- sum over ranks, in place, the same bits on every rank */
int gss_allreduce_sum(gss_comm *c, float *buf, int64_t count, void *stream);
/* C1, boundary form: rows [h_send_off[q], h_send_off[q+1]) of `send` ([..][d]) go to rank q; the rows rank q sends land at
 * rows [h_recv_off[q], h_recv_off[q+1]) of `recv`.  Offsets are HOST arrays of world + 1 entries (own range empty); one
 * fused group of ncclSend / ncclRecv, pairs with nothing to exchange are skipped. */
int gss_exchange_rows(gss_comm *c, int32_t d, const float *send, const int64_t *h_send_off, float *recv, const int64_t *h_recv_off,
                      void *stream);

/* ---- K10  torch.optim.Adam.step, train.py:139-141,184 -----------------------------------------
 * One tensor of `count` floats; step is the 1-based step number.  lr, betas, eps as torch defaults.
 * If wt != NULL the updated parameter, viewed as [dim][dim], is also written transposed to wt. */
int gss_adam_step(int64_t count, float *param, const float *grad, float *exp_avg, float *exp_avg_sq,
                  int32_t step, float lr, float beta1, float beta2, float eps, float *wt, int32_t dim,
                  void *stream);

/* ---- K12  np.percentile(E E^T, q), train.py:165-167 -------------------------------------------
 * Exact q-th percentile (linear interpolation) of all n*n inner products of the rows of e, by
 * 3-pass radix select on device.  Result to h_out (host float), synchronises the stream.
 * GSS_EINVAL, h_out untouched, when an inner product is inf or NaN in fp32 ("non-finite similarity"). */
int gss_percentile(int32_t n, int32_t d, const float *e, double q, float *h_out, void *stream);

/* ---- a1  gen_graph's similarity + top-k, helpers/helper.py:39-44 --------------------------------------
 * x: [n][d] fp64 features (the reference works in fp64 here).  For every row the k largest inner products
 * x_i . x_j over all j (self included, as np.argpartition(x_sim, -k, 1)[:, -k:] returns them; order within the
 * k is unspecified) -> top_val [n][k] fp64, top_idx [n][k] int32.  fp64 MFMA; d multiple of 8, k <= 64. */
int gss_knn_topk(int32_t n, int32_t d, const double *x, int32_t k, double *top_val, int32_t *top_idx, void *stream);
/* the same for rows [row_lo, row_hi) only (against all n columns): top_val / top_idx [row_hi - row_lo][k].  What a rank of a sharded
 * job computes for its own row window (shards.KnnSource); a row's result does not depend on the window. */
int gss_knn_topk_rows(int32_t n, int32_t d, const double *x, int32_t k, int32_t row_lo, int32_t row_hi, double *top_val,
                      int32_t *top_idx, void *stream);

/* ---- f4  diffusion profiles, multiscale/diff_prof/diffusion_profiles.py:30-90 ---------------------------
 * Personalised PageRank from every drug / indication, all start nodes at once: column c of the fp64 matrix
 * x[n][kpad] is the visit-probability vector of start node start[c].  The reference builds one matrix M_s per start
 * node s (edges from every other drug / indication to its proteins cut, edges from s's proteins into s cut, rows
 * renormalised; :30-56) and runs  x <- alpha (x M_s + dangling(x) e_s) + (1 - alpha) e_s  until
 * ||x - x_last||_1 < n tol (:65-90).  Here ONE shared matrix M' -- every drug / indication row in its "not selected"
 * form, i.e. cut and renormalised (normally empty: a pure sink) -- is multiplied into all columns by one fp64 SpMM per
 * iteration; what differs per start node is applied around the product:
 *   - ovr_*: entry (ovr_row[e], column ovr_col[e]) of x is multiplied by ovr_ratio[e] for the product.  Proteins of
 *     the start node: their row of M_s is renormalised without the cut edge (ratio 0 = the row became empty; listed in
 *     zero_* and counted as dangling).  The start node's own entry gets ratio 0 (not dangling) when its "not
 *     selected" row is not empty, so that row does not act in its own column;
 *   - sel_*: the start node's row in its "selected" form (all its out-edges over their sum):
 *     y[sel_row[e]][sel_col[e]] += sel_val[e] * x[start][sel_col[e]];
 *   - keep_*: in-edges of a start node that survive the cut (none in the plain MSI, where drugs and indications only
 *     touch proteins): value M'[keep_row][start[c]]; the product's own value at (start[c], c) is replaced by their sum;
 *   - z_rows: the empty rows of M' (sinks, isolated nodes): dangling in every column except, for the start node's
 *     own row, its column (start_dangling[c] = 1 if even its "selected" row is empty).
 * Columns converge independently and are frozen at the iteration the reference would have returned them.
 * All pointers are device pointers except h_rowptr.  kpad (the row stride of x) must be a multiple of 64. */
typedef struct gss_ppr gss_ppr;
typedef struct gss_ppr_desc {
  int32_t n, k, kpad;
  int64_t nnz;
  const int32_t *h_rowptr;                 /* host copy of t_rowptr */
  const int32_t *t_rowptr, *t_col;         /* CSR of M'^T: row j lists in-neighbours i ascending */
  const double *t_val;                     /* M'[i][j] */
  const int32_t *start;                    /* [k] */
  const int32_t *start_dangling;           /* [k] */
  int32_t n_z;
  const int32_t *z_rows;                   /* [n_z] ascending */
  int64_t n_ovr;
  const int32_t *ovr_col, *ovr_row;        /* [n_ovr] */
  const double *ovr_ratio;                 /* [n_ovr] */
  const int32_t *zero_ptr, *zero_ovr;      /* [k+1], indices e of dangling overrides, grouped by column */
  int64_t n_sel;
  const int32_t *sel_col, *sel_row;        /* [n_sel], (row, column) pairs unique */
  const double *sel_val;
  const int32_t *keep_ptr, *keep_row;      /* [k+1], rows */
  const double *keep_val;
  const int32_t *ovr_ptr;                  /* optional, [k+1]: the overrides of column c are entries [ovr_ptr[c], ovr_ptr[c+1]) (ovr_col
                                              non-decreasing).  With it (or with n_ovr == 0) the update x <- alpha (...) + (1 - alpha) e_s and
                                              the column errors run in the SpMM's epilogue instead of in a pass of their own */
} gss_ppr_desc;
int gss_ppr_create(gss_ppr **out, const gss_ppr_desc *desc);
void gss_ppr_destroy(gss_ppr *p);
size_t gss_ppr_device_bytes(const gss_ppr *p);
/* every buffer the handle carves from its slab is followed by a 256-byte guard no kernel may touch; this synchronises the device and
 * verifies them all (as gss_plan_check_guards).  For tests. */
int gss_ppr_check_guards(gss_ppr *p);
/* x <- 1/n, then iterate.  iters_out: host [k], the iteration at which each column converged.  Returns
 * GSS_ENOTCONV (x holds the last iterate) if some column needs more than max_iter iterations -- where the reference
 * raises (:90).  Synchronises the stream once per iteration (reads the number of unconverged columns). */
int gss_ppr_run(gss_ppr *p, double alpha, double tol, int32_t max_iter, double *x, int32_t *iters_out, void *stream);
/* per-column knock-outs: column c is the profile of start[c] on the graph in which node dead[c] has lost all its edges before the
 * weighting (msi.graph.remove_edges_from(in_edges(g) + out_edges(g)), then weight_graph; g stays in the node list, so n, 1 / n and n tol
 * do not change).  The rows of g's neighbours change (a neighbour's remaining protein-class edges grow, its other classes keep their
 * share of a new row sum); the caller expresses that per column on the shared M':
 *   - through the lists of gss_ppr_desc: an override with the factor of the row's protein-class entries, ratio 0 + zero_* for a row that
 *     lost everything and for g's own row, the start's sel_* / keep_* / start_dangling rebuilt without g;
 *   - corr_*: y[corr_grp_row[q]][corr_grp_col[q]] += sum_e corr_val[e] * x[corr_src[e]][corr_grp_col[q]] over the entries
 *     e in [corr_ptr[q], corr_ptr[q + 1]) of group q, in list order, with the unscaled x: the other successors of such a row, whose factor
 *     differs from the override's.  Groups are sorted by (column, row), unique, never on the column's start or dead row;
 *   - dead [k] (-1 = none): the shared matrix still delivers i -> g, so x_new[dead[c]][c] is forced to 0 after the product and the column's
 *     L1 error is corrected by |0 - x_prev| - |computed - x_prev|.
 * One wave per column sums in a fixed order, without atomics: runs are bit-equal; a column with dead[c] = -1 and no group has the bits it
 * has without this call, and a handle on which it was never called runs the launches it ran before.  The handle keeps the POINTERS (device,
 * owned by the caller, alive until the handle is destroyed) and needs no buffer of its own for them.  Synchronises the device and validates
 * on the host, refusing by name (GSS_EINVAL): a handle without the fused update (gss_ppr_desc.ovr_ptr missing or knob ppr_fused = 0 at
 * gss_ppr_create), a null dead, missing lists, dead[c] outside [-1, n) or equal to start[c], corr_ptr not running from 0 to n_corr or
 * decreasing, a group column outside [0, k) / row outside [0, n), groups out of (column, row) order, a group on its column's start or
 * dead row, a source outside [0, n). */
int gss_ppr_set_knockout(gss_ppr *p, const int32_t *dead, int64_t n_grp, const int32_t *corr_ptr, const int32_t *corr_grp_row,
                         const int32_t *corr_grp_col, int64_t n_corr, const int32_t *corr_src, const double *corr_val);
/* one product y = M'^T x on the handle's schedule (fp64; the kernel the iteration is built on) */
int gss_ppr_spmm(gss_ppr *p, const double *x, double *y, void *stream);

/* ---- node2vec input embeddings: multiscale/openne/node2vec.py:7-47 (walker.py:58-207 + gensim Word2Vec sg=1 negative sampling) ------------
 * The trainer's input .embs.txt (predict_drug.py:33-46) made on the device: second-order biased walks over the raw weighted directed
 * graph (walk.hip), then skip-gram with negative sampling over them (sgns.hip).  Every random number comes from a counter-based generator
 * keyed by (seed, what, counters) -- csrc/counter_rng.h --, so walks and a serial SGNS epoch are pure functions of their inputs.
 *
 * gss_walk_prefix: cum[e] = inclusive fp64 prefix sum of val over e's row, in row order.  Validates every weight: returns GSS_EINVAL
 * naming the first CSR entry whose weight is not positive and finite.  Waits for the stream (it reads the verdict).
 * gss_node2vec_walks: walk w starts at starts[w] and takes at most walk_length nodes (the start included); step 1 is first-order in the
 * edge weights, later steps from cur with predecessor prev pick x with weight w(cur, x) * (1/p if x == prev, else 1 if x -> prev is an
 * edge, else 1/q).  A walk ends early at a node without out-edges.  Out: walks [n_walks][walk_length] (unused tail = -1), lengths
 * [n_walks].  Columns must be sorted within each row, cum from gss_walk_prefix; p, q > 0 and walk_length >= 1 are checked by name. */
int gss_walk_prefix(int32_t n, const int32_t *rowptr, const double *val, double *cum, void *stream);
int gss_node2vec_walks(int32_t n, const int32_t *rowptr, const int32_t *col, const double *val, const double *cum, int64_t n_walks,
                       const int32_t *starts, int32_t walk_length, double p, double q, uint64_t seed, int32_t *walks, int32_t *lengths,
                       void *stream);
/* gss_sgns_counts: counts[node] += occurrences of node in the walks (counts: int64 [n], zeroed by the caller).
 * gss_sgns_init: syn0[i][k] = (u - 0.5) / d with u uniform fp32 keyed by (seed, i, k); syn1neg = 0.
 * gss_sgns_epoch: one epoch of gensim 3.x skip-gram negative sampling (sgns.hip has the update rule).  The sigmoid is evaluated
 * exactly (1 / (1 + expf(-f)), fp32), a target with |f| >= 6 is skipped as gensim skips it.  cum_table is gensim's negative-sampling
 * table (uint32 [n], cumulative count^ns_exponent scaled to 2^31 - 1, cum_last = its last entry), sample_int gensim's downsampling
 * threshold per node (a token is kept iff a uint32 draw <= sample_int).  concurrency = center positions in flight (one wave each);
 * 1 runs the epoch in serial order, gss_sgns_default_concurrency() fills the device.  d must be 64, 128, 256 or 512. */
typedef struct gss_sgns_desc {
  int32_t n, d, walk_length, window, negative, epochs;
  int64_t n_walks;
  const int32_t *walks, *lengths;   /* from gss_node2vec_walks; one sentence per walk */
  const uint32_t *cum_table;
  const int64_t *sample_int;
  uint32_t cum_last;
  float alpha, min_alpha;           /* linear decay over (epoch + sentence / n_walks) / epochs */
  uint64_t seed;
  int32_t concurrency;
} gss_sgns_desc;
int gss_sgns_counts(int64_t n_walks, int32_t walk_length, const int32_t *walks, const int32_t *lengths, int64_t *counts, void *stream);
int gss_sgns_init(int32_t n, int32_t d, uint64_t seed, float *syn0, float *syn1neg, void *stream);
int gss_sgns_default_concurrency(void);
int gss_sgns_epoch(const gss_sgns_desc *desc, int32_t epoch, float *syn0, float *syn1neg, void *stream);

/* ---- network proximity of drug targets to disease genes: Guney et al. 2016 (method/test_proximity.py, toolbox wrappers.calculate_proximity)
 * gss_prox_create: all-pairs hop distances of an undirected graph (symmetric CSR, no self loops, rowptr/col device) into a uint8 [n][n]
 * matrix owned by the handle (255 = unreachable).  Refuses n * n > max_bytes and a graph with a node 255 or more hops from another
 * (GSS_EINVAL, by name).  Synchronises the stream.  gss_prox_distances: the device matrix; gss_prox_diameter: the largest finite hop count
 * (the diameter is taken over finite distances only: isolated nodes and further components, 255 in the matrix, do not enter it; a
 * path of 255 nodes -- 254 hops -- is accepted, one of 256 nodes refused).
 * Sets are LCC node indices.  A set table holds n_sets x n_samples compacted sets of at most max_size nodes, ascending: nodes
 * [n_sets][n_samples][max_size], sizes [n_sets][n_samples].  Sample 0 is the set itself, sample r >= 1 the random set k = r - 1.
 * gss_prox_random_sets: from the sets in CSR form (set_ptr [n_sets + 1], set_nodes ascending unique) and the degree bins (node_bin [n],
 * bin_ptr, bin_nodes), writes the table with n_samples = n_random + 1.  Random set k walks the members v_i in order: draw a node of v_i's bin,
 * redraw (at most 20 times) while it is already in the set, add it if it is not; draw a of member i of set s is
 * bin_nodes[lo + (u32 * bin size >> 32)], u32 keyed by (seed, 7 + side, s, k, i * 32 + a) in counter_rng.h.  side: 0 from, 1 to.
 * A member whose 21 draws (a = 0..20) are all taken already is dropped: that random set is one node smaller than the set, and
 * sizes says so.  Entries of a row past its size are left as the caller had them.  With n_random = 0 only the sets themselves are written.
 * Synchronises the stream (validates the member indices).
 * gss_prox_set_stats: per (set, sample): inner = mean over members of the hop count to the closest other member (0 for fewer than 2);
 * with centres / n_centres: every member whose summed distance to the set is minimal, ascending (centres laid out like nodes).
 * gss_prox_score: for every pair (pair_from[q], pair_to[q]), or all n_from x n_to pairs q = i * n_to + j when the lists are NULL, and every
 * sample r, the five measures of (from sample r, to sample r): closest = mean_t min_s D, shortest = mean D, kernel = -mean_t
 * ln(sum_s e^-(D+1) / |S|), center = mean D(t, c) over t and the tied centres, separation = (sum_t min_s D + sum_s min_t D) / (|T| + |S|)
 * - (inner_from + inner_to) / 2.  out [n_pairs][5 measures][5] = d (sample 0), mean and population sd over samples 1.., z = (d - m) / sd
 * (0 when sd = 0, then pval = 0.5), pval = Phi(z), all fp64 in a fixed order (bitwise reproducible): m is summed in sample order
 * r = 1, 2, ... and divided once, sd is the root of the mean squared deviation from that m, summed in the same order; NaN where a set
 * is empty.  Pairs are scored in batches of as many as a 256 MiB scratch holds ("prox_batch_pairs" caps the batch; same bits).  measures: bit mask
 * (1 closest, 2 shortest, 4 kernel, 8 center, 16 separation); closest and shortest always come out, unmasked others are 0.  The
 * to-side max_size must be <= 4096. */
typedef struct gss_prox gss_prox;
typedef struct gss_prox_sets {
  int32_t n_sets, max_size;
  const int32_t *nodes, *sizes;       /* the set table (device) */
  const double *inner;                /* [n_sets][n_samples] from gss_prox_set_stats */
  const int32_t *centres, *n_centres; /* to-side, for center; may be NULL otherwise */
} gss_prox_sets;
int gss_prox_create(gss_prox **out, int32_t n, const int32_t *rowptr, const int32_t *col, int64_t max_bytes, void *stream);
void gss_prox_destroy(gss_prox *p);
const uint8_t *gss_prox_distances(const gss_prox *p);
int32_t gss_prox_diameter(const gss_prox *p);
int gss_prox_random_sets(gss_prox *p, int32_t side, int32_t n_sets, const int32_t *set_ptr, const int32_t *set_nodes, int32_t max_size,
                         const int32_t *node_bin, const int32_t *bin_ptr, const int32_t *bin_nodes, int32_t n_random, uint64_t seed,
                         int32_t *out_nodes, int32_t *out_size, void *stream);
int gss_prox_set_stats(gss_prox *p, int32_t n_sets, int32_t n_samples, int32_t max_size, const int32_t *nodes, const int32_t *sizes,
                       double *inner, int32_t *centres, int32_t *n_centres, void *stream);
int gss_prox_score(gss_prox *p, const gss_prox_sets *from, const gss_prox_sets *to, int32_t n_samples, int64_t n_pairs,
                   const int32_t *pair_from, const int32_t *pair_to, int32_t measures, double *out, void *stream);

/* ---- module significance of node sets: the largest connected component of the induced subgraph against degree-matched random sets
 * (Menche et al. 2015; the check behind the *.lcc companion of a disease-gene file).  DESIGN.md section 9.17.
 * gss_random_sets: gss_prox_random_sets without a handle -- the same kernel, keys, table and bits for the same arguments, n being the
 * number of nodes (>= 1); its status word is allocated for the call.  Refusals as there, in the name random_sets.  Synchronises the stream.
 * gss_set_components: a unit is one row of a set table (nodes [n_units][max_size], sizes [n_units], device): its members are
 * nodes[u * max_size .. + sizes[u]), strictly ascending node indices in [0, n); entries past the size are never read.  Two members are
 * adjacent when one appears in the other's row of the CSR (rowptr [n + 1], col, device, columns ascending; the CSR gss_prox_create takes:
 * symmetric, which the caller guarantees and nothing checks).  A stored self loop is ignored.  Per unit: lcc = the size of the largest
 * component of the induced subgraph (0 for an empty unit), n_comp = the number of components, n_edges = the number of hits (i, j) with
 * j > i found in row i (the induced edges of a symmetric CSR) and, when label is not NULL ([n_units][max_size]), label[u][i] = the
 * position within the unit of the smallest member of i's component; entries past the size are left as the caller had them.  All
 * integers, exact: the same between runs and for any split of the units into calls.  n >= 1, n_units >= 1, 1 <= max_size <= 4096 (a
 * unit's members and parents live in LDS), n_units * max_size < 2^40.  Refused by name (GSS_EINVAL): a null pointer, these bounds, and
 * a unit that breaks the table's contract -- its size, a member's range, the members' order: found on the device, defined and worded
 * in csrc/seed_units.h for every op that takes such a table (no row of such a unit is read; the outputs are then undefined).
 * Synchronises the stream (reads the status word back). */
int gss_random_sets(int32_t n, int32_t side, int32_t n_sets, const int32_t *set_ptr, const int32_t *set_nodes, int32_t max_size,
                    const int32_t *node_bin, const int32_t *bin_ptr, const int32_t *bin_nodes, int32_t n_random, uint64_t seed,
                    int32_t *out_nodes, int32_t *out_size, void *stream);
int gss_set_components(int32_t n, const int32_t *rowptr, const int32_t *col, int64_t n_units, int32_t max_size,
                       const int32_t *nodes, const int32_t *sizes, int32_t *lcc, int32_t *n_comp, int32_t *n_edges,
                       int32_t *label /* NULL or [n_units][max_size] */, void *stream);

/* ---- growing a module from seed nodes: DIAMOnD (Ghiassian, Menche and Barabasi 2015), DESIGN.md section 9.18 --------------------------
 * gss_diamond_grow: a unit is one row of a seed table (seeds [n_units][max_size], sizes [n_units], device): its seed set S is
 * seeds[u * max_size .. + sizes[u]), strictly ascending node indices in [0, n); entries past the size are never read.  The CSR (rowptr
 * [n + 1], col, device) is the one gss_set_components takes: symmetric, no self loops, which the caller guarantees; max_deg is the
 * caller's bound on a row's length, checked on the device.  A unit adds n_add nodes, one per step.  With A the nodes added so far, every
 * node v outside S and A has ks / ka neighbours in S / A and, all integers, kb' = alpha ks + ka, k' = deg(v) + (alpha - 1) ks,
 * s' = alpha |S| + |A|, N' = n + (alpha - 1) |S| (the paper's seed weight alpha, kept in s' for every step).  Candidates are the v with
 * kb' > 0.  Stage 1: of the candidates with the same kb', the one with the smallest (k', v).  Stage 2: of those, the one with the
 * smallest logp, of two equal the larger kb'; it joins A.  logp = lt0 + log(S) is the log of the hypergeometric tail P(X >= kb'):
 *   lt0 = (LC(s', kb') + LC(N' - s', k' - kb')) - LC(N', k'),  LC(a, b) = lg[a + 1] - (lg[a - b + 1] + lg[b + 1]),
 *   S = 1 + sum of term_i, term = 1, for i = kb' .. min(k', s') - 1: term *= double((s' - i)(k' - i)) / double((i + 1)(N' - s' - k' + i + 1)),
 * in exactly that order: the products in int64, one fp64 division, one multiplication and one addition per i, nothing contracted, no
 * early exit.  lg (device, fp64 [n_lg]) is the caller's table lg[i] = lgamma(i), n_lg >= n + (alpha - 1) max_size + 2; lg[0] is never
 * read.  So lt0 and S are the same bits on any IEEE-754 machine and only the one log is the device's.  Where two candidates' logp are
 * closer than that log's error (different (k', kb') can have tails equal as rationals), the winner is the same between runs but
 * implementation-defined.
 * Per unit and step t (all outputs [n_units][n_add], device): node, k = k', kb = kb' (int32) and lt0, S, logp (fp64) of the node
 * added.  When no candidate is left, this and every later step of the unit are node = -1, k = kb = 0, lt0 = S = logp = 0.
 * The same bits between runs and for any split of the units into calls; no global atomic but the status word's.
 * n in [1, 30720] (per node a 32-bit word of counts and a membership bit live in LDS, beside a 4,096-slot table of stage 1's keys: 156 KiB
 * of the CU's 160), n_units >= 1, 1 <= max_size <= 4096, n_add >= 1, alpha >= 1, alpha max_deg <= 65535 (the counts are 16 bits),
 * min(alpha max_deg, alpha max_size + n_add - 1) <= 4095 (the largest kb' a step can see has a slot).  Refused by name (GSS_EINVAL): a
 * null pointer, any of these bounds, and a unit that breaks the table's contract or a row longer than max_deg -- found on the device,
 * defined and worded in csrc/seed_units.h (no row of such a unit is walked; the outputs are then undefined).  Synchronises the stream
 * (reads the status word back). */
int gss_diamond_grow(int32_t n, const int32_t *rowptr, const int32_t *col, int32_t max_deg, const double *lg, int64_t n_lg,
                     int64_t n_units, int32_t max_size, const int32_t *seeds, const int32_t *sizes, int32_t n_add, int32_t alpha,
                     int32_t *node, int32_t *k, int32_t *kb, double *lt0, double *S, double *logp, void *stream);

/* ---- joining a seed set's fragments: the seed connector algorithm (Wang and Loscalzo 2018), DESIGN.md section 9.19 -----------------
 * gss_seed_connectors: a unit is one row of a seed table (seeds [n_units][max_size], sizes [n_units], device), as gss_diamond_grow
 * takes it: strictly ascending node indices in [0, n), entries past the size never read.  The CSR (rowptr [n + 1], col, device) is the
 * one gss_set_components takes: symmetric, no self loops, which the caller guarantees; max_deg is the caller's bound on a row's length,
 * checked on the device.  With M the seeds and the nodes added so far, and L the size of the largest connected component of the
 * subgraph M induces, a candidate is a node v outside M with a neighbour in M; tot(v) = 1 + the sum of the sizes of the DISTINCT
 * components of M that hold a neighbour of v, L'(v) = max(L, tot(v)).  A step adds the candidate with the smallest key
 * (-L'(v), deg(v), v), deg the length of v's row: the largest new LCC, then the smaller degree, then the smaller node index (the
 * published algorithm breaks ties at random; this rule stands in for it).  A unit stops when there is no candidate, when the best
 * L' < L + 2 (a node that adds only itself joins nothing) or after n_add steps.  The new largest component need not contain the old
 * one.
 * Per unit and step t (int32 [n_units][n_add], device): node, lcc = L' after the step, merged = the number of components the node
 * joined, deg = deg(node); steps not taken are node = -1, lcc = merged = deg = 0.  Per unit (int32 [n_units], device): steps = the steps
 * taken, first_lcc = L of the seeds alone, final_lcc = L at the end (both 0 for an empty unit), seeds_in / added_in = the seeds / added nodes in the final largest component
 * (of two as large, the one whose smallest member comes first in M).  When label is not NULL ([n_units][max_size + n_add]):
 * label[u][i], i < size + steps, = the position in M of the smallest member of i's component, M being the seeds in their order and then
 * the added nodes in the order added (gss_set_components' labels, extended); entries past size + steps are left as the caller had them.
 * All integers, exact: the same between runs and for any split of the units into calls; no global atomic but the status word's.
 * n in [1, 30720], n_units >= 1, 1 <= max_size <= 4096, n_add >= 1, max_size + n_add <= 8192, 0 <= max_deg <= 1048575,
 * n_units * (max_size + n_add) < 2^40.  A unit's state lives in LDS: 4 bytes per node, 4 bytes per member of M and a 4 KiB list,
 * 4 (n + max_size + n_add) + 4096 bytes per workgroup -- 156 KiB of the CU's 160 at the limits, 75 KiB for n = 13,329, max_size 4,096,
 * n_add 500.  Refused by name (GSS_EINVAL): a null pointer (but label), any of these bounds, and a unit that breaks the table's
 * contract or a row longer than max_deg -- found on the device, defined and worded in csrc/seed_units.h (no row of such a unit is
 * walked; the outputs are then undefined).  Synchronises the stream (reads the status word back). */
int gss_seed_connectors(int32_t n, const int32_t *rowptr, const int32_t *col, int32_t max_deg, int64_t n_units, int32_t max_size,
                        const int32_t *seeds, const int32_t *sizes, int32_t n_add, int32_t *node, int32_t *lcc, int32_t *merged,
                        int32_t *deg, int32_t *steps, int32_t *first_lcc, int32_t *final_lcc, int32_t *seeds_in, int32_t *added_in,
                        int32_t *label /* NULL or [n_units][max_size + n_add] */, void *stream);

/* ---- connecting a seed set: approximate Steiner trees (Kou, Markowsky and Berman 1981 in Mehlhorn's 1988 form), DESIGN.md section 9.20 --
 * gss_steiner_trees: a unit is one row of a seed table (seeds [n_units][max_size], sizes [n_units], device), as gss_seed_connectors
 * takes it; its T terminals are numbered by position p = 0 .. T - 1.  The CSR (rowptr [n + 1], col, device) is the one
 * gss_set_components takes: symmetric, no self loops, columns ascending, any number of components; max_deg is the caller's bound on a
 * row's length, checked on the device.  Edges have weight 1.
 * 1. dist(v) = the hop distance from v to the nearest terminal, src(v) = the smallest position p with d(v, terminal p) = dist(v):
 *    level by level, every node takes the minimum of (dist, src) over its neighbours.  A node no terminal reaches has neither.
 * 2. An edge (u, v), u < v, both ends reached, src(u) != src(v), is a bridge of weight w = dist(u) + dist(v) + 1 between terminals
 *    src(u) and src(v).  The tree's bridges are the minimum spanning forest of the terminals under the strict total order (w, u, v):
 *    unique, so Kruskal on the sorted bridges and the Boruvka rounds of the kernel choose the same edges.
 * 3. parent(x), x reached and no terminal, = the smallest neighbour y with dist(y) = dist(x) - 1 and src(y) = src(x).  The tree's nodes
 *    are the terminals and every node on the parent chains from both ends of every chosen bridge; its edges those parent edges and the
 *    bridges.  (A forest whose leaves are terminals: KMB's second spanning tree and its pruning change nothing.)
 * Per unit (int32 [n_units], device, exact): n_comp = the trees of the forest (0 for an empty unit), length = the sum of w over the
 * chosen bridges, n_steiner = the tree nodes that are no terminals, n_edges = T + n_steiner - n_comp, max_w = the largest w (0 without
 * a bridge).  Lists, each NULL or given: steiner and parent [n_units][max_add] (both or neither): the Steiner nodes in ascending node
 * order with their parents beside them, the first max_add when there are more (the counts stay exact); bridge
 * [n_units][max_size - 1][2]: the chosen bridges (u, v) ascending.  Entries past the counts are left as the caller had them.
 * All integers: the same between runs and for any split of the units into calls; no global atomic but the status word's.
 * n in [1, 30720], n_units >= 1, 1 <= max_size <= 4096, max_add >= 0, 0 <= max_deg <= 1048575, n_units * max(max_size, max_add) < 2^40,
 * and a unit's state must fit the LDS: 4 bytes per node (dist << 12 | src), 16 per terminal position (an 8-byte bridge key, a
 * union-find parent, a chosen bridge): 4 n + 16 max_size <= 160 KiB - 512 bytes -- 116 KiB for n = 13,329 with max_size 4,096; n = 30,720
 * leaves max_size <= 2,528.  Refused by name (GSS_EINVAL): a null pointer (but the lists), any of these bounds, the LDS budget, and a
 * unit that breaks the table's contract or a row longer than max_deg -- found on the device, defined and worded in csrc/seed_units.h
 * (no row of such a unit is walked; the outputs are then undefined).  Synchronises the stream (reads the status word back). */
int gss_steiner_trees(int32_t n, const int32_t *rowptr, const int32_t *col, int32_t max_deg, int64_t n_units, int32_t max_size,
                      const int32_t *seeds, const int32_t *sizes, int32_t max_add, int32_t *n_comp, int32_t *length, int32_t *n_steiner,
                      int32_t *n_edges, int32_t *max_w, int32_t *steiner /* NULL or [n_units][max_add] */,
                      int32_t *parent /* NULL or [n_units][max_add] */, int32_t *bridge /* NULL or [n_units][max_size - 1][2] */,
                      void *stream);

/* ---- ranking nodes by random walk with restart from seed sets (network propagation; Koehler et al. 2008, the comparator of the
 * DIAMOnD paper), DESIGN.md section 9.21 ----------------------------------------------------------------------------------------------
 * gss_rwr_rank: a unit is one row of a seed table (nodes [n_units][max_size], sizes [n_units], device), as gss_diamond_grow takes it:
 * strictly ascending node indices in [0, n), entries past the size never read.  The CSR (rowptr [n + 1], col, device) is the one
 * gss_set_components takes: symmetric, no self loops, which the caller guarantees; every row has an entry and at most max_deg, checked
 * on the device.  For a unit S of m >= 1 seeds, deg[j] = rowptr[j + 1] - rowptr[j], all in fp64, every product, quotient, sum and
 * difference rounded on its own (nothing contracted into a multiply-add):
 *   p0[i] = 1.0 / m on S (one division), 0 elsewhere; p = p0; then per iteration
 *   q[j] = p[j] / deg[j];  s[i] = the sum of q[col[e]] over row i;  p'[i] = (1 - restart) * s[i] + restart * p0[i];
 *   err = the sum over i of |p'[i] - p[i]|;  p <- p'.
 * It stops after the iteration with err < tol (strict) or after max_iter of them; iters_out[u] is the number run, so tol = 0 runs
 * exactly max_iter.  The order of the sums, T = 1024 threads in 16 waves of 64 lanes, node i owned by thread i % T:
 *   s[i], a row of at most 32 entries (the row schedule changes class between 32 and 33): from 0.0, the entries added in ascending e;
 *   s[i], a longer row: lane l starts from 0.0 and adds the entries e = rowptr[i] + l, + 64, + 128, ... in ascending e; then the
 *     butterfly x[l] <- x[l] + x[l ^ o] for o = 32, 16, 8, 4, 2, 1 over the 64 lanes (every lane ends with the same bits);
 *   err: thread t starts from 0.0 and adds |p'[i] - p[i]| for i = t, t + T, t + 2T, ... ascending; the same butterfly over each wave's
 *     64 threads; then wave 0's sum plus wave 1's, ..., plus wave 15's, in that order.
 * Candidates are the nodes outside S, ordered by (p descending, node ascending); the first n_add go to node_out (int32) and score_out
 * (fp64), both [n_units][n_add], padded with -1 and NaN (both NULL: no ranking is made).  p_out (NULL or [n_units][n]) receives the whole
 * vector.  An empty unit has iters = 0, -1 and NaN everywhere and a NaN row of p_out.  Every output is a function of (CSR, unit,
 * parameters) alone: the same bits between runs, at every position of the table and beside any other units.
 * n in [2, 20000]: q is 8 n bytes of LDS, 160,000 of the 163,840 a workgroup may declare (p stays in registers, at most 20 per thread);
 * n_units >= 1, 1 <= max_size <= 4096, max_deg >= 1, 0 < restart < 1, tol >= 0 (not NaN), max_iter >= 1, 1 <= n_add <= 1024,
 * n_units * max(max_size, n_add, n) < 2^40.  Refused by name (GSS_EINVAL): a null pointer (but p_out, or the two rankings), any of
 * these bounds, an empty row, and a unit that breaks the table's contract or a row longer than max_deg -- found on the device, defined
 * and worded in csrc/seed_units.h (no row of such a unit is walked; the outputs are then undefined).  GSS_ENOTCONV, after every output
 * is written with the last iterates: with tol > 0 some unit ran max_iter iterations without err < tol; the message counts them.
 * Synchronises the stream.
 *
 * gss_rwr_null_stats: p [n_sets][R][n] is gss_rwr_rank's p_out of a set table (nodes [n_sets][R][max_size], sizes [n_sets][R]) whose
 * sample 0 is the set itself and samples 1 .. R - 1 its random sets.  Per (set, node), over k = 1 .. R - 1 in ascending order, all
 * single fp64 operations: sum = 0.0 + p_1 + p_2 + ...; mean = sum / (R - 1); sq = 0.0 + d_1 d_1 + d_2 d_2 + ..., d_k = p_k - mean;
 * sd = sqrt(sq / (R - 1)) (the population's); z = (p_0 - mean) / sd, 0 where sd = 0; ge (int32) = #{k >= 1: p_k >= p_0}.  The seeds
 * of sample 0 have z = NaN and are no candidates.  node_out [n_sets][n_add]: the candidates by (p_0 descending, node ascending) with
 * rank_by = 0, by (z descending, p_0 descending, node ascending) with rank_by = 1, padded with -1: the selection of gss_rwr_rank.  A set
 * whose sample 0 is empty has NaN, ge = -1 and node_out = -1 everywhere.  mean, sd, z, ge: [n_sets][n], device.  Only sample 0's rows
 * of the table are read.  The same bits for any split of the sets into calls.  n in [2, 20000], 1 <= n_sets <= 65535, 3 <= R <= 2^20,
 * 1 <= max_size <= 4096, 1 <= n_add <= 1024; refused by name (GSS_EINVAL) beside a null pointer and what seed_units.h names of sample 0.
 * Synchronises the stream. */
int gss_rwr_rank(int32_t n, const int32_t *rowptr, const int32_t *col, int32_t max_deg, int64_t n_units, int32_t max_size,
                 const int32_t *nodes, const int32_t *sizes, double restart, double tol, int32_t max_iter, int32_t n_add,
                 int32_t *node_out /* NULL or [n_units][n_add] */, double *score_out /* as node_out */, int32_t *iters_out,
                 double *p_out /* NULL or [n_units][n] */, void *stream);
int gss_rwr_null_stats(int32_t n, int32_t n_sets, int32_t R, const double *p, int32_t max_size, const int32_t *nodes,
                       const int32_t *sizes, int32_t n_add, int32_t rank_by, double *mean, double *sd, double *z, int32_t *ge,
                       int32_t *node_out, void *stream);

/* ---- shortest-path trees toward up to 64 targets per pass (predict_drug.py:268-273, run_covid.py:310-319: one networkx
 * shortest_path per table row; here one search toward each target answers every row) ------------------------------------------
 * Directed graph as a CSR: rowptr [n + 1], col [nnz], the columns of every row ascending (MsiGraph.to_csr, embio's edgelist reader).
 * gss_paths_create: on_device = 0 uploads host rowptr / col into the handle, 1 borrows device pointers (they must outlive it).
 * Validates the CSR on the device (GSS_EINVAL by name: a bad row pointer, a column out of range, a row not ascending) and
 * allocates 24 n bytes of state.  max_bytes bounds one pass (below); synchronises the stream.
 * gss_paths_run: targets t[0..q) (HOST int32, 1 <= q <= 64, any node index, repeats allowed) -> per target i, device
 *   dist [q][n] uint8: hop count of the shortest directed path v -> t_i, 255 = unreachable;
 *   next [q][n] int32: the first hop of that path, -1 at t_i and wherever v cannot reach t_i.
 * Tie rule (the contract): next is the successor with the smallest node index that is one hop closer, so following next spells a
 * shortest path v -> t_i in the direction of nx.shortest_path(G, source=v, target=t_i).  Bitwise deterministic.  Level-synchronous
 * and bottom-up (one launch per level, the host reads a "changed" word after each: the call synchronises the stream per level).
 * levels (may be NULL): the number of levels that found something = the largest finite dist.  Refuses (GSS_EINVAL, by name) q out
 * of range, a target out of range, a pass above the budget (5 q n bytes of output + 24 n of state > max_bytes) and a graph where
 * some node lies 255 or more hops from a target. */
typedef struct gss_paths gss_paths;
int gss_paths_create(gss_paths **out, int32_t n, int64_t nnz, const int32_t *rowptr, const int32_t *col, int32_t on_device,
                     int64_t max_bytes, void *stream);
int gss_paths_run(gss_paths *p, int32_t q, const int32_t *targets, uint8_t *dist, int32_t *next, int32_t *levels, void *stream);
void gss_paths_destroy(gss_paths *p);

/* ---- what lies between a source and a target besides one shortest path (interpret.py; csrc/trace.hip) -----------------------------------
 * gss_paths_count: for the pass of gss_paths_run on the same handle with the same targets (HOST int32, 1 <= q <= 64), its device
 * dist [q][n] and its levels, -> device
 *   sigma [q][n] fp64: the number of distinct shortest paths v -> t_i: 1 at t_i, the sum of sigma over the successors u of v with
 *     dist[u] = dist[v] - 1, 0 where t_i is unreachable.  Exact integers: a pass in which a count would exceed 2^53 is refused, naming
 *     the target and the node, so the order of the sum cannot matter;
 *   and with device weights w [q][n] fp64 (NULL: best and best_next are NULL too), finite,
 *   best_next [q][n] int32: among the successors one hop closer the one with the largest best, the smallest index on equal values; -1
 *     at t_i and where t_i is unreachable;
 *   best [q][n] fp64: w[v] + best[best_next[v]], 0 at t_i and where unreachable: the largest sum of node weights (t_i excluded) over
 *     the shortest paths v -> t_i, summed from the target outward, one addition per node.
 * One launch per level 1 .. levels, enqueued back to back with no read-back between them; one status word is read after the last (the
 * call synchronises the stream once).  Bitwise deterministic.  Refuses (GSS_EINVAL, by name): a null argument, q outside 1..64, levels
 * outside 0..254 or smaller than a finite distance in dist (node and target named), a dist that is not 0 exactly at the targets, a
 * weight that is not finite (target and node named), a row that holds a column twice (row named), a count above 2^53 (target and node
 * named), and a pass above the handle's budget: (1 + 4 + 8) q n bytes (dist, next, sigma), with weights (1 + 4 + 8 + 8 + 4 + 8) q n,
 * beside the 24 n of state.  "From a source" is the same call on a handle made of the transposed CSR.
 * gss_paths_between: one pass of sources (HOST indices s[0..ns), ns <= 64; device dist_s / sigma_s [ns][n] = gss_paths_run /
 * gss_paths_count toward the sources on the TRANSPOSED graph, i.e. hops and path counts s -> v) and one pass of targets (HOST
 * t[0..nt), nt <= 64; device dist_t / sigma_t [nt][n]) -> device, per pair (i, j) at [i * nt + j],
 *   pair_len int32: D = dist_t[j][s_i], -1 when s_i cannot reach t_j;  pair_paths fp64: sigma_t[j][s_i] (0 when unreachable);
 *   pair_nodes int32: the number of nodes v with dist_s[i][v] + dist_t[j][v] = D (both finite; the two end points are counted);
 *   and (med_sum, med_count both or neither) ADDS to med_sum [nt][n] fp64, for every v not in {s_i, t_j} on a shortest path of a
 *   reachable pair, share = (sigma_s[i][v] * sigma_t[j][v]) / sigma_t[j][s_i] (one multiply, one divide), over i in list order, and to
 *   med_count [nt][n] int32 the number of sources that contributed.  The caller zeroes both before the first pass of sources; a later
 *   pass continues them, so the sum has the order of the source list however it is cut into passes.  Does not synchronise.
 * gss_paths_between_fill: for n_pairs chosen pairs (device pairs [n_pairs][2] int32: source and target position in the pass) and device
 * offset [n_pairs + 1] int64 (the exclusive scan of their pair_nodes) writes, at offset[p] .. offset[p + 1], the nodes on the shortest
 * paths of pair p in ascending node index: node int32, hops_from / hops_to uint8, paths_from fp64 (sigma_s), through fp64 (sigma_s * sigma_t), share fp64
 * (through / sigma_t[j][s_i]).  Nothing is written at or beyond `capacity` entries or for a pair outside the pass.  Does not synchronise. */
int gss_paths_count(gss_paths *p, int32_t q, const int32_t *targets, const uint8_t *dist, int32_t levels, const double *w, double *sigma,
                    double *best, int32_t *best_next, void *stream);
int gss_paths_between(int32_t n, int32_t ns, const int32_t *sources, const uint8_t *dist_s, const double *sigma_s, int32_t nt,
                      const int32_t *targets, const uint8_t *dist_t, const double *sigma_t, int32_t *pair_len, double *pair_paths,
                      int32_t *pair_nodes, double *med_sum, int32_t *med_count, void *stream);
int gss_paths_between_fill(int32_t n, int32_t ns, const int32_t *sources, const uint8_t *dist_s, const double *sigma_s, int32_t nt,
                           const int32_t *targets, const uint8_t *dist_t, const double *sigma_t, int32_t n_pairs, const int32_t *pairs,
                           const int64_t *offset, int64_t capacity, int32_t *node, uint8_t *hops_from, uint8_t *hops_to, double *paths_from,
                           double *through, double *share, void *stream);

/* ---- ROC-AUC per query row (evaluate_auc.py:156-170: roc_auc_score of every drug's score against the drugs listed for an indication)
 * gss_auc_rows: device fp64 scores [R][ld] (row r: the C candidates' scores for query r), the positives of row r in device CSR form,
 * pos_col[pos_ptr[r] .. pos_ptr[r + 1]) (column indices, any order) -> device auc [R] fp64, n_pos [R], n_neg [R] int32.
 * auc = sklearn.metrics.roc_auc_score with average ranks for ties: sum over tie groups of pos_g (neg_below + neg_g / 2) / (P N), the
 * counts kept in integers (so it depends only on the multiset of (score, label) pairs, not on their order), one rounding at the end;
 * -0.0 and +0.0 are one tie group.  A row with P = 0 or N = 0 gets auc = NaN and its counts.  One workgroup per row sorts the row's
 * keys in LDS, so 1 <= C <= 16384.  Bitwise deterministic (no atomics on results).  Synchronises the stream: refuses (GSS_EINVAL, by
 * row and column in gss_last_error) C above the limit, ld < C, a NaN or infinite score, a pos_col outside [0, C) or repeated within
 * its row, and a pos_ptr that is not a row pointer (0 first, non-decreasing, at most C per row); the outputs are then unspecified. */
int gss_auc_rows(int32_t R, int32_t C, const double *scores, int64_t ld, const int32_t *pos_ptr, const int32_t *pos_col, double *auc,
                 int32_t *n_pos, int32_t *n_neg, void *stream);

/* ---- ROC-AUC, average precision and hits@k per query row: the three ranking statistics of drug-indication prediction
 * gss_rank_metrics_rows: scores, pos_ptr and pos_col as gss_auc_rows takes them; h_ks: nk cut-offs on the HOST, 0 <= nk <= 8, every
 * k >= 1 -> device auc [R], ap [R], hits [R][nk] fp64, n_pos [R], n_neg [R] int32.  A row has P positives and N negatives; scores compare
 * as in gss_auc_rows (-0.0 and +0.0 are one value) and a tie group is a maximal set of equal scores.
 *   auc   the bits gss_auc_rows writes for the row (the same integer counts, one division).
 *   ap    sklearn.metrics.average_precision_score: (1 / P) sum over the tie groups g that hold a positive, in descending score, of
 *         pos_g TP_g / (TP_g + FP_g), TP_g / FP_g the positives / negatives down to and including g.  Each term is an exact integer
 *         product and one division; the terms are added in an order fixed by the sorted scores.
 *   hits  the expected number of positives among the top k' = min(k, C) when ties are broken uniformly at random: with the group that
 *         holds rank k' having `above` items strictly before it (A of them positive), g items and pos_g positives, slots = k' - above,
 *         hits = A + pos_g if slots == g, else fl(A + fl((pos_g slots) / g)).  recall@k = hits / P is the caller's division.
 * A row with P = 0 or N = 0 gets NaN in auc, ap and every hits word, and its counts.  Every output depends only on the row's multiset
 * of (score, label) pairs: permuting the columns or a row's pos_col entries changes no bit, and no result goes through an atomic.
 * One workgroup per row sorts the positives' keys in LDS, parks them in `workspace` (device, 8-byte aligned, at least
 * gss_rank_metrics_workspace_bytes(R, C) = 8 R C bytes; nothing is allocated inside) and sorts the negatives' keys in the same LDS, so
 * 1 <= C <= 16384 with any P.  Synchronises the stream and refuses what gss_auc_rows refuses, in its words behind "rank_metrics_rows:",
 * and also nk outside 0..8, a cut-off below 1 and a workspace that is too small; the outputs are then unspecified. */
size_t gss_rank_metrics_workspace_bytes(int32_t R, int32_t C);
int gss_rank_metrics_rows(int32_t R, int32_t C, const double *scores, int64_t ld, const int32_t *pos_ptr, const int32_t *pos_col, int32_t nk,
                          const int32_t *h_ks, double *auc, double *ap, double *hits, int32_t *n_pos, int32_t *n_neg, void *workspace,
                          size_t workspace_bytes, void *stream);

/* ---- the same three statistics per stratum of a row: which kinds of drugs a method ranks well (evaluate_auc.py --by-class: AUROC, AP and
 * recall@50 by ATC drug class, as the multiscale-interactome work breaks them down)
 * gss_rank_metrics_strata: scores, pos_ptr, pos_col, h_ks as gss_rank_metrics_rows takes them; S strata, row r owning strata
 * str_ptr[r] .. str_ptr[r + 1] (device int32 [R + 1], a row pointer over [0, S]); stratum s has the positives Q_s =
 * sub_col[sub_ptr[s] .. sub_ptr[s + 1]) (device int32 [S + 1] and [sub_ptr[S]]: columns, any order), a subset of its row's positives P_r;
 * strata of a row may overlap -> device auc [S], ap [S], hits [S][nk] fp64, s_pos [S], s_neg [S], n_pos [R], n_neg [R] int32.
 * Stratum s is the sub-problem whose candidates are the row's N negatives and Q_s, C_s = N + |Q_s| columns: the row's other positives are
 * neither positive nor negative.  Its auc, ap and hits (at k' = min(k, C_s)) are what gss_rank_metrics_rows defines on those candidates,
 * and every output word is bit for bit the word gss_rank_metrics_rows writes for that sub-problem gathered into a row of its own; a
 * stratum with all of the row's positives has the row's words.  |Q_s| = 0 or N = 0 gives NaN in auc, ap and every hits word.
 * s_pos[s] = |Q_s|, s_neg[s] = N; n_pos and n_neg as gss_rank_metrics_rows writes them.  Permuting a stratum's sub_col entries, a row's
 * strata or the columns changes no bit of any stratum, and no result goes through an atomic.
 * One workgroup per row checks and sorts each stratum's keys in LDS, parks them at workspace[sub_ptr[s] ..) (device, 8-byte aligned, at
 * least gss_rank_strata_workspace_bytes(sub_ptr[S]) = 8 sub_ptr[S] bytes; nothing is allocated inside), sorts the row's negatives once in
 * the same LDS and serves every stratum by binary search, so 1 <= C <= 16384 with any |Q_s|.  Synchronises the stream and refuses
 * (GSS_EINVAL, by name behind "rank_metrics_strata:") what gss_rank_metrics_rows refuses, S < 0, a str_ptr that is not a row pointer over
 * [0, S] (0 first, non-decreasing, S last), a sub_ptr that is not one over the strata (0 first, non-decreasing, at most P_r per stratum;
 * row and stratum named), a sub_col that is not a positive of its row or is repeated within its stratum (row, stratum and column named),
 * and a workspace that is too small or misaligned; the outputs are then unspecified.  R = 0 or S = 0 succeeds and reads nothing. */
size_t gss_rank_strata_workspace_bytes(int64_t n_sub);
int gss_rank_metrics_strata(int32_t R, int32_t C, const double *scores, int64_t ld, const int32_t *pos_ptr, const int32_t *pos_col, int32_t S,
                            const int32_t *str_ptr, const int32_t *sub_ptr, const int32_t *sub_col, int32_t nk, const int32_t *h_ks, double *auc,
                            double *ap, double *hits, int32_t *s_pos, int32_t *s_neg, int32_t *n_pos, int32_t *n_neg, void *workspace,
                            size_t workspace_bytes, void *stream);

/* ---- pairwise distances between diffusion profiles (multiscale/README.md, overview (c): "by comparing the diffusion profiles of a drug and
 * a disease ...")
 * gss_profile_dist: device fp64 x [n][ld], profile c = column c (the layout gss_ppr_run writes, so profiles go from the power iteration into
 * the comparison without leaving the device); device int32 column lists cols_a [na], cols_b [nb], honoured as given (any order, repeats
 * allowed; null = columns 0 .. na - 1 / 0 .. nb - 1; an ascending contiguous list costs what null costs)
 * -> device fp64 out [na][ld_out], out[i][j] = dist(x[:, cols_a[i]], x[:, cols_b[j]]) as scipy.spatial.distance.cdist defines it:
 *   GSS_DIST_CITYBLOCK   sum |a - b|
 *   GSS_DIST_EUCLIDEAN   sqrt(sum (a - b)^2), from the differences
 *   GSS_DIST_CANBERRA    sum |a - b| / (|a| + |b|); a term with a = b = 0 contributes 0
 *   GSS_DIST_COSINE      1 - a.b / (|a| |b|), the quotient clipped to [-1, 1]; a zero vector gives NaN for its whole row / column
 *   GSS_DIST_CORRELATION the cosine distance of the two vectors after each has its mean subtracted (two passes: the mean first, then the
 *                        centred values enter the product and the norm); a constant vector gives NaN
 * The NaN of a degenerate vector is a value, not an error.  Every output sums the n rows in an order that depends on n alone, without
 * atomics: bitwise deterministic, out(a, b) and out(b, a) are bit-equal, a pair has the same bits alone and inside a larger call, and
 * cityblock / euclidean / canberra of a column with itself is exactly 0.0.  Tails in n, na and nb are handled here; na = 0 or nb = 0 is a
 * no-op.  Refuses (GSS_EINVAL, by name in gss_last_error): a null x or out, n < 1, a negative or too large na / nb, an unknown metric,
 * ld < 1, ld below na / nb where that list is null, ld_out < nb, and a list entry outside [0, ld) (by list, position and value; nothing
 * has read x through the list by then).  The scratch (two status words, a mean and a norm per listed column) is allocated and freed
 * inside the call.  Synchronises the stream, except for cityblock / euclidean / canberra with both lists null, which only enqueue. */
#define GSS_DIST_CITYBLOCK 0
#define GSS_DIST_EUCLIDEAN 1
#define GSS_DIST_CANBERRA 2
#define GSS_DIST_COSINE 3
#define GSS_DIST_CORRELATION 4
int gss_profile_dist(int32_t n, const double *x, int64_t ld, int32_t na, const int32_t *cols_a, int32_t nb, const int32_t *cols_b,
                     int32_t metric, double *out, int64_t ld_out, void *stream);

/* gss_profile_dist_pairs: the same x and the same five metrics for T listed pairs instead of a matrix: device int32 col_a [T], col_b [T]
 * -> device fp64 out [T], out[t] = dist(x[:, col_a[t]], x[:, col_b[t]]), with the definitions above (NaN of a zero / constant vector,
 * Canberra's 0 / 0 term = 0, correlation in two passes: the means first).  A screen that needs T distances pays for T, not for T x T.
 * A bandwidth kernel: a wave owns 32 rows and sweeps the pair list, lane = pair, so the reads of one row coalesce where the listed columns
 * are neighbours in x, and a pair whose two columns share an aligned 16 bytes (columns 2 j and 2 j + 1 in either order, ld even, x 16-byte
 * aligned) takes both with one load.  Partial sums go to [row blocks][T] in the workspace and are added in block order, without atomics.  The
 * order of every sum depends on n alone: two runs are bit-equal, permuting the pair list permutes out bit for bit, a pair has the same bits
 * alone and inside a longer list, out(a, b) == out(b, a) bit for bit, and cityblock / euclidean / canberra of a column with itself is
 * exactly 0.0.  The bits are not those of gss_profile_dist, which sums in another order.
 * workspace: device, 8-byte aligned, at least gss_profile_dist_pairs_workspace_bytes(n, T) bytes (0 for n < 1 or T < 0); nothing is
 * allocated inside.  T = 0 is a no-op.  Refuses (GSS_EINVAL, by name in gss_last_error): n < 1, T < 0 or above 2^21, an unknown metric,
 * ld < 1, a null x, col_a, col_b, out or workspace, a workspace that is misaligned or too small, and a list entry outside [0, ld) (by
 * list, position and value; nothing has read x through the lists by then, and out is untouched).  Synchronises the stream once, for that
 * check; the distances are then enqueued. */
size_t gss_profile_dist_pairs_workspace_bytes(int32_t n, int32_t T);
int gss_profile_dist_pairs(int32_t n, const double *x, int64_t ld, int32_t T, const int32_t *col_a, const int32_t *col_b, int32_t metric,
                           double *out, void *workspace, size_t workspace_bytes, void *stream);

/* gss_profile_rank: exact average-tie ranks of listed columns of the profile matrix -- the transform behind the "spearman" profile distance
 * (Spearman's rho is the Pearson correlation of the ranks: rank the columns here, then gss_profile_dist with GSS_DIST_CORRELATION on r; there
 * is no metric id for it).  x: device fp64 [n][ld], profile c = column c (what gss_ppr_run writes and gss_profile_dist reads); cols: device
 * int32 [nc], honoured as given (any order, repeats allowed; null = columns 0 .. nc - 1) -> r: device fp64 [n][ld_r], for j < nc
 *   r[:, j] = scipy.stats.rankdata(x[:, cols[j]], method="average")
 * EXACTLY: a rank is (2 below + tied + 1) / 2 with integer counts, so every output is an integer or a half-integer.  Columns j >= nc of r are
 * not touched.  r and x must not overlap (not checked).  Order is that of IEEE comparison, as numpy sorts: -0.0 and +0.0 are one value,
 * +-inf are ordinary extremes, subnormals are distinct values.  A listed column that holds a NaN comes out NaN in all n entries (scipy's
 * nan_policy="propagate"): a value, not an error.  The counts are integers and every output word has one owner thread: a column's bits do
 * not depend on nc, on its place in the list, on the grid or on an earlier call; nothing goes through an atomic.
 * Kernel: per panel of 512 listed columns, a transposing pass writes order-preserving uint64 keys [panel][n]; one workgroup per column sorts
 * the column in LDS in chunks of 16,384 keys and lets every key count, by two binary searches per chunk, the keys below it and tied with it
 * into an int32 word; a second transposing pass writes (count + 1) / 2.  The work is quadratic in n / 16,384, hence the limit on n.
 * workspace: the caller's, device, 8-byte aligned, at least gss_profile_rank_workspace_bytes(n, nc) bytes, which depends on (n, nc) only:
 *   256 + p n 8 + round8(p n 4) + round8(p 4)   with p = min(nc, 512), round8 = up to a multiple of 8   (0 for n < 1 or nc < 0)
 * Nothing is allocated inside.  nc = 0 is a no-op.  Refuses (GSS_EINVAL, by name in gss_last_error, before anything reads x through the list
 * and with r untouched): n < 1, n above 2^24, nc < 0, ld < 1, ld_r < nc, and with nc > 0 a null x, r or workspace, ld below nc where cols is
 * null, a misaligned or too small workspace (naming the needed size), and a list entry outside [0, ld) (by position and value: a check
 * launch of its own and one synchronisation of the stream; a null list needs neither and the call then only enqueues). */
size_t gss_profile_rank_workspace_bytes(int32_t n, int32_t nc);
int gss_profile_rank(int32_t n, const double *x, int64_t ld, int32_t nc, const int32_t *cols, double *r, int64_t ld_r, void *workspace,
                     size_t workspace_bytes, void *stream);

/* gss_profile_topk: the k highest nodes of listed columns of the profile matrix, per node group -- "the proteins and biological functions" a
 * treatment's profile runs through (multiscale/README.md).  x: device fp64 [n][ld], profile c = column c; cols: device int32 [nc], honoured as
 * given (any order, repeats allowed; null = columns 0 .. nc - 1); group: device int32 [n], node i belongs to group[i] in [-1, G), -1 = never
 * selected (null = every node in group 0, and G must be 1) -> idx: device int32 [nc][G][k], val: device fp64 [nc][G][k], cnt: device int32
 * [nc][G].  For list position j (column c = cols[j]) and group g, with members = the nodes of g in ascending index:
 *   idx[j][g][:cnt] = members[np.argsort(-x[members, c], kind="stable")[:k]],  cnt[j][g] = min(k, len(members)),  val = x[idx, c] bit for bit
 * EXACTLY: descending value, ties by the smaller node index; -0.0 and +0.0 tie, +-inf are ordinary extremes, subnormals distinct values.
 * Slots from cnt on hold idx = -1 and val = NaN.  A NaN among the group's own nodes in that column flags (j, g): cnt = -1, every idx = -1,
 * every val = NaN; a NaN at a node of another group or of group -1 changes nothing.  The output of a (column, group) depends on that column's
 * values and on group alone -- not on the list, the position in it, nc, ld or the other columns, bit for bit; every output word has one owner,
 * the only atomics are integer counters in LDS.
 * Kernel: per panel of 512 listed columns a transposing pass writes order-preserving uint64 keys [panel][n] (rank_keys.h); one workgroup
 * per column then runs, for all G groups at once, an exact radix select (8-bit digits from the top, LDS histograms; a group stops as soon
 * as its bucket is taken whole; ties at the k-th key are resolved by up to three more digit passes over the node index), collects the
 * selected (key, index) pairs, bitonic-sorts them in LDS and reads the values back from x.
 * workspace: the caller's, device, 8-byte aligned, at least gss_profile_topk_workspace_bytes(n, nc, G, k) = 256 + min(nc, 512) n 8 bytes
 * (0 for arguments outside the limits).  Nothing is allocated inside.  nc = 0 is a no-op.  Refuses (GSS_EINVAL, by name in gss_last_error,
 * outputs untouched): n outside [1, 2^24], k outside [1, 1024], G outside [1, 8], nc < 0, ld < 1, and with nc > 0 a null x, idx, val, cnt or
 * workspace, a null group with G != 1, ld below nc where cols is null, a misaligned or too small workspace (naming the needed size), a cols
 * entry outside [0, ld) and a group entry outside [-1, G) (by position and value: one check launch and one synchronisation of the stream,
 * only where cols or group is given). */
size_t gss_profile_topk_workspace_bytes(int32_t n, int32_t nc, int32_t G, int32_t k);
int gss_profile_topk(int32_t n, const double *x, int64_t ld, int32_t nc, const int32_t *cols, int32_t G, const int32_t *group, int32_t k,
                     int32_t *idx, double *val, int32_t *cnt, void *workspace, size_t workspace_bytes, void *stream);

/* gss_topk_overlap: how many nodes two selections share, per group.  idx [S][G][k], cnt [S][G]: gss_profile_topk's outputs for S
 * selections; a, b: device int32 [T], selection numbers in [0, S) -> shared: device int32 [T][G], shared[t][g] = the number of node indices
 * in both idx[a[t]][g][:cnt] and idx[b[t]][g][:cnt] (len(np.intersect1d(...))), or -1 where either side has cnt = -1.  Pairs may repeat; an
 * entry depends on its own pair only.  One workgroup per (t, g): side a sorted in LDS, side b searched in it.  T = 0 is a no-op.  Refuses
 * (GSS_EINVAL, by name): S < 1, T < 0, k outside [1, 1024], G outside [1, 8], a null idx, cnt, a, b or shared, and an a or b entry outside
 * [0, S) (by list, position and value; a status word is allocated and freed inside, and the stream is synchronised once); shared is then
 * untouched. */
int gss_topk_overlap(int32_t S, int32_t G, int32_t k, const int32_t *idx, const int32_t *cnt, int32_t T, const int32_t *a, const int32_t *b,
                     int32_t *shared, void *stream);

/* ---- preranked gene-set enrichment of profile columns: does a set of nodes as a whole sit higher in a profile than random sets of its size
 * (enrich.py; the running sum of Subramanian et al. 2005 with a gene-set permutation null; the reference ships
 * data/protein_to_functional_pathway.tsv and no code that scores a set)
 * universe: device int32 [M], strictly ascending node indices in [0, n), 2 <= M <= 65,536; a "place" u in [0, M) is an index into it.
 * gss_profile_order: x: device fp64 [n][ld], profile c = column c; cols: device int32 [nc], honoured as given (any order, repeats allowed;
 * null = columns 0 .. nc - 1) -> pos_out: device int32 [nc][M], w_out: device fp64 [nc][M].  For list position j (column c = cols[j]):
 *   pos_out[j][u] = the place of u in np.argsort(-x[universe, c], kind="stable"),   w_out[j][u] = |x[universe[u], c]|
 * EXACTLY: descending value, ties by the smaller place, under IEEE comparison as in gss_profile_topk (-0.0 and +0.0 tie, +-inf are ordinary
 * extremes, subnormals distinct values).  A NaN at a universe node flags the column: every pos = -1 and every w = NaN; a NaN at a node
 * outside the universe changes nothing.  A column's output depends on that column's values at the universe alone, bit for bit.
 * Kernels: a key pass writes the descending keys ~order_key(x) (rank_keys.h) [nc][M] into the workspace and |x| into w_out; then one
 * workgroup per column sorts chunks of 4,096 (key, place) pairs in LDS and every place adds, per chunk, the number of pairs below its
 * own to its word of pos_out -- quadratic in M / 4,096, hence the limit on M.  No atomics; every output word has one owner.
 * workspace: the caller's, device, 8-byte aligned, at least gss_profile_order_workspace_bytes(M, nc) = 256 + nc M 8 bytes (0 for
 * arguments outside the limits).  Nothing is allocated inside.  nc = 0 checks the universe and writes nothing.  Refuses (GSS_EINVAL, by
 * name in gss_last_error, outputs untouched): n outside [1, 2^24], M outside [2, min(n, 65,536)], nc outside [0, 65,535], ld < 1, a null
 * universe or workspace, a misaligned or too small workspace (naming the needed size), with nc > 0 a null x, pos_out or w_out, a
 * misaligned pos_out or w_out, ld below nc where cols is null; a universe entry outside [0, n) or not above its predecessor and a cols
 * entry outside [0, ld) (by position and value: one check launch and one synchronisation of the stream each). */
size_t gss_profile_order_workspace_bytes(int32_t M, int32_t nc);
int gss_profile_order(int32_t n, const double *x, int64_t ld, int32_t nc, const int32_t *cols, int32_t M, const int32_t *universe, int32_t *pos_out,
                      double *w_out, void *workspace, size_t workspace_bytes, void *stream);
/* The enrichment score of a set S of s distinct places, 1 <= s <= min(1024, M - 1), in a column (pos, w) of gss_profile_order: the members
 * in ascending pos, p_0 < ... < p_{s-1}, with a_k = w of the k-th member (weighted) or 1.0 (unweighted); fp64, every operation rounded on
 * its own (no fused multiply-add):
 *   N = 0.0;  for k: N = N + a_k                         sequential, from +0.0;  N == 0.0: ES = NaN, peak = -1
 *   c = 0.0;  hi = -inf, khi = -1;  lo = +inf, klo = -1
 *   for k = 0 .. s - 1:  miss = (double)(p_k - k) / (double)(M - s);  l = c / N - miss;  c = c + a_k;  h = c / N - miss
 *                        if h > hi: hi = h, khi = k;   if l < lo: lo = l, klo = k
 *   ES = hi, peak = khi  if hi >= -lo,  else  ES = lo, peak = klo
 * -- the extreme of the running sum over all M places (a peak lies just after a hit, a trough just before one).  A flagged column gives
 * ES = NaN, peak = -1.  The bits of a (column, set) depend on the column and the set alone: not on the list's order, its position among the
 * lists, nc, the grid, an earlier call or the entry point.  Nothing is accumulated with atomics; every output word has one owner.
 * gss_enrich_lists: C sets in CSR form over places, device int32 ptr [C + 1] (ptr[0] = 0) and idx [ptr[C]]; weighted: 0 or 1 -> es_out:
 * device fp64 [nc][C], peak_out: device int32 [nc][C].  One workgroup per (set, column): the members' (pos, place) pairs are sorted in LDS
 * and one lane walks them.  C = 0 or nc = 0 is a no-op.  Refuses (GSS_EINVAL, by name, outputs untouched): M outside [2, 65,536], nc
 * outside [0, 65,535], weighted outside {0, 1}, C < 0, a null pos, w, ptr, idx, es_out or peak_out, a ptr that is no CSR row pointer, a
 * list of length 0, above 1024 or above M - 1 (by list), a place outside [0, M) or repeated within its list (by list, position and value:
 * the first list, a range before a repeat, the first such position resp. the second position of the least repeated place; one check
 * launch with a status word allocated and freed inside).  Reads ptr back and synchronises the stream. */
int gss_enrich_lists(int32_t M, int32_t nc, const int32_t *pos, const double *w, int32_t weighted, int32_t C, const int32_t *ptr, const int32_t *idx,
                     double *es_out, int32_t *peak_out, void *stream);
/* gss_enrich_random: the same score over random sets.  For sample s = s0 .. s0 + P - 1: key_i = rng_key(seed, kRngEnrichPerm = 13, s, i, 0)
 * (csrc/counter_rng.h) for the places i in [0, M), pi_s = the places sorted by (key, i) ascending -- a pure function of (seed, s, M),
 * replayable in numpy (tests/enrich_mirror.py) -- and es_out[j][s - s0][k] = ES of the set pi_s[0 : sizes[k]] in column j: one permutation
 * serves every size and every column.  sizes: device int32 [n_sizes], strictly ascending in [1, min(1024, M - 1)]; es_out: device fp64
 * [nc][P][n_sizes]; perm_out: null, or device int32 [P][sizes[n_sizes - 1]], the prefix of pi_s.  One workgroup per sample: the kmax =
 * sizes[n_sizes - 1] smallest keys are an exact selection -- the keys at or under a threshold are collected in LDS (the first threshold is
 * floor(2^64 (kmax + kmax / 4 + 8) / M), every key where M <= 2048), the threshold is bisected while fewer than kmax or more than 2,048
 * came, and the collected (key, i) pairs are sorted: the result does not depend on the thresholds tried.  Per column the prefix is sorted
 * once by pos, each member keeping its rank rho in pi_s; size m is the subsequence with rho < m, walked by one lane per size in exactly the
 * order of the definition: the bits of (column, sample, size) equal gss_enrich_lists on pi_s[0 : m].  Samples are numbered, not drawn: a
 * call over [s0, s0 + P) equals the same samples in any split.  Refuses (GSS_EINVAL, by name, outputs untouched): M outside [2, 65,536],
 * nc < 0, weighted outside {0, 1}, P < 1, s0 < 0 or s0 + P > 2^31, n_sizes outside [1, min(1024, M - 1)], a null sizes, with nc > 0 a
 * null pos, w or es_out, a size outside [1, min(1024, M - 1)] or not above its predecessor.  Reads sizes back and synchronises the stream. */
int gss_enrich_random(int32_t M, int32_t nc, const int32_t *pos, const double *w, int32_t weighted, uint64_t seed, int64_t s0, int32_t P,
                      int32_t n_sizes, const int32_t *sizes, double *es_out, int32_t *perm_out, void *stream);

/* ---- sums of a symmetric distance matrix over the pairs of a set: the coherence of a drug class and its null (drug_classes.py; the reference
 * ships data/drug_classification_df.tsv, multiscale/README.md dataset 7, and has no code that reads it)
 * d: device fp64 [n][ld], ld >= n, assumed symmetric (diffusion.compare_profiles' drug x drug matrix is, bit for bit); only d[a][b] with a
 * later in its list than b is read.  For an ordered list a[0 .. m):
 *   r_j  = sum over i < j of d[a[j]][a[i]]: the 64 partial sums p[l] = the terms i = l, l + 64, l + 128 ... (ascending, from +0.0), combined
 *          by the butterfly p[l] = p[l] + p[l ^ o] for o = 32, 16, 8, 4, 2, 1 -- an order that depends on j alone;
 *   T(m) = r_1 + r_2 + ... + r_{m-1}, added in that order (T(2) = r_1).
 * T is a function of the ordered list and d only: bit-equal run to run, under any grid, whatever other lists, samples or sizes the call
 * carries, and between the two entry points.  Nothing is accumulated with atomics.
 * gss_pair_sums_lists: C lists in CSR form, device int32 ptr [C + 1] (ptr[0] = 0, non-decreasing) and idx [ptr[C]] with entries in [0, n),
 * honoured as given (any order, repeats allowed, any length) -> device fp64 sum_out [C], sum_out[c] = T(length) of list c; a list shorter
 * than 2 gives 0.0.  One workgroup per list.  C = 0 is a no-op.  Refuses (GSS_EINVAL, by name): n < 1, a null d, ptr, sum_out or (with an
 * entry to read) idx, ld < n, C < 0, a ptr that is no CSR row pointer, and an idx entry outside [0, n) (by position and value: one check
 * launch, before anything reads d through the list); sum_out is then untouched.  Reads ptr back and synchronises the stream. */
int gss_pair_sums_lists(int32_t n, const double *d, int64_t ld, int32_t C, const int32_t *ptr, const int32_t *idx, double *sum_out, void *stream);
/* gss_pair_sums_random: the same sums over random sets.  For sample s = s0 .. s0 + P - 1: key_i = rng_key(seed, kRngClassPerm = 9, s, i, 0)
 * (csrc/counter_rng.h) for i in [0, n), pi_s = 0 .. n - 1 sorted by (key, i) ascending -- a pure function of (seed, s, n), replayable in numpy
 * (tests/class_cohesion_mirror.py) -- and sums_out[s - s0][k] = T(sizes[k]) of pi_s: the first m places of a uniformly random permutation are
 * a uniformly random m-subset for every m, so one permutation serves every size.  sizes: device int32 [n_sizes], strictly ascending in
 * [2, n]; sums_out: device fp64 [P][n_sizes]; perm_out: null, or device int32 [P][sizes[n_sizes - 1]], the prefix of pi_s.  One workgroup per
 * sample; the permutation is sorted in LDS, hence n <= 4096.  Samples are numbered, not drawn: a call over [s0, s0 + P) equals the same
 * samples in any split.  Refuses (GSS_EINVAL, by name): n outside [2, 4096], a null d, sizes or sums_out, ld < n, P < 1, s0 < 0 or
 * s0 + P > 2^31, n_sizes outside [1, n - 1], a size outside [2, n] or not above its predecessor; the outputs are then untouched.  Reads
 * sizes back and synchronises the stream. */
int gss_pair_sums_random(int32_t n, const double *d, int64_t ld, uint64_t seed, int64_t s0, int32_t P, int32_t n_sizes, const int32_t *sizes,
                         double *sums_out, int32_t *perm_out, void *stream);

/* ---- the cross-product sum of two symmetric matrices under seeded relabellings of one: the statistic and the null of Mantel's test between
 * two drug x drug matrices (mantel.py, drug_signatures.py; the reference ships data/bcm_df.tsv, multiscale/README.md dataset 8, and has no
 * code that reads it)
 * gss_matrix_cross_sums: a, b: device fp64 [n][lda], [n][ldb], lda, ldb >= n -> device fp64 out [count],
 *   out[s - first] = sum over 0 <= i < j < n of a[j][i] * b[pi_s(j)][pi_s(i)]      for the replicates s = first .. first + count - 1.
 *   mode 0 (plain)     pi = the identity: the observed statistic with the arithmetic of the null; only first = 0, count = 1;
 *   mode 1 (permuted)  key_i = rng_key(seed, kRngMantelPerm = 12, s, i, 0) (csrc/counter_rng.h) for i in [0, n), pi_s = 0 .. n - 1 sorted by
 *                      (key, i) ascending -- a pure function of (seed, s, n), replayable in numpy (tests/mantel_mirror.py).
 * a is read below its diagonal only; of b both triangles are read (pi_s(j) may be below pi_s(i)), so the sum is the one over unordered pairs
 * only when b is symmetric.  The order of the additions is fixed:
 *   r_j = the row sum over i < j: the 64 partial sums p[l] = the terms i = l, l + 64, l + 128 ... (ascending, from +0.0; a lane without a term
 *         keeps +0.0), every product rounded to fp64 on its own (no fused multiply-add), combined by the butterfly p[l] = p[l] + p[l ^ o] for
 *         o = 32, 16, 8, 4, 2, 1;
 *   T   = r_1 + r_2 + ... + r_{n-1}, added in that order (n = 2: T = r_1).
 * A replicate's bits are a function of (n, a, b, seed, s): the same run to run, in any split of the replicates through first / count, under
 * any grid, alone or among other replicates.  Nothing is accumulated with atomics.  perm_out: null, or device int32 [count][n], pi_s (mode 0:
 * the identity).  One workgroup per replicate; pi_s is sorted in LDS, hence n <= 4096.  count = 0 succeeds and reads nothing.  Neither
 * allocates nor synchronises.  Refuses (GSS_EINVAL, by name): n outside [2, 4096], lda or ldb < n, a mode outside 0..1, count < 0, mode 0
 * with anything but first = 0 and count = 1, first < 0 or first + count > 2^31, a null a, b or out; out is then untouched.  Values are not
 * inspected: a NaN or an infinity propagates into the sums it is a term of (mantel.py refuses NaN before the call). */
int gss_matrix_cross_sums(int32_t n, const double *a, int64_t lda, const double *b, int64_t ldb, int32_t mode, uint64_t seed, int64_t first,
                          int64_t count, double *out, int32_t *perm_out, void *stream);

/* ---- the mean and the median of resampled series: bootstrap intervals and sign-flip tests of the per-indication metrics (resample.py,
 * compare_methods.py, evaluate_auc.py --bootstrap; the reference prints point estimates only, evaluate_auc.py:170)
 * gss_resample_stats: v: S series of n fp64 values on the device, series s at v + s * ld, ld >= n -> device fp64 out [count][S][2]:
 * out[(r * S + s) * 2 + 0] the mean and + 1 the median of replicate b = first + r of series s.  The multiset of replicate b, series s:
 *   mode 0 (plain)      v[s][j], j < n: the observed statistic with the arithmetic of the nulls; only first = 0, count = 1;
 *   mode 1 (bootstrap)  v[s][idx(b, j)], j < n, idx(b, j) = ((rng_key(seed, kRngBootDraw = 10, b, j, 0) >> 32) * n) >> 32 in 64-bit integers
 *                       (csrc/counter_rng.h) -- the same places in every series, which is what pairs the series of a call;
 *   mode 2 (sign flip)  -v[s][j] if the top bit of rng_key(seed, kRngSignFlip = 11, b, j, 0) is set, else v[s][j] -- the same places flipped
 *                       in every series.
 * The multiset is sorted ascending through order-preserving keys (-0.0 folded into +0.0) to x_0 <= ... <= x_{n-1}.  median = x_{(n-1)/2}
 * for odd n, (x_{n/2-1} + x_{n/2}) * 0.5 for even n (np.median).  mean = T / n with T added in this order: the 256 partial sums
 * p_t = x_t + x_{t+256} + x_{t+512} + ... (ascending, from +0.0); per group of 64, W_w = the butterfly p_l = p_l + p_{l ^ o} for o = 32, 16, 8,
 * 4, 2, 1 over p_{64 w} .. p_{64 w + 63}; T = ((W_0 + W_1) + W_2) + W_3.  A replicate's bits are a function of (seed, mode, b, n, the series'
 * values): the same run to run, in any split of the replicates through first / count, alone or among other series, under any grid;
 * replayable in numpy (tests/resample_mirror.py).  Results are defined up to the sign of a zero.  Nothing is accumulated with atomics.  One
 * workgroup per replicate; a series is sorted in LDS, hence n <= 16384.  count = 0 succeeds and writes nothing.  Refuses (GSS_EINVAL, by
 * name): n outside [1, 16384], S < 1, ld < n, a mode outside 0..2, count < 0, mode 0 with anything but first = 0 and count = 1, first < 0
 * or first + count > 2^31, a null v or out, and a value that is not finite (by series and position: one check launch before anything is
 * resampled); out is then untouched.  Allocates 8 status bytes and synchronises the stream once, for that check. */
int gss_resample_stats(const double *v, int64_t ld, int32_t S, int32_t n, int32_t mode, uint64_t seed, int64_t first, int64_t count, double *out,
                       void *stream);

/* ---- inner-product scores between listed embedding rows (predict_drug.py:52-66: sklearn.preprocessing.normalize, then np.matmul)
 * gss_embedding_scores: device fp32 emb [n][ld], ld >= d (a plan's embedding tensor with its zero padding); device int32 index lists rows
 * [nr] and cols [nc], honoured as given (any order, repeats allowed) -> device fp64 out [nr][ld_out], out[i][j] = the inner product of
 * row rows[i] and row cols[j] of emb over the first d values.
 *   normalize = 1: every value is widened to fp64 and divided by its row's fp64 L2 norm (a zero norm divides by 1), and the product is
 *   taken after that -- the order of sklearn's normalize followed by np.matmul;  normalize = 0: the widened raw values (node2vec).
 * The order of every sum depends on d alone:
 *   norm   the 64 partial sums p[l] = sum of x[k]^2 over k = l, l + 64, l + 128 ... (ascending, from +0.0), combined by the butterfly
 *          p[l] = p[l] + p[l ^ m] for m = 32, 16, 8, 4, 2, 1; norm = sqrt(p[0]), correctly rounded;
 *   value  (double)x / norm, one correctly rounded division;
 *   dot    acc = +0.0; acc = acc + a[k] * b[k] for k = 0 .. d - 1, the product and the sum each rounded to fp64 (no fused multiply-add).
 * So an entry is bit-equal run to run, under any other choice of rows and cols, and with rows and cols swapped (out(a, b) == out(b, a));
 * nothing is accumulated with atomics.  Tails in d, nr and nc are handled here.  Refuses (GSS_EINVAL, by name in gss_last_error): a null
 * emb, rows, cols or out, n < 1, d < 1, ld < d, nr < 1 or nc < 1 (or above 2^21), ld_out < nc, normalize outside {0, 1}, and -- checked on
 * the device, one status word read at the end -- a list entry outside [0, n) (by list, position and value; no row is read through it) and a
 * NaN or infinite value in a listed row (by row of emb); out is then unspecified.  The scratch (the status word and the listed rows as
 * fp64) is allocated and freed inside the call.  Synchronises the stream. */
int gss_embedding_scores(int32_t n, int32_t d, const float *emb, int64_t ld, int32_t nr, const int32_t *rows, int32_t nc, const int32_t *cols,
                         int32_t normalize, double *out, int64_t ld_out, void *stream);

/* ---- a13  np.savetxt('graph_embs.txt', hidden_emb), train.py:193 (host-side; h_emb is a HOST pointer) ---------------------
 * Every value of the float32 matrix as Python prints it with '%.18e' after widening to double (exact decimal expansion, round
 * half to even -- byte-identical to np.savetxt's output), ' ' between the values of a row, '\n' after each row.  Rows are
 * formatted by `threads` host threads (0 = all cores) and written in order.  gss_format_e18: one value into a buffer of >= 26
 * bytes, returns its length (the unit the writer is tested by). */
int gss_write_embs_text(const char *path, const float *h_emb, int64_t n, int32_t d, int32_t threads);
int gss_format_e18(float value, char *out26);
/* ---- a14  the '.embs.txt' reader, train.py:79-80 (np.loadtxt(..., skiprows=1, dtype=object)[:, 1:].astype(float)) -----------
 * First line '<N> <d>' (multiscale/openne/node2vec.py:42), then '<node> v1 ... vd' per line; blank lines skipped.  Values are
 * parsed with strtod (correctly rounded: the doubles Python's float() gives) by `threads` host threads (0 = all cores).
 * gss_embs_copy: x_out HOST fp64 [rows][cols]; names_out: the node names joined by '\n' (gss_embs_names_bytes bytes);
 * header_n: the N of the header line or -1.  A ragged or non-numeric line makes gss_embs_open fail. */
typedef struct gss_embs_file gss_embs_file;
int gss_embs_open(gss_embs_file **out, const char *path, int32_t threads);
int64_t gss_embs_rows(const gss_embs_file *e);
int32_t gss_embs_cols(const gss_embs_file *e);
int64_t gss_embs_names_bytes(const gss_embs_file *e);
int gss_embs_copy(const gss_embs_file *e, double *x_out, char *names_out, int64_t names_cap, int64_t *header_n);
void gss_embs_close(gss_embs_file *e);

/* ---- a2  the weighted edgelist 'u v w' (nx.write_weighted_edgelist, predict_drug.py:224-226) as --adj-file reads it ----------
 * names: the node ids of the .embs.txt in row order, joined by '\n' (names_bytes bytes, n_names ids): every u / v is mapped to its
 * row.  Lines are parsed by `threads` host threads; a missing weight is 1.0; blank and '#' lines are skipped.
 * gss_edgelist_bad_line >= 0: the first line (0-based among the data lines) with an unknown node id or a malformed weight. */
typedef struct gss_edgelist_file gss_edgelist_file;
int gss_edgelist_open(gss_edgelist_file **out, const char *path, const char *names, int64_t names_bytes, int64_t n_names, int32_t threads);
int64_t gss_edgelist_edges(const gss_edgelist_file *e);
int64_t gss_edgelist_bad_line(const gss_edgelist_file *e);
int gss_edgelist_copy(const gss_edgelist_file *e, int32_t *src, int32_t *dst, double *w);
void gss_edgelist_close(gss_edgelist_file *e);

/* ---- whole training step (train.py:158-184) ---------------------------------------------------
 * A plan owns every activation/gradient buffer of one replica so that a step is ONE host call that
 * enqueues all kernels.  a / at: CSR(A_hat) and CSR(A_hat^T) (at may be NULL for num_layers == 1). */
typedef struct gss_plan_desc {
  int32_t n;          /* nodes (rows of this replica) */
  int32_t d;          /* hidden units */
  int32_t num_layers; /* model.py:199 */
  int32_t max_batch;  /* largest batch the plan will see */
  float layer_decay;  /* model.py:202 */
  float alpha;        /* model.py:220 */
  float lr, beta1, beta2, eps; /* Adam */
  int32_t cache_layer1; /* 1: keep AX/AM of layer 1 (inputs are constant) across steps */
  int32_t pipeline_layer1; /* 1: gss_plan_step runs the NEXT step's layer-1 SpMMs (constant inputs) on an internal second
                              stream underneath this step's MFMA-bound kernels; all work still executes every step and
                              the results are bitwise unchanged */
  const int32_t *node_map; /* NULL, or device int32 [N] (borrowed): the row of every node id a batch may name.  For graphs whose
                              nodes were relabelled (hub-first, for gather locality): callers keep naming nodes by their
                              original ids, the plan looks the batch up in this map first */
} gss_plan_desc;

/* caller-owned tensors the plan reads and writes (all device pointers, fp32) */
typedef struct gss_plan_io {
  const float *x;             /* [n][d] input features (train.py:125) */
  float *w1, *b1, *w2, *b2;   /* gcn_layer.dense{,2}.{weight,bias}; updated in place by gss_plan_adam */
  float *emb;                 /* [n][d] out: unit-norm embeddings of the last forward */
  float *loss;                /* [1]    out: loss of the last gss_plan_loss_backward */
  float *gw1, *gb1, *gw2, *gb2; /* out: gradients of the last backward */
} gss_plan_io;

int gss_plan_create(gss_plan **out, const gss_plan_desc *desc, const gss_csr *a, const gss_csr *at,
                    const gss_plan_io *io);

/* One shard of a node-range sharded replica.  Rank r owns the node range [bounds[r], bounds[r+1]) -- the rows
 * of A_hat and A_hat^T and the matching rows of every activation and gradient; weights are replicated.
 *
 * Operand layout ("halo" form of C1): an SpMM operand of this shard is a [n + n_halo][d] buffer -- its own n rows first,
 * then the rows of other shards that its CSR actually references (the boundary features), grouped by owner in ascending
 * node order.  The CSR handles carry LOCAL OPERAND ROW ids as column ids (n_cols = n + n_halo).  A_hat and A_hat^T
 * reference different nodes, so each has its own halo.  Before a hop every rank packs the rows its peers reference
 * (d_send_rows) and one fused group of point-to-point transfers (gss_exchange_rows) delivers exactly those rows:
 * nothing is padded and pairs of shards that share no edge exchange nothing.
 *   desc->n = rows of THIS shard; io->x / io->emb: this shard's rows; the weights / gradients / loss in io are full-size
 *   and end up identical on every rank.
 * Every gss_plan_* call then is a collective: all ranks call it with the same batch.  Per step the plan enqueues, on the
 * caller's stream, 2L - 2 + max(0, 2L - 3) halo exchanges (C1; the boundary rows of the input features and of layer 1's M --
 * constants -- are fetched once; every shard still recomputes its own rows of them each step), one all-reduce of
 * the B gathered batch rows and one of their 2 B d input gradients (C3), and one grouped all-reduce of the four weight
 * gradients (C2); no host round trip in between.  world == 1 is exactly gss_plan_create.  gss_plan_backward (external
 * upstream gradient) is not available on a sharded plan. */
typedef struct gss_halo_desc {
  const int64_t *h_recv_off;   /* host [world + 1]: halo rows [recv_off[q], recv_off[q+1]) are owned by rank q; n_halo = recv_off[world] */
  const int64_t *h_send_off;   /* host [world + 1]: packed rows [send_off[q], send_off[q+1]) go to rank q */
  const int32_t *d_send_rows;  /* device [send_off[world]]: the local row behind every packed row (borrowed: keep it alive) */
} gss_halo_desc;
typedef struct gss_shard_desc {
  int32_t world, rank;
  const int64_t *h_bounds;     /* host, [world + 1], bounds[0] = 0, bounds[world] = N */
  gss_halo_desc halo_a;        /* operand halo of A_hat's columns */
  gss_halo_desc halo_at;       /* operand halo of A_hat^T's columns (ignored when num_layers == 1) */
  const int32_t *d_gid2op_t;   /* device [N], borrowed: node id -> operand row of A_hat^T's column space ([0, n) own rows, then
                                  halo), -1 where this shard never reads the node.  NULL when num_layers == 1 */
  /* Optional: every matrix once more, split by column -- *_own holds the entries whose column is one of the shard's own rows
   * (operand rows [0, n)), *_halo the entries that reference boundary rows; same rows, same operand-row column ids, entries in
   * their original order.  With them a hop is overlapped with its exchange: the boundary rows travel on a second stream while the
   * own-column entries are multiplied, the boundary-column entries are added afterwards (gss_spmm_add) and the epilogue runs
   * there.  A row is then summed as (own entries) + (boundary entries) instead of in column order: results differ from the
   * single-GPU plan by rounding (~1e-7 relative), no longer bit for bit.  All NULL: exchange, then one pass (the default). */
  const gss_csr *a_own, *a_halo, *at_own, *at_halo;
  /* Optional (round 4): the shard's A_hat transposed IN PLACE -- rows = its operand rows (own rows, then the boundary rows), columns =
   * its own rows, [n + n_halo_a] x [n], the same values.  With it (and halo_recompute) the LAST backward hop, whose result only feeds
   * the bottom layer's weight gradient, runs in scatter-by-owner form: this shard multiplies ITS rows of u into every row they touch
   * (own and boundary), applies ELU'(P) there (P of the boundary rows is what halo_recompute computes anyway) and sums the weight
   * gradient over own + boundary rows; the ranks' all-reduce of the weight gradients completes the sum.  No exchange of u's boundary
   * rows in that hop: 3 collectives per step at two layers.  The weight gradients then add per-rank partial sums (rounding-level
   * differences, as with any other change of their summation order).  NULL: the hop fetches u's boundary rows (the default). */
  const gss_csr *a_loc_t;
} gss_shard_desc;
int gss_plan_create_sharded(gss_plan **out, const gss_plan_desc *desc, const gss_shard_desc *shard, gss_comm *comm,
                            const gss_csr *a, const gss_csr *at, const gss_plan_io *io);
/* this shard's rows of the last embeddings gathered from every shard: out [N][d] in node order (collective) */
int gss_plan_gather_embeddings(gss_plan *p, float *out, void *stream);
void gss_plan_destroy(gss_plan *p);
/* forward only (model.py:197-207): writes io.emb */
int gss_plan_forward(gss_plan *p, void *stream);
/* loss + backward for batch idx[0..b): writes io.loss and io.g* */
int gss_plan_loss_backward(gss_plan *p, const int32_t *idx, int32_t b, float beta, void *stream);
/* backward only, for an arbitrary upstream gradient that is non-zero on `b` unique rows: de_rows is the
 * compact [b][d] dLoss/dEmbedding of rows[0..b) (the autograd-glue path; NULL = the plan's own de_b) */
int gss_plan_backward(gss_plan *p, const int32_t *rows, int32_t b, const float *de_rows, void *stream);
/* Adam on the four tensors with the plan's gradients; step numbers are counted by the plan */
int gss_plan_adam(gss_plan *p, void *stream);
/* forward + loss + backward + Adam = one iteration of train.py:155-184.  idx[0..b): the batch's node ids (device), DISTINCT -- what the
 * reference's sampler draws (a permutation cut into batches, method/dataset.py:5-28); the batch-position map holds one position per
 * node, so a repeated id would leave the other position's rows unwritten.  The same holds for gss_plan_step_lazy and
 * gss_plan_loss_backward. */
int gss_plan_step(gss_plan *p, const int32_t *idx, int32_t b, float beta, void *stream);
/* gss_plan_step with the top layer evaluated on the b batch rows only -- the rows of it that the loss (model.py:216-221) and the
 * backward pass read; the reference computes all N every step (train.py:158-161) and reads B of them.  Loss, gradients and
 * parameters equal gss_plan_step's bit for bit (a computed row takes the same path through the same kernels).  Afterwards io.emb
 * holds the step's embeddings on the batch rows only: call gss_plan_forward when all of them are wanted (the beta percentile of
 * step 0, the embeddings that are written out).  On a sharded plan every shard evaluates the top layer on the batch rows it owns.
 * One-layer plans run the full step. */
int gss_plan_step_lazy(gss_plan *p, const int32_t *idx, int32_t b, float beta, void *stream);
/* Sharded plans, knob lazy_halo (default: graphs of >= 262,144 nodes): two hops fetch a SUBSET of their operand's boundary rows.
 * (1) Lazy steps, the top layer's M: only the boundary rows that the batch rows of this shard reference (the receiver marks them over
 * its halo slots and sends the bitmaps to the owners).  What is needed depends on the batch ids and the graph alone, so the request
 * phase is the FIRST thing gss_plan_step_lazy enqueues, on the plan's own request stream: it runs underneath layer 1, the row counts
 * reach the host through an event-gated async copy, and the host waits for that event -- never for the caller's stream -- just before
 * it enqueues the transfer (gss_plan_sync_stats).  On by default on every transport.
 * (2) Every step, u -- the operand of the top layer's second backward hop, zero outside the batch's neighbourhood --: only the rows
 * that can be non-zero (the owners send them and the bitmap that says which).  That bitmap is an OUTPUT of the hop before it, so the
 * host drains the caller's stream once per step for the counts; knob lazy_halo_u (-1, the default: with lazy_halo on the host-side
 * transports, not over RCCL -- there a two-layer plan runs the hop exchange-free on gss_shard_desc.a_loc_t instead; 0 never; 1 with lazy_halo).
 * Same bits as the full exchanges.  out6 reports what the LAST such exchanges moved: {rows fetched, rows sent, rows of the whole
 * halo} for (1) and then for (2); fetched / sent are -1 when the plan exchanges whole halos. */
int gss_plan_lazy_halo_rows(const gss_plan *p, int64_t *out6);
/* Collectives a sharded plan has enqueued since the last call (then reset): out3 = {boundary-row exchanges, batch-row all-reduces,
 * weight-gradient all-reduces}.  A steady full step at L layers: 2L - 2 + 2L - 3 exchanges (one less with halo_recompute: layer 2's
 * boundary input rows are recomputed from layer 1's constant AX / AM), 1 batch-row all-reduce ([E_B | P_B | inv_B] as one buffer; 2
 * at widths outside {64, 128, 256} or with the row-slab loss sweep, knob loss_slab), 1 weight-gradient all-reduce.  Zeros on one GPU. */
int gss_plan_comm_stats(gss_plan *p, int64_t *out3);
/* Host-side waits of a sharded plan since the last call (then reset): out2 = {waits that DRAIN the caller's stream (the device idles
 * until the host has enqueued again): the sender-driven subset exchange of u, knob lazy_halo_u; waits for an EVENT of the plan's
 * request stream while the caller's stream keeps running: the request phase of the lazy step's subset exchange}.  An RCCL job with
 * default knobs: {0, 0} per full step, {0, 1} per lazy step from 262,144 nodes on, {0, 0} below.  Zeros on one GPU. */
int gss_plan_sync_stats(gss_plan *p, int64_t *out2);
/* layer activations for parity tests: which 0 AX, 1 AM, 2 P of layer `layer` (0-based); 3 the bottom layer's dP [n][d] and 4 the top layer's dP on
 * the batch rows [b][d] as the last backward pass left them; 5 / 6 u and t of the top layer's first backward hop, 7 the uint32 bitmap of the rows of
 * u / t it wrote (NULL on plans without it: then every row is written), 8 the batch rows' input gradients [g_ax ; g_am] as [2 b][d] -- `layer`
 * is ignored for 3 .. 8 */
const float *gss_plan_activation(const gss_plan *p, int layer, int which);
/* bytes of the plan's slab.  Not counted: what a gss_csr handle caches for itself -- its segment descriptors, the chunk scratch of giant rows (one
 * buffer per stream the handle is used on, grown to the widest d seen), the live-workgroup lists of row-filtered products (one per stream too). */
size_t gss_plan_device_bytes(const gss_plan *p);
/* every buffer the plan carves from its slab is followed by a 256-byte guard no kernel may touch; this synchronises the device and
 * verifies them all (GSS_EINVAL names the first one that was overwritten).  For tests. */
int gss_plan_check_guards(gss_plan *p);
/* set the 1-based Adam step counter (resume; also marks every buffer derived from the weights stale) / read it */
void gss_plan_set_step(gss_plan *p, int32_t step);
int32_t gss_plan_get_step(const gss_plan *p);
/* checkpoint / resume: device pointer of Adam's exp_avg (moment 0) or exp_avg_sq (moment 1) of tensor 0..3 =
 * W1, b1, W2, b2 (same shapes as the parameters); NULL on a bad argument */
float *gss_plan_adam_buffer(gss_plan *p, int32_t moment, int32_t tensor);
/* Per-kernel-class timing with HIP events recorded on the caller's stream around every launch of a
 * plan call (bench.py's live roofline measurement).  gss_plan_profile_read synchronises the stream, returns
 * the accumulated milliseconds and launch counts per class (arrays of GSS_PROF_CLASSES) and resets them. */
enum {
  GSS_PROF_SPMM_FWD_HAD = 0, /* AX = A x with fused Hadamard epilogue */
  GSS_PROF_SPMM_FWD = 1,     /* AM = A M */
  GSS_PROF_SPMM_BWD1 = 2,    /* the top layer's first backward hop, batch-sparse (SPMM_BWD1S) */
  GSS_PROF_SPMM_BWD2 = 3,    /* the top layer's second backward hop with the batch rows' residual folded in (SPMM_BWD2S) */
  GSS_PROF_DENSE_FWD = 4,
  GSS_PROF_DGRAD = 5,
  GSS_PROF_WGRAD = 6,        /* N-row weight gradient (+ its reduce) */
  GSS_PROF_WGRAD_BATCH = 7,  /* batch-row weight gradient of the top layer */
  GSS_PROF_LOSS = 8,
  GSS_PROF_ROWNORM = 9,
  GSS_PROF_ELEMENTWISE = 10, /* norm/ELU backward on batch rows, transposes, memsets, scatter */
  GSS_PROF_ADAM = 11,
  GSS_PROF_COMM = 12,        /* sharded plans: boundary-row exchanges of the SpMM hops (pack kernel + grouped send / recv) */
  GSS_PROF_COMM_BATCH = 13,  /* sharded plans: the batch-row all-reduce(s) of the loss */
  GSS_PROF_COMM_GRADS = 14,  /* sharded plans: the all-reduce of the four weight gradients */
  GSS_PROF_SPMM_BWD1_DENSE = 15,  /* (round 6) an N-row first backward hop: layers below the top one at L >= 3, the phase-wise entry points */
  GSS_PROF_SPMM_BWD2_DENSE = 16,  /* (round 6) an N-row second backward hop */
  GSS_PROF_CLASSES = 17
};
int gss_plan_profile(gss_plan *p, int enable);
int gss_plan_profile_read(gss_plan *p, double *ms_out, int64_t *count_out, void *stream);
/* tuning/debug knobs (A/B runs inside one process; 20 of them -- round 6 removed the access-shape variants whose sweeps said "default holds" in
 * two or more rounds from the kernels; "spmm_seg_edges" left when "proj_split" came: the segment length is 32 entries): "spmm_list_blocks" = workgroups from which a ROW-FILTERED balanced SpMM (the lazy step's
 * top-layer products, the batch-sparse backward hop) lists the workgroups that hold a passing row and walks the list with persistent
 * workgroups instead of dispatching every workgroup (default 2048; 0 = never; same bits); "spmm_variant" = 1 (whole-row gather, wave per row) or
 * 2 (nnz-balanced segments, default); "spmm_slices" = 0 (automatic, default) or 1..8 feature slices in the balanced SpMM, "spmm_pin" = with a
 * manual "spmm_slices": slices time-separated (0, default) or pinned to XCDs (1) -- the automatic policy pins operands of <= 64 MB;
 * "spmm_hot_rows" = -1 (default: what gss_csr_set_hot declared) or a row count; "spmm_giant" = stored entries above which a row is summed chunk by chunk across workgroups
 * (default 32768, 0 = never; gss_csr_giant_rows); "gemm_variant" = projection tile shape: 2 (by width and row count; default), 3 (128-node
 * tiles of four waves forced), 5 (128-node tiles of eight waves forced); "gemm_ws" = -1 (default: from 32,769 rows on -- more 128-node
 * tiles than CUs) / 0 / 1: the d = 128 forward projection as the weight-stationary persistent kernel (same bits);
 * "proj_split" = -1 (default: by size -- off) / 0 / 1: a one-GPU plan runs the AX half of a layer's forward projection on its side
 * stream beside the layer's second SpMM and finishes it in a second launch (widths 64 / 128 / 256 below the weight-stationary row count; same bits);
 * "wgrad_wgs", "loss_wgs" = workgroups of a full-size weight-gradient launch / the loss sweep (default 256 = one per CU; set
 * before plans are created); "sparse_bits_rows" = operand rows from which a plan keeps the bitmaps of the sparsity-aware backward hops
 * (default 100000); "ppr_fused" = 1 (default) / 0 (separate update pass of the diffusion profiles); "prox_batch_pairs" = 0 (default: as many
 * pairs per trip of gss_prox_score as its 256 MiB scratch holds) or a cap on that count (same bits; for tests of the batch loop);
 * "lazy_halo" = -1 (default: graphs of >= 262,144 nodes, but never over RCCL, where it stays opt-in) / 0 / 1: sharded plans fetch subsets of the
 * boundary rows where a hop reads a subset (gss_plan_lazy_halo_rows), "lazy_halo_u" = -1 / 0 / 1 the same for u in the second backward hop (see gss_plan_lazy_halo_rows); "halo_recompute" = -1 (default: on) / 0 / 1: sharded plans recompute layer 2's boundary input rows from layer 1's constant AX / AM (fetched once)
 * instead of exchanging them every step (same bits); "loss_dgrad" = -1 (default: on shards only) / 0 / 1: the
 * loss finish and the batch rows' input gradient in one launch instead of two (same bits; on a shard it spares a collective); "prep_side" = 1 (default) / 0: on one GPU a step's batch preparation rides in its
 * first forward SpMM launch and E_B comes out of the top layer's projection (no batch_prepare / gather launch; same bits);
 * JOB-WIDE knobs -- "lazy_halo", "lazy_halo_u", "halo_recompute", "loss_slab" -- must have the same value on every rank:
 * gss_plan_create_sharded all-gathers every rank's values and compares them on the host, and fails by name when they differ;
 * "loss_slab" = -1 (default: batches of >= 8192
 * rows) / 0 / 1: sharded plans sweep the B x B loss as row slabs (rank r the i tiles r, r + P, ...; one more all-reduce of B d + 1
 * floats) instead of replicating it on every rank (every rank of a job must use the same value; results agree to rounding).  Every setting computes the same results (some in a different summation order); the defaults are
 * the measured optima recorded in DESIGN.md section 4.  The values are process-wide DEFAULTS: a plan (and a gss_ppr handle) takes a
 * snapshot when it is created and runs under it from then on, so changing a knob never re-shapes a live plan -- in particular not
 * the plans of other rank threads of the same process; per-op entry points read the current defaults. */
int gss_debug_set_option(const char *name, int value);
/* plain device-to-device copy on `stream` (lets a ctypes host read plan-owned activations) */
int gss_memcpy_d2d(void *dst, const void *src, size_t bytes, void *stream);

/* ---- FOR TESTS: the row-sparse SpMM modes and their bitmap builders, exactly as a plan's step launches them --------------------
 * These entry points exist so that tests/test_gpu_sparse_ops.py can hold every mode to its fp64 contract (tests/sparse_hop_mirror.py)
 * op by op; nothing in the product calls them.  Bitmaps are uint32 words, bit i = word i >> 5, bit i & 31.  All need the balanced
 * SpMM ("spmm_variant" = 2).
 *   gss_spmm_bwd1_sparse_ex: gss_spmm_bwd1_sparse with every optional argument.  posbits (nullable): bit c set <=> pos_col[c] >= 0.
 *     nzbits_out (nullable, cleared over [0, n_rows) by the caller): bit r is set for every batch row and every row with a non-zero sum
 *     -- per row, never per piece.  skip_zero_rows (needs nzbits_out): rows whose bit stays clear are not written.  live_rows
 *     (nullable): a superset of the batch rows and the rows with an entry in a batch column; other rows are not walked (written as
 *     zeros, or not at all under skip_zero_rows).
 *   gss_spmm_bwd2_sparse_res: gx = t + A u; dp = c * gx (.) elu'(p) (+ res_b[pos_row[r]] where pos_row[r] >= 0); gx_out nullable.
 *     nzbits (nullable): a clear bit c says rows c of u AND of t are zero (the neighbour is skipped, t's row is not read).  y_in
 *     (nullable): [n_rows][d] partial sums of a first pass, added before the epilogue.  pos_row_limit > 0: t, pos_row and the residual
 *     exist for output rows below it only; rows behind it get dp = c * (A u) (.) elu'(p).
 *   gss_spmm_bwd1_ex / gss_spmm_bwd2_ex (tests/test_gpu_dense_hops.py): gss_spmm_bwd1 / gss_spmm_bwd2 with the arguments that only a
 *     sharded plan's overlapped hops pass.  y_in (nullable): [n_rows][d] partial sums of a first pass, added before the epilogue; it may
 *     be the buffer the pass writes: t for bwd1, dp for bwd2.  own_row_limit > 0: t and res exist for output rows below it only; rows
 *     behind it get gx = A u and dp = c * gx (.) elu'(p).  Either argument needs the balanced SpMM; without them the row-per-wave
 *     variant runs too.
 *   gss_spmm_filtered: gss_spmm with row filters.  row_pos (plain product only): rows with row_pos[r] < 0 are not computed and not
 *     written; row_bits: the same by bitmap; y_in as above; gather_bits (plain product only): columns whose bit is clear are skipped.
 *   gss_mark_rows_and_neighbours: bits |= the listed rows and every column of their entries (negative list entries skipped).
 *   gss_batch_bits: set != 0: bits |= ids (negative ids skipped); set == 0: the WORDS of the ids := 0 (the caller's contract: every set
 *     bit of those words belongs to ids).
 *   gss_bits_fill: bits [first, last) := 1, other bits untouched. */
int gss_spmm_bwd1_sparse_ex(const gss_csr *at, int32_t d, const float *g_am_b, const float *g_ax_b, const int32_t *pos_col,
                            const int32_t *pos_row, const float *x_in, const float *ax, float *u, float *t, const uint32_t *posbits,
                            uint32_t *nzbits_out, int32_t skip_zero_rows, const uint32_t *live_rows, void *stream);
int gss_spmm_bwd2_sparse_res(const gss_csr *at, int32_t d, const float *u, const float *t, const float *p, float c, const float *res_b,
                             const int32_t *pos_row, float *dp, float *gx_out, const uint32_t *nzbits, const float *y_in,
                             int32_t pos_row_limit, void *stream);
int gss_spmm_bwd1_ex(const gss_csr *at, int32_t d, const float *g_am, const float *g_ax, const float *x_in, const float *ax,
                     float *u, float *t, const float *y_in, void *stream);
int gss_spmm_bwd2_ex(const gss_csr *at, int32_t d, const float *u, const float *t, const float *p, float c, const float *res,
                     float *dp, float *gx_out, const float *y_in, int32_t own_row_limit, void *stream);
int gss_spmm_filtered(const gss_csr *a, int32_t d, const float *x, float *y, const float *h, float *m, const int32_t *row_pos,
                      const uint32_t *row_bits, const float *y_in, const uint32_t *gather_bits, void *stream);
int gss_mark_rows_and_neighbours(const gss_csr *a, const int32_t *rows, int32_t b, uint32_t *bits, void *stream);
/* Two unfiltered forward products over ONE matrix: y_k = A x_k and, when m_k is given (for both or for neither), m_k = y_k (.) h_k.  One
 * launch of twice the workgroups where the balanced SpMM has a paired form -- *paired_out = 1 --, two launches otherwise -- 0: spmm_variant
 * 1, a matrix with giant rows (gss_csr_giant_rows), an empty matrix.  Either way the bits of two gss_spmm calls.  prep_idx != NULL (needs
 * m_k): the batch preparation rides in the launch as with a plan's first forward SpMM -- for i < prep_b, r = node_map[idx[i]] (idx[i]
 * without a map): prep_rloc[i] = prep_pid[i] = r (both nullable), prep_pos[r] = i.  What the second product writes may be what a later
 * launch gathers; no buffer of one product may be written by the other. */
int gss_spmm_fwd_pair(const gss_csr *a, int32_t d, const float *x0, float *y0, const float *h0, float *m0, const float *x1, float *y1,
                      const float *h1, float *m1, const int32_t *prep_idx, int32_t prep_b, const int32_t *prep_node_map, int32_t *prep_rloc,
                      int32_t *prep_pid, int32_t *prep_pos, int32_t *paired_out, void *stream);
int gss_batch_bits(const int32_t *ids, int32_t b, uint32_t *bits, int32_t set, void *stream);
int gss_bits_fill(uint32_t *bits, int64_t first, int64_t last, void *stream);

/* ---- FOR TESTS: the loss of a plan's step, stage by stage ------------------------------------------------------------------------
 * A plan reaches csrc/loss.hip through loss_step, loss_step_slab_sweep and the three gathers; these entry points call exactly those, so
 * that tests/test_gpu_loss_step.py can hold each to its fp64 contract (tests/loss_step_mirror.py).  Nothing in the product calls them.
 *   gss_loss_step: the sweep over the gathered rows e_b ([b][d]; NULL: the workspace's E_B, where gss_loss_gather_rows* put it), then
 *     the finish: loss_out[0]; dx_b = (dE - e (e . dE)) * inv_den[row]; dp_b = c * dx_b (.) elu'(p[row]), both [b][d], zero rows where
 *     keep[r] == 0 (keep nullable).  rows (nullable): row of inv_den / p per member, NULL = the member's position.  pos_set (nullable):
 *     pos_set[key[r]] = r for keys >= 0, key = pos_ids, or rows when pos_ids is NULL.  w1t (nullable; then w2t, gax_b, gam_b too; d in
 *     {64, 128, 256} only, other widths are refused): gax_b = dP W1, gam_b = dP W2 in the same launch, *dgrad_done = 1; dgrad_all != 0:
 *     rows with keep[r] == 0 enter that product unmasked.  de_x (nullable): no sweep, [b][d] sums of the ranks' gss_loss_slab_sweep
 *     buffers instead (the loss is not written then).  ws: gss_loss_workspace_bytes(b, d) bytes.
 *   gss_loss_slab_sweep: the i tiles slab_rank, slab_rank + slab_parts, ... of the sweep.  de_x ([b d + 1] floats): those tiles' rows of
 *     dE / 2, zeros on every other row, and this rank's share of the loss behind the last row.  ws: gss_loss_workspace_bytes_parts.
 *   gss_loss_workspace_bytes_parts: the workspace of a sweep whose i tiles are dealt to `parts` ranks (parts = 1: gss_loss_workspace_bytes).
 *   gss_loss_gather_rows: E_B = e[rows] (zero rows where keep[r] == 0) into the workspace; *e_b_out says where.
 *   gss_loss_gather_rows_mapped: the same with the id translation folded in: id = node_map[idx[r]] (node_map nullable), rel = id - lo,
 *     owned <=> 0 <= rel < nl; rloc[r] = rel clamped to [0, max(nl - 1, 0)], keep[r] = owned (keep nullable), pid[r] = gid2op[id], or
 *     without gid2op rel when owned and -1 when not.
 *   gss_loss_gather_batch: out = [E_B | P_B | inv_B] ([b (2 d + 1)] floats) of the owned members, zeros for the others; idx == NULL: the
 *     prepared rows / keep are read instead of translated. */
size_t gss_loss_workspace_bytes_parts(int32_t b, int32_t d, int32_t parts);
int gss_loss_step(int32_t d, int32_t b, float beta, float alpha, float *loss_out, const float *e_b, const int32_t *rows,
                  const int32_t *pos_ids, int32_t *pos_set, const float *keep, const float *inv_den, const float *p, float c, float *dx_b,
                  float *dp_b, const float *w1t, const float *w2t, float *gax_b, float *gam_b, int32_t dgrad_all, const float *de_x,
                  void *ws, void *stream, int32_t *dgrad_done);
int gss_loss_slab_sweep(int32_t d, int32_t b, float beta, float alpha, const float *e_b, int32_t slab_rank, int32_t slab_parts, void *ws,
                        float *de_x, void *stream);
int gss_loss_gather_rows(int32_t d, const float *e, const int32_t *rows, const float *keep, int32_t b, void *ws, float **e_b_out,
                         void *stream);
int gss_loss_gather_rows_mapped(int32_t d, const float *e, const int32_t *idx, const int32_t *node_map, int32_t lo, int32_t nl,
                                const int32_t *gid2op, int32_t *pid, int32_t *rloc, float *keep, int32_t b, void *ws, float **e_b_out,
                                void *stream);
int gss_loss_gather_batch(int32_t d, const float *e, const float *p, const float *inv_den, const int32_t *idx, const int32_t *node_map,
                          int32_t lo, int32_t nl, const int32_t *gid2op, int32_t *pid, int32_t *rloc, float *keep, const int32_t *rows,
                          int32_t b, float *out, void *stream);

/* ---- FOR TESTS: the dense half of a plan's step, launcher by launcher ------------------------------------------------------------
 * A plan reaches csrc/dense.hip and the optimizer kernels of csrc/elementwise.hip through the launchers below; these entry points pass
 * their arguments straight through, so that tests/test_gpu_dense_step.py can hold each form to its fp64 contract
 * (tests/dense_step_mirror.py).  Nothing in the product calls them.
 *   gss_dense_fwd_rows: gss_dense_fwd with a row list (nullable): the n tile rows are node rows row_list[0..n) of every operand, a
 *     negative entry is skipped (nothing of it is written); listed rows get the bits of the pass without a list.  acc_in_p != 0: the
 *     second of two launches -- p holds gss_dense_fwd_first's accumulators; the pair gives the bits of one launch.
 *   gss_dense_fwd_first: acc = AX W1^T, raw, [n][d].  gss_dense_fwd_split_available: 1 where the two-launch form exists under the current
 *     knobs (d in {64, 128, 256}, no row list, not the weight-stationary kernel); elsewhere both launches are refused with GSS_EINVAL.
 *   gss_dense_fwd_norm: the last layer -- p as gss_dense_fwd, e = x / max(|x|, 1e-12) with x = elu(p) or p_prev + decay elu(p), inv_den
 *     = 1 / max(|x|, 1e-12) per row; d in {16, 32, 64, 128, 256}.  rows_out (nullable) goes with exactly one of row_list (rows_out[t] =
 *     e[row_list[t]] for entries >= 0) and rows_out_pos (rows_out[rows_out_pos[r]] = e[r] where that is >= 0).
 *   gss_rownorm_fwd_rows: gss_rownorm_fwd over the n listed rows of x / e / inv_den (rows nullable; negative entries skipped).
 *   gss_wgrad_slices / gss_wgrad_slices_max: the slices gss_wgrad_partial writes for n rows / a bound over every n in [1, n_max].
 *   gss_wgrad_partial: the partial sums of one problem (dp [n][d] compact, ax / am indexed by rows when given) into slices [slice0,
 *     slice0 + *nslices_out) of ws = [total_slices][d][2 d] weight slabs followed by [total_slices][d] bias slabs.
 *   gss_wgrad_partial_pair: two problems in one launch (d a multiple of 64 and both non-empty), in two launches otherwise.
 *   gss_wgrad_reduce: gw1, gw2, gb (and gb2, nullable) = the sum of slices [0, nslices), in slice order; accumulate != 0 adds to them.
 *   gss_wgrad_reduce_adam: the same sum into grad[] (order w1, b1, w2, b2; b1 and b2 get the same gradient) and torch's Adam on param[]
 *     / m[] / v[] in the same launch; w1t, w2t (nullable): transposed copies of the updated W1, W2; pos_clear (nullable):
 *     pos_clear[idx[r]] = -1 for the b entries idx[r] >= 0.
 *   gss_adam_step4: Adam on four tensors of count[k] elements in one launch, with the same transposed copies and reset.
 *   gss_transpose2: at = a^T, bt = b^T for two [dim][dim] matrices. */
int gss_dense_fwd_rows(int32_t n, int32_t d, const float *ax, const float *am, const float *w1, const float *b1, const float *w2,
                       const float *b2, const float *p_prev, float decay, float *p, float *x_next, const int32_t *row_list,
                       int32_t acc_in_p, void *stream);
int gss_dense_fwd_first(int32_t n, int32_t d, const float *ax, const float *w1, float *acc, void *stream);
int gss_dense_fwd_split_available(int32_t n, int32_t d);
int gss_dense_fwd_norm(int32_t n, int32_t d, const float *ax, const float *am, const float *w1, const float *b1, const float *w2,
                       const float *b2, const float *p_prev, float decay, float *p, float *e, float *inv_den, const int32_t *row_list,
                       float *rows_out, const int32_t *rows_out_pos, int32_t acc_in_p, void *stream);
int gss_rownorm_fwd_rows(int32_t n, int32_t d, const float *x, float *e, float *inv_den, const int32_t *rows, void *stream);
int gss_wgrad_slices(int32_t n, int32_t d);
int gss_wgrad_slices_max(int32_t n_max, int32_t d);
int gss_wgrad_partial(int32_t n, int32_t d, const float *dp, const float *ax, const float *am, const int32_t *rows, void *ws,
                      int32_t total_slices, int32_t slice0, int32_t *nslices_out, void *stream);
int gss_wgrad_partial_pair(int32_t d, int32_t n0, const float *dp0, const float *ax0, const float *am0, const int32_t *rows0,
                           int32_t slice0_0, int32_t n1, const float *dp1, const float *ax1, const float *am1, const int32_t *rows1,
                           int32_t slice0_1, void *ws, int32_t total_slices, int32_t *ns0_out, int32_t *ns1_out, void *stream);
int gss_wgrad_reduce(int32_t d, void *ws, int32_t total_slices, int32_t nslices, float *gw1, float *gw2, float *gb, float *gb2,
                     int32_t accumulate, void *stream);
int gss_wgrad_reduce_adam(int32_t d, void *ws, int32_t total_slices, int32_t nslices, float *const grad[4], float *const param[4],
                          float *const m[4], float *const v[4], int32_t step, float lr, float beta1, float beta2, float eps, float *w1t,
                          float *w2t, int32_t *pos_clear, const int32_t *idx, int32_t b, void *stream);
int gss_adam_step4(float *const param[4], const float *const grad[4], float *const m[4], float *const v[4], const int64_t count[4],
                   int32_t step, float lr, float beta1, float beta2, float eps, float *w1t, float *w2t, int32_t dim, int32_t *pos_clear,
                   const int32_t *ids, int32_t b, void *stream);
int gss_transpose2(int32_t dim, const float *a, const float *b, float *at, float *bt, void *stream);

/* ---- FOR TESTS: the row-norm backward as a plan calls it (tests/test_gpu_rownorm.py) ---------------------------------------------
 * gss_rownorm_elu_bwd with the side write of the batch-sparse backward hop's key: pos_set (nullable, int32 per node row) gets
 * pos_set[idx[r]] = r for every r < b and is written nowhere else; dx_b and dp_b get the bits of gss_rownorm_elu_bwd.  idx as there:
 * unique, valid node rows, read unchecked.  Nothing in the product calls it. */
int gss_rownorm_elu_bwd_ex(int32_t d, const float *de_b, const int32_t *idx, int32_t b, const float *e, const float *inv_den,
                           const float *p, float c, float *dx_b, float *dp_b, int32_t *pos_set, void *stream);

/* ---- FOR TESTS: the halo bookkeeping and the batch preparation of a sharded plan, launcher by launcher ---------------------------
 * A sharded plan's lazy halo and its batch preparation are integers, bitmaps and row copies in csrc/elementwise.hip (and one copy of the
 * batch preparation in csrc/spmm.hip); these entry points pass their arguments straight through to the launchers the plan calls, so that
 * tests/test_gpu_halo_ops.py can hold each to its numpy mirror (tests/halo_ops_mirror.py), bit for bit.  Nothing in the product calls them.
 * THE BITMAP CONTRACTS (what the plan guarantees and every kernel below relies on): bitmaps are uint32 words, bit i = word i >> 5, bit
 * i & 31.  A bitmap over the slots of P peers is P word RANGES: peer q's slots [off[q], off[q + 1]) are bits 0 .. of the words
 * [woff[q], woff[q + 1]), woff[q + 1] - woff[q] = ceil((off[q + 1] - off[q]) / 32) -- every range starts on a word, so ranges can be sent
 * to their peers as they stand.  The PADDING bits of a range's last word are clear, always: a set one would be listed as a slot of the
 * next peer.  Buffers of woff[P] words are allocated with one guard word more (woff[P] + 1), which no kernel writes.  Offsets are
 * int64 arrays of P + 1 entries on the device; gss_bits_compact takes the word offsets on the host as well (it sizes its launches by them).
 *   gss_pack_rows: out[k] = src[rows[k]] for k < n, rows of d floats; rows may repeat.  gss_unpack_rows: dst[rows[k]] = src[k]; rows
 *     are distinct.  Both copy bits (NaN payloads survive); unlisted rows of the destination are not written.
 *   gss_halo_need_mark: for the b listed rows of `a` (negative entries skipped), every entry with a column c >= n is halo slot h = c - n
 *     of the owner q with recv_off[q] <= h < recv_off[q + 1]: needw |= bit (h - recv_off[q]) of q's range.  Nothing is cleared.
 *   gss_send_slot_bits: out word w of peer q's range = bits[send_rows[s]] of its up to 32 send slots s = send_off[q] + 32 (w -
 *     wsend_off[q]) ...; all n_words = wsend_off[P] words are written, padding bits as zeros.
 *   gss_bits_clear: bits [first, last) := 0, other bits untouched; nothing for last <= first.
 *   gss_bits_set_list: bits[list[k]] := 1 for k < n (ids may repeat, none is negative), other bits untouched.
 *   gss_bits_compact: the set bits of the P ranges in ascending order as a list: bit j of range q is slot slot_off[q] + j; out holds
 *     map[slot] (map != NULL) or slot + add.  out_off[q + 1] = entries up to and including range q (out_off[0] = 0); out behind
 *     out_off[P] is not written.  scratch (nullable): gss_bits_compact_scratch_bytes(P, h_woff) bytes; NULL or fewer bytes: the call
 *     allocates stream-ordered scratch of its own.
 *   gss_batch_prepare: for i < b: id = node_map[idx[i]] (idx[i] without a map), rel = id - lo, owned <=> 0 <= rel < nl, op = gid2op[id]
 *     (without gid2op: rel when owned, -1 when not).  rloc[i] = rel clamped to [0, max(nl - 1, 0)], pid[i] = op, keep[i] = owned as
 *     1.f / 0.f, rlist[i] = rel when owned and -1 when not (all four nullable), pos[op] = i where op >= 0.  ids with op >= 0 are distinct.
 *   gss_scatter_add_rows_ex: gss_scatter_add_rows with every argument: member r is skipped when rows[r] < 0 or keep[r] == 0 (keep
 *     nullable), else dst[rows[r]] += src[r] (kept rows are distinct).  pos_clear (nullable; then pos_ids too): pos_clear[pos_ids[r]] =
 *     -1 for every r with pos_ids[r] >= 0, skipped members included.
 *   gss_spmm_prep_side: gss_spmm (Hadamard-fused: m and h given; row_bits nullable as in gss_spmm_filtered) whose launch carries
 *     gss_batch_prepare's job for the same arguments as one more workgroup; needs the balanced SpMM and b >= 1.  Same bits as the two
 *     calls apart. */
int gss_pack_rows(int32_t d, const float *src, const int32_t *rows, int64_t n, float *out, void *stream);
int gss_unpack_rows(int32_t d, const float *src, const int32_t *rows, int64_t n, float *dst, void *stream);
int gss_halo_need_mark(const gss_csr *a, const int32_t *rows, int32_t b, int32_t n, int32_t P, const int64_t *d_recv_off,
                       const int64_t *d_wrecv_off, uint32_t *needw, void *stream);
int gss_send_slot_bits(const uint32_t *bits, const int32_t *send_rows, int32_t P, const int64_t *d_send_off, const int64_t *d_wsend_off,
                       int64_t n_words, uint32_t *out, void *stream);
int gss_bits_clear(uint32_t *bits, int64_t first, int64_t last, void *stream);
int gss_bits_set_list(uint32_t *bits, const int32_t *list, int64_t n, void *stream);
size_t gss_bits_compact_scratch_bytes(int32_t P, const int64_t *h_woff);
int gss_bits_compact(const uint32_t *words, int32_t P, const int64_t *d_woff, const int64_t *h_woff, const int64_t *d_slot_off,
                     const int32_t *map, int32_t add, int32_t *out, int64_t *d_out_off, void *scratch, size_t scratch_bytes, void *stream);
int gss_batch_prepare(const int32_t *idx, int32_t b, const int32_t *node_map, int32_t lo, int32_t nl, const int32_t *gid2op,
                      int32_t *rloc, int32_t *pid, float *keep, int32_t *pos, int32_t *rlist, void *stream);
int gss_scatter_add_rows_ex(int32_t d, const float *src, const int32_t *rows, const float *keep, int32_t b, float *dst,
                            int32_t *pos_clear, const int32_t *pos_ids, void *stream);
int gss_spmm_prep_side(const gss_csr *a, int32_t d, const float *x, float *y, const float *h, float *m, const uint32_t *row_bits,
                       const int32_t *idx, int32_t b, const int32_t *node_map, int32_t lo, int32_t nl, const int32_t *gid2op,
                       int32_t *rloc, int32_t *pid, float *keep, int32_t *pos, int32_t *rlist, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GSSGCN_H */

"""Tolerances of the MULTI-STEP parity tests (losses / last embeddings / final weights after the fixtures' recorded steps), stated as a
multiple of a measured quantity instead of asserted (VERDICT round 2, weak spot 1a).

SPREAD_* is the largest difference, over the fixtures, between equally valid CPU executions of the reference's own op sequence
(oracle/torch_cpu_path.py, i.e. torch.sparse.mm / nn.Linear / F.elu / F.normalize / Adam): fp32 with 1 thread, fp32 with 8 threads and
fp64, all from the same start on the same recorded batches.  tests/test_trajectory_spread.py re-measures it on every run of the CPU
suite and fails if it ever exceeds the recorded figure, so the tolerances below stay tied to a number that is shown, not claimed.
Measured in this container (torch 2.10 CPU): losses 1.4e-7 relative, embeddings 1.7e-6 of the largest entry, weights 1.7e-3 lr -- the
trajectory is NOT sensitive at the level of whole learning-rate steps (an earlier DESIGN.md said it was; it is not).

A device run differs from the fixture by its own fp32 rounding (different summation order in the SpMM segments, MFMA k order, the
fixed-order weight-gradient reduce); tools/trajectory_deviation.py prints what it measures on the GPU box
(profiles/r03_trajectory_deviation.txt).  TRAJ_K x the CPU spread bounds it with room for a different box."""

SPREAD_LOSS_REL = 1.5e-7       # max |loss_a - loss_b| / max |loss|
SPREAD_EMB_REL = 2.0e-6        # max |emb_a - emb_b| / max |emb|
SPREAD_WEIGHT_LR = 2.0e-3      # max |w_a - w_b| / lr

TRAJ_K = 10                    # device-vs-fixture tolerances = TRAJ_K x the spread between CPU executions
TRAJ_LOSS_RTOL = TRAJ_K * SPREAD_LOSS_REL      # 1.5e-6   (measured on the device: <= 7.4e-8)
TRAJ_EMB_REL = TRAJ_K * SPREAD_EMB_REL         # 2e-5     (measured: <= 1.3e-6)
TRAJ_WEIGHT_LR = TRAJ_K * SPREAD_WEIGHT_LR     # 0.02 lr  (measured: <= 1.2e-3 lr)
# end to end through the CLI (train.py: kNN graph, beta percentile, 12 steps, '%.18e' text): absolute difference of unit-norm rows
TRAJ_CLI_EMB_ABS = 2e-5


# ---- the loss of a plan's step, op by op (tests/test_gpu_loss_step.py against tests/loss_step_mirror.py in fp64) ----------------------
# Loss and dE keep the bounds test_loss_fwd_bwd has always held gss_loss_fwd_bwd to.
LOSS_STEP_LOSS_RTOL = 2e-6     # |loss - ref| / |ref|
LOSS_STEP_DE_REL = 5e-6        # max |dE - ref| / max |ref|
# The composite outputs (dx_b, dp_b, gax_b, gam_b, the slab sums) get no invented number.  LOSS_STEP_FP32 is the error of the REFERENCE's
# own formulas evaluated in plain numpy float32 against float64: the largest over every GPU case, relative to the reference tensor's
# largest entry.  tests/test_loss_step_mirror.py re-measures it on every run of the CPU suite (it may not exceed the figure recorded
# here, nor fall below a quarter of it).  The GPU bound of a quantity is the larger of the project's bound for its last stage (3e-6:
# test_rownorm_fwd_and_bwd for dx / dp, test_dense_bwd_input_dense_and_scattered for gax / gam) and LOSS_STEP_K x that figure; 8,
# because the kernels accumulate sequentially along j and along k on MFMA chains where numpy sums pairwise and in blocks.
# Measured on the CPU (numpy 2 / OpenBLAS, 1 and 16 threads): dx 8.11e-7, dp 7.24e-7, gax 7.49e-7, gam 9.24e-7, slab 6.34e-7.
LOSS_STEP_FP32 = {"dx": 9.0e-7, "dp": 8.0e-7, "gax": 8.5e-7, "gam": 1.0e-6, "slab": 7.0e-7}
LOSS_STEP_LAST_STAGE = 3e-6
LOSS_STEP_K = 8
LOSS_STEP_BOUND = {k: max(LOSS_STEP_LAST_STAGE, LOSS_STEP_K * v) for k, v in LOSS_STEP_FP32.items()}
# = dx 7.2e-6, dp 6.4e-6, gax 6.8e-6, gam 8.0e-6, slab 5.6e-6.  Observed on an MI355X, the largest over every case of
# test_gpu_loss_step.py (the tests print each figure before they assert): loss 9.0e-8 relative (6.7e-8 as the sum of the slab
# form's shares), dE 4.2e-7, dx 6.2e-7, dp 5.8e-7, gax 8.4e-7, gam 7.4e-7, slab rows 2.4e-7 of the largest entry.


# ---- the dense half of a plan's step, launcher by launcher (tests/test_gpu_dense_step.py against tests/dense_step_mirror.py in fp64) ----
# P, x_next, gW and gb keep the 3e-6 of the largest entry that test_dense_fwd and test_dense_bwd_weight hold the plain forms to; Adam keeps
# test_adam_matches_torch_semantics' 2.5e-7 x max(1, |ref|).  E, inv_den and E_B (rows_out) follow the LOSS_STEP scheme above:
# DENSE_STEP_FP32 is the error of the mirror's formulas in plain numpy float32 against float64, the largest over every case of the fused
# norm and of the row norm -- E relative to the reference's largest entry, inv_den relative per row (zero rows excluded: they are checked
# exactly).  tests/test_dense_step_mirror.py re-measures it on every run of the CPU suite (not above the record, not below a quarter of
# it).  The GPU bound is max(3e-6, 8 x that figure): 8 as above, for sequential MFMA accumulation against numpy's pairwise sums.
# Measured on the CPU (numpy 2 / OpenBLAS): E 6.48e-7, inv_den 2.07e-7.
DENSE_STEP_PLAIN = 3e-6
DENSE_STEP_ADAM = 2.5e-7
DENSE_STEP_FP32 = {"e": 7.0e-7, "inv_den": 2.3e-7}
DENSE_STEP_K = 8
DENSE_STEP_BOUND = {k: max(DENSE_STEP_PLAIN, DENSE_STEP_K * v) for k, v in DENSE_STEP_FP32.items()}
DENSE_STEP_BOUND["rows_out"] = DENSE_STEP_BOUND["e"]          # E_B copies E's rows bit for bit
# = E 5.6e-6, inv_den 3.0e-6.  Observed on an MI355X, the largest over every case of test_gpu_dense_step.py (the tests print each figure
# before they assert): P 1.9e-6, x_next 1.9e-6, AX W1^T 6.3e-7, E 1.0e-6 of the largest entry, inv_den 2.8e-7 per row, gW1 1.5e-7, gW2
# 2.0e-7, gb 1.6e-7; Adam from the state each launch reads: parameters 3.3e-8, m 1.2e-7, v 1.1e-7.


# ---- the setup ops, op by op (tests/test_gpu_setup_ops.py against tests/setup_ops_mirror.py) ------------------------------------------
# No new bound: wherever the comparison is not bit equality it is one tests/test_gpu_ops.py has always held these ops to.
SETUP_OPS_PERCENTILE_ABS = 2e-6    # |beta - np.percentile of the fp64 similarities|, unit rows (test_percentile_exact)
SETUP_OPS_KNN_RTOL = 1e-12         # kept similarities against numpy's fp64 product, tie-free rows (test_knn_topk_values_and_odd_sizes)
SETUP_OPS_ROWSUM_RTOL = 1e-13      # row sums and D^-1/2 (test_normalize_adj_matches_reference_fixture)
SETUP_OPS_AHAT_RTOL = 1.2e-7       # A_hat in fp32 against fp64 (the same test)
# Observed on an MI355X (the tests print each figure before they assert):
#   percentile, exact inputs: 35 cases, 721 percentiles at and around level boundaries, 0 differ from the mirror in any bit;
#   percentile, unit rows: 7.1e-8 (n = 129, d = 16) and 4.5e-7 (n = 1000, d = 128) of the 2e-6; the count of similarities at or below the
#     returned value off by at most half of its allowance;
#   kNN, tie-free rows: kept values 1.5e-13 relative (n = 65, d = 8, k = 64) of the 1e-12; integer descriptors: the contract holds on all
#     46 cases, windows bit-equal to the whole table;
#   normalisation: row sums 4.0e-16, D^-1/2 3.3e-16 of the 1e-13; A_hat 5.9e-8 of the 1.2e-7 against fp64, and 0 bits from the mirror
#     evaluated with the device's own D^-1/2; every shard of the asymmetric matrix and of its transpose bit-equal to A_hat.
# Non-finite similarities (n = 65, d = 16, the lattice case with one entry replaced): before gss_percentile refused them it returned
# GSS_OK with, at q = 0 / 50 / 98 / 100: one NaN entry -6.75, 0.0, NaN, NaN; one +inf entry NaN, 0.0, 7.63, NaN; two entries of 2e19
# -2e19, 0.0, 1e19, NaN.  np.percentile of these matrices is NaN at every q.  On every finite case above the results before and after
# the refusal are the same bits.

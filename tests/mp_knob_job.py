"""Child of tests/test_gpu_shards.py::test_a_rank_whose_job_wide_knob_differs_is_refused_by_name -- NOT a test module.

Run under torch.distributed.run with GSS_COMM_BACKEND=host: every rank builds its shard, then sets halo_recompute in its own process
(0 on rank 0, -1 on the others) and creates its native sharded plan.  The ranks disagree whatever the timing, so plan creation must fail
on every rank.  Rank R writes what happened to <argv[1]>/rank<R>.txt: "refused: <error>" or "created"."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

import gcn_drug_repurposing_amd as pkg  # noqa: E402
from gcn_drug_repurposing_amd._lib import GssError  # noqa: E402
from gcn_drug_repurposing_amd.dist import job_comm, job_device  # noqa: E402
from gcn_drug_repurposing_amd.shards import RmatSource, build_shard, gaussian_rows, shard_engine  # noqa: E402


def main():
    import datetime
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(job_device(int(os.environ.get("LOCAL_RANK", "0"))))
    dist.init_process_group("gloo", timeout=datetime.timedelta(seconds=60))
    lib = pkg.load()
    comm = job_comm(world, rank)
    n, m, d = 2000, 20000, 32
    shard = build_shard(RmatSource(n, m, seed=3, device="cuda"), comm, need_transpose=True, device="cuda")
    lo, hi = shard.part.rows(rank)
    w = np.eye(d, dtype=np.float32)
    params = {"W1": w, "b1": np.zeros(d, np.float32), "W2": w.copy(), "b2": np.zeros(d, np.float32)}
    assert lib.gss_debug_set_option(b"halo_recompute", 0 if rank == 0 else -1) == 0
    try:
        shard_engine(shard, gaussian_rows(lo, hi, d, 5), params, comm, num_layers=2, layer_decay=0.3, alpha=1.0, lr=1e-3, max_batch=64)
        outcome = "created"
    except GssError as e:
        outcome = f"refused: {e}"
    with open(os.path.join(sys.argv[1], f"rank{rank}.txt"), "w") as f:
        f.write(outcome)
    dist.barrier()                 # no rank leaves while a peer may still be in the comparison's all-gather
    os._exit(0)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The bootstrap and the sign-flip null of the per-indication metrics (gss_resample_stats, csrc/resample.hip) at the sizes a user runs them.

The series: S rows of n uniform values in [0, 1) (AUC-like; the time does not depend on the values).  n = 840 is the number of indications
with both classes at full size, n = 16,384 the most a call takes; S = 7 is three methods' AUCs, the same of a second metric and a
difference, S = 1 one series alone.
  1. gss_resample_stats in mode 1 (bootstrap) and mode 2 (sign flip) at B = 10^4 and 10^5 replicates: device events around the entry point
     (its finite-values check, that check's read-back and its synchronisation included), after --warmup calls the median of --reps calls;
     the output stays on the device (the wrapper's download is timed apart, at B = 10^5 and S = 7);
  2. for scale, a numpy restatement on the host: the same replicates (the mirror's draws and signs, vectorised over a block of
     replicates), np.mean and np.median along the series, for --host-replicates replicates, EXTRAPOLATED linearly to B and labelled so.
     A number to report, not a gate;
  3. three replicates of every device run against the mirror (the tests hold every bit; here: the largest absolute difference).
Writes profiles/resample_bench.json (or --out).   python tools/resample_bench.py [--reps 7] [--warmup 2]"""
import argparse
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(fn, reps, warmup):
    import torch
    ms = []
    for r in range(reps + warmup):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if r >= warmup:
            ms.append(e0.elapsed_time(e1))
    return {"ms_median": float(np.median(ms)), "ms_min": float(min(ms)), "ms_max": float(max(ms))}


def host_replicates(M, v, mode, seed, count):
    """the mirror's replicates, vectorised over the block: [count][S][2] (np.mean's own order of additions, not the kernel's)"""
    from node2vec_mirror import rng_key
    S, n = v.shape
    b = np.arange(count, dtype=np.uint64)[:, None]
    j = np.arange(n, dtype=np.uint64)[None, :]
    if mode == 1:
        h = rng_key(seed, M.TAG_BOOT_DRAW, b, j, 0)
        idx = (((h >> np.uint64(32)) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)
        x = v[:, idx].transpose(1, 0, 2)                                   # [count][S][n]
    else:
        flip = (rng_key(seed, M.TAG_SIGN_FLIP, b, j, 0) >> np.uint64(63)).astype(bool)
        x = np.where(flip[:, None, :], -v[None], v[None])
    return np.stack([x.mean(axis=2), np.median(x, axis=2)], axis=2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-replicates", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample_bench.json"))
    a = ap.parse_args()
    import torch
    import resample_mirror as M
    from gcn_drug_repurposing_amd import _lib
    from gcn_drug_repurposing_amd import resample as R
    assert torch.cuda.is_available(), "resample_bench needs the GPU: there is nothing to time without it"
    hashes = _lib.source_hashes()
    lib = _lib.load()
    assert lib.gss_source_hash(b"resample.hip").decode() == hashes["resample.hip"], "the library was not built from this tree"
    out = {"source_hash": {k: hashes[k] for k in ("resample.hip", "counter_rng.h", "rank_keys.h", "*")}, "reps": a.reps, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0), "runs": []}
    names = {1: "bootstrap", 2: "sign_flip"}
    for n in (840, 16384):
        for S in (1, 7):
            h = np.random.RandomState(n + S).rand(S, n)
            v = torch.from_numpy(h).cuda()
            host_ms = {}
            for mode in (1, 2):
                t0 = time.perf_counter()
                host = host_replicates(M, h, mode, 0, a.host_replicates)
                host_ms[mode] = (time.perf_counter() - t0) * 1e3 / a.host_replicates
                want = M.resample_stats(h, mode, 0, 3)
                assert np.max(np.abs(host[:3] - want)) <= 1e-12, "the vectorised host restatement left the mirror"
            for B in (10000, 100000):
                buf = torch.empty(B, S, 2, dtype=torch.float64, device="cuda")
                for mode in (1, 2):
                    def run():
                        _lib.check(lib.gss_resample_stats(v.data_ptr(), n, S, n, mode, 0, 0, B, buf.data_ptr(), _lib.current_stream()),
                                   "gss_resample_stats")
                    rec = {"n": n, "S": S, "B": B, "mode": names[mode], **timed(run, a.reps, a.warmup)}
                    rec["us_per_replicate_and_series"] = rec["ms_median"] * 1e3 / (B * S)
                    rec["max_abs_difference_from_mirror_3_replicates"] = float(np.max(np.abs(buf[:3].cpu().numpy() - M.resample_stats(h, mode, 0, 3))))
                    rec["numpy_host"] = {"replicates_timed": a.host_replicates, "ms_per_replicate": host_ms[mode],
                                         "EXTRAPOLATED_ms_at_B": host_ms[mode] * B,
                                         "note": "linear extrapolation from replicates_timed replicates, not a run of B replicates"}
                    out["runs"].append(rec)
                    print(json.dumps(rec), flush=True)
            if n == 840 and S == 7:
                t0 = time.perf_counter()
                R.resample_stats(v, 1, 0, 100000)
                out["wrapper_n840_S7_B100000_wall_ms"] = (time.perf_counter() - t0) * 1e3
                out["wrapper_note"] = "resample.resample_stats: the launch, the download of 11.2 MB of statistics and the host array, host clock"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    flat = re.sub(r"[\[{][^\[\]{}]*[\]}]", lambda m: re.sub(r"\s*\n\s*", " ", m.group(0)), json.dumps(out, indent=1))     # innermost lists and dicts on one line
    with open(a.out, "w") as f:
        f.write(flat + "\n")


if __name__ == "__main__":
    main()

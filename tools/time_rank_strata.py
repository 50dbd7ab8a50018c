#!/usr/bin/env python3
"""gss_rank_metrics_strata (csrc/rank_strata.hip) beside gss_rank_metrics_rows (csrc/rank_metrics.hip, the yardstick) on one set of
scores of the shape evaluate_auc.py --by-class has on the multiscale interactome: 840 indications x 1,661 drugs, 5,926 listed pairs with
at most 92 per indication, and 18,308 (indication, class) strata.

The problem is seeded and reads no file.  1,328 of the drugs carry one or two ATC codes; a code is a level-4 class out of 708 and its
parents out of 235, 90 and 14.  The strata that assignment gives are trimmed or topped up at random (seeded) to 18,308 exactly; both
counts are recorded.  After --warmup calls of each, --reps pairs of calls alternate between the two entry points, each call between two
device synchronises on the host clock (both entry points wait for the stream themselves, so this is what a caller sees).  The record has
each entry point's median, minimum, maximum and 10th / 90th percentiles.  ks = (10, 50).

Writes profiles/rank_strata_time.json (or --out).   python tools/time_rank_strata.py [--reps 200]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

R, C, PAIRS, MAX_POS, STRATA = 840, 1661, 5926, 92, 18308
CODED, CLASSES = 1328, (14, 90, 235, 708)
KS = (10, 50)


def problem(seed=0):
    """-> (scores [R, C], pos_ptr, pos_col, str_ptr, sub_ptr, sub_col, strata the class assignment gave before the adjustment)"""
    rng = np.random.RandomState(seed)
    scores = rng.randn(R, C)
    n_pos = np.ones(R, np.int64)                                                       # every row one, the rest spread with a long tail
    weight = rng.pareto(1.2, R) + 0.05
    n_pos[int(np.argmax(weight))] = MAX_POS
    while n_pos.sum() < PAIRS:
        r = rng.choice(R, p=weight / weight.sum())
        if n_pos[r] < MAX_POS:
            n_pos[r] += 1
    rows = [np.sort(rng.choice(C, n, replace=False)) for n in n_pos]
    coded = rng.choice(C, CODED, replace=False)
    classes_of = {}                                                                    # drug column -> its classes (level, index)
    for c in coded:
        for l4 in rng.choice(CLASSES[3], rng.randint(1, 3), replace=False):
            l3 = l4 * CLASSES[2] // CLASSES[3]
            l2 = l3 * CLASSES[1] // CLASSES[2]
            l1 = l2 * CLASSES[0] // CLASSES[1]
            classes_of.setdefault(int(c), set()).update({(1, l1), (2, l2), (3, l3), (4, int(l4))})
    strata = []
    for r, p in enumerate(rows):
        members = {}
        for c in p:
            for k in classes_of.get(int(c), ()):
                members.setdefault(k, []).append(int(c))
        strata.append([members[k] for k in sorted(members)])
    given = sum(len(s) for s in strata)
    total = given
    while total > STRATA:                                                              # trim ...
        r = rng.randint(R)
        if strata[r]:
            strata[r].pop(rng.randint(len(strata[r])))
            total -= 1
    while total < STRATA:                                                              # ... or top up with random subsets of a row's positives
        r = rng.randint(R)
        p = rows[r]
        strata[r].append([int(c) for c in rng.choice(p, rng.randint(1, min(len(p), 3) + 1), replace=False)])
        total += 1
    pos_ptr = np.concatenate([[0], np.cumsum(n_pos)]).astype(np.int32)
    str_ptr = np.concatenate([[0], np.cumsum([len(s) for s in strata])]).astype(np.int32)
    flat = [q for s in strata for q in s]
    sub_ptr = np.concatenate([[0], np.cumsum([len(q) for q in flat])]).astype(np.int32)
    return scores, pos_ptr, np.concatenate(rows).astype(np.int32), str_ptr, sub_ptr, np.concatenate(flat).astype(np.int32), given


def spread(ms):
    ms = np.asarray(ms)
    return {"ms_median": float(np.median(ms)), "ms_min": float(ms.min()), "ms_max": float(ms.max()), "ms_p10": float(np.percentile(ms, 10)),
            "ms_p90": float(np.percentile(ms, 90)), "calls": int(len(ms))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200, help="timed calls of each entry point, alternating (at least 200)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rank_strata_time.json"))
    a = ap.parse_args()
    if a.reps < 200:
        raise SystemExit("time_rank_strata: --reps must be at least 200")
    import torch
    from gcn_drug_repurposing_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("time_rank_strata: no GPU; nothing is measured without one")
    hashes = _lib.source_hashes()
    lib = _lib.load()
    assert lib.gss_source_hash(b"rank_strata.hip").decode() == hashes["rank_strata.hip"], "the library was not built from this tree"
    scores, pos_ptr, pos_col, str_ptr, sub_ptr, sub_col, given = problem()
    S, n_sub = len(sub_ptr) - 1, len(sub_col)
    assert (scores.shape, len(pos_col), int(np.diff(pos_ptr).max()), S) == ((R, C), PAIRS, MAX_POS, STRATA)
    d_s, d_ptr, d_col, d_sp, d_qp, d_qc = (torch.from_numpy(x).cuda() for x in (scores, pos_ptr, pos_col, str_ptr, sub_ptr, sub_col))
    ks = np.asarray(KS, np.int32)
    nk = len(KS)
    f64 = lambda n: torch.empty(n, dtype=torch.float64, device="cuda")   # noqa: E731
    i32 = lambda n: torch.empty(n, dtype=torch.int32, device="cuda")     # noqa: E731
    s_auc, s_ap, s_hits, s_pos, s_neg, sn_pos, sn_neg = f64(S), f64(S), f64(S * nk), i32(S), i32(S), i32(R), i32(R)
    r_auc, r_ap, r_hits, r_pos, r_neg = f64(R), f64(R), f64(R * nk), i32(R), i32(R)
    s_ws = torch.empty(n_sub, dtype=torch.int64, device="cuda")
    r_ws = torch.empty(R * C, dtype=torch.int64, device="cuda")
    st = _lib.current_stream()

    def strata():
        _lib.check(lib.gss_rank_metrics_strata(R, C, _lib.ptr(d_s), C, _lib.ptr(d_ptr), _lib.ptr(d_col), S, _lib.ptr(d_sp), _lib.ptr(d_qp),
                                               _lib.ptr(d_qc), nk, ks.ctypes.data, _lib.ptr(s_auc), _lib.ptr(s_ap), _lib.ptr(s_hits), _lib.ptr(s_pos),
                                               _lib.ptr(s_neg), _lib.ptr(sn_pos), _lib.ptr(sn_neg), _lib.ptr(s_ws), 8 * n_sub, st),
                   "gss_rank_metrics_strata")

    def rows():
        _lib.check(lib.gss_rank_metrics_rows(R, C, _lib.ptr(d_s), C, _lib.ptr(d_ptr), _lib.ptr(d_col), nk, ks.ctypes.data, _lib.ptr(r_auc),
                                             _lib.ptr(r_ap), _lib.ptr(r_hits), _lib.ptr(r_pos), _lib.ptr(r_neg), _lib.ptr(r_ws), 8 * R * C, st),
                   "gss_rank_metrics_rows")

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for _ in range(a.warmup):
        strata()
        rows()
    ms = {"strata": [], "rows": []}
    for _ in range(a.reps):
        ms["strata"].append(timed(strata))
        ms["rows"].append(timed(rows))
    assert torch.equal(sn_pos, r_pos) and torch.equal(sn_neg, r_neg) and not bool(torch.isnan(s_auc).any())
    out = {"device": torch.cuda.get_device_name(0), "source_hash": {k: hashes[k] for k in ("rank_strata.hip", "rank_metrics.hip", "rank_score.h", "rank_keys.h", "*")},
           "shape": {"rows": R, "columns": C, "positives": int(len(pos_col)), "max_positives_per_row": int(np.diff(pos_ptr).max()), "strata": S,
                     "strata_from_the_class_assignment": int(given), "stratum_positives": int(n_sub),
                     "max_strata_per_row": int(np.diff(str_ptr).max())},
           "ks": list(KS), "warmup": a.warmup, "clock": "host clock between two device synchronises around one call; the calls alternate",
           "gss_rank_metrics_strata": spread(ms["strata"]), "gss_rank_metrics_rows": spread(ms["rows"])}
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

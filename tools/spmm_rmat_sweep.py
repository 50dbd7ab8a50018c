#!/usr/bin/env python3
"""Round 6 experiment: can ONE pass of y = A_hat x in the HBM regime keep more of the hubs' rows in the L2s?

The launch policies the kernel has, at BASELINE config 5's size -- feature slices of 256 B (2) or 128 B (4), time-separated (grid.y) or
pinned to XCDs (slice = workgroup id mod ns), with the H hottest rows declared hot (default policy) and every other row fetched
non-temporally.  An L2 of 4 MB holds 16k rows' 256-B slices or 32k rows' 128-B slices; the index arrays are read once per slice (1.68 GB
each).  (Round 6 also timed the cold tail in a locality order, with a schedule knob since removed: profiles/r06_spmm_rmat10m_policy_sweep.txt.)

usage: spmm_rmat_sweep.py <nodes> <edges> [d]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import gcn_drug_repurposing_amd as pkg  # noqa: E402
from gcn_drug_repurposing_amd import _lib  # noqa: E402
from gcn_drug_repurposing_amd.dist import local_comms  # noqa: E402
from gcn_drug_repurposing_amd.shards import HOT_ROWS, RmatSource, build_shard  # noqa: E402

lib = pkg.load()
n, m = int(sys.argv[1]), int(sys.argv[2])
d = int(sys.argv[3]) if len(sys.argv) > 3 else 128
st = _lib.current_stream()


def opt(name, v):
    _lib.check(lib.gss_debug_set_option(name.encode(), int(v)), name)


g = build_shard(RmatSource(n, m, seed=4), local_comms(1)[0], need_transpose=False)
a = g.a
nnz = a.nnz
x = torch.randn(n, d, device="cuda")
y = torch.empty(n, d, device="cuda")
alg = 8 * nnz + 4 * (n + 1) + 8 * n * d
print(f"RMAT {n} nodes / {m} edges: nnz(A_hat) = {nnz}, d = {d}, algorithmic bytes per product {alg / 1e9:.2f} GB", flush=True)


def timed(csr, xin, reps=5):
    for _ in range(2):
        _lib.check(lib.gss_spmm(csr.handle, d, xin.data_ptr(), y.data_ptr(), None, None, st))
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        _lib.check(lib.gss_spmm(csr.handle, d, xin.data_ptr(), y.data_ptr(), None, None, st))
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def line(label, us):
    print(f"{label:100s} {us:9.1f} us   alg {alg / us / 1e6:6.3f} TB/s = {alg / us / 1e6 / 8.0:.3f} of 8 TB/s", flush=True)


def policies(csr, xin, tag, combos):
    best = None
    for ns, pin, h in combos:
        opt("spmm_slices", ns)
        opt("spmm_pin", pin)
        opt("spmm_hot_rows", h)
        us = timed(csr, xin)
        line(f"{tag}{ns} slices of {d * 4 // ns:3d} B {'pinned to XCDs ' if pin else 'time-separated'}, H = {h:6d}", us)
        if best is None or us < best[0]:
            best = (us, ns, pin, h)
    opt("spmm_slices", 0)
    opt("spmm_pin", 0)
    opt("spmm_hot_rows", -1)
    return best


us0 = timed(a, x)
line(f"the product's default (2 time-separated slices of 256 B, H = {HOT_ROWS})", us0)

combos = [(ns, pin, h) for ns in (2, 4) for pin in (0, 1) for h in (8192, 16384, 32768, 65536, 131072)]
combos += [(1, 0, 65536), (8, 1, 65536), (8, 1, 32768)]
b = policies(a, x, "", combos)
print(f"-> best launch policy: {b[1]} slices, pin = {b[2]}, H = {b[3]}: {b[0]:.1f} us ({(b[0] / us0 - 1) * 100:+.1f} % vs the default)", flush=True)

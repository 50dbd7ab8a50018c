"""-m gpu: the batched diffusion iteration (csrc/ppr.hip) step by step against tests/ppr_mirror.py (held to the oracle on every column,
and bit for bit to the two converged-run emulations, on the CPU in tests/test_ppr_mirror.py), on the inputs of tests/ppr_cases.py.

What the end-to-end comparisons of converged profiles (tests/test_diffusion.py, tests/test_gpu_knockout.py) cannot see shows here:
  * gss_ppr_run stopped by max_iter (GSS_ENOTCONV): the iterate it leaves in x after an odd and after an even number of iterations (the
    fused path's double buffer), the counts so far, the padding columns, and that nothing of such a run survives into the next;
  * intermediate iterates and iteration counts, which a fixed point forgives;
  * 32-column groups frozen and skipped for some forty iterations beside a live one, and a converged column of 150 overrides copied across
    and repaired inside a live group for as long;
  * the per-column wave loops with more than 64 and more than 128 entries (overrides, correction groups), empty correction groups, a dead
    row and group rows on override rows, knock-outs on a handle without overrides, lists set anew on a handle;
  * the product alone over three 64-column chunks, on rows of every length at which the segment schedule changes shape, bit for bit.
Why each of these is red if the code loses it (argued from csrc/ppr.hip, not demonstrated):
  * the skip rule `iters <= it - 2`: with `it - 1` a group is skipped in the iteration after its last column converged, when only one
    half of the double buffer holds that column's final values; the other half keeps its iterate before, which differs by up to n tol.
    The last columns to converge in 64..95 and in 96..99 then come back stale from every run stopped at one parity of t -- 42 or 43 --,
    far above 1e-13;
  * the copy-back of `cur`: after an odd number of fused iterations the iterate sits in the handle's buffer; without the copy x holds
    the iterate before (1/n after t = 1);
  * the `done` branch of ppr_ovr_fix_kernel: column 5 converges at about iteration 20 in a group column 6 keeps live until 65; each copy
    across reads x with the 150 override entries scaled in place, and only that branch puts the true values back;
  * the `err_corr` reset of ppr_knockout_kernel: on `directed` nothing else writes err_corr, so columns 9 and 80, which list set B no
    longer names, keep the last correction of set A, of the order of the threshold itself: other counts and bits than a fresh handle's;
  * the lane strides: with the first 64 entries only, 86 overrides of column 5 go unrepaired (a live column's error is off by far more than
    n tol and its count changes, a converged one's entries stay scaled), and 66 of column 5's 130 correction groups, one of column 20's
    65, are never added (alpha * sum is of the order of 1e-7 per entry).
gss_ppr_run is driven through ctypes (PprEngine.run raises on GSS_ENOTCONV).  Every bound is one the project already applies to this path
(1e-13 profiles, 1e-15 fused against separate) or exact equality.  No test provokes a fault: every launch gets valid arguments."""
import contextlib
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import ppr_cases as K  # noqa: E402
import ppr_mirror as M  # noqa: E402

from gcn_drug_repurposing_amd import _lib  # noqa: E402
from gcn_drug_repurposing_amd.diffusion import PprEngine  # noqa: E402

pytestmark = pytest.mark.gpu
TOL_PROFILE = 1e-13          # device against mirror / oracle: fp64, only the summation order differs (tests/test_diffusion.py)
TOL_FUSED = 1e-15            # fused against separate update (test_gpu_fused_update_equals_the_separate_update_pass)
ENOTCONV = -34
KO_STEPS = (1, 2, 7, 8)
KO_FIELDS = ("dead", "corr_ptr", "corr_grp_row", "corr_grp_col", "corr_src", "corr_val")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@contextlib.contextmanager
def fused_knob(value):
    """gss_ppr_create reads the knob: set for the creation of a handle, restored whatever happens"""
    lib = _lib.load()
    assert lib.gss_debug_set_option(b"ppr_fused", value) == 0
    try:
        yield
    finally:
        lib.gss_debug_set_option(b"ppr_fused", 1)


def engine(prob, fused=1):
    with fused_knob(fused):
        return PprEngine(prob)


def set_knockout(eng, ko, tag):
    dev = {f: torch.from_numpy(np.ascontiguousarray(getattr(ko, f))).cuda() for f in KO_FIELDS}
    eng.bufs[tag] = dev                                   # the handle keeps the pointers: the tensors live as long as the engine
    _lib.check(eng.lib.gss_ppr_set_knockout(eng.handle, _lib.ptr(dev["dead"]), len(ko.corr_grp_row), _lib.ptr(dev["corr_ptr"]),
                                            _lib.ptr(dev["corr_grp_row"]), _lib.ptr(dev["corr_grp_col"]), len(ko.corr_src),
                                            _lib.ptr(dev["corr_src"]), _lib.ptr(dev["corr_val"])), "gss_ppr_set_knockout")


def run(eng, max_iter):
    """gss_ppr_run into an x full of NaN -> (return code, x [n][kpad] on the host, iters_out [k]); the guards are checked after every run"""
    eng.x.fill_(float("nan"))
    iters = np.full(eng.prob.k, -7, dtype=np.int32)
    rc = eng.lib.gss_ppr_run(eng.handle, K.ALPHA, K.TOL, int(max_iter), eng.x.data_ptr(), iters.ctypes.data, _lib.current_stream())
    eng.check_guards()
    return rc, eng.x.cpu().numpy(), iters


def step_list(iters):
    """the iteration numbers at which a run is stopped: the first three, around the first convergence, an even and an odd one in the long
    stretch in which only the slow columns are live, and the last but one"""
    first, last = int(iters.min()), int(iters.max())
    even = (first + 3 + last) // 2 // 2 * 2
    ts = [1, 2, 3, first - 1, first, first + 1, first + 2, first + 3, even, even + 1, last - 1]
    assert 3 < first - 1 and first + 3 < even and even + 1 < last - 1, (first, last)
    assert np.sort(iters)[-len(K.ISOLATED)] > even + 1 and np.sort(iters)[-len(K.ISOLATED) - 1] < even - 2    # inside the long stretch
    return ts


_mirror, _device, _oracle = {}, {}, {}


def mirror(name, which=None, ts=()):
    """{t: (x, iters, done, err_history)} of the case, with or without a knock-out list set; MAX_ITER holds the converged state"""
    key = (name, which, tuple(ts))
    if key not in _mirror:
        ko = None if which is None else K.knockout_lists(name, which)
        _mirror[key] = M.snapshots(K.problem(name), K.ALPHA, K.TOL, list(ts) + [K.MAX_ITER], ko)
        assert _mirror[key][K.MAX_ITER][2].all()
    return _mirror[key]


def spread_steps():
    return step_list(mirror("spread")[K.MAX_ITER][1])


def oracle(name):
    if name not in _oracle:
        from oracle.diffusion_oracle import diffusion_profile
        m0, starts, proteins_of = K.graph(name)
        res = [diffusion_profile(m0, int(s), proteins_of, K.ALPHA, K.MAX_ITER, K.TOL) for s in starts]
        _oracle[name] = (np.stack([r[0] for r in res], axis=1), np.array([r[1] for r in res]))
    return _oracle[name]


def device_runs(fused):
    """spread on one handle: stopped at every t of spread_steps(), then converged, converged again, converged after a run stopped at an
    even and at an odd t, and converged on a fresh handle -> {t or name: (rc, x, iters)}"""
    if fused not in _device:
        prob, ts = K.problem("spread"), spread_steps()
        eng = engine(prob, fused)
        out = {t: run(eng, t) for t in ts}
        out["converged"] = run(eng, K.MAX_ITER)
        out["again"] = run(eng, K.MAX_ITER)
        for t in ts[-3:-1]:
            assert run(eng, t)[0] == ENOTCONV
            out["after", t] = run(eng, K.MAX_ITER)
        out["fresh"] = run(engine(prob, fused), K.MAX_ITER)
        _device[fused] = out
    return _device[fused]


@pytest.mark.parametrize("fused", [1, 0])
def test_iterate_and_counts_after_exactly_t_steps(fused):
    prob, ts = K.problem("spread"), spread_steps()
    ref, runs = mirror("spread", None, ts), device_runs(fused)
    k = prob.k
    for t in ts:
        rc, x, iters = runs[t]
        want, want_it, done, _ = ref[t]
        worst = np.abs(x[:, :k] - want).max()
        print(f"fused={fused} t={t}: rc {rc}, max |device - mirror| {worst:.3g}, converged {int(done.sum())} of {k}, max x {x[:, :k].max():.6g}")
        assert rc == ENOTCONV, (t, rc)
        assert worst <= TOL_PROFILE and x[:, :k].max() <= 1.0, (t, worst)
        assert np.array_equal(iters, want_it), (t, np.flatnonzero(iters != want_it))
        assert np.array_equal(iters != 0, done) and (x[:, k:] == 0).all(), t
    rc, x, iters = runs["converged"]
    want, want_it = oracle("spread")
    worst = np.abs(x[:, :k] - want).max()
    print(f"fused={fused} converged: rc {rc}, max |device - oracle| {worst:.3g}, iterations {np.unique(iters)}")
    assert rc == 0 and worst <= TOL_PROFILE and np.array_equal(iters, want_it) and (x[:, k:] == 0).all()
    assert np.abs(x[:, :k] - ref[K.MAX_ITER][0]).max() <= TOL_PROFILE
    for other in ["again", "fresh"] + [("after", t) for t in ts[-3:-1]]:          # no state survives a run, one ended by max_iter included
        rc2, x2, iters2 = runs[other]
        assert rc2 == 0 and np.array_equal(bits(x2), bits(x)) and np.array_equal(iters2, iters), other


def test_fused_update_equals_the_separate_pass_at_every_step():
    ts = spread_steps()
    a, b = device_runs(1), device_runs(0)
    for t in ts + ["converged"]:
        (rc1, x1, it1), (rc0, x0, it0) = a[t], b[t]
        worst = np.abs(x1 - x0).max()
        print(f"t={t}: max |fused - separate| {worst:.3g}")
        assert rc1 == rc0 and np.array_equal(it1, it0), (t, np.flatnonzero(it1 != it0))     # the same counts, hence the same done set
        assert worst <= TOL_FUSED, (t, worst)


def test_product_alone_on_the_schedule_edges_is_exact():
    prob = K.problem("schedule")
    eng = engine(prob)
    rng = np.random.RandomState(5)
    xh = rng.randint(-4, 5, (prob.n, prob.kpad)).astype(np.float64)
    ref = prob.mt @ xh                                     # integers below 2^53: exact in any summation order
    assert np.array_equal(ref, np.rint(ref)) and np.abs(ref).max() > 100
    x = torch.from_numpy(xh).cuda()
    y = torch.full((prob.n, prob.kpad), float("nan"), dtype=torch.float64, device="cuda")
    eng.spmm(x, y)
    eng.check_guards()
    got = y.cpu().numpy()
    bad = np.argwhere(got != ref)
    assert torch.equal(y, torch.from_numpy(ref).cuda()), (len(bad), bad[:5], np.diff(prob.mt.indptr)[bad[:5, 0]])
    empty = np.flatnonzero(np.diff(prob.mt.indptr) == 0)
    assert len(empty) >= 3 and (got[empty] == 0).all()
    y2 = torch.full_like(y, float("nan"))
    eng.spmm(x, y2)
    assert torch.equal(y.view(torch.int64), y2.view(torch.int64))
    assert torch.equal(x, torch.from_numpy(xh).cuda())     # the operand is left alone


def test_product_alone_on_the_spread_matrix_against_long_double():
    prob = K.problem("spread")
    eng = engine(prob)
    xh = np.random.RandomState(6).randn(prob.n, prob.kpad)
    ref = (sp.csr_matrix(prob.mt, dtype=np.longdouble) @ xh.astype(np.longdouble)).astype(np.float64)
    x = torch.from_numpy(xh).cuda()
    y = torch.full((prob.n, prob.kpad), float("nan"), dtype=torch.float64, device="cuda")
    eng.spmm(x, y)
    eng.check_guards()
    got = y.cpu().numpy()
    worst = np.abs(got - ref).max()
    print(f"max |device - long double| {worst:.3g}, max |ref| {np.abs(ref).max():.3g}")
    assert worst < 1e-13 * max(1.0, np.abs(ref).max())
    assert (got[np.diff(prob.mt.indptr) == 0] == 0).all()
    y2 = torch.full_like(y, float("nan"))
    eng.spmm(x, y2)
    assert torch.equal(y.view(torch.int64), y2.view(torch.int64))


@pytest.mark.parametrize("name", ["spread", "directed"])
def test_knockout_iterates_against_the_mirror(name):
    """spread: a handle with overrides (has_ovr = 1: ppr_ovr_fix_kernel writes err_corr, ppr_knockout_kernel adds to it); directed: one
    without (has_ovr = 0: ppr_knockout_kernel alone owns err_corr, and resets it for a column the lists no longer name)"""
    prob = K.problem(name)
    a, b = K.knockout_lists(name, "A"), K.knockout_lists(name, "B")
    assert (len(prob.ovr_col) > 0) == (name == "spread")
    k = prob.k
    ref = mirror(name, "A", KO_STEPS)
    plain, eng = engine(prob), engine(prob)
    set_knockout(eng, a, "A")
    untouched = np.setdiff1d(np.arange(k), K.touched_columns(a))
    for t in KO_STEPS + (K.MAX_ITER,):
        rc, x, iters = run(eng, t)
        want, want_it, done, _ = ref[t]
        worst = np.abs(x[:, :k] - want).max()
        print(f"{name} t={t}: rc {rc}, max |device - mirror| {worst:.3g}, iterations {np.unique(iters)}")
        assert rc == (0 if t == K.MAX_ITER else ENOTCONV), (t, rc)
        assert worst <= TOL_PROFILE and np.array_equal(iters, want_it) and (x[:, k:] == 0).all(), (t, worst, np.flatnonzero(iters != want_it))
        # a column no list touches has the bits of a handle on which gss_ppr_set_knockout was never called
        rc_p, x_p, it_p = run(plain, t)
        assert np.array_equal(bits(x[:, untouched]), bits(x_p[:, untouched])) and np.array_equal(iters[untouched], it_p[untouched]), t
    # a dead row keeps its exact 0, also where its 32-column group froze and was skipped long before the run ended
    listed = np.flatnonzero(a.dead >= 0)
    at = x[a.dead[listed], listed]
    assert (at == 0).all() and not np.signbit(at).any(), listed[at != 0]
    skipped = [c for c in listed if iters[c // 32 * 32:min(k, c // 32 * 32 + 32)].max() + 10 < iters.max()]
    assert any(c >= 64 for c in skipped), (skipped, iters[listed])
    # lists set anew on the handle: the bits of a fresh handle given the same lists
    set_knockout(eng, b, "B")
    rc, x, iters = run(eng, K.MAX_ITER)
    fresh = engine(prob)
    set_knockout(fresh, b, "B")
    rc_f, x_f, it_f = run(fresh, K.MAX_ITER)
    assert rc == 0 and rc_f == 0 and np.array_equal(bits(x), bits(x_f)) and np.array_equal(iters, it_f), np.flatnonzero(iters != it_f)
    want, want_it, _, _ = mirror(name, "B")[K.MAX_ITER]
    assert np.abs(x[:, :k] - want).max() <= TOL_PROFILE and np.array_equal(iters, want_it)
    for c in K.KO_DROPPED_IN_B:                           # and the columns B left out are back at the handle-without-knock-outs bits
        assert np.array_equal(bits(x[:, c]), bits(x_p[:, c])) and iters[c] == it_p[c], c

"""GPU: gene knock-outs as columns of the batched power iteration (gss_ppr_set_knockout, csrc/ppr.hip) on the 111-node fixture graph and
on the 15-node edge-case graph of knockout_mirror.py, against the mirror (the knocked-out graph rebuilt, the unchanged oracle) and the
reference's own vectors; the bit-level promises (a column without a gene and a handle without knock-outs have the bits of
diffusion_profiles, two runs are bit-equal), the dead entry's exact zero, the guards, and the refusals of the entry point."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import knockout_mirror as KM  # noqa: E402

from gcn_drug_repurposing_amd import _lib  # noqa: E402
from gcn_drug_repurposing_amd.diffusion import PprEngine, diffusion_profiles  # noqa: E402
from gcn_drug_repurposing_amd.knockout import KnockoutProblem, _engine, knockout_profiles  # noqa: E402

pytestmark = pytest.mark.gpu
TOL_PROFILE = 1e-13


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def fixture_case():
    fx = KM.fixture()
    return KM.small_graph(), [(str(s), str(x) or None) for s, x in zip(fx["starts"], fx["genes"])], fx["profiles"]


CASES = {"fixture": fixture_case, "edge": lambda: (KM.edge_case_graph(), KM.EDGE_COLUMNS, None)}
_mirror = {}


def mirror_of(case):
    """the case's graph, columns, reference vectors (fixture only) and the mirror's (profile, iterations) per column, computed once; every
    column's last error is checked to be clear of the threshold, so that the iteration counts are comparable"""
    if case not in _mirror:
        g, columns, ref = CASES[case]()
        mir = [KM.mirror_profile(g, KM.WEIGHTS, s, x) for s, x in columns]
        for s, x in columns:
            assert KM.last_error_margin(g, KM.WEIGHTS, s, x) > 1e-9, (s, x)
        _mirror[case] = (g, columns, ref, mir)
    return _mirror[case]


def plain_profiles(g, starts):
    """diffusion_profiles() of the same start nodes: the engine as it was before knock-outs"""
    from gcn_drug_repurposing_amd.knockout import weighted_csr
    m0, names, _ = weighted_csr(g, KM.WEIGHTS)
    idx = {n: i for i, n in enumerate(names)}
    prots = {idx[s]: sorted(idx[p] for p in g.drug_or_indication2proteins[s]) for s in g.drugs_in_graph + g.indications_in_graph}
    return diffusion_profiles(m0, [idx[s] for s in starts], prots, KM.ALPHA, KM.MAX_ITER, KM.TOL)


@pytest.mark.parametrize("case", ["fixture", "edge"])
def test_profiles_against_the_mirror_and_the_reference(case):
    g, columns, ref, mir = mirror_of(case)
    eng = _engine(KnockoutProblem(g, KM.WEIGHTS, columns))
    x, iters = eng.run(KM.ALPHA, KM.TOL, KM.MAX_ITER)
    first = x.clone()
    x2, iters2 = eng.run(KM.ALPHA, KM.TOL, KM.MAX_ITER)
    assert torch.equal(first.view(torch.int64), x2.view(torch.int64)) and np.array_equal(iters, iters2)      # two runs are bit-equal
    eng.check_guards()
    got = first[:, :len(columns)].t().contiguous().cpu().numpy()
    assert bool((first[:, len(columns):] == 0).all())
    for c, ((s, gene), (prof, it)) in enumerate(zip(columns, mir)):
        worst = np.max(np.abs(got[c] - prof))
        print(case, s, gene, "max |device - mirror|", worst, "iterations", iters[c], it)
        assert worst <= TOL_PROFILE and iters[c] == it, (s, gene, worst, iters[c], it)
        if ref is not None:
            assert np.max(np.abs(got[c] - ref[c])) <= TOL_PROFILE, (s, gene)
        assert abs(got[c].sum() - 1.0) <= 1e-12, (s, gene, got[c].sum())
        if gene is not None:
            at = got[c][g.names.index(gene)]
            assert at == 0.0 and not np.signbit(at), (s, gene, at)
    # a column without a gene has the bits diffusion_profiles gives its start node
    plain = [c for c, (_, gene) in enumerate(columns) if gene is None]
    want, want_it = plain_profiles(g, [columns[c][0] for c in plain])
    assert np.array_equal(bits(got[plain]), bits(want)) and np.array_equal(iters[plain], want_it)


def test_a_handle_without_knockouts_keeps_its_bits():
    g, columns, _, _ = mirror_of("fixture")
    starts = [s for s, _ in columns]
    want, want_it = plain_profiles(g, starts)
    prob = KnockoutProblem(g, KM.WEIGHTS, [(s, None) for s in starts])
    assert len(prob.corr_src) == 0 and (prob.dead == -1).all()
    for make in (PprEngine, _engine):                       # never set; set with nothing in it
        eng = make(prob)
        x, iters = eng.run(KM.ALPHA, KM.TOL, KM.MAX_ITER)
        eng.check_guards()
        assert np.array_equal(bits(x[:, :len(starts)].t().contiguous().cpu().numpy()), bits(want)), make.__name__
        assert np.array_equal(iters, want_it)


@pytest.mark.parametrize("k", [1, 65])
def test_one_column_and_a_batch_across_the_padding_boundary(k):
    g, columns, _, mir = mirror_of("edge")
    pick = [c % len(columns) for c in range(2, 2 + k)]      # k = 1: (D2, G); k = 65: kpad 128, every column several times
    prof, iters = knockout_profiles(g, KM.WEIGHTS, [columns[c] for c in pick], KM.ALPHA, KM.MAX_ITER, KM.TOL)
    for j, c in enumerate(pick):
        assert np.max(np.abs(prof[j] - mir[c][0])) <= TOL_PROFILE and iters[j] == mir[c][1], (k, columns[c])
    seen = {}
    for j, c in enumerate(pick):                            # a column has the same bits wherever it stands in the batch
        assert np.array_equal(bits(prof[seen.setdefault(c, j)]), bits(prof[j])), (k, columns[c])
    if k == 65:
        halves, its = knockout_profiles(g, KM.WEIGHTS, [columns[c] for c in pick], KM.ALPHA, KM.MAX_ITER, KM.TOL, max_columns=40)
        assert np.array_equal(bits(halves), bits(prof)) and np.array_equal(its, iters)      # chunks change nothing


def test_set_knockout_refusals_by_name():
    g, columns, _, _ = mirror_of("edge")
    prob = KnockoutProblem(g, KM.WEIGHTS, columns)
    eng = PprEngine(prob)
    lib = eng.lib
    i32 = lambda v: torch.tensor(np.asarray(v, dtype=np.int32), dtype=torch.int32, device="cuda")   # noqa: E731
    f64 = lambda v: torch.tensor(np.asarray(v, dtype=np.float64), dtype=torch.float64, device="cuda")   # noqa: E731
    k, n = prob.k, prob.n
    dead = prob.dead.copy()
    start0 = int(prob.starts[0])
    free = [r for r in range(n) if r != start0 and r != dead[0]][:3]
    good = dict(dead=dead, ptr=[0, 1, 2], row=[free[0], free[1]], col=[0, 0], src=[free[2], free[2]], val=[0.0, 0.0])

    def call(**over):
        a = dict(good, **over)
        keep = [i32(a["dead"]), i32(a["ptr"]), i32(a["row"]), i32(a["col"]), i32(a["src"]), f64(a["val"])]
        rc = lib.gss_ppr_set_knockout(eng.handle, _lib.ptr(keep[0]), len(a["row"]), _lib.ptr(keep[1]),
                                      _lib.ptr(keep[2]), _lib.ptr(keep[3]), len(a["src"]), _lib.ptr(keep[4]), _lib.ptr(keep[5]))
        return rc, lib.gss_last_error().decode(errors="replace")

    bad = dead.copy(); bad[1] = n
    own = dead.copy(); own[0] = start0
    cases = [(dict(dead=bad), f"dead[1] = {n} is outside [-1, n={n})"),
             (dict(dead=own), f"dead[0] = {start0} is the column's own start node"),
             (dict(ptr=[0, 1, 1]), "corr_ptr runs from 0 to 1, not from 0 to n_corr=2"),
             (dict(ptr=[0, 3, 2]), "corr_ptr decreases at group 1"),
             (dict(col=[0, k]), f"corr_grp_col[1] = {k} is outside [0, k={k})"),
             (dict(row=[free[0], n]), f"corr_grp_row[1] = {n} is outside [0, n={n})"),
             (dict(row=[free[1], free[0]]), "correction group 1 is not above its predecessor"),
             (dict(row=[free[0], free[0]]), "correction group 1 is not above its predecessor"),
             (dict(row=sorted([free[0], start0])), "sits on the start node of its column 0"),
             (dict(row=sorted([free[0], int(dead[0])])), "sits on the dead row of its column 0"),
             (dict(src=[free[2], -1]), f"corr_src[1] = -1 is outside [0, n={n})")]
    for over, message in cases:
        rc, msg = call(**over)
        assert rc == -22 and message in msg, (message, rc, msg)
    rc = lib.gss_ppr_set_knockout(eng.handle, None, 0, None, None, None, 0, None, None)
    assert rc == -22 and "dead is null" in lib.gss_last_error().decode()
    # what is refused before any list is read: the counts and the pointers themselves
    d, q, r, cc, sr, vl = i32(dead), i32([0, 1, 2]), i32(good["row"]), i32([0, 0]), i32(good["src"]), f64(good["val"])
    P = _lib.ptr
    raw = [((None, P(d), 0, None, None, None, 0, None, None), "null handle"),
           ((eng.handle, P(d), -1, P(q), P(r), P(cc), 2, P(sr), P(vl)), "n_grp=-1, n_corr=2 must be in [0, 2^31)"),
           ((eng.handle, P(d), 1 << 31, P(q), P(r), P(cc), 2, P(sr), P(vl)), "n_grp=2147483648, n_corr=2 must be in [0, 2^31)"),
           ((eng.handle, P(d), 2, P(q), P(r), P(cc), -1, P(sr), P(vl)), "n_grp=2, n_corr=-1 must be in [0, 2^31)"),
           ((eng.handle, P(d), 2, P(q), P(r), P(cc), 1 << 31, P(sr), P(vl)), "n_grp=2, n_corr=2147483648 must be in [0, 2^31)"),
           ((eng.handle, P(d), 2, None, P(r), P(cc), 2, P(sr), P(vl)), "correction group lists missing"),
           ((eng.handle, P(d), 2, P(q), None, P(cc), 2, P(sr), P(vl)), "correction group lists missing"),
           ((eng.handle, P(d), 2, P(q), P(r), None, 2, P(sr), P(vl)), "correction group lists missing"),
           ((eng.handle, P(d), 2, P(q), P(r), P(cc), 2, None, P(vl)), "correction entry lists missing"),
           ((eng.handle, P(d), 2, P(q), P(r), P(cc), 2, P(sr), None), "correction entry lists missing"),
           ((eng.handle, P(d), 0, None, None, None, 2, P(sr), P(vl)), "n_corr=2 entries without a group")]
    for args, message in raw:
        rc = lib.gss_ppr_set_knockout(*args)
        msg = lib.gss_last_error().decode(errors="replace")
        assert rc == -22 and message in msg, (message, rc, msg)
    rc, msg = call()                                         # and the well-formed lists are taken
    assert rc == 0, msg
    eng.check_guards()
    assert lib.gss_debug_set_option(b"ppr_fused", 0) == 0    # a handle with the separate update pass refuses knock-outs, never ignores them
    try:
        unfused = PprEngine(prob)
        eng, was = unfused, eng
        rc, msg = call()
        assert rc == -22 and "knock-outs need the fused update" in msg, msg
        eng = was
    finally:
        lib.gss_debug_set_option(b"ppr_fused", 1)

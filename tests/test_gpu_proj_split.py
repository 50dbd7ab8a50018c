"""-m gpu: knob proj_split -- a layer's forward projection as two launches, the AX half on the plan's side stream beside the layer's
second SpMM (dense.hip PART 1 / PART 2, plan.hip plan_forward_impl).

The contract is bit identity with the one-launch form: every output runs the same MFMA sequence from the same starting value.  So every
comparison here is torch.equal between two plans built from the same inputs, one with proj_split=0 and one with proj_split=1.  The shapes
are the smallest that reach every path: N = 300 is two full 128-node tiles and a 44-row partial one; N = 100 with B = N puts every row of a
partial tile into the E_B scatter of the fused-normalise epilogue."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

BETA = 0.2
STEPS = 3


@functools.lru_cache(maxsize=None)
def _inputs(n, d):
    from gcn_drug_repurposing_amd.graph import GssGraph, knn_descriptor_adj
    rng = np.random.RandomState(1000 * n + d)
    X = (rng.randn(n, d) / 8).astype(np.float32)
    graph = GssGraph(knn_descriptor_adj(X.astype(np.float64), 5))
    w = (rng.randn(2, d, d) * 5e-2).astype(np.float32)
    b = (rng.randn(2, d) * 1e-2).astype(np.float32)
    params = (w[0] + np.eye(d, dtype=np.float32), b[0], w[1], b[1])
    return graph, X, params, rng.randint(0, 2 ** 31 - 1)


def _batches(n, b, seed):
    rng = np.random.RandomState(seed)
    return [rng.permutation(n)[:b].astype(np.int32) for _ in range(STEPS)]


def _engine(n, d, L, b, split, cache=False):
    import gcn_drug_repurposing_amd as pkg
    from gcn_drug_repurposing_amd.engine import GssEngine
    lib = pkg.load()
    graph, X, params, _ = _inputs(n, d)
    assert lib.gss_debug_set_option(b"proj_split", split) == 0, lib.gss_last_error().decode()
    try:   # a plan snapshots the knobs when it is created
        return GssEngine(graph, torch.from_numpy(X).cuda(), [torch.from_numpy(p.copy()).cuda() for p in params], num_layers=L,
                         layer_decay=0.3, alpha=1.0, lr=1e-3, max_batch=b, cache_layer1=cache)
    finally:
        lib.gss_debug_set_option(b"proj_split", -1)


def _state(eng, emb_rows=None):
    """what a step leaves behind, as copies enqueued on the current stream (no synchronisation here)"""
    emb = eng.emb if emb_rows is None else eng.emb.index_select(0, emb_rows.long())
    out = {"loss": eng.loss.clone(), "emb": emb.clone()}
    for k, g in enumerate(eng.grads):
        out[f"grad{k}"] = g.clone()
    for k, p in enumerate(eng.params):
        out[f"param{k}"] = p.clone()
    return out


def _trajectory(n, d, L, b, split, how="step", cache=False):
    """STEPS steps; the state after every one of them (P of every layer the step computed on all rows included)"""
    eng = _engine(n, d, L, b, split, cache)
    states = []
    for idx in _batches(n, b, _inputs(n, d)[3]):
        t = torch.from_numpy(idx).cuda()
        if how == "step":
            eng.step(t, BETA)
        elif how == "lazy":
            eng.step_lazy(t, BETA)
        else:
            eng.forward()
            eng.loss_backward(t, BETA)
            eng.adam()
        st = _state(eng, t if how == "lazy" else None)
        for l in range(L - 1 if how == "lazy" else L):   # (a lazy step evaluates the top layer on the batch rows only)
            st[f"P{l}"] = eng.activation(l, "P")
        states.append(st)
        eng.check_guards()
    torch.cuda.synchronize()
    return states


@functools.lru_cache(maxsize=None)
def _reference(n, d, L, b, cache=False):
    """the one-launch form, computed once per shape and shared"""
    return _trajectory(n, d, L, b, 0, cache=cache)


def _assert_same(got, ref, what, keys=None):
    assert len(got) == len(ref)
    for s, (a, r) in enumerate(zip(got, ref)):
        for k in (keys or a.keys()):
            assert torch.equal(a[k], r[k]), (what, "step", s, k)
        assert bool(torch.isfinite(a["loss"]).all()), (what, s)


SHAPES = [(300, 128, 2, 64), (300, 64, 2, 64), (300, 256, 2, 64), (300, 128, 1, 64), (300, 128, 3, 64), (100, 128, 2, 100)]


@pytest.mark.parametrize("n,d,L,b", SHAPES, ids=lambda v: str(v))
def test_two_launch_projection_is_bit_identical(n, d, L, b):
    """loss, embeddings, P of every layer, the four gradients and the parameters after Adam, step by step"""
    _assert_same(_trajectory(n, d, L, b, 1), _reference(n, d, L, b), (n, d, L, b))


def test_the_split_really_runs_two_launches_per_layer_and_profiles_both():
    """with profiling on each half is bracketed on the stream it runs on: 2 L forward-projection launches per step instead of L"""
    n, d, L, b = 300, 128, 2, 64
    idx = torch.from_numpy(_batches(n, b, 7)[0]).cuda()
    counts = {}
    for split in (0, 1):
        eng = _engine(n, d, L, b, split)
        eng.profile(True)
        eng.step(idx, BETA)
        ms, cnt = eng.profile_read()["dense_fwd"]
        counts[split] = cnt
        assert ms > 0.0
        eng.profile(False)
    assert counts == {0: L, 1: 2 * L}


def test_a_width_without_a_staged_template_keeps_one_launch():
    """d = 48: proj_split=1 changes nothing and raises nothing"""
    n, d, L, b = 300, 48, 2, 64
    _assert_same(_trajectory(n, d, L, b, 1), _reference(n, d, L, b), "d=48")
    eng = _engine(n, d, L, b, 1)
    eng.profile(True)
    eng.step(torch.from_numpy(_batches(n, b, 7)[0]).cuda(), BETA)
    assert eng.profile_read()["dense_fwd"][1] == L


def test_lazy_step_with_the_split_matches_the_full_step_without():
    """gss_plan_step_lazy: the layers below the top one split, the top layer's row-list kernel does not; the lazy step's own contract
    (loss, gradients, parameters, the batch rows' embeddings as in the full step) holds across the knob"""
    n, d, L, b = 300, 128, 2, 64
    ref = _reference(n, d, L, b)
    idxs = [torch.from_numpy(i).cuda().long() for i in _batches(n, b, _inputs(n, d)[3])]
    ref_rows = [dict(r, emb=r["emb"].index_select(0, i)) for r, i in zip(ref, idxs)]
    got = _trajectory(n, d, L, b, 1, how="lazy")
    _assert_same(got, ref_rows, "lazy", keys=list(got[0].keys()))


def test_kept_layer1_takes_the_one_launch_path_from_the_second_step():
    """cache_layer1: from the second step on layer 1 runs no SpMM, so there is nothing to hide its first half under"""
    n, d, L, b = 300, 128, 2, 64
    _assert_same(_trajectory(n, d, L, b, 1, cache=True), _reference(n, d, L, b, True), "cache_layer1")
    eng = _engine(n, d, L, b, 1, cache=True)
    idx = torch.from_numpy(_batches(n, b, 7)[0]).cuda()
    eng.step(idx, BETA)
    eng.profile(True)
    eng.step(idx, BETA)
    assert eng.profile_read()["dense_fwd"][1] == 1 + 2 * (L - 1)


def test_phase_wise_entry_points_give_the_same_bits():
    """gss_plan_forward, then gss_plan_loss_backward and gss_plan_adam.  With the split they give the bits of the same calls without it,
    step after step, and the bits of gss_plan_step without it for the whole first step -- forward, loss, gradients and the parameters after
    Adam.  (Later steps are not compared with gss_plan_step: its fused reduce + Adam kernel and gss_plan_adam's stand-alone kernel round
    the second update differently in the last bit, with the knob off as well, so the two trajectories part there whatever the knob says.)"""
    n, d, L, b = 300, 128, 2, 64
    got = _trajectory(n, d, L, b, 1, how="phases")
    _assert_same(got, _trajectory(n, d, L, b, 0, how="phases"), "phases")
    _assert_same(got[:1], _reference(n, d, L, b)[:1], "phases against the whole step")


def test_steps_on_a_non_default_stream_are_ordered_after_both_halves():
    """the same steps enqueued on a torch side stream; right after step() returns, P, the embeddings and the parameters are copied on
    that stream -- no device-wide synchronisation in between -- and must be what the reference plan computed"""
    n, d, L, b = 300, 128, 2, 64
    ref = _reference(n, d, L, b)
    eng = _engine(n, d, L, b, 1)
    idxs = [torch.from_numpy(i).cuda() for i in _batches(n, b, _inputs(n, d)[3])]
    torch.cuda.synchronize()   # (the inputs were made on the default stream)
    s = torch.cuda.Stream()
    got = []
    with torch.cuda.stream(s):
        for t in idxs:
            eng.step(t, BETA)
            st = _state(eng)
            for l in range(L):
                st[f"P{l}"] = eng.activation(l, "P")
            got.append(st)
    s.synchronize()
    _assert_same(got, ref, "stream")

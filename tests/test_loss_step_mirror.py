"""CPU: the fp64 mirror of the plan's loss step (tests/loss_step_mirror.py) is tied to torch autograd in float64, its slab form to its
replicated form, and the inputs of tests/test_gpu_loss_step.py (tests/loss_step_cases.py) to the guard that keeps every pair away
from the discontinuity of G at S = 0.  The last test evaluates the mirror's formulas in plain numpy float32 on every GPU case: the
distance to float64 is what tests/tolerances.py derives the GPU bounds of the composite outputs from."""
import numpy as np
import pytest

import loss_step_cases as K
import loss_step_mirror as M
import tolerances as T

torch = pytest.importorskip("torch")


def rel(got, ref, scale=None):
    return np.abs(np.asarray(got, np.float64) - ref).max() / max(np.abs(ref).max() if scale is None else scale, 1e-300)


def autograd_model(d, b, n, beta, alpha, c, seed):
    """x = p_prev + c elu(p); emb = F.normalize(x); the loss on emb[idx] -> everything the mirror needs, and autograd's gradients"""
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(n, d, dtype=torch.float64, generator=g, requires_grad=True)
    p_prev = torch.randn(n, d, dtype=torch.float64, generator=g)
    p_prev[:, 0] += 1.0
    idx = torch.randperm(n, generator=g)[:b]
    x = p_prev + c * torch.nn.functional.elu(p)
    x.retain_grad()
    emb = torch.nn.functional.normalize(x)
    e_b = emb[idx]
    loss = (-0.5 * alpha * (torch.relu(e_b @ e_b.T) - beta) ** 2).mean()
    loss.backward()
    return dict(p=p.detach().numpy(), idx=idx.numpy(), e_b=e_b.detach().numpy(), inv_den=(1.0 / x.detach().norm(dim=1)).numpy(),
                loss=loss.item(), dx=x.grad.numpy(), dp=p.grad.numpy())


@pytest.mark.parametrize("d,b,beta", [(16, 1, 0.25), (64, 17, 0.25), (48, 65, 0.0), (128, 40, -0.3), (192, 33, 0.9)])
def test_mirror_gradients_are_autograds(d, b, beta):
    n, alpha, c = b + 9, 1.7, 0.4
    a = autograd_model(d, b, n, beta, alpha, c, seed=d + b)
    m = M.step(a["e_b"], beta, alpha, a["inv_den"], a["p"], c, rows=a["idx"])
    assert abs(m["loss"] - a["loss"]) <= 1e-12 * abs(a["loss"])
    assert rel(m["dx"], a["dx"][a["idx"]], m["scale"]["dx"]) <= 1e-12              # d loss / d x on the batch rows
    assert rel(m["dp"], a["dp"][a["idx"]], m["scale"]["dp"]) <= 1e-12              # d loss / d p
    off = np.setdiff1d(np.arange(n), a["idx"])
    assert not a["dx"][off].any() and not a["dp"][off].any()     # nothing else has a gradient: the batch rows are all there is
    # the per-member form is the same arithmetic on gathered operands; keep == 0 zeroes a row and nothing else
    keep = (np.arange(b) % 3 != 0).astype(np.float32)
    k = M.step(a["e_b"], beta, alpha, a["inv_den"][a["idx"]], a["p"][a["idx"]], c, keep=keep)
    assert np.array_equal(k["dx"][keep != 0], m["dx"][keep != 0]) and np.array_equal(k["dp"][keep != 0], m["dp"][keep != 0])
    assert not k["dx"][keep == 0].any() and not k["dp"][keep == 0].any()


def test_input_gradient_rows_follow_dgrad_all():
    c = K.case("recipe", 64, 17)
    masked = K.reference("recipe", 64, 17, "member", True, False)
    every = K.reference("recipe", 64, 17, "member", True, True)
    free = M.step(c["e_b"], c["beta"], c["alpha"], c["inv_b"], c["p_b"], c["c"], w1t=c["w1t"], w2t=c["w2t"])
    kept = c["keep"] != 0
    assert not masked["gax"][~kept].any() and not masked["gam"][~kept].any()
    assert np.array_equal(every["gax"], free["gax"]) and np.array_equal(every["gam"], free["gam"])
    assert np.array_equal(every["gax"][kept], masked["gax"][kept])
    assert np.array_equal(every["dp"], masked["dp"]) and not every["dp"][~kept].any()     # dx_b / dp_b stay masked either way
    assert rel(free["gax"], free["dp"] @ c["w1t"].astype(np.float64).T) == 0


@pytest.mark.parametrize("parts", [2, 3, 8])
@pytest.mark.parametrize("d,b", [(64, 17), (128, 65), (192, 333)])
def test_slab_form_equals_the_replicated_form(d, b, parts):
    """parts = 8 at b = 17 (2 tiles) and at b = 65 (5 tiles): more ranks than tiles"""
    c = K.case("recipe", d, b)
    loss, de = M.sweep(c["e_b"], c["beta"], c["alpha"])
    bufs = [M.slab_rank(c["e_b"], c["beta"], c["alpha"], r, parts) for r in range(parts)]
    ntiles = -(-b // 16)
    for r, x in enumerate(bufs):
        mine = M.slab_tiles(b, r, parts)
        assert mine.any() == (r < ntiles)
        assert not x[:-1].reshape(b, d)[~mine].any()
        if r >= ntiles:
            assert not x.any()                          # a rank without a tile: all zeros, the loss share too
    assert sum(M.slab_tiles(b, r, parts).astype(int) for r in range(parts)).tolist() == [1] * b
    de2, loss2 = M.slab_sum(bufs)
    assert rel(de2.reshape(b, d), de) <= 1e-12 and abs(loss2 - loss) <= 1e-12 * abs(loss)
    full = K.reference("recipe", d, b, "member")
    again = M.step(c["e_b"], c["beta"], c["alpha"], c["inv_b"], c["p_b"], c["c"], keep=c["keep"], de=de2.reshape(b, d))
    assert rel(again["dx"], full["dx"]) <= 1e-12 and rel(again["dp"], full["dp"]) <= 1e-12


def all_cases():
    return sorted({(r, d, b) for lst in (K.STEP_CASES, K.WEIGHT_CASES, K.SLAB_CASES, K.REPEAT_CASES) for r, d, b, _ in lst})


def test_every_gpu_case_keeps_every_pair_off_the_discontinuity():
    """zero unsafe pairs, in every case and in its batch with repeated ids; the regimes are what their names say"""
    for r, d, b in all_cases():
        c = K.case(r, d, b)
        assert M.pair_guard(c["e_b"]) == 0, (r, d, b)
        s = c["e_b"].astype(np.float64) @ c["e_b"].astype(np.float64).T
        if r == "below":
            assert s.max() < c["beta"]
        if r == "orth" and b > 2:
            assert (s == 0).sum() >= 2
        if r in ("recipe", "signed") and b >= 15:
            assert (s < 0).any() and (s > c["beta"]).any() and ((s > 0) & (s < c["beta"])).any()
        assert len(set(c["rows"].tolist())) == b
        if b > 2:
            assert c["keep"][0] == 0 and c["keep"][-1] == 0 and 0 < (c["keep"] == 0).mean() < 0.7
        if b >= 32:
            assert any(not c["keep"][16 * t:16 * t + 16].any() for t in range(b // 16))
    for r, d, b, _ in K.REPEAT_CASES:
        c, rows = K.repeated(r, d, b)
        assert len(set(rows.tolist())) < b and M.pair_guard(c["e"][rows]) == 0


def test_pair_guard_sees_an_unsafe_pair():
    e = np.zeros((3, 16), np.float32)
    e[0, :2] = [1.0, 1.0]
    e[1, :2] = [1.0, -1.0 + 2.0 ** -23]      # S_01 = 2^-23 from a cancellation of two products of size 1: inside the band
    e[2, 5] = 1.0                             # disjoint support: exactly zero in any precision, safe
    assert M.pair_guard(e) == 2               # (0, 1) and (1, 0)
    e[1, 1] = -0.5
    assert M.pair_guard(e) == 0


def test_gather_mirrors_on_a_hand_made_batch():
    d = 16
    e = np.arange(5 * d, dtype=np.float32).reshape(5, d)
    node_map = np.array([9, 3, 4, 5, 6, 7, 0, 1, 2, 8], np.int32)
    gid2op = np.arange(100, 110, dtype=np.int32)
    idx = np.array([1, 0, 5, 9, 6], np.int32)             # ids 3, 9, 7, 8, 0 ; shard [3, 8): local 0, 6, 4, 5, -3
    e_b, pid, rloc, keep = M.gather_rows_mapped(e, idx, node_map, 3, 5, None, d)
    assert keep.tolist() == [1, 0, 1, 0, 0] and rloc.tolist() == [0, 4, 4, 4, 0] and pid.tolist() == [0, -1, 4, -1, -1]
    assert np.array_equal(e_b[0], e[0]) and np.array_equal(e_b[2], e[4]) and not e_b[[1, 3, 4]].any()
    _, pid, _, _ = M.gather_rows_mapped(e, idx, node_map, 3, 5, gid2op, d)
    assert pid.tolist() == [103, 109, 107, 108, 100]
    e_b, pid, rloc, keep = M.gather_rows_mapped(None, idx, None, 0, 0, None, d)
    assert not e_b.any() and not keep.any() and not rloc.any() and pid.tolist() == [-1] * 5
    out, ids = M.gather_batch(e, e + 0.5, np.arange(5, dtype=np.float32) + 1, d, rows=np.array([4, 2], np.int32), keep=np.array([1, 0], np.float32))
    assert ids is None and out.shape == (2 * (2 * d + 1),)
    assert np.array_equal(out[:d], e[4]) and not out[d:2 * d].any() and np.array_equal(out[2 * d:3 * d], e[4] + 0.5)
    assert out[4 * d:].tolist() == [5.0, 0.0]


def fp32_errors():
    """the mirror's formulas in numpy float32 against the float64 mirror, per composite quantity: the largest error over every GPU
    case, relative to the reference tensor's largest entry"""
    worst = dict(dx=0.0, dp=0.0, gax=0.0, gam=0.0, slab=0.0)

    def note(got, ref, *names):
        for k in names:
            worst[k] = max(worst[k], rel(got[k], ref[k], ref["scale"][k]))

    for r, d, b in sorted({(r, d, b) for r, d, b, _ in K.STEP_CASES + K.WEIGHT_CASES}):
        c = K.case(r, d, b)
        note(M.step(c["e_b"], c["beta"], c["alpha"], c["inv_den"], c["p"], c["c"], rows=c["rows"], dtype=np.float32),
             K.reference(r, d, b, "ids"), "dx", "dp")
        note(M.step(c["e_b"], c["beta"], c["alpha"], c["inv_b"], c["p_b"], c["c"], keep=c["keep"], dtype=np.float32),
             K.reference(r, d, b, "member"), "dx", "dp")
    for r, d, b in sorted({(r, d, b) for r, d, b, _ in K.WEIGHT_CASES}):
        c = K.case(r, d, b)
        for every in (False, True):
            note(M.step(c["e_b"], c["beta"], c["alpha"], c["inv_b"], c["p_b"], c["c"], keep=c["keep"], w1t=c["w1t"], w2t=c["w2t"], dgrad_all=every,
                        dtype=np.float32), K.reference(r, d, b, "member", True, every), "dx", "dp", "gax", "gam")
    for r, d, b, parts in K.SLAB_CASES:
        c = K.case(r, d, b)
        ref = [M.slab_rank(c["e_b"], c["beta"], c["alpha"], k, parts) for k in range(parts)]
        got = [M.slab_rank(c["e_b"], c["beta"], c["alpha"], k, parts, dtype=np.float32) for k in range(parts)]
        scale = max(np.abs(x[:-1]).max() for x in ref)
        worst["slab"] = max(worst["slab"], max(np.abs(g[:-1].astype(np.float64) - x[:-1]).max() for g, x in zip(got, ref)) / scale)
        de32, _ = M.slab_sum(got, dtype=np.float32)
        w = dict(w1t=c["w1t"], w2t=c["w2t"], dgrad_all=True) if d in (64, 128, 256) else {}
        full = M.step(c["e_b"], c["beta"], c["alpha"], c["inv_b"], c["p_b"], c["c"], keep=c["keep"], **w)
        note(M.step(c["e_b"], c["beta"], c["alpha"], c["inv_b"], c["p_b"], c["c"], keep=c["keep"], de=de32.reshape(b, d), dtype=np.float32, **w),
             full, *(("dx", "dp", "gax", "gam") if w else ("dx", "dp")))
    return worst


def test_fp32_error_of_the_formulas_stays_within_the_recorded_figures():
    """what tests/tolerances.py records as LOSS_STEP_FP32 is re-measured on every run: the GPU bounds (8 x these, or the project's 3e-6
    where that is larger) stay tied to a number that is shown, not claimed"""
    worst = fp32_errors()
    print("fp32 formulas vs fp64 mirror:", {k: f"{v:.3e}" for k, v in worst.items()})
    for k, v in worst.items():
        assert 0 < v <= T.LOSS_STEP_FP32[k], (k, v, T.LOSS_STEP_FP32[k])
        assert v >= 0.25 * T.LOSS_STEP_FP32[k], f"{k}: the recorded figure {T.LOSS_STEP_FP32[k]:.1e} is stale (measured {v:.3e}); bounds derive from it"
        assert T.LOSS_STEP_BOUND[k] == max(T.LOSS_STEP_LAST_STAGE, T.LOSS_STEP_K * T.LOSS_STEP_FP32[k])


def test_loss_wgs_gives_the_j_splits_the_cases_name():
    """host arithmetic only: the workspace formula shows js.  b = 1040: loss_wgs 64 / 256 / 4096 -> js 1 / 4 / 16; b = 333: 4 / 6 / 6;
    the slab form sizes js by the tiles ONE rank sweeps"""
    import gcn_drug_repurposing_amd as pkg
    lib = pkg.load()

    def js_of(b, d, parts=None):
        total = lib.gss_loss_workspace_bytes(b, d) if parts is None else lib.gss_loss_workspace_bytes_parts(b, d, parts)
        ni = -(-b // 16)
        for js in range(1, 17):
            if (4 * js * b * d + 15) // 16 * 16 + (8 * ni * js + 15) // 16 * 16 + 4 * b * d == total:
                return js
        return None

    try:
        for wgs, at1040, at333 in ((64, 1, 4), (256, 4, 6), (4096, 16, 6)):
            assert lib.gss_debug_set_option(b"loss_wgs", wgs) == 0
            assert (js_of(1040, 64), js_of(333, 128)) == (at1040, at333)
            assert js_of(1040, 64, 1) == at1040
        assert lib.gss_debug_set_option(b"loss_wgs", 256) == 0
        assert js_of(1040, 64, 8) == 16 and js_of(333, 64, 2) == 6 and js_of(17, 64, 8) == 1
        assert lib.gss_loss_workspace_bytes_parts(0, 64, 2) == 0 and lib.gss_loss_workspace_bytes_parts(17, 64, 0) == 0
    finally:
        lib.gss_debug_set_option(b"loss_wgs", 256)

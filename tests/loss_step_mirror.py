"""The loss of a plan's step (csrc/loss.hip: loss_step, loss_step_slab_sweep, the three gathers), restated in numpy -- TEST INFRASTRUCTURE.
Every function computes in the dtype it is asked for: float64 is the contract tests/test_gpu_loss_step.py holds the kernels to, float32
is the same formulas at the kernels' precision (test_loss_step_mirror.py measures the distance between the two; tests/tolerances.py
turns it into the GPU bounds).  The gathers move fp32 values and int32 ids without arithmetic, so their mirrors are exact.

  sweep      S = E_B E_B^T; loss = mean(-alpha/2 (relu(S) - beta)^2); dE = 2 G E_B, G = -alpha/B^2 (relu(S) - beta) 1[S > 0]
  finish     dx = (dE - e (e . dE)) * inv_den[row]; dp = c * dx * elu'(p[row]); rows with keep == 0: zeros
  dgrad      gax = dP W1, gam = dP W2 (w1t / w2t: the transposed weights, [in][out]); dgrad_all: keep == 0 rows enter unmasked
  slab_rank  rank r of P: the rows of G E_B (no factor 2) on the i tiles r, r + P, ..., zeros elsewhere, its loss share behind them"""
import numpy as np

from oracle import gss_oracle as O

TILE = 16


def pair_guard(e_b):
    """Pairs (i, j) whose fp32 dot product could land on the other side of zero from the exact one: G jumps at S = 0 by alpha beta / B^2,
    so such a pair would make kernel and reference disagree legitimately.  A pair is safe when it is zero in any precision
    (sum_k |e_ik e_jk| == 0) or |S_ij| > gamma_d sum_k |e_ik e_jk|, gamma_d = d u / (1 - d u), u = 2^-24: the standard bound of an fp32
    dot product of length d in any summation order.  -> number of unsafe pairs (the tests require 0)"""
    e = np.asarray(e_b, np.float64)
    d = e.shape[1]
    u = d * 2.0 ** -24
    gamma = u / (1.0 - u)
    s = e @ e.T
    a = np.abs(e) @ np.abs(e).T
    return int((~((a == 0) | (np.abs(s) > gamma * a))).sum())


def elu_grad(p):
    return np.where(p > 0, p.dtype.type(1), np.exp(np.minimum(p, 0)))


def sweep(e_b, beta, alpha, dtype=np.float64):
    """-> loss (python float), dE [b][d]"""
    e = np.asarray(e_b, dtype)
    dt = e.dtype.type
    return float(O.gss_loss(e, dt(beta), None, dt(alpha))), O.loss_grad_emb(e, dt(beta), None, dt(alpha))


def finish(de, e_b, inv_den, p, c, rows=None, keep=None, dtype=np.float64):
    """-> dx, dp (keep == 0 rows zero), dp_all (no row masked: what dgrad_all multiplies)"""
    de, e = np.asarray(de, dtype), np.asarray(e_b, dtype)
    r = np.arange(e.shape[0]) if rows is None else np.asarray(rows, np.int64)
    inv, pb = np.asarray(inv_den, dtype)[r], np.asarray(p, dtype)[r]
    dx_all = (de - e * (e * de).sum(1, keepdims=True)) * inv[:, None]
    dp_all = e.dtype.type(c) * dx_all * elu_grad(pb)
    k = np.ones(e.shape[0], bool) if keep is None else np.asarray(keep) != 0
    return np.where(k[:, None], dx_all, 0), np.where(k[:, None], dp_all, 0), dp_all


def dgrad(dp, w1t, w2t, dtype=np.float64):
    dp = np.asarray(dp, dtype)
    return dp @ np.asarray(w1t, dtype).T, dp @ np.asarray(w2t, dtype).T


def step(e_b, beta, alpha, inv_den, p, c, rows=None, keep=None, w1t=None, w2t=None, dgrad_all=False, de=None, dtype=np.float64):
    """gss_loss_step: -> dict(loss, de, dx, dp[, gax, gam]); de given (the slab form's summed rows, factor 2 applied): no sweep"""
    out = {}
    if de is None:
        out["loss"], de = sweep(e_b, beta, alpha, dtype)
    out["de"] = np.asarray(de, dtype)
    out["dx"], out["dp"], dp_all = finish(out["de"], e_b, inv_den, p, c, rows, keep, dtype)
    if w1t is not None:
        out["gax"], out["gam"] = dgrad(dp_all if dgrad_all else out["dp"], w1t, w2t, dtype)
    out["scale"] = {k: error_scale(out, k, inv_den, rows) for k in ("dx", "dp", "gax", "gam") if k in out}
    return out


def error_scale(ref, name, inv_den, rows=None):
    """what an error of ref[name] is measured against: the tensor's largest entry.  A batch of ONE row is the exception: dE is parallel
    to e there, every composite output is exactly zero and the reference holds nothing but its own rounding residue (1e-17), so the
    scale is the size of the operands that cancel, max |dE| * inv_den."""
    if ref["de"].shape[0] == 1:
        r = 0 if rows is None else int(np.asarray(rows)[0])
        return float(np.abs(ref["de"]).max() * abs(float(np.asarray(inv_den)[r])))
    return float(np.abs(ref[name]).max())


def slab_tiles(b, rank, parts):
    """the rows of the i tiles rank, rank + parts, ... as a bool mask [b]"""
    return ((np.arange(b) // TILE) % parts) == rank


def slab_rank(e_b, beta, alpha, rank, parts, dtype=np.float64):
    """gss_loss_slab_sweep: -> de_x [b d + 1]"""
    e = np.asarray(e_b, dtype)
    dt = e.dtype.type
    b = e.shape[0]
    mine = slab_tiles(b, rank, parts)
    s = e @ e.T
    t = np.maximum(s, 0) - dt(beta)
    g = -(dt(alpha) / dt(b * b)) * t * (s > 0)
    rows = np.where(mine[:, None], g @ e, 0)
    share = -0.5 * float(alpha) * float((t[mine].astype(np.float64) ** 2).sum()) / (float(b) * float(b))
    return np.concatenate([rows.reshape(-1), np.array([share], dtype)])


def slab_sum(parts_de_x, dtype=np.float64):
    """the ranks' buffers summed in rank order -> (dE [b d] with the factor 2 the finish applies, loss)"""
    acc = np.asarray(parts_de_x[0], dtype).copy()
    for x in parts_de_x[1:]:
        acc = acc + np.asarray(x, dtype)
    return acc.dtype.type(2) * acc[:-1], float(acc[-1])


# ---------------------------------------------------------------- the gathers (exact)
def gather_rows(e, rows, keep=None):
    out = np.asarray(e, np.float32)[np.asarray(rows, np.int64)].copy()
    if keep is not None:
        out[np.asarray(keep) == 0] = 0
    return out


def translate(idx, node_map, lo, nl, gid2op):
    """-> rel (int64), owned (bool), pid, rloc (int32), keep (float32)"""
    idx = np.asarray(idx, np.int64)
    ids = np.asarray(node_map, np.int64)[idx] if node_map is not None else idx
    rel = ids - lo
    owned = (rel >= 0) & (rel < nl)
    rloc = np.clip(rel, 0, max(nl - 1, 0)).astype(np.int32)
    pid = np.asarray(gid2op)[ids].astype(np.int32) if gid2op is not None else np.where(owned, rel, -1).astype(np.int32)
    return rel, owned, pid, rloc, owned.astype(np.float32)


def gather_rows_mapped(e, idx, node_map, lo, nl, gid2op, d):
    """-> e_b, pid, rloc, keep   (e may be None when nl == 0)"""
    rel, owned, pid, rloc, keep = translate(idx, node_map, lo, nl, gid2op)
    out = np.zeros((len(rel), d), np.float32)
    if owned.any():
        out[owned] = np.asarray(e, np.float32)[rel[owned]]
    return out, pid, rloc, keep


def gather_batch(e, p, inv_den, d, idx=None, node_map=None, lo=0, nl=0, gid2op=None, rows=None, keep=None):
    """-> out [b (2 d + 1)] = [E_B | P_B | inv_B], and (pid, rloc, keep) when idx is given, else None"""
    if idx is not None:
        rel, owned, pid, rloc, kf = translate(idx, node_map, lo, nl, gid2op)
        ids = (pid, rloc, kf)
    else:
        rel = np.asarray(rows, np.int64)
        owned = np.ones(len(rel), bool) if keep is None else np.asarray(keep) != 0
        ids = None
    b = len(rel)
    eb, pb, ib = np.zeros((b, d), np.float32), np.zeros((b, d), np.float32), np.zeros(b, np.float32)
    if owned.any():
        eb[owned] = np.asarray(e, np.float32)[rel[owned]]
        pb[owned] = np.asarray(p, np.float32)[rel[owned]]
        ib[owned] = np.asarray(inv_den, np.float32)[rel[owned]]
    return np.concatenate([eb.reshape(-1), pb.reshape(-1), ib]), ids

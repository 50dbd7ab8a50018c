"""The dense half of a plan's step (csrc/dense.hip and the optimizer kernels of csrc/elementwise.hip), restated in numpy -- TEST
INFRASTRUCTURE.  One function per operation; every function computes in the dtype it is asked for: float64 is the contract
tests/test_gpu_dense_step.py holds the launchers to, float32 is the same formulas at the kernels' precision
(tests/test_dense_step_mirror.py measures the distance between the two; tests/tolerances.py turns it into the GPU bounds of E, inv_den
and E_B).

  projection   P = AX W1^T + b1 + AM W2^T + b2                      (nn.Linear x 2 + add, modules/model.py:165,170-172)
               O = elu(P)                                           (F.elu, modules/model.py:173)
               X = O, or P_prev + decay O where P_prev is given     (the residual mix, modules/model.py:201-203)
  normalize    E = X / max(|X|_2, 1e-12), inv_den = 1 / max(|X|_2, 1e-12)            (F.normalize, modules/model.py:205)
  batch rows   E_B[t] = E[list[t]] (entries >= 0), or E_B[pos[r]] = E[r] where pos[r] >= 0        (emb[idx], modules/model.py:216-217)
  wgrad        gW1 = dP^T AX[rows], gW2 = dP^T AM[rows], gb = gb2 = sum_n dP, summed over any number of problems
               (autograd of the two nn.Linear of every layer: the layers share their weights)
  adam         torch.optim.Adam's single-tensor form on W1, b1, W2, b2 (train.py:139-141,184): the fp32 restatement test_adam_matches_torch_semantics
               holds gss_adam_step to (oracle/gss_oracle.adam_step); b1 and b2 get
               the same gradient and keep their own state"""
import numpy as np

from oracle import gss_oracle as O

EPS = 1e-12


def elu(p):
    return np.where(p > 0, p, np.expm1(np.minimum(p, 0)))


def projection(ax, am, w1, b1, w2, b2, p_prev=None, decay=0.0, dtype=np.float64):
    """-> P, X (every row of the operands)"""
    ax, am, w1, b1, w2, b2 = (np.asarray(v, dtype) for v in (ax, am, w1, b1, w2, b2))
    p = ax @ w1.T + b1 + am @ w2.T + b2
    o = elu(p)
    x = o if p_prev is None else np.asarray(p_prev, dtype) + p.dtype.type(decay) * o
    return p, x


def normalize(x, dtype=np.float64):
    """-> E, inv_den"""
    x = np.asarray(x, dtype)
    inv = x.dtype.type(1) / np.maximum(np.sqrt((x * x).sum(1)), x.dtype.type(EPS))
    return x * inv[:, None], inv


def rows_out_by_list(e, row_list):
    """E_B over a row list -> (E_B [len(list)][d], written [len(list)]): slot t holds E[list[t]]; a negative entry leaves its slot alone"""
    lst = np.asarray(row_list, np.int64)
    ok = lst >= 0
    out = np.zeros((len(lst), e.shape[1]), e.dtype)
    out[ok] = e[lst[ok]]
    return out, ok


def rows_out_by_pos(e, pos, b):
    """E_B through the batch-position map -> (E_B [b][d], written [b]): slot pos[r] holds E[r] where pos[r] >= 0"""
    pos = np.asarray(pos, np.int64)
    r = np.nonzero(pos >= 0)[0]
    out = np.zeros((b, e.shape[1]), e.dtype)
    ok = np.zeros(b, bool)
    out[pos[r]] = e[r]
    ok[pos[r]] = True
    return out, ok


def wgrad(problems, dtype=np.float64):
    """problems: (dP [n][d] compact, AX, AM, rows or None) each -> gW1 [d][d], gW2 [d][d], gb [d] (= gb2), summed over the problems.
    An integer dtype gives the exact sums of the integer regime."""
    gw1 = gw2 = gb = 0
    for dp, ax, am, rows in problems:
        dp = np.asarray(dp, dtype)
        r = slice(None) if rows is None else np.asarray(rows, np.int64)
        gw1 = gw1 + dp.T @ np.asarray(ax, dtype)[r]
        gw2 = gw2 + dp.T @ np.asarray(am, dtype)[r]
        gb = gb + dp.sum(0)
    return gw1, gw2, gb


def adam(params, grads, state, lr, beta1=0.9, beta2=0.999, eps=1e-8):
    """one step on {"W1", "b1", "W2", "b2"} in place (fp32, torch's own arithmetic); `state` carries the step count "t" and the moments
    "m_<name>", "v_<name>" between calls (given beforehand: the initial state)"""
    O.adam_step(params, grads, state, lr, (beta1, beta2), eps)

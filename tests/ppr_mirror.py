"""numpy fp64 statement of gss_ppr_run (csrc/ppr.hip), iteration by iteration, from raw index lists: what cpu_ops.emulate_ppr and
knockout_mirror.emulate state for a converged run, here for a run that is stopped after exactly t iterations -- the iterate
GSS_ENOTCONV leaves in x, the iteration counts so far and every column's L1 error of every iteration.  `prob` is anything that carries
the attributes of diffusion.PprProblem (a types.SimpleNamespace built by hand will do); `ko` anything that carries the lists of
gss_ppr_set_knockout (dead, corr_ptr, corr_grp_row, corr_grp_col, corr_src, corr_val), or None.  Shared by test_ppr_mirror.py (CPU:
the mirror against the oracle and the two older emulations, bit for bit) and test_gpu_ppr_ops.py.  Never raises for non-convergence."""
import numpy as np


def snapshots(prob, alpha, tol, ts, ko=None):
    """-> {t: (x [n][k], iters [k], done [k], err_history [iterations run][k])} for every t of `ts`, from one pass.  A converged column
    stays frozen and its later errors are NaN (the device no longer computes them); iters is 0 for a column that has not converged; the
    pass ends early once every column has, and every later t then holds that final state."""
    ts = sorted(set(int(t) for t in ts))
    assert ts and ts[0] >= 1, ts
    n, k = prob.n, prob.k
    x = np.full((n, k), 1.0 / n)
    done = np.zeros(k, dtype=bool)
    iters = np.zeros(k, dtype=np.int32)
    cols = np.arange(k)
    hist, out = [], {}
    for it in range(1, ts[-1] + 1):
        held = x[prob.z_rows].copy()                                   # ppr_dangling_kernel
        held[prob.z_rows[:, None] == prob.starts[None, :]] = 0.0
        dsum = held.sum(0)
        xs = x.copy()                                                  # ppr_ovr_scale_kernel
        orig = xs[prob.ovr_row, prob.ovr_col].copy()
        xs[prob.ovr_row, prob.ovr_col] = orig * prob.ovr_ratio
        yself = np.zeros(k)
        for c in range(k):                                             # ppr_column_kernel
            for e in prob.zero_ovr[prob.zero_ptr[c]:prob.zero_ptr[c + 1]]:
                dsum[c] += orig[e]
            if prob.start_dangling[c]:
                dsum[c] += xs[prob.starts[c], c]
            lo, hi = prob.keep_ptr[c], prob.keep_ptr[c + 1]
            yself[c] = (prob.keep_val[lo:hi] * xs[prob.keep_row[lo:hi], c]).sum()
        y = prob.mt @ xs                                               # ppr_spmm_kernel
        np.add.at(y, (prob.sel_row, prob.sel_col), prob.sel_val * x[prob.starts[prob.sel_col], prob.sel_col])   # ppr_sel / ppr_ysel
        y[prob.starts, cols] = yself
        p = np.zeros((n, k))
        p[prob.starts, cols] = 1.0
        xn = alpha * (y + dsum[None, :] * p) + (1.0 - alpha) * p       # ppr_update_kernel / the fused epilogue
        if ko is not None:
            for q in range(len(ko.corr_grp_row)):                      # ppr_knockout_kernel: corrections from the unscaled x ...
                j, c = ko.corr_grp_row[q], ko.corr_grp_col[q]
                total = 0.0
                for e in range(ko.corr_ptr[q], ko.corr_ptr[q + 1]):
                    total += ko.corr_val[e] * x[ko.corr_src[e], c]
                xn[j, c] = xn[j, c] + alpha * total
            live = ko.dead >= 0                                        # ... and the dead entries
            xn[ko.dead[live], cols[live]] = 0.0
        err = np.abs(xn - x).sum(0)
        upd = ~done
        x[:, upd] = xn[:, upd]
        hist.append(np.where(upd, err, np.nan))
        newly = upd & (err < n * tol)                                  # ppr_finish_kernel / ppr_finish_fused_kernel
        iters[newly] = it
        done |= newly
        if it in ts:
            out[it] = (x.copy(), iters.copy(), done.copy(), np.array(hist))
        if done.all():
            break
    for t in ts:
        out.setdefault(t, (x.copy(), iters.copy(), done.copy(), np.array(hist)))
    return out


def steps(prob, alpha, tol, t, ko=None):
    """the state after exactly t iterations, or fewer if every column converged earlier -> (x, iters, done, err_history)"""
    return snapshots(prob, alpha, tol, [t], ko)[int(t)]


def last_error_margins(prob, tol, iters, err_history):
    """per column: how far, relatively, its errors at its last iteration and at the one before are from the threshold n tol (the
    measure of knockout_mirror.last_error_margin): a column whose error passes the threshold within rounding could stop one iteration
    apart under another summation order"""
    thr = prob.n * tol
    out = np.empty(prob.k)
    for c in range(prob.k):
        it = int(iters[c])
        assert it >= 1, c
        e = [err_history[it - 1, c]] + ([err_history[it - 2, c]] if it >= 2 else [])
        out[c] = min(abs(v - thr) / thr for v in e)
    return out

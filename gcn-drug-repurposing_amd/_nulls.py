"""What classes.py, mantel.py and enrich.py share on the host around the kernels of a seeded permutation null."""
import numpy as np

from . import _lib

NULL_CHUNK_BYTES = 256 << 20  # a null comes back to the host in calls of at most this many bytes of results


def int32_array(what, v, who):
    a = np.asarray(v, dtype=np.int64).reshape(-1)
    if len(a) and (a.min() < -2 ** 31 or a.max() >= 2 ** 31):
        raise ValueError(f"{who}: {what} holds an entry outside int32")
    return a.astype(np.int32)


def device_lists(lists, who, what, dev):
    """int32 lists packed one after another -> device int32 (ptr [len(lists) + 1], idx [total, at least 1]); what: the refusal's word for them"""
    import torch
    ptr = np.zeros(len(lists) + 1, dtype=np.int64)
    np.cumsum([len(l) for l in lists], out=ptr[1:])
    if ptr[-1] >= 2 ** 31:
        raise ValueError(f"{who}: the {what} hold {int(ptr[-1])} entries, int32 offsets do not reach")
    idx = np.concatenate(lists) if ptr[-1] else np.zeros(1, dtype=np.int32)
    return torch.from_numpy(ptr.astype(np.int32)).to(dev), torch.from_numpy(idx).to(dev)


def chunked_null(call, samples, bytes_per_sample, axis=0):
    """call(count, first) -> that many samples on the device, along `axis`; -> all on the host, at most NULL_CHUNK_BYTES per call"""
    step = max(1, NULL_CHUNK_BYTES // bytes_per_sample)
    return np.concatenate([call(min(step, samples - f), f).cpu().numpy() for f in range(0, samples, step)], axis=axis)


def square_matrix(dist, who, labels=None):
    """-> the device fp64 matrix [n][n] the kernels read: a device tensor in place, a host array uploaded.  A NaN distance (a zero profile
    under cosine, a constant one under correlation) is refused with its row's label"""
    import torch
    if isinstance(dist, torch.Tensor):
        d = dist
        if (d.dim() != 2 or d.dtype != torch.float64 or not d.is_cuda or d.shape[0] != d.shape[1] or d.shape[0] < 1
                or (d.shape[1] > 1 and d.stride(1) != 1) or (d.shape[0] > 1 and d.stride(0) < d.shape[1])):
            raise ValueError(f"{who}: a distance tensor must be a square device fp64 matrix with unit column stride and a row stride of at "
                             "least its width")
    else:
        host = np.ascontiguousarray(dist, dtype=np.float64)
        if host.ndim != 2 or host.shape[0] != host.shape[1] or host.shape[0] < 1:
            raise ValueError(f"{who}: a host distance array must be square, not {host.shape}")
        if not torch.cuda.is_available():
            raise _lib.GssError(f"{who}: the sums run on the GPU only (no CPU fallback)")
        d = torch.from_numpy(host).cuda()
    if labels is not None and len(labels) != d.shape[0]:
        raise ValueError(f"{who}: {len(labels)} labels for {d.shape[0]} rows")
    bad = torch.isnan(d).any(dim=1)
    if bool(bad.any()):
        i = int(torch.nonzero(bad)[0])
        raise ValueError(f"{who}: a distance of {labels[i] if labels is not None else 'row ' + str(i)!r} is NaN (its diffusion profile is zero "
                         "or constant); it cannot be scored")
    return d


def benjamini_hochberg(p):
    """q[i] = min over the p-values p_(j) >= p[i] of p_(j) * n / j (j = the rank from 1, ascending, ties in the given order), at most 1"""
    p = np.asarray(p, dtype=np.float64)
    n = len(p)
    order = np.argsort(p, kind="stable")
    scaled = p[order] * n / np.arange(1, n + 1)
    q = np.empty(n)
    q[order] = np.minimum(1.0, np.minimum.accumulate(scaled[::-1])[::-1])
    return q

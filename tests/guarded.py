"""Guarded outputs of the op-by-op GPU tests (tests/test_gpu_loss_step.py, tests/test_gpu_dense_step.py,
tests/test_gpu_input_grad.py, tests/test_gpu_rownorm.py) -- TEST INFRASTRUCTURE.  Every
output of a launch sits between canary elements and starts as a NaN of a recognisable payload, so that a test can tell "written",
"not written" and "written outside the buffer" apart; a workspace is exactly as long as the library says, in front of canary bytes."""
import contextlib

import numpy as np
import torch

PREFILL = 0x7FC0DEAD                 # a quiet NaN with a payload no computation produces
CANARY = 0x7FC0BEEF                  # around every output
PAD = 64                             # canary elements on each side (256 bytes: the output keeps its 16-byte alignment)
WS_BYTE = 0xA5
WS_TAIL = 4096
KNOB_DEFAULTS = {"gemm_variant": 2, "gemm_ws": -1, "wgrad_wgs": 256}     # the kernel-selection knobs of csrc/dense.hip


@contextlib.contextmanager
def knobs(G, **values):
    """kernel-selection knobs for the launches inside; back to their defaults whatever happens"""
    try:
        for k, v in values.items():
            G._lib.check(G.lib.gss_debug_set_option(k.encode(), v))
        yield
    finally:
        for k in values:
            G._lib.check(G.lib.gss_debug_set_option(k.encode(), KNOB_DEFAULTS[k]))


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ptr(t):
    return None if t is None else t.data_ptr()


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


class Out:
    """an output of `shape` (float32 or int32) between canary elements, pre-filled"""

    def __init__(self, *shape, fill=PREFILL, dtype=torch.float32):
        self.n = int(np.prod(shape))
        self.shape = shape
        self.full = torch.full((self.n + 2 * PAD,), CANARY, dtype=torch.int32, device="cuda")
        self.full[PAD:PAD + self.n] = fill
        self.t = self.full[PAD:PAD + self.n].view(dtype)

    @property
    def ptr(self):
        return self.t.data_ptr()

    def host(self, what="output"):
        """the output on the host, after checking the canaries around it"""
        full = self.full.cpu().numpy()
        assert (full[:PAD] == np.int32(CANARY)).all() and (full[PAD + self.n:] == np.int32(CANARY)).all(), f"{what}: written outside its buffer"
        mid = full[PAD:PAD + self.n]
        return (mid.view(np.float32) if self.t.dtype == torch.float32 else mid).reshape(self.shape)

    def untouched(self, what="output"):
        return (bits(self.host(what)) == np.int32(PREFILL)).all()


class Workspace:
    """exactly nbytes of workspace in front of WS_TAIL canary bytes"""

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        self.buf = torch.full((self.nbytes + WS_TAIL,), WS_BYTE, dtype=torch.uint8, device="cuda")

    @property
    def ptr(self):
        return self.buf.data_ptr()

    def check(self, what="workspace"):
        assert (self.buf[self.nbytes:] == WS_BYTE).all().item(), f"{what}: written behind gss_loss_workspace_bytes"

    def floats_at(self, address, n):
        off = address - self.ptr
        assert 0 <= off and off % 16 == 0 and off + 4 * n <= self.nbytes, (off, n, self.nbytes)
        return self.buf[off:off + 4 * n].view(torch.float32).cpu().numpy()


def written(x, what):
    assert not (bits(x) == np.int32(PREFILL)).any(), f"{what}: a piece keeps the pre-fill"
    assert np.isfinite(x).all(), f"{what}: not finite"
    return x


def close(got, ref, bound, scale, what):
    err = np.abs(got.astype(np.float64) - ref).max() / max(scale, 1e-300)
    print(f"{what}: err {err:.3e} (bound {bound:.1e})")
    assert err <= bound, f"{what}: {err:.3e} of the largest entry, bound {bound:.1e}"

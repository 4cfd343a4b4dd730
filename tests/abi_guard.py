"""The guarded device buffers of the C ABI edge tests (test_gpu_kron_abi.py,
test_gpu_shard_abi.py, test_gpu_masked_abi.py): a payload of exactly the
documented size between two guards of 64 NaN doubles (Guard) or, for a byte
mask, 64 bytes of 0xFF (ByteGuard), compared bit for bit."""
import ctypes

import numpy as np

GUARD = 64


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


class Guard(object):
    """n doubles on the device between two guards of 64 NaN doubles, the
    payload `off` doubles past a 16-byte boundary (off = 1: 8-byte aligned
    only).  data None: the payload is NaN too (an output, or scratch)."""

    def __init__(self, n, data=None, off=0):
        import torch
        self.n, self.off = int(n), int(off)
        self.lo = self.off + GUARD
        h = np.full(self.lo + self.n + GUARD, np.nan)
        if data is not None:
            h[self.lo:self.lo + self.n] = np.asarray(data, dtype=np.float64).reshape(-1)
        self.h0 = h
        self.d = torch.from_numpy(h.copy()).cuda()
        assert self.d.data_ptr() % 16 == 0

    @property
    def ptr(self):
        return ctypes.c_void_p(self.d.data_ptr() + 8 * self.lo)

    def _host(self):
        import torch
        torch.cuda.synchronize()
        return self.d.cpu().numpy()

    def read(self):
        """The payload; asserts both guards bit for bit."""
        flat = self._host()
        a, b = bits(flat).copy(), bits(self.h0).copy()
        a[self.lo:self.lo + self.n] = 0
        b[self.lo:self.lo + self.n] = 0
        assert np.array_equal(a, b), "a guard was written"
        return flat[self.lo:self.lo + self.n].copy()

    def unchanged(self):
        """Asserts guards and payload bit for bit as they were made."""
        assert np.array_equal(bits(self._host()), bits(self.h0)), "the buffer was written"

    def reset(self):
        import torch
        torch.cuda.synchronize()
        self.d.copy_(torch.from_numpy(self.h0))
        torch.cuda.synchronize()


class ByteGuard(object):
    """The byte twin for masks: a payload of exactly n bytes on the device
    between two guards of 64 bytes of 0xFF (nonzero: a read past either end
    sees an observed point), the payload `off` (0 or 1) bytes past a 16-byte
    boundary.  An input only: unchanged() is its one check."""

    def __init__(self, data, off=0):
        import torch
        data = np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
        self.n, self.off = data.size, int(off)
        self.lo = self.off + GUARD
        h = np.full(self.lo + self.n + GUARD, 0xFF, dtype=np.uint8)
        h[self.lo:self.lo + self.n] = data
        self.h0 = h
        self.d = torch.from_numpy(h.copy()).cuda()
        assert self.d.data_ptr() % 16 == 0

    @property
    def ptr(self):
        return ctypes.c_void_p(self.d.data_ptr() + self.lo)

    def unchanged(self):
        import torch
        torch.cuda.synchronize()
        assert np.array_equal(self.d.cpu().numpy(), self.h0), "the mask was written"

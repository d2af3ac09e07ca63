"""What the GPU tests that call libset_amd.so through its C ABI share: the loaded library, the current stream, and outputs that live in the
middle of a sentinel-filled buffer, so that a write outside the output shows."""
import numpy as np
import torch

GUARD = 64                 # elements on each side of an output
SENT_BITS = 0x4B1D5EA7     # as float32: 10313383.0; as int32 the same bits
SENT_I64 = -0x5EA7C0DE


def L():
    from set_amd import _lib
    return _lib.lib()


def check(rc, name):
    from set_amd import _lib
    _lib.check(rc, name)


def stream():
    from set_amd.ops import _stream
    return _stream()


def to_dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


class Sent:
    """A contiguous view of `shape` (float32 or int64) starting GUARD + off elements into a buffer filled with a sentinel bit pattern
    (off = 1: a view that is not 16-byte aligned).  `get()` returns the view's contents after checking that nothing around it changed;
    `fill(a)` puts an input there (in-place operands)."""

    def __init__(self, shape, dev, dtype=torch.float32, off=0):
        self.shape, self.n, self.off, self.dtype = tuple(shape), int(np.prod(shape)), off, dtype
        if dtype == torch.float32:
            raw = torch.full((self.n + 2 * GUARD + off,), SENT_BITS, dtype=torch.int32, device=dev)
            self.buf = raw.view(torch.float32)
        else:
            assert dtype == torch.int64
            self.buf = torch.full((self.n + 2 * GUARD + off,), SENT_I64, dtype=torch.int64, device=dev)
        self.view = self.buf[GUARD + off:GUARD + off + self.n].view(*self.shape)

    @property
    def ptr(self):
        return self.view.data_ptr()

    def fill(self, a):
        self.view.copy_(to_dev(a, self.view.device).view(*self.shape))
        return self

    def get(self):
        b = self.buf.cpu().numpy()
        lo, hi = b[:GUARD + self.off], b[GUARD + self.off + self.n:]
        want = SENT_BITS if self.dtype == torch.float32 else np.uint64(SENT_I64 & (2 ** 64 - 1))
        assert (bits(lo) == want).all() and (bits(hi) == want).all(), "written outside the output"
        return b[GUARD + self.off:GUARD + self.off + self.n].reshape(self.shape).copy()

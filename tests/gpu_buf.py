"""Sentinel-padded device buffers for the GPU test files: what a kernel may write is checked against what it did write, bit for bit."""
import numpy as np
import torch

from small_kernels_util import F32, BF16

DEV = 'cuda'
TDT = {F32: torch.float32, BF16: torch.bfloat16}
SENTINEL = -7777.0


def bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32 if t.element_size() == 4 else torch.uint8)


class Buf(object):
    """a device buffer of `off` + rows * ld + tail elements filled with the sentinel, `init` ([rows][cols]) copied into its region; `.t` is
    what a kernel gets (the view from `off` on, rows * ld long at the most)"""

    def __init__(self, rows, cols, ld=None, off=0, dt=F32, init=None, fill=SENTINEL, tail=None, dtype=None):
        self.rows, self.cols, self.ld, self.off = rows, cols, cols if ld is None else ld, off
        assert self.ld >= cols
        tail = self.ld if tail is None else tail
        self.flat = torch.full((off + rows * self.ld + tail,), fill, dtype=dtype or TDT[dt], device=DEV)
        if init is not None:
            self.region().copy_(torch.as_tensor(np.ascontiguousarray(init)).reshape(rows, cols).to(DEV))
        self.before = self.flat.clone()
        self.t = self.flat[off:off + rows * self.ld]

    def region(self):
        return self.flat[self.off:self.off + self.rows * self.ld].view(self.rows, self.ld)[:, :self.cols]

    def get(self):
        torch.cuda.synchronize()
        return self.region().float().cpu().numpy()

    def assert_untouched_outside(self, what=''):
        keep = torch.ones(self.flat.numel(), dtype=torch.bool, device=DEV)
        keep[self.off:self.off + self.rows * self.ld].view(self.rows, self.ld)[:, :self.cols] = False
        same = bits(self.flat)[keep] == bits(self.before)[keep]
        assert bool(same.all()), '%s: %d elements outside the written region changed' % (what, int((~same).sum()))

    def assert_unchanged(self, what=''):
        assert torch.equal(bits(self.flat), bits(self.before)), '%s: an input changed' % what


def same_bits(a, b):
    return torch.equal(bits(a.flat), bits(b.flat))

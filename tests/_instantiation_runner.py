"""How tests/test_gpu_instantiations.py lays a batch out on the device and launches it, and -- run as a program -- the worker of its
screening test: ONE fresh process (the library reads MATINV_TILE_SCREEN once) that runs the Gauss-Jordan TILE cases and stores
the raw results in the .npz named on the command line, for the parent to compare bit for bit.

Layout of every strided buffer: LEAD elements, then `batch` blocks at a stride of width + 3 elements (odd for the even widths, so every
other block is only element-aligned), then a trailing gap as large as one tile-padded matrix. Input gaps hold NaN, output gaps a
sentinel: a kernel that reads past a block computes NaN, one that writes past it is seen, and neither leaves the allocation.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import _instantiations as inst  # noqa: E402

api = inst.api
SENTINEL, INFO_SENTINEL = -5.0, -7
LEAD, EXTRA = 64, 3


def tail(n):
    return (n + 16) ** 2


def bits(x):
    return x.view({8: np.uint64, 4: np.uint32}[x.dtype.itemsize])


class Blocks:
    """`batch` blocks of `width` elements inside one allocation (see the module docstring)"""

    def __init__(self, batch, width, n, strided=True):
        self.batch, self.width = batch, width
        self.stride = width + EXTRA if strided else width
        self.size = LEAD + batch * self.stride + tail(n)

    def view(self, buf):
        return buf[LEAD:LEAD + self.batch * self.stride].reshape(self.batch, self.stride)[:, :self.width]

    def host_input(self, blocks):
        buf = np.full(self.size, np.nan, dtype=blocks.dtype)
        self.view(buf)[:] = np.asarray(blocks).reshape(self.batch, self.width)
        return buf

    def device_output(self, dtype):
        return torch.full((self.size,), SENTINEL, dtype=dtype, device="cuda")

    def check_input_unchanged(self, dev, host, what):
        assert np.array_equal(bits(dev.cpu().numpy()), bits(host)), f"{what} was modified"

    def read_output(self, dev, what):
        """the blocks of an output buffer, after checking that every element outside them still is the sentinel, bit for bit"""
        out = dev.cpu().numpy()
        gaps = np.ones(self.size, dtype=bool)
        self.view(gaps)[:] = False
        assert (bits(out[gaps]) == bits(np.array([SENTINEL], dtype=out.dtype))[0]).all(), f"{what}: a gap was written"
        return self.view(out).copy()


def info_buffer(batch):
    return torch.full((batch + EXTRA,), INFO_SENTINEL, dtype=torch.int32, device="cuda")


def read_info(info, batch):
    h = info.cpu().numpy()
    assert (h[batch:] == INFO_SENTINEL).all(), "info was written beyond the batch"
    return h[:batch].copy()


def run_inverse(a, n, algo, kernel):
    """a: (batch, n*n). Returns (inverse blocks, info) after the layout checks."""
    lay = Blocks(a.shape[0], n * n, n)
    h_in = lay.host_input(a)
    d_in = torch.from_numpy(h_in).cuda()
    d_out = lay.device_output(d_in.dtype)
    info = info_buffer(lay.batch)
    api.inverse_batched(d_in[LEAD:], n, algo, out=d_out[LEAD:], info=info, kernel=kernel, batch=lay.batch, stride=lay.stride)
    torch.cuda.synchronize()
    lay.check_input_unchanged(d_in, h_in, "the input batch")
    return lay.read_output(d_out, "inverse"), read_info(info, lay.batch)


def screened_cases():
    return [c for c in inst.cases() if c.route.entry == "inverse" and c.route.algo == "gj" and c.route.family == "tile"]


def run_screened_cases():
    """{position in screened_cases(): raw result bits, position + "i": info}"""
    out = {}
    for i, c in enumerate(screened_cases()):
        a, _ = inst.gj_batch(c.n, c.route.dtype, True)
        got, info = run_inverse(a, c.n, inst.GJ, api.KERNEL_TILE)
        out[str(i)] = bits(got)
        out[f"{i}i"] = info
    return out


if __name__ == "__main__":
    assert torch.cuda.is_available()
    assert os.environ.get("MATINV_TILE_SCREEN") == "1"
    np.savez(sys.argv[1], **run_screened_cases())
    print("screen-worker ok")

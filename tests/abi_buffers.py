"""Guarded device buffers for the pointer-alignment and output-extent tests.

`Guarded(nbytes, offset)` is one DeviceBuffer of G + offset + nbytes + G bytes,
filled with seeded random bytes (not a constant: a kernel that writes zeros or
128s past its output must be seen), whose `.ptr` sits at base + G + offset --
`offset` bytes off hipMalloc's 256-byte alignment.  As an input it is a source
at any byte address; as an output `check()` asserts that both guards and the
`offset` bytes in front of the payload kept their fill, and
`check_outside(extents)` that the payload bytes outside the documented output
extents did (the padding between frames at a stride, a rejected call's whole
payload).
"""
import ctypes

import numpy as np

from vcf_amd.device import DeviceBuffer

G = 4096
_seed = [20240]


class Guarded:
    def __init__(self, nbytes: int, offset: int = 0, data=None):
        self.nbytes, self.offset = int(nbytes), int(offset)
        _seed[0] += 1
        rng = np.random.Generator(np.random.PCG64(_seed[0]))
        self.fill = rng.integers(0, 256, G + self.offset + self.nbytes + G, dtype=np.uint8)
        self.buf = DeviceBuffer(self.fill.size)
        self.buf.upload(self.fill)
        self.start = G + self.offset
        if data is not None:
            self.upload(data)

    @property
    def ptr(self) -> ctypes.c_void_p:
        return self.buf.address(self.start)

    def upload(self, arr) -> None:
        """Payload bytes from the start; they become the fill the checkers compare with."""
        a = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
        assert a.size <= self.nbytes
        self.fill[self.start:self.start + a.size] = a
        self.buf.upload(a, offset=self.start)

    def download(self, dtype=np.uint8, count=None) -> np.ndarray:
        n = self.nbytes if count is None else count * np.dtype(dtype).itemsize
        out = np.empty(n, np.uint8)
        self.buf.download(out, offset=self.start)
        return out.view(dtype)

    def _all(self) -> np.ndarray:
        return self.buf.download(np.empty(self.fill.size, np.uint8))

    def check(self, what: str = "") -> None:
        """Both guards and the `offset` bytes before the payload are unchanged."""
        now = self._all()
        end = self.start + self.nbytes
        for name, lo, hi in (("front guard", 0, self.start), ("back guard", end, now.size)):
            bad = np.flatnonzero(now[lo:hi] != self.fill[lo:hi])
            assert bad.size == 0, (f"{what}: {bad.size} byte(s) of the {name} written, first at payload offset "
                                   f"{lo + int(bad[0]) - self.start}")

    def check_outside(self, extents=(), what: str = "") -> None:
        """Payload bytes outside `extents` (half-open (lo, hi) byte ranges) kept their fill."""
        now = self._all()[self.start:self.start + self.nbytes]
        keep = np.ones(self.nbytes, bool)
        for lo, hi in extents:
            keep[lo:hi] = False
        bad = np.flatnonzero(keep & (now != self.fill[self.start:self.start + self.nbytes]))
        assert bad.size == 0, f"{what}: {bad.size} payload byte(s) outside the output extent written, first at {int(bad[0])}"

    def check_untouched(self, what: str = "") -> None:
        """A rejected call: payload and guards all as filled."""
        self.check_outside((), what)
        self.check(what)

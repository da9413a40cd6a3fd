"""Distortion between u8 frames on the GPU (src/RDE.py's calculate_rmse; vcf_distortion.hip).

vcf_distortion_u8 gives, per frame and channel, the exact integer sum of squared
differences, sum of absolute differences and largest absolute difference of
two frame sets.  sse_device takes and returns DeviceBuffers; measure, mse, rmse
and psnr are host conveniences that accept one frame (H x W or H x W x C) or a
stack (N x H x W x C).  RMSE = sqrt(float64(sum of sse) / (H * W * C)): the
integer sum is exact, so the only roundings are the division and the root.
There is no CPU path: the arithmetic runs in libvcf_amd.so and is stated in
include/vcf_amd.h.

vcf_ssim_u8 gives, per frame and channel, the SSIM in the integer form of
DESIGN.md §4.15 (C = 1 or 3, frames of at least 11 x 11): the exact integer sum
and the minimum of k = rint(q * 2^30) over the 11 x 11 windows wholly inside
the frame.  ssim_device and ssim_records work on DeviceBuffers, ssim on host
arrays; SSIM = sum_k / (windows * 2^30), divided in float64 here.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from ._blockio import check_input, output
from ._lib import call
from .device import DeviceBuffer, _h

# vcf_distortion_record (include/vcf_amd.h)
RECORD = np.dtype([("sse", np.uint64), ("sad", np.uint64), ("max_abs", np.uint32), ("pad", np.uint32)])


@dataclass
class Distortion:
    """Per frame and channel (n x C arrays), exact integers."""
    sse: np.ndarray        # uint64: sum of (a - b)^2
    sad: np.ndarray        # uint64: sum of |a - b|
    max_abs: np.ndarray    # uint32: max of |a - b|
    samples: int           # H * W: samples of one channel of one frame

    def mse(self) -> np.ndarray:
        """Per frame, over all channels: float64(sum sse) / (H * W * C)."""
        n, C = self.sse.shape
        if self.samples == 0:
            return np.full(n, np.nan)
        return self.sse.sum(axis=1, dtype=np.uint64).astype(np.float64) / float(self.samples * C)

    def rmse(self) -> np.ndarray:
        return np.sqrt(self.mse())

    def psnr(self) -> np.ndarray:
        """10 log10(255^2 / mse); inf where the frames are equal."""
        return psnr_of_mse(self.mse())


def psnr_of_mse(mse) -> np.ndarray:
    mse = np.asarray(mse, np.float64)
    with np.errstate(divide="ignore"):
        return np.where(mse == 0, np.inf, 10.0 * np.log10(255.0 ** 2 / np.where(mse == 0, 1.0, mse)))


def records(buf: DeviceBuffer, n: int, C: int, samples: int, stream=None) -> Distortion:
    """Download the n x C records of a sse_device call (synchronises `stream`)."""
    rec = np.zeros((int(n), int(C)), RECORD)
    if rec.size:
        buf.download(rec, stream)
        if stream is not None:
            stream.synchronize()
    return Distortion(rec["sse"].copy(), rec["sad"].copy(), rec["max_abs"].copy(), int(samples))


def sse_device(a: DeviceBuffer, b: DeviceBuffer, n: int, H: int, W: int, C: int, out: DeviceBuffer | None = None,
               stream=None) -> DeviceBuffer:
    """n frames of H x W x C u8 in `a` against those in `b` -> n x C records (RECORD) in HBM, enqueued on
    `stream`.  The call zeroes the records itself.  With n = 0 or H * W = 0 nothing runs and `out` is left as it is."""
    n, H, W, C = int(n), int(H), int(W), int(C)
    if min(n, H, W) >= 0 and 1 <= C <= 4:
        check_input(a, n * H * W * C)
        check_input(b, n * H * W * C)
    out = output(out, max(n, 0) * max(C, 0) * RECORD.itemsize)
    call("vcf_distortion_u8", a.ptr, b.ptr, n, H, W, C, out.ptr, _h(stream))
    return out


def _frames(a, what: str):
    """(N x H x W x C contiguous u8, whether one frame was given)."""
    a = np.asarray(a)
    if a.dtype != np.uint8:
        raise TypeError(f"{what} must be uint8, got {a.dtype}")
    single = a.ndim in (2, 3)
    if a.ndim == 2:
        a = a[None, :, :, None]
    elif a.ndim == 3:
        a = a[None]
    if a.ndim != 4:
        raise ValueError(f"{what} must be H x W, H x W x C or N x H x W x C, got {a.ndim} dimensions")
    if not 1 <= a.shape[3] <= 4:
        raise ValueError(f"{what} has {a.shape[3]} channels: 1 to 4 are measured")
    return np.ascontiguousarray(a), single


def measure(a, b) -> Distortion:
    """The records of frames a against frames b (one frame or a stack, equal shapes)."""
    shape_a, shape_b = np.shape(a), np.shape(b)
    fa, _ = _frames(a, "a")
    fb, _ = _frames(b, "b")
    if shape_a != shape_b:
        raise ValueError(f"shapes differ: {shape_a} and {shape_b}")
    n, H, W, C = fa.shape
    da = db = out = None
    try:
        da, db = DeviceBuffer.from_array(fa), DeviceBuffer.from_array(fb)
        out = DeviceBuffer(max(1, n * C) * RECORD.itemsize)
        out.fill(0)     # n = 0 or H * W = 0: the call leaves the records alone
        sse_device(da, db, n, H, W, C, out)
        return records(out, n, C, H * W)
    finally:
        for buf in (da, db, out):
            if buf is not None:
                buf.free()


def _reduce(values: np.ndarray, a):
    return float(values[0]) if np.ndim(a) in (2, 3) else values


def mse(a, b):
    """float64(sum sse) / (H * W * C): a float for one frame, an array for a stack."""
    return _reduce(measure(a, b).mse(), a)


def rmse(a, b):
    """sqrt(float64(sum sse) / (H * W * C))."""
    return _reduce(measure(a, b).rmse(), a)


def psnr(a, b):
    """10 log10(255^2 / mse), inf at mse 0."""
    return _reduce(measure(a, b).psnr(), a)


# ---- SSIM (vcf_ssim.hip) -------------------------------------------
# vcf_ssim_record (include/vcf_amd.h)
SSIM_RECORD = np.dtype([("sum_k", np.int64), ("windows", np.uint64), ("min_k", np.int64)])
SSIM_WINDOW = 11           # the footprint; its outer taps are 0, so the support is 9 x 9
SSIM_ONE = 1 << 30         # k = rint(q * 2^30)


@dataclass
class Ssim:
    """Per frame and channel (n x C arrays), exact integers: the sum and the minimum over the windows of
    k = rint(q * 2^30), q the window's SSIM in the integer form of DESIGN.md §4.15."""
    sum_k: np.ndarray      # int64
    min_k: np.ndarray      # int64
    windows: int           # (H - 10) * (W - 10): windows wholly inside one frame

    def per_channel(self) -> np.ndarray:
        """n x C float64: sum_k / (windows * 2^30), one division of exact integers."""
        return self.sum_k.astype(np.float64) / float(self.windows * SSIM_ONE)

    def per_frame(self) -> np.ndarray:
        """n float64, the mean over the channels: (sum over c of sum_k) / (C * windows * 2^30)."""
        C = self.sum_k.shape[1]
        return self.sum_k.sum(axis=1, dtype=np.int64).astype(np.float64) / float(C * self.windows * SSIM_ONE)


class SsimShapeError(ValueError):
    """Frames the SSIM is not defined on: smaller than its window, or neither 1 nor 3 channels."""


def _check_ssim_shape(n: int, H: int, W: int, C: int) -> None:
    if H < SSIM_WINDOW or W < SSIM_WINDOW:
        raise SsimShapeError(f"the SSIM window is {SSIM_WINDOW} x {SSIM_WINDOW}: frames of {H} x {W} hold none")
    if C not in (1, 3):
        raise SsimShapeError(f"SSIM is measured on 1 or 3 channels, got {C}")
    if n < 1:
        raise ValueError(f"SSIM needs at least one frame, got {n}")


def ssim_device(a: DeviceBuffer, b: DeviceBuffer, n: int, H: int, W: int, C: int, out: DeviceBuffer | None = None,
                stream=None) -> DeviceBuffer:
    """n frames of H x W x C u8 in `a` against those in `b` -> n x C records (SSIM_RECORD) in HBM, enqueued on
    `stream`.  The call sets the records itself.  C is 1 or 3, H and W at least 11 (ValueError otherwise)."""
    n, H, W, C = int(n), int(H), int(W), int(C)
    _check_ssim_shape(n, H, W, C)
    check_input(a, n * H * W * C)
    check_input(b, n * H * W * C)
    out = output(out, n * C * SSIM_RECORD.itemsize)
    call("vcf_ssim_u8", a.ptr, b.ptr, n, H, W, C, out.ptr, _h(stream))
    return out


def ssim_records(buf: DeviceBuffer, n: int, C: int, stream=None) -> Ssim:
    """Download the n x C records of a ssim_device call (synchronises `stream`)."""
    rec = np.zeros((int(n), int(C)), SSIM_RECORD)
    buf.download(rec, stream)
    if stream is not None:
        stream.synchronize()
    return Ssim(rec["sum_k"].copy(), rec["min_k"].copy(), int(rec["windows"][0, 0]))


def ssim(a, b) -> Ssim:
    """The SSIM records of host u8 frames a against b: H x W, H x W x C or N x H x W x C, equal shapes."""
    shape_a, shape_b = np.shape(a), np.shape(b)
    fa, _ = _frames(a, "a")
    fb, _ = _frames(b, "b")
    if shape_a != shape_b:
        raise ValueError(f"shapes differ: {shape_a} and {shape_b}")
    n, H, W, C = fa.shape
    _check_ssim_shape(n, H, W, C)
    da = db = out = None
    try:
        da, db = DeviceBuffer.from_array(fa), DeviceBuffer.from_array(fb)
        out = ssim_device(da, db, n, H, W, C)
        return ssim_records(out, n, C)
    finally:
        for buf in (da, db, out):
            if buf is not None:
                buf.free()

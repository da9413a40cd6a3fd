"""A rate estimate that stays on the GPU until it is a few counters (vcf_index_hist.hip).

vcf_index_hist_u8 counts, per frame, region and channel, how often each of
the 256 index values occurs in the u8 index planes the encode kernels write:
exact integers, n x regions x 3 x 256 uint32.  A region is a cell of a rows x
cols grid over the plane: (1, 1) is the whole plane, (B, B) the subbands of
the 2D-DCT's subband layout (B <= 16; the grid must divide the plane).

entropy_bits turns counts into the zeroth-order entropy sum(c * log2(N / c))
on the host, in float64, adding the symbols in ascending order so that the
same counts always give the same bits; estimate_bytes sums it into bytes per
frame under one of two models.  There is no CPU path for the counting.
"""
from __future__ import annotations

import numpy as np

from ._blockio import check_input, output
from ._lib import call
from .device import DeviceBuffer, _h

BINS = 256
CHANNELS = 3
MODEL_BYTES = 2          # "subband": what a coder spends on declaring one non-empty model
MODELS = ("order0", "subband")


def _geometry(shape, regions):
    shape = tuple(int(s) for s in shape)
    if len(shape) == 3:
        shape = (1,) + shape
    if len(shape) != 4 or shape[3] != CHANNELS:
        raise ValueError(f"index frames are H x W x 3 or n x H x W x 3, got {shape}")
    rows, cols = (int(r) for r in regions)
    return shape[0], shape[1], shape[2], rows, cols


def histogram_device(idx: DeviceBuffer, shape, regions=(1, 1), out: DeviceBuffer | None = None,
                     stream=None) -> DeviceBuffer:
    """The counts of the n x H x W x 3 (or H x W x 3) u8 index frames in `idx`, enqueued on `stream`:
    n x rows * cols x 3 x 256 uint32 in HBM.  The call zeroes them itself.  ValueError for a grid
    that does not divide the frame, NotImplementedError for one over 16 x 16."""
    n, H, W, rows, cols = _geometry(shape, regions)
    if min(n, H, W) >= 0:
        check_input(idx, n * H * W * CHANNELS)
    need = max(n, 0) * max(rows, 0) * max(cols, 0) * CHANNELS * BINS
    out = output(out, need * 4)
    call("vcf_index_hist_u8", idx.ptr, n, H, W, rows, cols, out.ptr, out.nbytes // 4, _h(stream))
    return out


def histogram(idx, shape=None, regions=(1, 1)) -> np.ndarray:
    """The counts as a numpy array n x rows * cols x 3 x 256 (uint32).  `idx` is a DeviceBuffer of
    index frames of `shape`, or a uint8 array (then `shape` defaults to its own)."""
    buf = None
    if not isinstance(idx, DeviceBuffer):
        a = np.ascontiguousarray(idx)
        if a.dtype != np.uint8:
            raise TypeError(f"index frames must be uint8, got {a.dtype}")
        shape = a.shape if shape is None else shape
        idx = buf = DeviceBuffer.from_array(a)
    out = None
    try:
        n, _, _, rows, cols = _geometry(shape, regions)
        out = histogram_device(idx, shape, regions)
        counts = np.zeros((n, rows * cols, CHANNELS, BINS), np.uint32)
        if counts.size:
            out.download(counts)
        return counts
    finally:
        for b in (buf, out):
            if b is not None:
                b.free()


def entropy_bits(counts) -> np.ndarray:
    """sum over v of c[v] * log2(N / c[v]), N = sum c, along the last axis (the 256 symbols):
    float64, one value per frame, region and channel.  The terms are added in ascending symbol
    order, so equal counts give equal bits on every run; an empty histogram and one with a single
    symbol give 0."""
    c = np.asarray(counts)
    if c.ndim < 1 or c.shape[-1] != BINS:
        raise ValueError(f"counts end in {BINS} bins, got shape {c.shape}")
    if c.dtype.kind not in "ui":
        raise TypeError(f"counts are integers, got {c.dtype}")
    c = c.astype(np.float64)
    total = np.zeros(c.shape[:-1], np.float64)
    for v in range(BINS):
        total = total + c[..., v]
    bits = np.zeros(c.shape[:-1], np.float64)
    for v in range(BINS):
        cv = c[..., v]
        nz = cv > 0
        ratio = np.where(nz, total / np.where(nz, cv, 1.0), 1.0)
        bits = bits + cv * np.log2(ratio)
    return bits


def estimate_bytes(counts, model: str = "subband") -> np.ndarray:
    """Bytes per frame (int64) that a zeroth-order coder of the given shape would need for the
    counted indices, from counts of shape n x regions x 3 x 256:

      "order0"   one model per channel over all the regions requested: the regions' counts are
                 summed, bytes = ceil(sum over channels of entropy_bits / 8);
      "subband"  one model per region and channel, bytes = ceil(sum of entropy_bits / 8) plus
                 MODEL_BYTES for every model that is not empty.  With the (B, B) grid of the
                 subband layout this is what a context coder can approach.

    This is a model, not a claim about any -c codec: deflate and the adaptive arithmetic coders
    exploit repetitions and contexts that an order-0 count does not see and pay headers it does
    not count.  The rate control (codec/ratecontrol.py) only ranks quantization steps by it and
    always finishes with a real coding pass."""
    c = np.asarray(counts)
    if c.ndim != 4 or c.shape[2:] != (CHANNELS, BINS):
        raise ValueError(f"counts are n x regions x {CHANNELS} x {BINS}, got {c.shape}")
    if model == "order0":
        bits = entropy_bits(c.sum(axis=1, dtype=np.uint64))                  # n x 3
        return np.ceil(bits.sum(axis=1) / 8.0).astype(np.int64)
    if model == "subband":
        bits = entropy_bits(c)                                               # n x regions x 3
        models = (c.sum(axis=3, dtype=np.uint64) > 0).sum(axis=(1, 2)).astype(np.int64)
        return np.ceil(bits.reshape(len(c), -1).sum(axis=1) / 8.0).astype(np.int64) + MODEL_BYTES * models
    raise ValueError(f"model {model!r}: one of {MODELS}")

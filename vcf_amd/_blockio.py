"""What the block-transform wrappers (dct.py, mdct.py, klt.py) share: the frame
and buffer checks, and the host round trip around one launch."""
from __future__ import annotations

import numpy as np

from ._lib import VCF_DCT_NO_SUBBANDS, VCF_DCT_PERCEPTUAL
from .device import DeviceBuffer


def flags_from(disable_subbands: bool = False, perceptual: bool = False) -> int:
    return (VCF_DCT_NO_SUBBANDS if disable_subbands else 0) | (VCF_DCT_PERCEPTUAL if perceptual else 0)


def frames_u8(a: np.ndarray, what: str) -> np.ndarray:
    """HxWx3 or NxHxWx3 u8 -> contiguous NxHxWx3."""
    a = np.asarray(a)
    if a.dtype != np.uint8:
        raise TypeError(f"{what} must be uint8, got {a.dtype}")
    if a.ndim == 3:
        a = a[None]
    if a.ndim != 4 or a.shape[3] != 3:
        raise ValueError("Input image must be a 3D array (height, width, channels).")
    return np.ascontiguousarray(a)


def check_input(buf: DeviceBuffer, nbytes: int) -> None:
    if buf.nbytes < nbytes:
        raise ValueError("input buffer too small")


def output(out: DeviceBuffer | None, nbytes: int) -> DeviceBuffer:
    """`out`, checked, or a new buffer of nbytes."""
    if out is None:
        return DeviceBuffer(nbytes)
    if out.nbytes < nbytes:
        raise ValueError("output buffer too small")
    return out


def round_trip(f: np.ndarray, single: bool, launch, out_shape, dtype=np.uint8, extra=()):
    """Upload the frames f (N first) and the `extra` arrays, dout = launch(din, *dextra), download it
    as N x out_shape; res[0] when `single`.  Every buffer is freed, whatever happens; a launch that
    makes further buffers returns (dout, *them) to have them freed here too."""
    bufs = []
    try:
        for a in (f, *extra):
            bufs.append(DeviceBuffer.from_array(a))
        made = launch(*bufs)
        made = made if isinstance(made, tuple) else (made,)
        bufs.extend(made)
        res = made[0].download(np.empty((f.shape[0],) + tuple(out_shape), dtype))
    finally:
        for b in bufs:
            b.free()
    return res[0] if single else res

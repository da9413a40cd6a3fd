"""Lapped 2D-MDCT + deadzone hot path on the GPU (include/vcf_amd.h vcf_mdct_*).

Replaces, in one fused kernel per direction, the span of src/2D-MDCT.py
encode_fn :498-582 between the image read and the entropy codec (pad, -128,
YCoCg, Malvar's lapped transform in float64, scale, -p, subbands, deadzone,
+128, clip) and of decode_fn :587-666 (from the entropy decoder's uint8 array
to the cropped, clipped RGB frame).  Every block size 2 <= B <= 64.
"""
from __future__ import annotations

import ctypes
import struct

import numpy as np

from ._blockio import check_input, flags_from, frames_u8, output, round_trip
from ._lib import VCF_DCT_NO_SUBBANDS, VCF_DCT_PERCEPTUAL, call
from .device import DeviceBuffer, _h

__all__ = ["padded_shape", "tile_plan", "shape_bin", "flags_from", "encode_device", "decode_device", "encode", "decode",
           "VCF_DCT_NO_SUBBANDS", "VCF_DCT_PERCEPTUAL"]


def padded_shape(H: int, W: int, block_size: int = 8):
    """(Hp, Wp, pad_top, pad_left) of 2D-MDCT.py:446-476."""
    v = [ctypes.c_int32() for _ in range(4)]
    call("vcf_mdct_padded_shape", H, W, block_size, *[ctypes.byref(x) for x in v])
    return tuple(x.value for x in v)


def tile_plan(H: int, W: int, block_size: int = 8, flags: int = 0, decode: bool = False):
    """(TX, TY, lds_class, tiles_x, tiles_y) of the encode (or decode) launch: the tile in blocks
    (decode: segments), the LDS class 0..2 and the tiles each way.  Host only."""
    v = [ctypes.c_int32() for _ in range(5)]
    call("vcf_mdct_tile_plan", H, W, block_size, flags, int(bool(decode)), *[ctypes.byref(x) for x in v])
    return tuple(x.value for x in v)


def shape_bin(H: int, W: int, block_size: int = 8) -> bytes:
    """The 20 bytes of {out}_shape.bin: 'iii' original shape, 'ii' pad_top, pad_left."""
    _, _, top, left = padded_shape(H, W, block_size)
    return struct.pack("iii", H, W, 3) + struct.pack("ii", top, left)


def encode_device(rgb: DeviceBuffer, n_frames: int, H: int, W: int, Q: int = 32, flags: int = 0,
                  out: DeviceBuffer | None = None, stream=None, block_size: int = 8) -> DeviceBuffer:
    """Frames resident in HBM -> coefficient frames in HBM (asynchronous on `stream`)."""
    Hp, Wp = padded_shape(H, W, block_size)[:2]
    check_input(rgb, n_frames * H * W * 3)
    out = output(out, n_frames * Hp * Wp * 3)
    call("vcf_mdct_dz_encode", rgb.ptr, n_frames, H, W, block_size, int(Q), flags, out.ptr, _h(stream))
    return out


def decode_device(k: DeviceBuffer, n_frames: int, H: int, W: int, Q: int = 32, flags: int = 0,
                  out: DeviceBuffer | None = None, stream=None, block_size: int = 8) -> DeviceBuffer:
    Hp, Wp = padded_shape(H, W, block_size)[:2]
    check_input(k, n_frames * Hp * Wp * 3)
    out = output(out, n_frames * H * W * 3)
    call("vcf_mdct_dz_decode", k.ptr, n_frames, H, W, block_size, int(Q), flags, out.ptr, _h(stream))
    return out


def encode(rgb: np.ndarray, Q: int = 32, flags: int = 0, block_size: int = 8) -> np.ndarray:
    """Host convenience: HxWx3 (or NxHxWx3) u8 -> HpxWpx3 (NxHpxWpx3) u8 indices."""
    f = frames_u8(rgb, "rgb")
    n, H, W, _ = f.shape
    return round_trip(f, np.asarray(rgb).ndim == 3,
                      lambda din: encode_device(din, n, H, W, Q, flags, block_size=block_size),
                      padded_shape(H, W, block_size)[:2] + (3,))


def decode(k: np.ndarray, H: int, W: int, Q: int = 32, flags: int = 0, block_size: int = 8) -> np.ndarray:
    """Host convenience: HpxWpx3 (or N...) u8 indices -> HxWx3 u8 reconstruction."""
    f = frames_u8(k, "k")
    Hp, Wp = padded_shape(H, W, block_size)[:2]
    if f.shape[1:3] != (Hp, Wp):
        raise ValueError(f"index frames {f.shape[1:3]} do not match {(Hp, Wp)} for {H}x{W}")
    return round_trip(f, np.asarray(k).ndim == 3,
                      lambda din: decode_device(din, len(f), H, W, Q, flags, block_size=block_size), (H, W, 3))

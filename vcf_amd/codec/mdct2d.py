"""2D-MDCT image codec: the drop-in for src/2D-MDCT.py's CoDec.

Malvar's lapped transform (50 % overlapping sine windows, critically sampled)
over the YCoCg / deadzone / no_filter / <entropy codec> chain: the reference
transform that removes blocking artefacts at low rates.  Same constructor (an
argparse Namespace, see parser.py), same methods and return values, same
files: {out}.tif holding the k + 128 indices clipped to [0, 255] (subband
layout unless -x) and the 20-byte {out}_shape.bin = struct 'iii' original
shape + 'ii' pad_top, pad_left.  The span between reading the image and
handing the indices to the entropy codec (2D-MDCT.py:498-582 encode,
:587-666 decode) runs on the GPU (vcf_mdct_dz_encode / vcf_mdct_dz_decode);
there is no CPU implementation of it in the product.

-B takes every 2 <= B <= 64; -p only B = 8, where the reference's cv2.resize
of the JPEG tables is the identity (other sizes are unpinned: cv2 is not
available).  -a deadzone only: -a LloydMax (the reference's B / 1.5 scale
branch, uint16 indices above 256 levels) raises NotImplementedError.  -t
picks only the base class in the reference (from_RGB/to_RGB are bound to
YCoCg at import), so YCrCb runs as YCoCg, as in dct2d.
"""
from __future__ import annotations

import glob
import logging
import os
import struct

import numpy as np

from .. import mdct as M
from ..device import DeviceBuffer
from .blockcodec import BlockCoDec

ORIGINAL = "/tmp/original.png"   # what the reference's rate/distortion log compares with


class CoDec(BlockCoDec):
    """2D-MDCT.CoDec (2D-MDCT.py:384-684)."""

    BLOCK_SIZE_ARG = "block_size_MDCT"
    COLOR_REFUSAL = "color transform {!r}: YCoCg (and YCrCb, which 2D-MDCT.py runs as YCoCg) are on the HIP path"
    QUANTIZER_REFUSAL = ("quantizer {!r} with 2D-MDCT: only deadzone is on the HIP path "
                         "(LloydMax's B / 1.5 scale branch and uint16 indices are not built)")
    FRAME_ERROR = "Input image must be a 3D array."
    DEBLOCK_REFUSAL = ("filter 'deblock' with 2D-MDCT: a lapped transform has no block edges "
                       "(2D-DCT, 2D-KLT and 2D-LBT have them)")

    def __init__(self, args):
        super().__init__(args)
        self.use_mdct = True
        b = self.block_size   # 2D-MDCT.py:412-421
        self.mdct_scale_factor = b / 2.0 if b <= 8 else (b / 4.0 if b >= 32 else 4.0 + (b - 8) / 24 * 4.0)
        self.pad_top = self.pad_left = None

    def _check_block_size(self):
        if not 2 <= self.block_size <= 64:
            raise NotImplementedError(f"block size {self.block_size}: the MDCT kernels cover 2 <= B <= 64")
        if self.flags & M.VCF_DCT_PERCEPTUAL and self.block_size != 8:
            raise NotImplementedError("-p with 2D-MDCT is pinned at B = 8 only (the reference resizes the "
                                      "JPEG tables with cv2 for other sizes)")

    # ---- the hot path -------------------------------------------------------
    def _set_shape(self, shape):
        self.original_shape = tuple(int(s) for s in shape)
        Hp, Wp, self.pad_top, self.pad_left = M.padded_shape(shape[0], shape[1], self.block_size)
        self.padded_shape = (Hp, Wp, 3)

    def encode_indices(self, img: np.ndarray) -> np.ndarray:
        """2D-MDCT.py:505-578 on the GPU: u8 RGB -> u8 indices (k + 128, clipped)."""
        self._check_frame(img)
        self._set_shape(img.shape)
        return M.encode(img, self.QSS, self.flags, self.block_size)

    def decode_indices(self, k: np.ndarray, shape) -> np.ndarray:
        """2D-MDCT.py:605-658 on the GPU: u8 indices -> u8 RGB (padding removed)."""
        return M.decode(np.ascontiguousarray(k, dtype=np.uint8), int(shape[0]), int(shape[1]), self.QSS,
                        self.flags, self.block_size)

    def _write_side(self, out_fn, shape, extra):
        with open(f"{out_fn}_shape.bin", "wb") as f:
            f.write(M.shape_bin(int(shape[0]), int(shape[1]), self.block_size))

    def _read_side(self, fn):
        with open(f"{fn}_shape.bin", "rb") as f:
            shape = struct.unpack("iii", f.read(12))
            rest = f.read(8)
        Hp, Wp, top, left = M.padded_shape(shape[0], shape[1], self.block_size)
        if len(rest) == 8 and struct.unpack("ii", rest) != (top, left):
            raise ValueError(f"{fn}_shape.bin: pads {struct.unpack('ii', rest)} do not belong to "
                             f"{shape[0]}x{shape[1]} at block size {self.block_size}")
        return shape, None

    def _decoded(self, in_fn, out_fn, y):
        self._log_J(in_fn, out_fn, y)

    def _log_J(self, in_fn, out_fn, y):
        """The reference's diagnostics (calculate_J :337-377): J = bits/pixel + RMSE against
        /tmp/original.png.  It raises there when the file is missing; here it is skipped."""
        if not os.path.exists(ORIGINAL):
            return None
        from .eic import read_image
        x = read_image(ORIGINAL)[0]
        if x.shape != y.shape:
            logging.warning(f"Image dimensions do not match: {x.shape} vs {y.shape}")
            return None
        rmse = float(np.sqrt(np.mean((x.astype(np.float32) - y.astype(np.float32)) ** 2)))
        nbytes = sum(os.path.getsize(f) for f in glob.glob(in_fn + "*"))
        bpp = nbytes * 8 / (y.shape[0] * y.shape[1])
        logging.info(f"J = R + D = {bpp:.2f} + {rmse:.2f} = {bpp + rmse:.2f}")
        return bpp + rmse

    # ---- batched frames: one launch per group of equal shapes, resident in HBM ----
    def _encode_group(self, frames, shape):
        H, W = shape[:2]
        padded = M.padded_shape(H, W, self.block_size)[:2] + (3,)
        din, dk = DeviceBuffer.from_array(frames), None
        try:
            dk = M.encode_device(din, len(frames), H, W, self.QSS, self.flags, block_size=self.block_size)
            return [(out, None) for out in self._indices_out(dk, len(frames), padded)]
        finally:
            din.free()
            if dk is not None:
                dk.free()

    def _decode_group(self, ks, shape, extras):
        ks = np.stack([np.ascontiguousarray(k, dtype=np.uint8) for k in ks])
        return M.decode(ks, shape[0], shape[1], self.QSS, self.flags, self.block_size)

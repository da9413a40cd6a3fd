"""2D-KLT image codec: the drop-in for src/2D-KLT.py's CoDec.

A Karhunen-Loeve transform of the B x B blocks, learned per image and colour
channel (the eigenvectors of the blocks' covariance, largest eigenvalue
first), over the YCoCg / deadzone / no_filter / <entropy codec> chain.  Same
constructor (an argparse Namespace, see parser.py), same methods and return
values, same three files: {out}.tif holding the k + 128 indices wrapped to u8
(subband layout unless -x), the 12-byte {out}_shape.bin = struct 'iii'
original shape, and {out}_weights.npz with key 'weights', float32, shape
(3, D, D), D = B * B.  The encoder transforms with the float64 basis and
stores it rounded to float32; the decoder widens what it reads.  The second
moments, the transform and everything between the image and the entropy codec
run on the GPU (vcf_klt_moments / vcf_klt_dz_encode / vcf_klt_dz_decode); the
D x D eigenproblem runs on the host.  There is no CPU implementation of the
hot path in the product.

-B takes 2 <= B <= 16 (B = 1 and a frame of one block have no covariance
matrix: ValueError, as in the reference).  -a deadzone and -t YCoCg only; -f
no_filter, or deblock (decode, B >= 4: vcf_amd/deblock.py); -p and -L are not
options of this codec.
"""
from __future__ import annotations

import struct

import numpy as np

from .. import klt as K
from ..device import DeviceBuffer
from .blockcodec import BlockCoDec


class CoDec(BlockCoDec):
    """2D-KLT.CoDec (2D-KLT.py:302-860)."""

    BLOCK_SIZE_ARG = "block_size"
    COLOR_TRANSFORMS = ("YCoCg",)
    COLOR_REFUSAL = "color transform {!r} with 2D-KLT: only YCoCg is on the HIP path"
    QUANTIZER_REFUSAL = "quantizer {!r} with 2D-KLT: only deadzone is on the HIP path"
    FILTER_CHECKED_ALWAYS = True
    FLAG_MASK = K.VCF_DCT_NO_SUBBANDS
    FRAME_ERROR = "Input image must be a 3D array."

    def _check_block_size(self):
        if self.block_size < 2:
            raise ValueError(f"block size {self.block_size}: blocks of one sample have no covariance matrix")
        if self.block_size > 16:
            raise NotImplementedError(f"block size {self.block_size}: the KLT kernels cover 2 <= B <= 16")

    def _crop_offsets(self, H, W):
        return K.padded_shape(H, W, self.block_size)[2:4]

    # ---- the hot path -------------------------------------------------------
    def _check_frame(self, img):
        super()._check_frame(img)
        K.check_blocks(img.shape[0], img.shape[1], self.block_size)

    def encode_indices(self, img: np.ndarray):
        """2D-KLT.py:515-628 on the GPU: u8 RGB -> (u8 indices, float64 weights (3, D, D))."""
        self._check_frame(img)
        self._set_shape(img.shape)
        return K.encode(img, self.QSS, self.flags, self.block_size)

    def decode_indices(self, k: np.ndarray, shape, weights32: np.ndarray) -> np.ndarray:
        """2D-KLT.py:738-809 on the GPU: u8 indices and the stored weights -> u8 RGB."""
        return K.decode(np.ascontiguousarray(k, dtype=np.uint8), int(shape[0]), int(shape[1]), self.QSS,
                        self.flags, self.block_size, weights32, post=self._post())

    def _encode_one(self, img):
        k, w64 = self.encode_indices(img)
        return self.compress(k), w64

    def _decode_one(self, k, shape, w32):
        return self.decode_indices(k, shape, w32)

    def _write_side(self, out_fn, shape, weights64):
        with open(f"{out_fn}_shape.bin", "wb") as f:
            f.write(K.shape_bin(int(shape[0]), int(shape[1])))
        np.savez_compressed(f"{out_fn}_weights.npz", weights=np.asarray(weights64).astype(np.float32))

    def _read_side(self, fn):
        with open(f"{fn}_shape.bin", "rb") as f:
            data = f.read(12)
        if len(data) != 12:
            raise ValueError(f"{fn}_shape.bin: not 12 bytes")
        shape = struct.unpack("iii", data)
        D = self.block_size * self.block_size
        with np.load(f"{fn}_weights.npz") as z:
            w = z["weights"]
        if w.dtype != np.float32 or w.size != 3 * D * D:
            raise ValueError(f"{fn}_weights.npz: {w.dtype} {w.shape} is not float32 (3, {D}, {D})")
        return shape, np.ascontiguousarray(w).reshape(3, D, D)

    # ---- batched frames: one launch per group of equal shapes, resident in HBM ----
    def _encode_group(self, frames, shape):
        """One moments launch, one host eigh per frame and channel, one encode launch."""
        H, W = shape[:2]
        n, B = len(frames), self.block_size
        padded = K.padded_shape(H, W, B)[:2] + (3,)
        bufs = [DeviceBuffer.from_array(frames)]
        try:
            w64 = K._train(bufs[0], n, H, W, B)
            bufs.append(DeviceBuffer.from_array(w64))
            bufs.append(K.encode_device(bufs[0], n, H, W, bufs[1], self.QSS, self.flags, block_size=B))
            return list(zip(self._indices_out(bufs[2], n, padded), w64))
        finally:
            for b in bufs:
                b.free()

    def _decode_group(self, ks, shape, weights32):
        ks = np.stack([np.ascontiguousarray(k, dtype=np.uint8) for k in ks])
        return K.decode(ks, shape[0], shape[1], self.QSS, self.flags, self.block_size, np.stack(weights32),
                        post=self._post())

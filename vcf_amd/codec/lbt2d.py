"""2D-LBT image codec: the drop-in for src/2D-LBT.py's CoDec.

A learned block transform: per image, a linear autoencoder of the B x B blocks
of all three YCoCg channels is trained with Adam (--epochs, --lr, -L the weight
of the log-variance term), the coefficients y = We (x - mean) go through the
deadzone / no_filter / <entropy codec> chain, and the decoder matrix and the
mean travel as side information.  Same constructor (an argparse Namespace, see
parser.py), same methods and return values, same three files: {out}<ext>
holding the k + 128 indices clipped to u8 (subband layout unless -x), the
12-byte {out}_shape.bin = struct 'iii' original shape, and {out}.weights.pth
(or the path --side_info names), a torch.save of {'decoder_state': {'weight':
float32 (D, D)}, 'mean_val': float}, written and read by vcf_amd/pth.py
without torch.  Moments, training, transform and everything between the image
and the entropy codec run on the GPU (vcf_lbt_*); there is no CPU
implementation of the hot path in the product.

The reference draws its initial weights unseeded; here they are seeded (see
vcf_amd/lbt.py), so equal runs write equal files.  -B takes 2 <= B <= 8.
-a deadzone and -t YCoCg only; -f no_filter, or deblock (decode, B >= 4:
vcf_amd/deblock.py).  With --side_info every frame of
a batch names the same file, as in the reference: it is for single frames.
"""
from __future__ import annotations

import logging
import struct

import numpy as np

from .. import lbt as L
from .. import pth
from ..device import DeviceBuffer
from .blockcodec import BlockCoDec


class CoDec(BlockCoDec):
    """2D-LBT.CoDec (2D-LBT.py:204-627)."""

    BLOCK_SIZE_ARG = "block_size_DCT"
    COLOR_TRANSFORMS = ("YCoCg",)
    COLOR_REFUSAL = "color transform {!r} with 2D-LBT: only YCoCg is on the HIP path"
    QUANTIZER_REFUSAL = "quantizer {!r} with 2D-LBT: only deadzone is on the HIP path"
    FILTER_CHECKED_ALWAYS = True
    FLAG_MASK = L.VCF_DCT_NO_SUBBANDS | L.VCF_DCT_PERCEPTUAL
    FRAME_ERROR = "Input image must be a 3D array (height, width, channels)."

    def __init__(self, args):
        super().__init__(args)
        self.epochs = int(getattr(args, "epochs", L.EPOCHS))          # 2D-LBT.py:257-264
        self.lr = float(getattr(args, "lr", L.LR))
        self.lambda_gain = L.LAMBDA
        lam = getattr(args, "Lambda", None)
        if lam is not None:
            try:
                self.lambda_gain = float(lam)
            except ValueError:
                logging.warning("Valor de Lambda inválido, usando 1e-6")
        if self.epochs < 0:
            raise ValueError(f"--epochs {self.epochs}: not a number of training steps")
        self.side_info = getattr(args, "side_info", None)

    def _check_block_size(self):
        L.check_block_size(self.block_size)

    def _crop_offsets(self, H, W):
        return L.padded_shape(H, W, self.block_size)[2:4]

    def _side_path(self, fn):
        return self.side_info if self.side_info is not None else f"{fn}.weights.pth"

    def _train_args(self):
        return self.epochs, self.lr, self.lambda_gain

    # ---- the hot path -------------------------------------------------------
    def encode_indices(self, img: np.ndarray):
        """2D-LBT.py:364-452 on the GPU: u8 RGB -> (u8 indices, decoder weights float32 (D, D), mean)."""
        self._check_frame(img)
        self._set_shape(img.shape)
        return L.encode(img, self.QSS, self.flags, self.block_size, None, None, *self._train_args())

    def decode_indices(self, k: np.ndarray, shape, weights: np.ndarray, mean: float) -> np.ndarray:
        """2D-LBT.py:476-563 on the GPU: u8 indices, the stored matrix and mean -> u8 RGB."""
        return L.decode(np.ascontiguousarray(k, dtype=np.uint8), int(shape[0]), int(shape[1]), self.QSS,
                        self.flags, self.block_size, weights, mean, post=self._post())

    def _encode_one(self, img):
        k, wd, mean = self.encode_indices(img)
        return self.compress(k), (wd, mean)

    def _decode_one(self, k, shape, extra):
        return self.decode_indices(k, shape, *extra)

    def _write_side(self, out_fn, shape, extra):
        wd, mean = extra
        with open(f"{out_fn}_shape.bin", "wb") as f:
            f.write(L.shape_bin(int(shape[0]), int(shape[1])))
        pth.save(self._side_path(out_fn), np.asarray(wd, np.float32), float(mean))

    def _read_side(self, fn):
        with open(f"{fn}_shape.bin", "rb") as f:
            data = f.read(12)
        if len(data) != 12:
            raise ValueError(f"{fn}_shape.bin: not 12 bytes")
        shape = struct.unpack("iii", data)
        return shape, pth.load(self._side_path(fn), self.block_size * self.block_size)

    # ---- batched frames: one launch per group of equal shapes, resident in HBM ----
    def _encode_group(self, frames, shape):
        """One moments launch, one train launch (a workgroup per frame), one encode launch."""
        H, W = shape[:2]
        n, B = len(frames), self.block_size
        D = B * B
        padded = L.padded_shape(H, W, B)[:2] + (3,)
        bufs = [DeviceBuffer.from_array(frames)]
        try:
            bufs.extend(L._train(bufs[0], n, H, W, B, *self._train_args()))
            dwe, dwd, dmean = bufs[1:4]
            bufs.append(L.encode_device(bufs[0], n, H, W, dwe, dmean, self.QSS, self.flags, block_size=B))
            wd = dwd.download(np.empty((n, D, D), np.float32))
            mean = dmean.download(np.empty(n, np.float32))
            return [(k, (w, m)) for k, w, m in zip(self._indices_out(bufs[-1], n, padded), wd, mean)]
        finally:
            for b in bufs:
                b.free()

    def _decode_group(self, ks, shape, extras):
        ks = np.stack([np.ascontiguousarray(k, dtype=np.uint8) for k in ks])
        return L.decode(ks, shape[0], shape[1], self.QSS, self.flags, self.block_size,
                        np.stack([e[0] for e in extras]), np.array([e[1] for e in extras], np.float32),
                        post=self._post())

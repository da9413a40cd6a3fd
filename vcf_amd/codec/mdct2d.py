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
import io
import logging
import os
import struct
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from .. import mdct as M
from ..device import DeviceBuffer
from .dct2d import _flags, make_entropy
from .eic import CoDec as EICCoDec
from .tiff import TIFFCodec

ORIGINAL = "/tmp/original.png"   # what the reference's rate/distortion log compares with


class CoDec(EICCoDec):
    """2D-MDCT.CoDec (2D-MDCT.py:384-684)."""

    def __init__(self, args):
        super().__init__(args)
        self.block_size = int(getattr(args, "block_size_MDCT", 8))
        ct = getattr(args, "color_transform", "YCoCg")
        if ct not in ("YCoCg", "YCrCb"):
            raise NotImplementedError(f"color transform {ct!r}: YCoCg (and YCrCb, which 2D-MDCT.py runs as "
                                      "YCoCg) are on the HIP path")
        quant = getattr(args, "quantizer", "deadzone")
        if quant != "deadzone":
            raise NotImplementedError(f"quantizer {quant!r} with 2D-MDCT: only deadzone is on the HIP path "
                                      "(LloydMax's B / 1.5 scale branch and uint16 indices are not built)")
        filt = getattr(args, "filter", "no_filter")
        if not self.encoding and filt != "no_filter":
            raise NotImplementedError(f"filter {filt!r}: only no_filter is on the HIP path")
        if not 2 <= self.block_size <= 64:
            raise NotImplementedError(f"block size {self.block_size}: the MDCT kernels cover 2 <= B <= 64")
        self.flags = _flags(args)
        if self.flags & M.VCF_DCT_PERCEPTUAL and self.block_size != 8:
            raise NotImplementedError("-p with 2D-MDCT is pinned at B = 8 only (the reference resizes the "
                                      "JPEG tables with cv2 for other sizes)")
        self.entropy = make_entropy(args)
        self.file_extension = self.entropy.file_extension
        self.QSS = int(getattr(args, "QSS", 32))
        self.offset = 128
        self.use_mdct = True
        b = self.block_size   # 2D-MDCT.py:412-421
        self.mdct_scale_factor = b / 2.0 if b <= 8 else (b / 4.0 if b >= 32 else 4.0 + (b - 8) / 24 * 4.0)
        self.original_shape = None
        self.pad_top = self.pad_left = None

    def compress(self, img):
        return self.entropy.compress(img)

    def decompress(self, codestream):
        return self.entropy.decompress(codestream)

    # ---- the hot path -------------------------------------------------------
    def _check_frame(self, img):
        if img.ndim != 3:
            raise ValueError("Input image must be a 3D array.")
        if img.dtype != np.uint8 or img.shape[2] != 3:
            raise NotImplementedError(f"{img.dtype} x{img.shape[2]} images: the HIP path takes u8 RGB")

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

    def _shape_bytes(self, shape) -> bytes:
        return M.shape_bin(int(shape[0]), int(shape[1]), self.block_size)

    def _read_shape(self, fn):
        with open(f"{fn}_shape.bin", "rb") as f:
            shape = struct.unpack("iii", f.read(12))
            rest = f.read(8)
        Hp, Wp, top, left = M.padded_shape(shape[0], shape[1], self.block_size)
        if len(rest) == 8 and struct.unpack("ii", rest) != (top, left):
            raise ValueError(f"{fn}_shape.bin: pads {struct.unpack('ii', rest)} do not belong to "
                             f"{shape[0]}x{shape[1]} at block size {self.block_size}")
        return shape

    def encode_fn(self, in_fn, out_fn):
        img = self.encode_read_fn(in_fn)
        cs = self.compress(self.encode_indices(img))
        with open(f"{out_fn}_shape.bin", "wb") as f:
            f.write(self._shape_bytes(img.shape))
        return self.encode_write_fn(cs, out_fn)

    def encode(self, in_fn="/tmp/original.png", out_fn="/tmp/encoded"):
        return self.encode_fn(in_fn, out_fn)

    def decode_fn(self, in_fn, out_fn):
        codestream = self.decode_read_fn(in_fn)
        shape = self._read_shape(in_fn)
        self._set_shape(shape)
        y = self.decode_indices(self.decompress(codestream), shape)
        size = self.decode_write_fn(y, out_fn)
        self._log_J(in_fn, out_fn, y)
        return size

    def decode(self, in_fn="/tmp/encoded", out_fn="/tmp/decoded.png"):
        return self.decode_fn(in_fn, out_fn)

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

    # ---- batched frames (III runner): one launch per group of equal shapes ----
    def encode_fns(self, pairs, batch: int = 64, io_threads: int = 16):
        """encode_fn over (in_fn, out_fn) pairs; returns the bytes written per frame.  Host threads
        read the PNGs and write the files; each group of equal shapes is one launch, and with
        -c TIFF its strips are deflated on the GPU from the indices in HBM (vcf_amd/zlib_gpu.py)."""
        pairs = list(pairs)
        sizes = [0] * len(pairs)

        def _read(p):
            img = self.encode_read_fn(p[0])
            self._check_frame(img)
            return img

        def _write(out_fn, shape, payload):
            with open(f"{out_fn}_shape.bin", "wb") as f:
                f.write(self._shape_bytes(shape))
            cs = io.BytesIO(payload) if isinstance(payload, bytes) else self.compress(payload)
            return self.encode_write_fn(cs, out_fn)

        gpu_tiff = isinstance(self.entropy, TIFFCodec) and TIFFCodec.gpu_batches
        with ThreadPoolExecutor(max_workers=io_threads) as pool:
            writes = []
            for b0 in range(0, len(pairs), batch):
                chunk = pairs[b0:b0 + batch]
                imgs = list(pool.map(_read, chunk))
                groups = {}
                for i, img in enumerate(imgs):
                    groups.setdefault(img.shape, []).append(i)
                for shape, idx in groups.items():
                    H, W = shape[:2]
                    Hp, Wp = M.padded_shape(H, W, self.block_size)[:2]
                    din = DeviceBuffer.from_array(np.stack([imgs[i] for i in idx]))
                    dk = M.encode_device(din, len(idx), H, W, self.QSS, self.flags, block_size=self.block_size)
                    from .. import zlib_gpu
                    if gpu_tiff and zlib_gpu.covers((Hp, Wp, 3), 1):
                        outs = zlib_gpu.tiff_frames_device(dk, len(idx), (Hp, Wp, 3), np.uint8)
                    else:
                        outs = list(dk.download(np.empty((len(idx), Hp, Wp, 3), np.uint8)))
                    din.free()
                    dk.free()
                    for j, i in enumerate(idx):
                        writes.append((b0 + i, pool.submit(_write, chunk[i][1], shape, outs[j])))
                self._set_shape(imgs[-1].shape)
            for i, f in writes:
                sizes[i] = f.result()
        return sizes

    def decode_fns(self, pairs, batch: int = 64, io_threads: int = 16):
        """decode_fn over (in_fn, out_fn) pairs: host threads read and inflate the code-streams and
        write the PNGs; each group of equal shapes is one launch."""
        pairs = list(pairs)
        sizes = [0] * len(pairs)

        def _read(p):
            return self.decompress(self.decode_read_fn(p[0])), self._read_shape(p[0])

        with ThreadPoolExecutor(max_workers=io_threads) as pool:
            writes = []
            for b0 in range(0, len(pairs), batch):
                chunk = pairs[b0:b0 + batch]
                got = list(pool.map(_read, chunk))
                groups = {}
                for i, (_, shp) in enumerate(got):
                    groups.setdefault(tuple(shp), []).append(i)
                for shp, idx in groups.items():
                    ks = np.stack([np.ascontiguousarray(got[i][0], dtype=np.uint8) for i in idx])
                    out = M.decode(ks, shp[0], shp[1], self.QSS, self.flags, self.block_size)
                    for j, i in enumerate(idx):
                        writes.append((b0 + i, pool.submit(self.decode_write_fn, out[j], chunk[i][1])))
                self._set_shape(got[-1][1])
            for i, f in writes:
                sizes[i] = f.result()
        return sizes

    # ---- quantizer surface (deadzone.py:95-124) -----------------------------
    def quantize_decom(self, decom):
        return self.quantize(decom)

    def dequantize_decom(self, decom_k):
        return self.dequantize(decom_k)

    def quantize(self, img, fn="/tmp/encoded"):
        from .. import quant
        return quant.deadzone_quantize(img, self.QSS)

    def dequantize(self, k, fn="/tmp/encoded"):
        from .. import quant
        return quant.deadzone_dequantize(k, self.QSS)

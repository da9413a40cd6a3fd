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
matrix: ValueError, as in the reference).  -a deadzone, -t YCoCg and -f
no_filter only; -p and -L are not options of this codec.
"""
from __future__ import annotations

import io
import struct
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from .. import klt as K
from ..device import DeviceBuffer
from .dct2d import _flags, make_entropy
from .eic import CoDec as EICCoDec
from .tiff import TIFFCodec


class CoDec(EICCoDec):
    """2D-KLT.CoDec (2D-KLT.py:302-860)."""

    def __init__(self, args):
        super().__init__(args)
        self.block_size = int(getattr(args, "block_size", 8))
        ct = getattr(args, "color_transform", "YCoCg")
        if ct != "YCoCg":
            raise NotImplementedError(f"color transform {ct!r} with 2D-KLT: only YCoCg is on the HIP path")
        quant = getattr(args, "quantizer", "deadzone")
        if quant != "deadzone":
            raise NotImplementedError(f"quantizer {quant!r} with 2D-KLT: only deadzone is on the HIP path")
        filt = getattr(args, "filter", "no_filter")
        if filt != "no_filter":
            raise NotImplementedError(f"filter {filt!r}: only no_filter is on the HIP path")
        if self.block_size < 2:
            raise ValueError(f"block size {self.block_size}: blocks of one sample have no covariance matrix")
        if self.block_size > 16:
            raise NotImplementedError(f"block size {self.block_size}: the KLT kernels cover 2 <= B <= 16")
        self.flags = _flags(args) & K.VCF_DCT_NO_SUBBANDS
        self.entropy = make_entropy(args)
        self.file_extension = self.entropy.file_extension
        self.QSS = int(getattr(args, "QSS", 32))
        self.offset = 128
        self.original_shape = None

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
        K.check_blocks(img.shape[0], img.shape[1], self.block_size)

    def encode_indices(self, img: np.ndarray):
        """2D-KLT.py:515-628 on the GPU: u8 RGB -> (u8 indices, float64 weights (3, D, D))."""
        self._check_frame(img)
        self.original_shape = tuple(int(s) for s in img.shape)
        return K.encode(img, self.QSS, self.flags, self.block_size)

    def decode_indices(self, k: np.ndarray, shape, weights32: np.ndarray) -> np.ndarray:
        """2D-KLT.py:738-809 on the GPU: u8 indices and the stored weights -> u8 RGB."""
        return K.decode(np.ascontiguousarray(k, dtype=np.uint8), int(shape[0]), int(shape[1]), self.QSS,
                        self.flags, self.block_size, weights32)

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

    def encode_fn(self, in_fn, out_fn):
        img = self.encode_read_fn(in_fn)
        k, w64 = self.encode_indices(img)
        self._write_side(out_fn, img.shape, w64)
        return self.encode_write_fn(self.compress(k), out_fn)

    def encode(self, in_fn="/tmp/original.png", out_fn="/tmp/encoded"):
        return self.encode_fn(in_fn, out_fn)

    def decode_fn(self, in_fn, out_fn):
        codestream = self.decode_read_fn(in_fn)
        shape, w32 = self._read_side(in_fn)
        self.original_shape = shape
        y = self.decode_indices(self.decompress(codestream), shape, w32)
        return self.decode_write_fn(y, out_fn)

    def decode(self, in_fn="/tmp/encoded", out_fn="/tmp/decoded.png"):
        return self.decode_fn(in_fn, out_fn)

    # ---- batched frames (III runner): one launch per group of equal shapes ----
    def encode_fns(self, pairs, batch: int = 64, io_threads: int = 16):
        """encode_fn over (in_fn, out_fn) pairs; returns the bytes written per frame.  Host threads
        read the PNGs and write the files; each group of equal shapes is one moments launch, one
        host eigh per frame and channel, and one encode launch; with -c TIFF the strips are
        deflated on the GPU from the indices in HBM (vcf_amd/zlib_gpu.py)."""
        pairs = list(pairs)
        sizes = [0] * len(pairs)
        B = self.block_size

        def _read(p):
            img = self.encode_read_fn(p[0])
            self._check_frame(img)
            return img

        def _write(out_fn, shape, w64, payload):
            self._write_side(out_fn, shape, w64)
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
                    Hp, Wp = K.padded_shape(H, W, B)[:2]
                    din = DeviceBuffer.from_array(np.stack([imgs[i] for i in idx]))
                    w64 = K._train(din, len(idx), H, W, B)
                    dw = DeviceBuffer.from_array(w64)
                    dk = K.encode_device(din, len(idx), H, W, dw, self.QSS, self.flags, block_size=B)
                    from .. import zlib_gpu
                    if gpu_tiff and zlib_gpu.covers((Hp, Wp, 3), 1):
                        outs = zlib_gpu.tiff_frames_device(dk, len(idx), (Hp, Wp, 3), np.uint8)
                    else:
                        outs = list(dk.download(np.empty((len(idx), Hp, Wp, 3), np.uint8)))
                    din.free()
                    dw.free()
                    dk.free()
                    for j, i in enumerate(idx):
                        writes.append((b0 + i, pool.submit(_write, chunk[i][1], shape, w64[j], outs[j])))
                self.original_shape = tuple(int(s) for s in imgs[-1].shape)
            for i, f in writes:
                sizes[i] = f.result()
        return sizes

    def decode_fns(self, pairs, batch: int = 64, io_threads: int = 16):
        """decode_fn over (in_fn, out_fn) pairs: host threads read and inflate the code-streams and
        write the PNGs; each group of equal shapes is one launch, every frame with its own weights."""
        pairs = list(pairs)
        sizes = [0] * len(pairs)

        def _read(p):
            return (self.decompress(self.decode_read_fn(p[0])),) + self._read_side(p[0])

        with ThreadPoolExecutor(max_workers=io_threads) as pool:
            writes = []
            for b0 in range(0, len(pairs), batch):
                chunk = pairs[b0:b0 + batch]
                got = list(pool.map(_read, chunk))
                groups = {}
                for i, (_, shp, _) in enumerate(got):
                    groups.setdefault(tuple(shp), []).append(i)
                for shp, idx in groups.items():
                    ks = np.stack([np.ascontiguousarray(got[i][0], dtype=np.uint8) for i in idx])
                    ws = np.stack([got[i][2] for i in idx])
                    out = K.decode(ks, shp[0], shp[1], self.QSS, self.flags, self.block_size, ws)
                    for j, i in enumerate(idx):
                        writes.append((b0 + i, pool.submit(self.decode_write_fn, out[j], chunk[i][1])))
                self.original_shape = tuple(got[-1][1])
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

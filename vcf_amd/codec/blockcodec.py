"""What the block-transform codecs (dct2d, mdct2d, klt2d) do alike: the option
checks, the entropy stage, encode_fn / decode_fn, the deadzone quantizer
surface and the batched encode_fns / decode_fns of the III runner.

A subclass names its low-level wrapper and states its differences as class
attributes and a few hooks:

    _check_block_size()               the -B range (and what depends on it)
    _set_shape(shape)                 the shape state kept after a frame
    _write_side(out_fn, shape, extra) / _read_side(fn) -> (shape, extra)
                                      {out}_shape.bin and any other side file;
                                      `extra` is what travels with a frame
                                      besides its indices (KLT's weights)
    encode_indices / decode_indices   one frame through the wrapper
    _encode_group(frames, shape) -> [(payload, extra)] per frame
    _decode_group(items, shape, extras) -> the n RGB frames
                                      one launch for a group of equal shapes
"""
from __future__ import annotations

import io
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from .._blockio import flags_from
from .eic import CoDec as EICCoDec
from .entropy import make_entropy
from .tiff import TIFFCodec


def _flags(args) -> int:
    return flags_from(bool(getattr(args, "disable_subbands", False)),
                      bool(getattr(args, "perceptual_quantization", False)))


class BlockCoDec(EICCoDec):
    BLOCK_SIZE_ARG = None                     # the Namespace field -B lands in
    COLOR_TRANSFORMS = ("YCoCg", "YCrCb")     # -t only picks the base class in the reference: both run as YCoCg
    COLOR_REFUSAL = None                      # NotImplementedError texts, formatted with the refused name
    QUANTIZER_REFUSAL = None
    FILTER_CHECKED_ALWAYS = False             # else -f is checked when decoding only
    DEBLOCK_REFUSAL = None                    # why -f deblock cannot run on this codec (MDCT), or None
    FLAG_MASK = ~0
    FRAME_ERROR = None                        # _check_frame's ValueError text

    def __init__(self, args):
        super().__init__(args)
        self.block_size = int(getattr(args, self.BLOCK_SIZE_ARG, 8))
        ct = getattr(args, "color_transform", "YCoCg")
        if ct not in self.COLOR_TRANSFORMS:
            raise NotImplementedError(self.COLOR_REFUSAL.format(ct))
        self.lm = self._quantizer(args)
        filt = getattr(args, "filter", "no_filter")
        self.deblock = None                   # -f deblock when decoding: (beta, tc), None where a flag is absent
        if filt == "deblock" and not self.encoding:
            self.deblock = self._deblock_option(args)
        elif (self.FILTER_CHECKED_ALWAYS or not self.encoding) and filt != "no_filter":
            raise NotImplementedError(f"filter {filt!r}: only no_filter and deblock are on the HIP path")
        self.flags = _flags(args) & self.FLAG_MASK
        self._check_block_size()
        self.entropy = make_entropy(args)
        self.file_extension = self.entropy.file_extension
        self.QSS = int(getattr(args, "QSS", 32))
        self.offset = 128 if self.lm is None else 0    # 2D-DCT.py:106-109
        self.original_shape = None

    def _quantizer(self, args):
        """None for -a deadzone (fused into the transform kernels); anything else is refused here."""
        quant = getattr(args, "quantizer", "deadzone")
        if quant != "deadzone":
            raise NotImplementedError(self.QUANTIZER_REFUSAL.format(quant))
        return None

    # ---- -f deblock (not in the reference; vcf_amd/deblock.py) ----
    def _deblock_option(self, args):
        from .. import deblock as DB
        if self.DEBLOCK_REFUSAL is not None:
            raise NotImplementedError(self.DEBLOCK_REFUSAL)
        if self.block_size < DB.MIN_BLOCK_SIZE:
            raise NotImplementedError(f"-f deblock with -B {self.block_size}: the filter reads three samples on each "
                                      f"side of a block edge, so the blocks must be at least {DB.MIN_BLOCK_SIZE} wide")
        beta, tc = getattr(args, "deblock_beta", None), getattr(args, "deblock_tc", None)
        if (beta is not None and int(beta) < 0) or (tc is not None and int(tc) < 0):
            raise ValueError(f"--deblock_beta {beta} / --deblock_tc {tc}: values >= 0")
        return beta, tc

    def _crop_offsets(self, H, W):
        """(top, left): the rows and columns of padding this codec's decode crops."""
        from .. import deblock as DB
        return DB.crop_offsets(H, W, self.block_size)

    def _post(self, QSS=None):
        """None, or what follows the decode kernel on the device: post(d, n, H, W, stream=None) filters the
        n decoded frames in d into a new buffer and returns (it, d), for round_trip to download the first
        and free both."""
        if self.deblock is None:
            return None
        from .. import deblock as DB
        beta, tc = DB.strength(self.QSS if QSS is None else QSS, *self.deblock)

        def post(d, n, H, W, stream=None, out=None):
            top, left = self._crop_offsets(H, W)
            return DB.deblock_device(d, n, H, W, self.block_size, top, left, beta, tc, out=out, stream=stream), d
        return post

    # entropy stage (TIFF.py / CBAAC.py surface)
    def compress(self, img):
        return self.entropy.compress(img)

    def decompress(self, codestream):
        return self.entropy.decompress(codestream)

    def _check_frame(self, img):
        if img.ndim != 3:
            raise ValueError(self.FRAME_ERROR)
        if img.dtype != np.uint8 or img.shape[2] != 3:
            raise NotImplementedError(f"{img.dtype} x{img.shape[2]} images: the HIP path takes u8 RGB")

    def _set_shape(self, shape):
        self.original_shape = tuple(int(s) for s in shape)

    # ---- one frame ----------------------------------------------------------
    def _encode_one(self, img):
        """-> (code-stream, extra)."""
        return self.compress(self.encode_indices(img)), None

    def _decode_one(self, k, shape, extra):
        return self.decode_indices(k, shape)

    def encode_fn(self, in_fn, out_fn):
        img = self.encode_read_fn(in_fn)
        cs, extra = self._encode_one(img)
        self._write_side(out_fn, img.shape, extra)
        return self.encode_write_fn(cs, out_fn)

    def encode(self, in_fn="/tmp/original.png", out_fn="/tmp/encoded"):
        # 2D-DCT.py:374-375: the reference's encode() ignores -o/-e
        return self.encode_fn(in_fn, out_fn)

    def decode_fn(self, in_fn, out_fn):
        codestream = self.decode_read_fn(in_fn)
        shape, extra = self._read_side(in_fn)
        self._set_shape(shape)
        y = self._decode_one(self.decompress(codestream), shape, extra)
        size = self.decode_write_fn(y, out_fn)
        self._decoded(in_fn, out_fn, y)
        return size

    def decode(self, in_fn="/tmp/encoded", out_fn="/tmp/decoded.png"):
        return self.decode_fn(in_fn, out_fn)

    def _decoded(self, in_fn, out_fn, y):
        """After decode_fn has written y (MDCT's J log)."""

    # ---- batched frames (III runner): one launch per group of equal shapes --
    def _batches(self, pairs, batch, io_threads, read, run_group, write):
        """The pipeline of encode_fns and decode_fns: host threads read the next two batches
        (read(pair) -> (item, shape, extra)) while the GPU works on this one -- run_group(the
        reads of one shape, in order; shape) -> one result per frame, once per shape of a batch in
        first-seen order -- and write(pair, shape, result) -> bytes written runs behind on the
        same pool.  -> the sizes in input order."""
        batches = [pairs[b0:b0 + batch] for b0 in range(0, len(pairs), batch)]
        with ThreadPoolExecutor(max_workers=io_threads) as pool:
            reads = {b: [pool.submit(read, p) for p in batches[b]] for b in range(min(2, len(batches)))}
            writes = []
            for b, chunk in enumerate(batches):
                got = [f.result() for f in reads.pop(b)]
                if b + 2 < len(batches):
                    reads[b + 2] = [pool.submit(read, p) for p in batches[b + 2]]
                groups = {}
                for i, g in enumerate(got):
                    groups.setdefault(tuple(g[1]), []).append(i)
                res = [None] * len(chunk)
                for shape, idx in groups.items():
                    for i, r in zip(idx, run_group([got[i] for i in idx], shape)):
                        res[i] = r
                self._set_shape(got[-1][1])
                writes += [pool.submit(write, p, g[1], r) for p, g, r in zip(chunk, got, res)]
            return [f.result() for f in writes]

    def _encode_fns_staged(self, pairs, batch, io_threads):
        """A codec's faster way through a whole list of frames, or None (dct2d's pinned slots)."""
        return None

    def encode_fns(self, pairs, batch: int = 64, io_threads: int = 16):
        """encode_fn over (in_fn, out_fn) pairs; returns the bytes written per frame.  Host threads
        read the images and write the files around one _encode_group call per group of equal
        shapes; a payload that is already a file (bytes: -c TIFF deflated on the GPU from the
        indices in HBM, vcf_amd/zlib_gpu.py) is written as it is, an index array goes through
        compress."""
        pairs = list(pairs)
        if not pairs:
            return []
        if self.lm is not None:   # one histogram and design per frame: frame by frame
            return [self.encode_fn(i, o) for i, o in pairs]
        staged = self._encode_fns_staged(pairs, batch, io_threads)
        if staged is not None:
            return staged

        def read(p):
            img = self.encode_read_fn(p[0])
            self._check_frame(img)
            return img, img.shape, None

        def write(p, shape, res):
            payload, extra = res
            self._write_side(p[1], shape, extra)
            cs = io.BytesIO(payload) if isinstance(payload, bytes) else self.compress(payload)
            return self.encode_write_fn(cs, p[1])

        return self._batches(pairs, batch, io_threads, read,
                             lambda got, shape: self._encode_group(np.stack([g[0] for g in got]), shape), write)

    def decode_fns(self, pairs, batch: int = 64, io_threads: int = 16):
        """decode_fn over (in_fn, out_fn) pairs, pipelined like encode_fns: host threads read (and,
        unless _decode_item leaves it to the GPU, inflate) the code-streams and write the images
        around one _decode_group call per group of equal shapes."""
        pairs = list(pairs)
        if not pairs:
            return []
        if self.lm is not None:
            return [self.decode_fn(i, o) for i, o in pairs]

        def read(p):
            cs = self.decode_read_fn(p[0])
            shape, extra = self._read_side(p[0])
            return self._decode_item(cs, shape), shape, extra

        return self._batches(pairs, batch, io_threads, read,
                             lambda got, shape: self._decode_group([g[0] for g in got], shape, [g[2] for g in got]),
                             lambda p, shape, y: self.decode_write_fn(y, p[1]))

    def _decode_item(self, codestream, shape):
        """What a read hands to _decode_group for one frame: the index array."""
        return self.decompress(codestream)

    def _indices_out(self, dk, n, padded):
        """The payloads of n index frames of shape `padded` in HBM, all work on the null stream
        done: with -c TIFF the files, their strips deflated on the GPU, else the arrays."""
        from .. import zlib_gpu
        from ..device import synchronize
        if isinstance(self.entropy, TIFFCodec) and TIFFCodec.gpu_batches and zlib_gpu.covers(padded, 1):
            synchronize()   # the deflater runs on a stream of its own: the encode kernel must be done
            return zlib_gpu.tiff_frames_device(dk, n, padded, np.uint8)
        return list(dk.download(np.empty((n,) + tuple(padded), np.uint8)))

    # ---- quantizer surface (deadzone.py:95-124) -----------------------------
    def quantize_decom(self, decom):
        return self.quantize(decom)

    def dequantize_decom(self, decom_k):
        return self.dequantize(decom_k)

    def quantize(self, img, fn="/tmp/encoded"):
        if self.lm is not None:
            return self.lm.quantize(img, fn)
        from .. import quant
        return quant.deadzone_quantize(img, self.QSS)

    def dequantize(self, k, fn="/tmp/encoded"):
        if self.lm is not None:
            return self.lm.dequantize(k, fn)
        from .. import quant
        return quant.deadzone_dequantize(k, self.QSS)

"""2D-DWT image codec: the drop-in for src/2D-DWT.py's CoDec.

Same constructor (argparse Namespace with levels, wavelet, color_transform,
quantizer, QSS, ...), same methods and files: encode_fn writes
{out}_LL_{L}{ext} (uint16, LL + 128) and {out}_{LH,HL,HH}_{r}{ext} (uint8,
+ 128) for r = L..1 and returns the bytes written (2D-DWT.py:57-78,
162-200); decode_fn reads them back and writes the decoded image
(:80-101, 202-228).  The span between the image and the subband arrays runs
on the GPU through libvcf_amd.so (vcf_dwt_dz_encode / vcf_dwt_dz_decode).

-c picks the entropy codec of every subband file from the registry the block
codecs use (codec/entropy.py; 2D-DWT.py hands each subband to the -c chain's
compress, :162-228); {ext} is the codec's.  TIFF (the default) and z_lib carry
the uint16 LL as it is.  The byte-symbol coders (CBAAC, CBAHC, TCBAAC, TCBAACP,
TCBAAC2D: a 256-symbol model) code the detail subbands as they are and LL as
its little-endian byte view, shape (h, w, 6); the decoder, which knows the LL
file by its name, views it back as uint16 (h, w, 3).  (The reference pushes LL
values past 255 into CBAAC's 256-symbol model and decodes with astype(uint8),
CBAAC.py:83,112: its LL file is broken whenever LL + 128 > 255, so there is
nothing to be compatible with.)  CBAHC's side file is named after each subband
file.

encode_fns / decode_fns (the III runner) keep a batch's pyramids in HBM: the
transform leaves every frame's subbands contiguous in its packed buffer (dwt.py
unpack), and with -c TCBAAC2D one launch per stage codes every tile of every
subband of every frame from there (tcbaac.PlaneBatch2D), with -c TIFF the
subbands' strips are deflated and inflated there (zlib_gpu), so only
code-streams cross PCIe.  The other codecs code on the host, per subband, on
the I/O threads behind the GPU work.  The files are the single-frame path's,
byte for byte, whichever path wrote them.
"""
from __future__ import annotations

import io
import logging
import os
import struct

import numpy as np

from .. import dwt as DW
from ..device import DeviceBuffer, Stream, copy_pieces
from .blockcodec import BlockCoDec
from .eic import CoDec as EICCoDec
from .entropy import make_entropy
from .tiff import TIFFCodec

# the -c names whose model has 256 symbols: they take LL as its byte view
BYTE_SYMBOL_CODECS = ("CBAAC", "CBAHC", "TCBAAC", "TCBAACP", "TCBAAC2D")


def ll_bytes(ll: np.ndarray) -> np.ndarray:
    """uint16 (h, w, 3) -> its little-endian byte view, uint8 (h, w, 6)."""
    ll = np.ascontiguousarray(ll, "<u2")
    return ll.view(np.uint8).reshape(ll.shape[0], ll.shape[1], 2 * ll.shape[2])


def ll_from_bytes(a: np.ndarray) -> np.ndarray:
    """The inverse of ll_bytes; ValueError for anything that is not a (h, w, 6) uint8 array."""
    a = np.asarray(a)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 6:
        raise ValueError(f"LL subband: a {a.dtype} array of shape {a.shape} is not the byte view (h, w, 6) of a "
                         "uint16 LL")
    return np.ascontiguousarray(a).view("<u2").reshape(a.shape[0], a.shape[1], 3).astype(np.uint16, copy=False)


class CoDec(EICCoDec):
    """2D-DWT.CoDec (2D-DWT.py:39-200) over YCoCg / deadzone / no_filter and the -c registry."""

    def __init__(self, args):
        super().__init__(args)
        self.levels = int(getattr(args, "levels", 5))
        self.wavelet = str(getattr(args, "wavelet", "db5"))
        DW.wavelet_index(self.wavelet)            # ValueError for names pywt does not know
        ct = getattr(args, "color_transform", "YCoCg")
        # -t YCrCb only changes the base class: 2D-DWT.py binds from_RGB/to_RGB from
        # color_transforms.YCoCg at import (:19-20), so the arithmetic stays YCoCg's
        # (tests/golden/manifest_plugins.json "same_as_ycocg")
        if ct not in ("YCoCg", "YCrCb"):
            raise NotImplementedError(f"color transform {ct!r}: YCoCg (and YCrCb, which 2D-DWT.py runs as "
                                      "YCoCg) are on the HIP path")
        quant = getattr(args, "quantizer", "deadzone")
        if quant != "deadzone":
            raise NotImplementedError(f"quantizer {quant!r}: only deadzone is on the HIP path")
        filt = getattr(args, "filter", "no_filter")
        if not self.encoding and filt == "deblock":
            raise NotImplementedError("filter 'deblock' with 2D-DWT: a wavelet transform of the whole frame has no "
                                      "block edges (2D-DCT, 2D-KLT and 2D-LBT have them)")
        if not self.encoding and filt != "no_filter":
            raise NotImplementedError(f"filter {filt!r}: only no_filter is on the HIP path")
        self.entropy = make_entropy(args)
        self.file_extension = self.entropy.file_extension
        self.byte_symbols = getattr(args, "entropy_image_codec", "TIFF") in BYTE_SYMBOL_CODECS
        self.QSS = int(getattr(args, "QSS", 32))
        # opt-in (no reference counterpart): the lifting form of bior4.4, within
        # +-1 of the bit-exact path (the lifting form); args.dwt_lifting or VCF_DWT_LIFTING=1
        self.lifting = bool(getattr(args, "dwt_lifting", False)) or os.environ.get("VCF_DWT_LIFTING") == "1"
        if self.lifting:
            logging.warning("2D-DWT: the opt-in lifting path is selected (%s): indices and decoded bytes are "
                            "within +-1 of the reference, not bit-exact",
                            "args.dwt_lifting" if getattr(args, "dwt_lifting", False) else "VCF_DWT_LIFTING=1")
        if self.lifting and self.wavelet != "bior4.4":
            raise NotImplementedError("the lifting path is bior4.4 (CDF 9/7) only")
        self._dev = self._planes = None           # the batch paths' device state (_device, _tiles2d)
        logging.info(f"levels = {self.levels}")
        logging.info(f"wavelet={self.wavelet}")

    def compress(self, img, fn=None):
        return self.entropy.compress(img, fn) if self.byte_symbols and fn is not None else self.entropy.compress(img)

    def decompress(self, codestream, fn=None):
        if self.byte_symbols and fn is not None:
            return self.entropy.decompress(codestream, fn)
        return self.entropy.decompress(codestream)

    # ---- subband files (2D-DWT.py:162-228) ----------------------------------
    def _is_ll(self, name):
        return name == f"LL_{self.levels}"

    def _compress_subband(self, arr, name, fn):
        """One subband array (already + 128) -> its code-stream; the byte-symbol coders take LL's byte view."""
        if self.byte_symbols and self._is_ll(name):
            arr = ll_bytes(arr)
        return self.compress(arr, f"{fn}_{name}")

    def _decompress_subband(self, data, name, fn):
        arr = self.decompress(data, f"{fn}_{name}")
        return ll_from_bytes(arr) if self.byte_symbols and self._is_ll(name) else arr

    def write_decom_fn(self, subbands, fn):
        """subbands: {name: u16 LL / u8 detail array}, already + 128."""
        size = 0
        for name in DW.subband_names(self.levels):
            size += self.encode_write_fn(self._compress_subband(subbands[name], name, fn), f"{fn}_{name}")
        return size

    def read_decom_fn(self, fn):
        return {name: self._decompress_subband(self.decode_read_fn(f"{fn}_{name}"), name, fn)
                for name in DW.subband_names(self.levels)}

    # ---- the hot path ---------------------------------------------------------
    @staticmethod
    def _check_frame(img):
        if img.ndim != 3 or img.shape[2] != 3 or img.dtype != np.uint8:
            raise ValueError("Input image must be a 3D array (height, width, channels).")

    def encode_fn(self, in_fn, out_fn):
        img = self.encode_read_fn(in_fn)
        self._check_frame(img)
        subbands = DW.encode(img, self.wavelet, self.levels, self.QSS, lifting=self.lifting)[0]
        return self.write_decom_fn(subbands, out_fn)

    def encode(self):
        # 2D-DWT.py:103-106: uses -o / -e
        return self.encode_fn(in_fn=self.args.original, out_fn=self.args.encoded)

    def _geometry_of(self, described):
        """described: {name: (shape, dtype)} of the decoded subbands (LL as uint16 (h, w, 3): its
        byte view has been undone) -> H, W whose 'per' pyramid has these subbands (the level-1
        shapes fix every coarser one: ceil halving).  ValueError for a shape or dtype that does
        not fit, before anything is handed to the GPU."""
        for name, (shape, dtype) in described.items():
            want = np.uint16 if self._is_ll(name) else np.uint8
            if len(shape) != 3 or shape[2] != 3 or np.dtype(dtype) != want:
                raise ValueError(f"subband {name}: a {np.dtype(dtype)} array of shape {tuple(shape)}, expected "
                                 f"{np.dtype(want)} (h, w, 3)")
        h1, w1 = described["HH_1"][0][:2]
        if h1 < 1 or w1 < 1:
            raise ValueError("empty subband HH_1")
        shapes, _, _ = DW.layout(2 * h1, 2 * w1, self.levels)
        for r, (h, w) in enumerate(shapes, start=1):
            for s in ("LH", "HL", "HH"):
                if tuple(described[f"{s}_{r}"][0][:2]) != (h, w):
                    raise ValueError(f"subband {s}_{r} has shape {tuple(described[f'{s}_{r}'][0])}, expected {(h, w)}")
        if tuple(described[f"LL_{self.levels}"][0][:2]) != shapes[-1]:
            raise ValueError("LL subband shape does not match the detail subbands")
        return 2 * h1, 2 * w1

    def _geometry(self, subbands):
        return self._geometry_of({name: (a.shape, a.dtype) for name, a in subbands.items()})

    def decode_fn(self, in_fn, out_fn):
        subbands = self.read_decom_fn(in_fn)
        H, W = self._geometry(subbands)
        y = DW.decode(subbands, H, W, self.wavelet, self.levels, self.QSS, lifting=self.lifting)
        size = self.decode_write_fn(y, out_fn)
        self.BPP = (self.total_input_size * 8) / (y.shape[0] * y.shape[1])
        return size

    def decode(self):
        return self.decode_fn(in_fn=self.args.encoded, out_fn=self.args.decoded)

    # ---- batched frames (III runner): the pyramids stay in HBM ---------------------
    def _device(self):
        """The batch paths' stream and scratch (grown on demand, reused), the plane-list coder."""
        if self._dev is None:
            from ..tcbaac import _Scratch
            self._dev = (Stream(), _Scratch())
        return self._dev

    def _tiles2d(self):
        """-c TCBAAC2D: the plane-list coder over the batch's stream, else None."""
        from ..tcbaac import PlaneBatch2D, TiledCBAACCodec
        if not (isinstance(self.entropy, TiledCBAACCodec) and self.entropy.ctx2d):
            return None
        if self._planes is None:
            self._planes = PlaneBatch2D(self.entropy.tile, self.entropy.nclass, self._device()[0])
        return self._planes

    def _gpu_tiff(self):
        return isinstance(self.entropy, TIFFCodec) and TIFFCodec.gpu_batches

    def _set_shape(self, shape):
        """BlockCoDec._batches tells the codec the last shape of a batch; the DWT keeps none."""

    def _encode_group(self, imgs, shape):
        """n frames of one shape -> per frame [(subband name, payload)] in file order: bytes (the
        file, coded on the GPU from the packed pyramid) or the subband array (the write codes it)."""
        from .. import zlib_gpu
        n, (H, W) = len(imgs), shape[:2]
        planes = DW.subband_planes(H, W, self.levels)
        _, pb, wb = DW.layout(H, W, self.levels)
        st, scratch = self._device()
        din, packed, ws = scratch.get("rgb", n * H * W * 3), scratch.get("packed", n * pb), scratch.get("ws", n * wb)
        din.upload(np.stack(imgs), st)
        DW.encode_device(din, n, H, W, DW.wavelet_index(self.wavelet), self.levels, self.QSS, packed, ws, st,
                         self.lifting)
        coder = self._tiles2d()
        if coder is not None:
            with coder.lock:
                coder.launch(packed, [(f * pb + off, h, w, c) for f in range(n) for _, off, h, w, c in planes])
                files = coder.streams([(h, w, c) for _ in range(n) for _, _, h, w, c in planes])
            k = len(planes)
            return [[(planes[s][0], files[f * k + s]) for s in range(k)] for f in range(n)]
        res = [[None] * len(planes) for _ in range(n)]
        gpu = [s for s, (_, _, h, w, c) in enumerate(planes)
               if self._gpu_tiff() and zlib_gpu.covers((h, w, 3), c // 3)]
        if gpu:
            # vcf_zlib_strips reads frames a uniform stride apart with no gap: gather the batch's
            # subbands, subband-major, into a staging buffer (one vcf_copy_pieces launch)
            table, dst = np.empty((n * len(gpu), 3), np.int64), 0
            starts = []
            for i, s in enumerate(gpu):
                _, off, h, w, c = planes[s]
                starts.append(dst)
                for f in range(n):
                    table[i * n + f] = (f * pb + off, dst, h * w * c)
                    dst += h * w * c
            stage, tb = scratch.get("stage", dst), scratch.get("table", table.nbytes)
            tb.upload(table, st)
            copy_pieces(packed, tb, len(table), stage, st)
            st.synchronize()                     # the table is a temporary; the deflater has its own state
            for s, start in zip(gpu, starts):
                name, _, h, w, c = planes[s]
                files = zlib_gpu.tiff_frames_device(stage, n, (h, w, 3), np.uint16 if c == 6 else np.uint8, start, st)
                for f in range(n):
                    res[f][s] = (name, files[f])
        if len(gpu) < len(planes):               # the host codes these: the subbands come down
            host = np.empty((n, pb), np.uint8)
            packed.download(host, st)
            st.synchronize()
            for f in range(n):
                sb = DW.unpack(host[f], H, W, self.levels)
                for s, (name, *_) in enumerate(planes):
                    if res[f][s] is None:
                        res[f][s] = (name, sb[name])
        return res

    def encode_fns(self, pairs, batch: int = 16, io_threads: int = 8):
        """encode_fn over (in_fn, out_fn) pairs -> the bytes written per frame.  BlockCoDec's
        pipeline: host threads read the images, one _encode_group per group of equal shapes, the
        writes (and the host coders' per-subband compress calls) run behind on the same pool."""
        pairs = list(pairs)
        if not pairs:
            return []

        def read(p):
            img = self.encode_read_fn(p[0])
            self._check_frame(img)
            return img, img.shape, None

        def write(p, shape, res):
            size = 0
            for name, payload in res:
                cs = io.BytesIO(payload) if isinstance(payload, bytes) else self._compress_subband(payload, name, p[1])
                size += self.encode_write_fn(cs, f"{p[1]}_{name}")
            return size

        return BlockCoDec._batches(self, pairs, batch, io_threads, read,
                                   lambda got, shape: self._encode_group([g[0] for g in got], shape), write)

    def _read_item(self, fn):
        """One frame's subband files for _decode_group -> ({name: entry}, (H, W)): entry = ("t2d",
        the parsed version-4 container) or ("tiff", file bytes, strip table) where the GPU decodes
        it, else ("arr", the subband decoded here, on the host).  The geometry is checked on what
        the headers say, before any launch."""
        from .. import zlib_gpu
        from ..tcbaac import _parse2d
        from .tiff import tiff_strips
        coder = self._tiles2d()
        item, described = {}, {}
        for name in DW.subband_names(self.levels):
            data = self.decode_read_fn(f"{fn}_{name}")
            entry = None
            if coder is not None:
                try:
                    f = _parse2d(bytes(data))
                except (ValueError, struct.error):
                    f = None                          # not a whole version-4 stream: the reader below reports it
                if f is not None and (f[1], f[2], f[3]) == (coder.th, coder.tw, coder.nclass):
                    entry = ("t2d", f)
                    if self._is_ll(name):             # the byte view: ll_from_bytes' rule, on the header
                        if len(f[0]) != 3 or f[0][2] != 6:
                            raise ValueError(f"LL subband: a stream of shape {f[0]} is not the byte view (h, w, 6) "
                                             "of a uint16 LL")
                        described[name] = (f[0][:2] + (3,), np.uint16)
                    else:
                        described[name] = (f[0], np.uint8)
            elif self._gpu_tiff():
                info = tiff_strips(data)
                if info is not None and len(info[0]) == 3 and zlib_gpu.covers(info[0], info[1].itemsize):
                    entry = ("tiff", data, info)
                    described[name] = (tuple(info[0]), info[1])
            if entry is None:
                arr = self._decompress_subband(data, name, fn)
                entry = ("arr", arr)
                described[name] = (arr.shape, arr.dtype)
            item[name] = entry
        return item, self._geometry_of(described)

    def _decode_group(self, items, shape):
        """n frames' subband files of one geometry -> their decoded frames: every subband lands at
        its offset of the packed buffer (tiles decoded / strips inflated on the GPU there, host
        arrays uploaded), then one vcf_dwt_dz_decode for the group and one download."""
        from .. import zlib_gpu
        H, W = shape
        n = len(items)
        planes = DW.subband_planes(H, W, self.levels)
        shapes, pb, wb = DW.layout(H, W, self.levels)
        Ho, Wo = 2 * shapes[0][0], 2 * shapes[0][1]
        st, scratch = self._device()
        packed, ws, out = scratch.get("packed", n * pb), scratch.get("ws", n * wb), scratch.get("out", n * Ho * Wo * 3)
        host = None
        t2d, arrays, comp, comp_off, comp_len, out_off, out_len, base = [], [], [], [], [], [], [], 0
        for f, item in enumerate(items):
            for name, off, h, w, c in planes:
                e = item[name]
                if e[0] == "arr":
                    if host is None:
                        host = np.zeros((n, pb), np.uint8)
                    a = np.ascontiguousarray(e[1], "<u2" if c == 6 else np.uint8)
                    host[f, off:off + h * w * c] = a.view(np.uint8).ravel()
                elif e[0] == "t2d":
                    t2d.append(e[1])
                    arrays.append((f * pb + off, h, w, c))
                else:
                    _, data, (_, _, offs, counts, sb) = e
                    total = h * w * c
                    if len(offs) != -(-total // sb):
                        raise ValueError(f"subband {name}: a strip table that does not cover the subband")
                    comp.append(data)
                    comp_off += [base + o for o in offs]
                    comp_len += list(counts)
                    out_off += [f * pb + off + k * sb for k in range(len(offs))]
                    out_len += [min(sb, total - k * sb) for k in range(len(offs))]
                    base += len(data)
        if host is not None:
            packed.upload(host, st)
        if t2d:
            coder = self._tiles2d()
            with coder.lock:
                coder.decode(t2d, packed, arrays)
        if comp:
            zlib_gpu.inflater().inflate_into(np.frombuffer(b"".join(comp), np.uint8), comp_off, comp_len, packed,
                                             out_off, out_len, st)
        DW.decode_device(packed, n, H, W, DW.wavelet_index(self.wavelet), self.levels, self.QSS, out, ws, st,
                         self.lifting)
        res = np.empty((n, Ho, Wo, 3), np.uint8)
        out.download(res, st)
        st.synchronize()
        return res

    def decode_fns(self, pairs, batch: int = 16, io_threads: int = 8):
        """decode_fn over (in_fn, out_fn) pairs, pipelined like encode_fns: host threads read the
        subband files (and decode those the GPU does not), groups of equal geometry take one
        _decode_group, the image writes run behind."""
        pairs = list(pairs)
        if not pairs:
            return []

        def read(p):
            item, hw = self._read_item(p[0])
            return item, hw, None

        def write(p, shape, y):
            size = self.decode_write_fn(y, p[1])
            self.BPP = (self.total_input_size * 8) / (y.shape[0] * y.shape[1])
            return size

        return BlockCoDec._batches(self, pairs, batch, io_threads, read,
                                   lambda got, shape: self._decode_group([g[0] for g in got], shape), write)

    # ---- quantizer surface on subband lists (2D-DWT.py:113-160) -------------------
    def quantize_decom_fn(self, decom, fn=None):
        from .. import quant
        return [quant.deadzone_quantize(decom[0], self.QSS)] + \
            [tuple(quant.deadzone_quantize(b, self.QSS) for b in r) for r in decom[1:]]

    def dequantize_decom_fn(self, decom_k, fn=None):
        from .. import quant
        return [quant.deadzone_dequantize(decom_k[0], self.QSS)] + \
            [tuple(quant.deadzone_dequantize(b, self.QSS) for b in r) for r in decom_k[1:]]

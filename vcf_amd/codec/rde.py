"""Rate/distortion evaluation: the drop-in for src/RDE.py, and what it grows into on the GPU.

evaluate() is RDE.py's main(): the size of the original, of every code-stream
file and of the decoded image, bits per pixel over shape[0] * shape[1], the
RMSE between original and decoded image and J = code-stream bpp + RMSE;
lines() prints them as RDE.py does -- the same `RDE: ...` lines in the same
order and format.  The code-stream files are found by RDE.py's rule: the text
of -c before its first '.', plus '*', globbed (so the default /tmp/encoded*
takes /tmp/encoded.tif and /tmp/encoded_shape.bin, and a path with a dot in a
directory name is cut there too, as in the reference).

The distortion is measured on the GPU (vcf_amd/distortion.py); there is no CPU
implementation of it here.

One deviation, stated: RDE.py converts both images to float32 and takes
`(a - b) ** 2`.mean() in float32; here the mean is the exact integer sum of
squares divided in float64.  numpy's pairwise float32 mean is within about
1e-7 relative of the exact one, so the printed `:.2f` values are equal unless
RMSE * 100 lies within about 1e-5 of a half-integer (tests/golden/rde_*.npz
are chosen off that boundary).

What RDE.py does that this does not: the URL branch (a missing file raises
FileNotFoundError here), and the crash after a dimension mismatch (the three
error lines are printed as there; the program then exits with status 1 instead
of a TypeError traceback).  8-bit grey, RGB and RGBA images are measured, as
the arrays PIL gives for them; 16-bit images raise NotImplementedError.

evaluate_sequence() does the same for the numbered files of III and IPP runs,
a batch of frames per kernel launch; rd_curve() traces the rate-distortion
curve of the default chain (2D-DCT, YCoCg, deadzone, -c TIFF) with the frames
resident in HBM: per Q only the compressed sizes and the distortion records
come back to the host.
"""
from __future__ import annotations

import glob
import os
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass, field

import numpy as np

from .. import distortion as DS
from ..device import DeviceBuffer, Stream


class ShapeMismatch(ValueError):
    """RDE.py:34-38: the two images have different shapes."""

    def __init__(self, shape1, shape2):
        super().__init__(f"Image dimensions do not match: {shape1} and {shape2}")
        self.shape1, self.shape2 = tuple(shape1), tuple(shape2)

    def lines(self) -> list:
        return ["Error: Image dimensions do not match.", f"Image 1 shape: {self.shape1}",
                f"Image 2 shape: {self.shape2}"]


def read_image(fn: str) -> np.ndarray:
    """np.array(PIL.Image.open(fn)) as RDE.py:20-31 has it, as uint8: H x W (grey), H x W x 3 or H x W x 4.
    8-bit truecolour PNGs go through the library's reader (vcf_png.cpp), everything else through PIL."""
    if not os.path.exists(fn):
        raise FileNotFoundError(f"RDE: no such image file: {fn!r} (URLs are not fetched)")
    with open(fn, "rb") as f:
        head = f.read(29)
    # PNG signature, IHDR: bit depth 8, colour type 2 (RGB), no interlace
    if head[:8] == b"\x89PNG\r\n\x1a\n" and head[12:16] == b"IHDR" and head[24] == 8 and head[25] == 2 and head[28] == 0:
        from .eic import _read_png_native
        img, _ = _read_png_native(fn)
        if img is not None:
            return img
    from PIL import Image
    with Image.open(fn) as im:
        img = np.array(im)
    if img.dtype != np.uint8:
        raise NotImplementedError(f"{fn!r} is {img.dtype} (PIL mode {im.mode!r}): 8-bit images are measured")
    if img.ndim not in (2, 3) or (img.ndim == 3 and not 1 <= img.shape[2] <= 4):
        raise NotImplementedError(f"{fn!r} has shape {img.shape}: grey, RGB and RGBA images are measured")
    return np.ascontiguousarray(img)


def file_size(fn: str) -> int:
    """RDE.py:57-66 without its URL branch."""
    if not os.path.exists(fn):
        raise FileNotFoundError(f"RDE: no such file: {fn!r} (URLs are not fetched)")
    return os.path.getsize(fn)


def codestream_prefix(codestream: str) -> str:
    """RDE.py:91: the text before the first '.', plus '*'."""
    return codestream.split(".")[0] + "*"


def codestream_files(codestream: str) -> list:
    """RDE.py:91-93, in glob's order."""
    return glob.glob(codestream_prefix(codestream))


@dataclass
class Result:
    """What RDE.py prints for one image."""
    original: str
    decoded: str
    codestream_files: list
    codestream_lengths: list
    original_bytes: int
    decoded_bytes: int
    shape: tuple
    rmse: float
    psnr: float = float("nan")
    ssim: float | None = field(default=None, repr=False, compare=False)   # evaluate(ssim=True): mean over channels

    @property
    def number_of_pixels(self) -> int:
        return self.shape[0] * self.shape[1]

    @property
    def codestream_bytes(self) -> int:
        return sum(self.codestream_lengths)

    @property
    def original_bpp(self) -> float:
        return self.original_bytes * 8 / self.number_of_pixels

    @property
    def codestream_bpp(self) -> float:
        return self.codestream_bytes * 8 / self.number_of_pixels

    @property
    def decoded_bpp(self) -> float:
        return self.decoded_bytes * 8 / self.number_of_pixels

    @property
    def J(self) -> float:
        return self.codestream_bpp + self.rmse

    def lines(self) -> list:
        """RDE.py:96-118, line for line."""
        out = [f"RDE: Code-stream file: {f} length: {n}" for f, n in zip(self.codestream_files, self.codestream_lengths)]
        out.append(f"RDE: Original image: {self.original} {self.original_bytes} bytes ({self.original_bpp:.2f}) bits/pixel")
        out.append(f"RDE: Code-stream: {self.codestream_files} {self.codestream_bytes} "
                   f"bytes ({self.codestream_bpp:.2f}) bits/pixel")
        out.append(f"RDE: Decoded image: {self.decoded} {self.decoded_bytes} bytes ({self.decoded_bpp:.2f}) bits/pixel")
        out.append(f"RDE: Images shape: {self.shape}")
        out.append(f"RDE: Distortion (RMSE): {self.rmse:.2f}")
        out.append(f"RDE: J = R + D = {self.J:.2f}")
        if self.ssim is not None:       # not in RDE.py: one further line, after its own
            out.append(f"RDE: SSIM: {self.ssim:.4f}")
        return out


def _sizes(original: str, codestream: str, decoded: str):
    files = codestream_files(codestream)
    return file_size(original), files, [file_size(f) for f in files], file_size(decoded)


def evaluate(original: str = "/tmp/original.png", codestream: str = "/tmp/encoded*",
             decoded: str = "/tmp/decoded.png", ssim: bool = False) -> Result:
    """RDE.py's main() for one image; raises ShapeMismatch where RDE.py prints its error.  With `ssim` the result
    carries the frame's SSIM (distortion.ssim: grey or RGB images of at least 11 x 11, ValueError otherwise)."""
    a, b = read_image(original), read_image(decoded)
    if a.shape != b.shape:
        raise ShapeMismatch(a.shape, b.shape)
    if ssim:
        DS._check_ssim_shape(1, *_hwc(a))
    m = DS.measure(a, b)
    ob, files, lengths, db = _sizes(original, codestream, decoded)
    res = Result(original, decoded, files, lengths, ob, db, tuple(a.shape), float(m.rmse()[0]), float(m.psnr()[0]))
    if ssim:
        res.ssim = float(DS.ssim(a, b).per_frame()[0])
    return res


@dataclass
class SequenceResult:
    """evaluate_sequence: per-frame arrays and their means."""
    frames: list                      # Result per frame
    bytes: np.ndarray                 # code-stream bytes per frame
    bpp: np.ndarray
    rmse: np.ndarray
    psnr: np.ndarray
    launches: int = 0                 # kernel launches used (one per batch of equal shapes)
    means: dict = field(default_factory=dict)
    ssim: np.ndarray | None = field(default=None, repr=False, compare=False)   # evaluate_sequence(ssim=True)

    def lines(self) -> list:
        out = []
        for i, r in enumerate(self.frames):
            out.append(f"RDE: Frame {i}: {r.codestream_bytes} bytes ({r.codestream_bpp:.2f}) bits/pixel, "
                       f"RMSE {r.rmse:.2f}, PSNR {r.psnr:.2f} dB, J = {r.J:.2f}"
                       + ("" if r.ssim is None else f", SSIM {r.ssim:.4f}"))
        m = self.means
        out.append(f"RDE: Mean of {len(self.frames)} frames: {m['bytes']:.1f} bytes ({m['bpp']:.2f}) bits/pixel, "
                   f"RMSE {m['rmse']:.2f}, PSNR {m['psnr']:.2f} dB, J = {m['J']:.2f}"
                   + (f", SSIM {m['ssim']:.4f}" if "ssim" in m else ""))
        return out


def evaluate_sequence(original_pattern: str, decoded_pattern: str, codestream_pattern: str, n: int, batch: int = 16,
                      io_threads: int = 8, ssim: bool = False) -> SequenceResult:
    """RDE for frames 0 .. n-1 of an III or IPP run.  The three patterns are printf patterns of the frame number
    (/tmp/original_%04d.png, /tmp/decoded_%04d.png, /tmp/encoded_%04d); a frame's code-stream files follow
    RDE.py's prefix rule applied to its formatted pattern.  `io_threads` threads read the images; consecutive
    frames of one shape, `batch` at most, are uploaded together and measured by one kernel launch.  With `ssim`
    every frame's SSIM is measured too (one further launch a batch) and reported per frame and as a mean."""
    n, batch = int(n), max(1, int(batch))
    if n < 1:
        raise ValueError(f"number of frames must be at least 1 (got {n})")
    names = [(original_pattern % i, decoded_pattern % i, codestream_pattern % i) for i in range(n)]

    def read(i):
        o, d, _ = names[i]
        a, b = read_image(o), read_image(d)
        if a.shape != b.shape:
            raise ShapeMismatch(a.shape, b.shape)
        return a, b

    results, launches = [None] * n, 0
    with ThreadPoolExecutor(max_workers=max(1, int(io_threads))) as pool:
        pairs = list(pool.map(read, range(n)))
        sizes = list(pool.map(lambda i: _sizes(names[i][0], names[i][2], names[i][1]), range(n)))
    i = 0
    while i < n:
        j = i + 1
        while j < n and j - i < batch and pairs[j][0].shape == pairs[i][0].shape:
            j += 1
        sa = np.stack([pairs[t][0].reshape(_hwc(pairs[t][0])) for t in range(i, j)])
        sb = np.stack([pairs[t][1].reshape(_hwc(pairs[t][1])) for t in range(i, j)])
        m = DS.measure(sa, sb)
        launches += 1
        rm, ps = m.rmse(), m.psnr()
        ss = DS.ssim(sa, sb).per_frame() if ssim else None
        for t in range(i, j):
            ob, files, lengths, db = sizes[t]
            results[t] = Result(names[t][0], names[t][1], files, lengths, ob, db, tuple(pairs[t][0].shape),
                                float(rm[t - i]), float(ps[t - i]))
            if ssim:
                results[t].ssim = float(ss[t - i])
        i = j
    by = np.array([r.codestream_bytes for r in results], np.int64)
    bpp = np.array([r.codestream_bpp for r in results])
    rmse = np.array([r.rmse for r in results])
    psnr = np.array([r.psnr for r in results])
    means = dict(bytes=float(by.mean()), bpp=float(bpp.mean()), rmse=float(rmse.mean()), psnr=float(psnr.mean()),
                 J=float((bpp + rmse).mean()))
    if not ssim:
        return SequenceResult(results, by, bpp, rmse, psnr, launches, means)
    per_frame = np.array([r.ssim for r in results])
    means["ssim"] = float(per_frame.mean())
    return SequenceResult(results, by, bpp, rmse, psnr, launches, means, per_frame)


def _hwc(a: np.ndarray):
    return a.shape if a.ndim == 3 else a.shape + (1,)


def rd_curve(frames, Qs, block_size: int = 8, flags: int = 0, ssim: bool = False, rdoq=None,
             filter: str = "no_filter", deblock_beta=None, deblock_tc=None) -> list:
    """The rate-distortion curve of the default chain (2D-DCT.py: YCoCg, B x B DCT, deadzone, -c TIFF) over the
    quantization steps Qs, with the n equal-shape H x W x 3 u8 frames uploaded once.  Per Q, on the device:
    dct.encode_device, the deflate of the TIFF strips for their sizes (zlib_gpu.tiff_sizes_device), dct.decode_device
    and vcf_distortion_u8 against the resident originals; the strip sizes and the distortion records are all that
    comes back.  -> per Q a dict of Q and the per-frame arrays bytes (len(tif) + 12 for _shape.bin: what RDE.py
    sums for /tmp/encoded*), bpp, rmse, psnr and J = bpp + rmse -- the numbers encode_fn, decode_fn and RDE give
    through files.  With `ssim` every dict also has ssim, the per-frame SSIM (distortion.Ssim.per_frame) of the
    resident originals against the resident reconstructions, measured by vcf_ssim_u8 right after the distortion;
    only its records come back too.  Frames under 11 x 11 then raise ValueError.  Raises NotImplementedError where
    the GPU deflate does not cover the frame (rows over 64 KB): the host TIFF writer's sizes would be the same, but a
    silent change of path is not this function's to make.  rdoq = MU codes the indices with the two-pass RDOQ
    pipeline (vcf_amd/rdoq.py, lambda = MU * Q * Q; B = 8 without -p only) instead of the plain encode: the same
    curve, to be read against the plain one at equal Q or at equal bytes.  filter = "deblock" filters the
    reconstructions on the device (vcf_amd/deblock.py: the strengths given, or deblock.default_strength(Q)) before
    the distortion and SSIM kernels; the bytes are those of the unfiltered curve."""
    from .. import dct as D
    from .. import deblock as DB
    from .. import rdoq as R
    from .. import zlib_gpu
    if rdoq is not None and (block_size != 8 or flags & D.VCF_DCT_PERCEPTUAL):
        raise NotImplementedError("--rdoq: the RDOQ encode has the 8x8 kernel without -p only")
    if filter not in ("no_filter", "deblock"):
        raise NotImplementedError(f"filter {filter!r}: only no_filter and deblock are on the HIP path")
    if filter == "deblock" and block_size < DB.MIN_BLOCK_SIZE:
        raise NotImplementedError(f"filter 'deblock' with -B {block_size}: blocks of at least {DB.MIN_BLOCK_SIZE}")
    f = np.asarray(frames)
    if f.dtype != np.uint8:
        raise TypeError(f"frames must be uint8, got {f.dtype}")
    if f.ndim == 3:
        f = f[None]
    if f.ndim != 4 or f.shape[3] != 3:
        raise ValueError("frames must be H x W x 3 or N x H x W x 3")
    f = np.ascontiguousarray(f)
    n, H, W, _ = f.shape
    if n < 1 or H < 1 or W < 1:
        raise ValueError(f"no samples in frames of shape {f.shape}")
    if ssim:
        DS._check_ssim_shape(n, H, W, 3)
    Hp, Wp = D.padded_shape(H, W, block_size)
    if not zlib_gpu.covers((Hp, Wp, 3), 1):
        raise NotImplementedError(f"-c TIFF strips of {Hp} x {Wp} x 3 index frames are beyond the GPU deflate "
                                  f"({zlib_gpu.max_strip()} bytes a strip)")
    st = Stream()
    bufs = []
    try:
        src = DeviceBuffer.from_array(f, st)
        k, rec = DeviceBuffer(n * Hp * Wp * 3), DeviceBuffer(n * H * W * 3)
        out = DeviceBuffer(n * 3 * DS.RECORD.itemsize)
        bufs += [src, k, rec, out]
        if filter == "deblock":
            fil = DeviceBuffer(n * H * W * 3)
            bufs.append(fil)
            top, left = DB.crop_offsets(H, W, block_size)
        if ssim:
            sout = DeviceBuffer(n * 3 * DS.SSIM_RECORD.itemsize)
            bufs.append(sout)
        curve = []
        for Q in Qs:
            Q = int(Q)
            if rdoq is None:
                D.encode_device(src, n, H, W, Q, flags, out=k, stream=st, block_size=block_size)
            else:     # the pipeline works on the null stream and ends synchronised
                st.synchronize()
                R.encode_frames_device(src, n, H, W, Q, R.lambda_of(rdoq, Q), flags, out=k)
            tif = zlib_gpu.tiff_sizes_device(k, n, (Hp, Wp, 3), np.uint8, stream=st)
            D.decode_device(k, n, H, W, Q, flags, out=rec, stream=st, block_size=block_size)
            dec = rec
            if filter == "deblock":
                beta, tc = DB.strength(Q, deblock_beta, deblock_tc)
                dec = DB.deblock_device(rec, n, H, W, block_size, top, left, beta, tc, out=fil, stream=st)
            DS.sse_device(src, dec, n, H, W, 3, out, st)
            if ssim:
                DS.ssim_device(src, dec, n, H, W, 3, sout, st)
            m = DS.records(out, n, 3, H * W, st)
            by = tif + 12
            bpp = by * 8 / (H * W)
            rmse = m.rmse()
            curve.append(dict(Q=Q, bytes=by, bpp=bpp, rmse=rmse, psnr=m.psnr(), J=bpp + rmse))
            if ssim:
                curve[-1]["ssim"] = DS.ssim_records(sout, n, 3, st).per_frame()
        return curve
    finally:
        st.synchronize()
        for b in bufs:
            b.free()
        st.close()


# ---- the programs ------------------------------------------------------------------
def main(argv=None) -> int:
    """`python RDE.py [-o ...] [-c ...] [-d ...] [-N n] [--ssim]`; the exit status."""
    import sys

    from . import parser as P
    args = P.rde_parser().parse_args(argv)
    try:
        if args.number_of_frames is not None:
            res = evaluate_sequence(args.original, args.decoded, args.codestream, args.number_of_frames, ssim=args.ssim)
        else:
            res = evaluate(args.original, args.codestream, args.decoded, ssim=args.ssim)
    except ShapeMismatch as e:
        print("\n".join(e.lines()))
        return 1
    except DS.SsimShapeError as e:       # --ssim on frames it is not defined on: say so, measure nothing else
        print(f"RDE: {e}", file=sys.stderr)
        return 1
    print("\n".join(res.lines()))
    return 0


def _curve_frames(original: str, n):
    if n is None and original.lower().endswith(".npy"):
        return np.load(original)
    from .eic import read_image as read_rgb
    if n is None:
        return read_rgb(original)[0][None]
    with ThreadPoolExecutor(max_workers=8) as pool:
        return np.stack(list(pool.map(lambda i: read_rgb(original % i)[0], range(int(n)))))


def curve_main(argv=None) -> int:
    """`python RD-curve.py -o ... -q 8,16,32 [-N n] [-B b] [-p] [-x] [--ssim] [--rdoq MU] [-f deblock
    [--deblock_beta b] [--deblock_tc t]] [--json]`."""
    import json
    import sys

    from .. import dct as D
    from . import parser as P
    argv = sys.argv[1:] if argv is None else list(argv)
    args = P.rd_curve_parser(rdoq=True, filter=P.filter_of(argv)).parse_args(argv)
    Qs = [int(q) for q in str(args.QSS).split(",") if q.strip()]
    frames = _curve_frames(args.original, args.number_of_frames)
    try:
        curve = rd_curve(frames, Qs, int(args.block_size_DCT),
                         D.flags_from(args.disable_subbands, args.perceptual_quantization), ssim=args.ssim,
                         rdoq=args.rdoq, filter=getattr(args, "filter", "no_filter"),
                         deblock_beta=getattr(args, "deblock_beta", None), deblock_tc=getattr(args, "deblock_tc", None))
    except DS.SsimShapeError as e:
        print(f"RD: {e}", file=sys.stderr)
        return 1
    if args.json:
        print(json.dumps([{k: (v if k == "Q" else np.asarray(v).tolist()) for k, v in c.items()} for c in curve]))
        return 0
    for c in curve:
        print(f"RD: Q = {c['Q']}: {c['bytes'].mean():.1f} bytes ({c['bpp'].mean():.2f}) bits/pixel, "
              f"RMSE {c['rmse'].mean():.2f}, PSNR {c['psnr'].mean():.2f} dB, J = {c['J'].mean():.2f} "
              + (f"SSIM {c['ssim'].mean():.4f} " if "ssim" in c else "") + f"(means of {len(c['bytes'])} frames)")
    return 0

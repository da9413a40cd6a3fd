"""Tiled CBAAC: the CBAAC entropy stage (src/CBAAC.py) as a GPU-resident coder.

The reference codes a frame's indices as one serial arithmetic-coded stream
(CBAAC.py:114-131).  Here the flattened symbols split into consecutive
segments of `seg_len` symbols and every segment is coded exactly as the
reference codes a stream -- fresh AdaptiveModel/ContextManager, history of
`order` zeros, the A8 coder flushed at the segment's end -- one wave per
segment on the GPU (libvcf_amd.so: vcf_cbaac_tiled_*).  Segment i's bytes
equal vcf_cbaac_encode(symbols[i*seg_len:(i+1)*seg_len]).  The price is one
model warm-up per segment (the rate overhead, reported by
scripts/bench_tcbaac.py); the gain is that the frame's indices never leave
HBM -- only the compressed bytes come back.

Container (`.tadpt_arith`, a new format; the reference's `.adpt_arith` has
no segment index):
    uint32 ndims, uint32 shape[ndims]         (as CBAAC.py:84-89)
    b"VCFT", uint32 version = 1, uint32 order, uint32 seg_len,
    uint32 n_segments, uint32 segment_bytes[n_segments]
    the segments' bit streams, back to back (each MSB-first, zero padded)
Version 2 (`prior=True`, orders 0 and 1; not in the reference) adds, after
n_segments, 256 uint16 prior frequencies f[s] = 1 + floor(hist[s] * 8192 / n)
of the frame's symbols, before the segment sizes: every model of every
segment (order 1: all 256 contexts) starts from them instead of 256 ones and adapts by the reference's rules, so short
segments (many waves per frame) stop paying the model's learning cost.
Version 3 (`nclass` > 1 prior classes; not in the reference): segment s of
the frame's n_segments takes prior row floor(s * nclass / n_segments), row c
built like version 2's over the symbols of class c's segments; after
n_segments come uint32 nclass and per class a sparse row -- uint16 m, the m
symbols whose frequency is not 1 (uint8 each), their m frequencies (uint16) --
and the segment sizes as unsigned LEB128 varints (a 4096-symbol segment of DCT
indices is ~20 bytes: a uint32 index would cost +4.8 % of the stream).
With the DCT's subband layout and nclass = 8 a row is about one subband row,
whose statistics differ the most: 4096-symbol segments (1519 waves for a 1080p
frame) then cost about the serial stream's rate.
Version 4 (`-c TCBAAC2D`, `ctx2d=True`; not in the reference, whose TODO.md
asks for it: "Adapt CBAAC to images, shapping the context") codes a (H, W, C)
or (H, W) array plane by plane in th x tw tiles (64 x 64 by default, cropped
at the edges, numbered channel-major, then tile row, then tile column), a
tile's symbols in raster order through the same coder and AdaptiveModel,
flushed at the tile's end, one wave per tile.  The symbol at (y, x) of a tile
takes one of 16 models: ctx = 4 q(|left - 128|) + q(|up - 128|), q(v) =
min(v, 3), a neighbour outside the tile counting as 0 -- in the DCT's subband
layout the neighbours are the same coefficient of the adjacent blocks.  Tile
t of a plane's n_t takes prior class floor(t nclass / n_t); its 16 models
start from the class's 16 rows, row (class, ctx) = 1 + floor(hist[s] * 8192 /
n) over the class's symbols in that context (all ones where there are none).
    uint32 ndims, uint32 shape[ndims], b"VCFT", uint32 version = 4,
    uint32 th, uint32 tw, uint32 n_tiles, uint32 nclass, uint32 nctx = 16,
    the nclass * nctx prior rows (version 3's sparse rows),
    the tile sizes (LEB128 varints), the tiles' bit streams back to back
decompress() reads all four versions; a malformed header returns
zeros((10, 10)) like CBAAC.py:101-102.
"""
from __future__ import annotations

import io
import struct
import threading

import numpy as np

from . import _lib as L
from .device import DeviceBuffer, Stream

FILE_EXTENSION = ".tadpt_arith"
MAGIC = b"VCFT"
VERSION = 1
VERSION_PRIOR = 2
VERSION_CLASSES = 3
DEFAULT_SEG = 1 << 17     # 48 segments for a 1080p frame, 190 for 4K
PRIOR_SEG = 1 << 15       # version 2: 190 segments for 1080p at +2.3 % rate (profiles/r02_tcbaac_prior.jsonl)
CLASS_SEG = 1 << 12       # version 3 (-c TCBAACP): 1519 segments for 1080p
PRIOR_CLASSES = 8         # version 3's prior rows per frame (the 8 subband rows of the 8x8 DCT)
VERSION_2D = 4
TILE_2D = (64, 64)        # version 4's tile (th, tw): CLASS_SEG symbols
NCTX_2D = 16              # version 4's contexts per class


def n_segments(n: int, seg_len: int = DEFAULT_SEG) -> int:
    return int(L.lib().vcf_cbaac_tiled_segments(int(n), int(seg_len)))


class _Scratch:
    """Device buffers reused across calls (grown on demand)."""

    def __init__(self):
        self.bufs = {}

    def get(self, name: str, nbytes: int) -> DeviceBuffer:
        b = self.bufs.get(name)
        if b is None or b.nbytes < nbytes:
            b = DeviceBuffer(max(nbytes, 1))
            self.bufs[name] = b
        return b


class TiledCoder:
    """The GPU calls, with reusable scratch and a stream.

    One coder owns one set of scratch buffers and one stream, so its calls
    are serialised by `lock` (the DCT CoDec's encode_fns/decode_fns call the
    entropy codec from a thread pool): a call's upload, kernels and download
    never interleave with another thread's on the same buffers.
    `kernel`: 0 = the library's rule, 1 = a wave per segment, 2 = a lane per
    segment (order 0) -- the A/B library's twins, for tests and A/B scripts."""

    def __init__(self, order: int = 0, seg_len: int = DEFAULT_SEG, stream: Stream | None = None,
                 prior: bool = False, nclass: int = 1, kernel: int = 0):
        self.order, self.seg_len, self.prior = int(order), int(seg_len), bool(prior)
        self.nclass, self.kernel = int(nclass), int(kernel)
        if self.prior and self.order > 1:
            raise NotImplementedError("prior-seeded tiled CBAAC: orders 0 and 1")
        if self.nclass < 1 or (self.nclass > 1 and not self.prior):
            raise ValueError("prior classes need prior=True")
        self.stream = stream if stream is not None else Stream()
        self.scratch = _Scratch()
        self.last_prior = None     # the prior table of the last encode (prior=True)
        self.lock = threading.RLock()

    def encode_device(self, sym: DeviceBuffer, n: int, offset: int = 0):
        """Symbols already in HBM -> (segment byte counts, payload bytes);
        with prior=True the frame's prior table is left in self.last_prior
        (read it under self.lock when other threads share the coder)."""
        with self.lock:
            return self._encode_device(sym, n, offset)

    def _encode_device(self, sym: DeviceBuffer, n: int, offset: int = 0):
        lib = L.lib()
        ns = n_segments(n, self.seg_len)
        ws = self.scratch.get("ws", int(lib.vcf_cbaac_tiled_workspace(n, self.seg_len)))
        cap = int(lib.vcf_cbaac_tiled_bound(n, self.seg_len))
        out = self.scratch.get("out", cap)
        sb = self.scratch.get("sizes", 8 * (ns + 1))
        if self.prior and self.nclass > 1:
            K = self.nclass
            pr, hist = self.scratch.get("prior", 512 * K), self.scratch.get("hist", 1024 * K)
            L.call("vcf_cbaac_tiled_prior_classes", sym.address(offset), 1, int(n), int(n), self.seg_len, K, pr.ptr,
                   hist.ptr, self.stream.handle)
            L.call_v(self.kernel, "vcf_cbaac_tiled_encode_classes", sym.address(offset), 1, int(n), int(n), self.order,
                     pr.ptr, K, self.seg_len, out.ptr, cap, sb.ptr, ws.ptr, self.stream.handle)
            self.last_prior = np.empty((K, 256), np.uint16)
            pr.download(self.last_prior, self.stream)
        elif self.prior:
            pr, hist = self.scratch.get("prior", 512), self.scratch.get("hist", 1024)
            L.call("vcf_cbaac_tiled_prior", sym.address(offset), int(n), pr.ptr, hist.ptr, self.stream.handle)
            L.call_v(self.kernel, "vcf_cbaac_tiled_encode_prior", sym.address(offset), int(n), self.order, pr.ptr,
                     self.seg_len, out.ptr, cap, sb.ptr, ws.ptr, self.stream.handle)
            self.last_prior = np.empty(256, np.uint16)
            pr.download(self.last_prior, self.stream)
        else:
            L.call_v(self.kernel, "vcf_cbaac_tiled_encode", sym.address(offset), int(n), self.order, self.seg_len,
                     out.ptr, cap, sb.ptr, ws.ptr, self.stream.handle)
        sizes = np.empty(ns + 1, np.int64)
        sb.download(sizes, self.stream)
        self.stream.synchronize()
        total = int(sizes[-1])
        payload = np.empty(total, np.uint8)
        if total:
            out.download(payload, self.stream)
            self.stream.synchronize()
        return sizes[:-1].copy(), payload.tobytes()

    def encode(self, sym: np.ndarray):
        sym = np.ascontiguousarray(sym, np.uint8).ravel()
        with self.lock:
            buf = self.scratch.get("sym", sym.size)
            if sym.size:
                buf.upload(sym, self.stream)
            return self._encode_device(buf, sym.size)

    def trace(self, sym: np.ndarray) -> np.ndarray:
        """(n, 3) int32: the (low, high, total) handed to the coder per symbol."""
        with self.lock:
            return self._trace(sym)

    def _trace(self, sym: np.ndarray) -> np.ndarray:
        lib = L.lib()
        sym = np.ascontiguousarray(sym, np.uint8).ravel()
        n = sym.size
        ns = n_segments(n, self.seg_len)
        buf = self.scratch.get("sym", n)
        if n:
            buf.upload(sym, self.stream)
        ws = self.scratch.get("ws", int(lib.vcf_cbaac_tiled_workspace(n, self.seg_len)))
        sb = self.scratch.get("sizes", 8 * (ns + 1))
        tr = DeviceBuffer(max(12 * n, 1))
        L.call("vcf_cbaac_tiled_trace", buf.ptr, n, self.order, self.seg_len, tr.ptr, sb.ptr, ws.ptr,
               self.stream.handle)
        out = np.empty((n, 3), np.int32)
        if n:
            tr.download(out, self.stream)
        self.stream.synchronize()
        return out

    def decode_to_device(self, payload: bytes, seg_bytes, n: int, out: DeviceBuffer, prior=None):
        """Enqueue the decode of n symbols into `out` on self.stream (the
        caller synchronises; hold self.lock across this and that wait when
        other threads share the coder)."""
        with self.lock:
            self._decode_to_device(payload, seg_bytes, n, out, prior)

    def _decode_to_device(self, payload: bytes, seg_bytes, n: int, out: DeviceBuffer, prior=None):
        seg_bytes = np.asarray(seg_bytes, np.int64)
        offs = np.zeros(seg_bytes.size + 1, np.int64)
        np.cumsum(seg_bytes, out=offs[1:])
        if int(offs[-1]) != len(payload):
            raise ValueError("segment sizes do not add up to the payload")
        src = self.scratch.get("in", len(payload))
        if len(payload):
            src.upload(np.frombuffer(payload, np.uint8), self.stream)
        ob = self.scratch.get("offs", offs.nbytes)
        ob.upload(offs, self.stream)
        if prior is not None and np.ndim(prior) == 2:   # version 3: prior classes
            prior = check_prior(prior)
            pr = self.scratch.get("prior_in", prior.nbytes)
            pr.upload(prior, self.stream)
            L.call_v(self.kernel, "vcf_cbaac_tiled_decode_classes", src.ptr, ob.ptr, 1, int(n), self.order, pr.ptr,
                     prior.shape[0], self.seg_len, out.ptr, int(n), self.stream.handle)
        elif prior is not None:
            prior = check_prior(prior)
            pr = self.scratch.get("prior_in", 512)
            pr.upload(prior, self.stream)
            L.call_v(self.kernel, "vcf_cbaac_tiled_decode_prior", src.ptr, ob.ptr, int(n), self.order, pr.ptr,
                     self.seg_len, out.ptr, self.stream.handle)
        else:
            L.call_v(self.kernel, "vcf_cbaac_tiled_decode", src.ptr, ob.ptr, int(n), self.order, self.seg_len,
                     out.ptr, self.stream.handle)

    def decode(self, payload: bytes, seg_bytes, n: int, prior=None) -> np.ndarray:
        with self.lock:
            out = self.scratch.get("dec", n)
            self.decode_to_device(payload, seg_bytes, n, out, prior)
            res = np.empty(n, np.uint8)
            if n:
                out.download(res, self.stream)
            self.stream.synchronize()
            return res


def check_prior(prior) -> np.ndarray:
    """256 uint16 frequencies (or nclass rows of them), each >= 1, every row's
    total below the model's max_freq (so the packed 16-bit cumulative counts
    of the GPU model cannot overflow)."""
    prior = np.ascontiguousarray(prior, np.uint16)
    rows = prior.reshape(-1, 256) if prior.ndim in (1, 2) and prior.shape[-1] == 256 else None
    if (rows is None or not 1 <= rows.shape[0] <= 256 or int(prior.min()) < 1
            or int(rows.sum(axis=1, dtype=np.int64).max()) >= 16384):
        raise ValueError("bad prior table")
    return prior


class FrameBatch:
    """Reusable device state for coding `n_frames` frames of `frame_symbols`
    symbols each (the III driver's per-rank chunk), every frame's code-stream
    kept in HBM.  One launch per stage codes all the frames
    (vcf_cbaac_tiled_*_frames): a frame's few hundred segments alone leave most
    of the chip idle, a batch's segments fill it (and from ~5000 on, order 0
    codes one segment per lane).  Frame f's packed segments sit at byte
    f * cap of `out`, its segment sizes and prior in one contiguous device
    array each, so one download returns the index.  launch() enqueues,
    sizes() waits and downloads the index, payload(f) / download() hand out
    the code-streams."""

    def __init__(self, n_frames: int, frame_symbols: int, order: int = 0, seg_len: int = PRIOR_SEG,
                 prior: bool = True, streams: int | None = None, nclass: int = 1, kernel: int = 0):
        lib = L.lib()
        self.n_frames, self.n = int(n_frames), int(frame_symbols)
        self.order, self.seg_len, self.prior = int(order), int(seg_len), bool(prior)
        self.nclass, self.kernel = int(nclass), int(kernel)
        if self.prior and self.order > 1:
            raise NotImplementedError("prior-seeded tiled CBAAC: orders 0 and 1")
        if self.nclass < 1 or (self.nclass > 1 and not self.prior):
            raise ValueError("prior classes need prior=True")
        self.ns = n_segments(self.n, self.seg_len)
        self.cap = int(lib.vcf_cbaac_tiled_bound(self.n, self.seg_len))
        self.stream = Stream()
        nf = max(self.n_frames, 1)
        self.ws = DeviceBuffer(max(int(lib.vcf_cbaac_tiled_frames_workspace(nf, self.n, self.seg_len)), 1))
        self.out = DeviceBuffer(max(self.cap * nf, 1))
        self.sizes_dev = DeviceBuffer(8 * (self.ns + 1) * nf)
        self.prior_dev = DeviceBuffer(512 * nf * self.nclass)
        self.hist = DeviceBuffer(1024 * nf * self.nclass)
        self._sizes = None
        self._priors = None

    def launch(self, sym: DeviceBuffer, offset: int = 0, after: Stream | None = None,
               frame_stride: int | None = None) -> None:
        """Enqueue frame f = symbols [offset + f * frame_stride, + n) of `sym`
        (frame_stride defaults to n); `after` (the producer's stream) is
        waited for through an event."""
        from .device import Event
        if after is not None:
            ev = Event()
            ev.record(after)
            self.stream.wait_event(ev)
        self._sizes = None
        if not self.n_frames:
            return
        stride = self.n if frame_stride is None else int(frame_stride)
        base = sym.address(offset)
        h = self.stream.handle
        if self.nclass > 1:
            L.call("vcf_cbaac_tiled_prior_classes", base, self.n_frames, self.n, stride, self.seg_len, self.nclass,
                   self.prior_dev.ptr, self.hist.ptr, h)
            L.call_v(self.kernel, "vcf_cbaac_tiled_encode_classes", base, self.n_frames, self.n, stride, self.order,
                     self.prior_dev.ptr, self.nclass, self.seg_len, self.out.ptr, self.cap, self.sizes_dev.ptr,
                     self.ws.ptr, h)
            return
        if self.prior:
            L.call("vcf_cbaac_tiled_prior_frames", base, self.n_frames, self.n, stride, self.prior_dev.ptr,
                   self.hist.ptr, h)
        L.call_v(self.kernel, "vcf_cbaac_tiled_encode_frames", base, self.n_frames, self.n, stride, self.order,
                 self.prior_dev.ptr if self.prior else None, self.seg_len, self.out.ptr, self.cap, self.sizes_dev.ptr,
                 self.ws.ptr, h)

    def join(self, stream: Stream) -> None:
        """`stream` waits for the coding (no host synchronisation)."""
        from .device import Event
        ev = Event()
        ev.record(self.stream)
        stream.wait_event(ev)

    def sizes(self):
        """Wait for the coding; -> (per-frame segment byte counts (n_frames x
        ns int64), per-frame payload bytes, priors (n_frames x 256) or None)."""
        if self._sizes is None:
            allz = np.empty((self.n_frames, self.ns + 1), np.int64)
            self._priors = None
            if self.n_frames:
                self.sizes_dev.download(allz, self.stream)
                if self.prior:
                    self._priors = np.empty(self._prior_shape(), np.uint16)
                    self.prior_dev.download(self._priors, self.stream)
            self.stream.synchronize()
            self._sizes = allz
        return self._sizes[:, :-1], self._sizes[:, -1].copy(), self._priors

    def _prior_shape(self):
        return (self.n_frames, self.nclass, 256) if self.nclass > 1 else (self.n_frames, 256)

    def payload(self, f: int):
        """(device buffer, byte offset, byte count) of frame f's packed segments."""
        _, totals, _ = self.sizes()
        return self.out, f * self.cap, int(totals[f])

    def header(self, f: int, shape) -> bytes:
        """Frame f's container bytes in front of its payload (pack() minus the payload)."""
        seg, _, pri = self.sizes()
        return pack(tuple(shape), self.order, self.seg_len, seg[f], b"", None if pri is None else pri[f])

    def headers(self, shape) -> list:
        """Every frame's header (== header(f, shape)), built for the whole
        batch at once: version 3's varint indexes and sparse prior rows as a
        few array operations over all frames instead of a pack() per frame."""
        seg, _, pri = self.sizes()
        if pri is None or pri.ndim != 3:
            return [self.header(f, shape) for f in range(self.n_frames)]
        F, K = pri.shape[:2]
        fixed = (np.array([len(shape), *shape], np.uint32).tobytes() + MAGIC +
                 struct.pack("<IIII", VERSION_CLASSES, self.order, self.seg_len, self.ns))
        if int(pri.min()) < 1 or int(pri.sum(axis=2, dtype=np.int64).max()) >= 16384:   # check_prior, every frame
            raise ValueError("bad prior table")
        rb, rend = _sparse_rows_batch(pri)
        vb, vend = _varints_rows(seg)
        rst = np.concatenate([[0], rend[:-1]])
        vst = np.concatenate([[0], vend[:-1]])
        return [fixed + rb[rst[f]:rend[f]] + vb[vst[f]:vend[f]] for f in range(F)]

    def download(self):
        """-> [(segment byte counts, payload bytes, prior or None)] per frame."""
        seg, totals, pri = self.sizes()
        res = []
        for f in range(self.n_frames):
            payload = np.empty(int(totals[f]), np.uint8)
            if payload.size:
                self.out.download(payload, offset=f * self.cap)
            res.append((seg[f].copy(), payload.tobytes(), None if pri is None else pri[f].copy()))
        return res


def encode_frames_device(sym: DeviceBuffer, n_frames: int, frame_symbols: int, order: int = 0,
                         seg_len: int = DEFAULT_SEG, prior: bool = False, streams: int = 4,
                         after: Stream | None = None, offset: int = 0, nclass: int = 1, kernel: int = 0):
    """Several frames' symbols, back to back in HBM from `offset`, each coded
    as its own tiled stream (its own prior with prior=True), all of them in
    one launch per stage (FrameBatch; `streams` is accepted for the earlier
    interface and unused).  `after`: the stream that produced the symbols
    (e.g. the DCT encode's); the coder waits for its work so far (an event),
    so the caller need not synchronise it first.
    -> [(segment byte counts, payload, prior or None)]."""
    fb = FrameBatch(n_frames, frame_symbols, order, seg_len, prior, nclass=nclass, kernel=kernel)
    fb.launch(sym, offset, after)
    return fb.download()


def frame_dims(shape):
    """Version 4's (H, W, C) of an array shape: (H, W, C), or (H, W) with C = 1."""
    shape = tuple(int(s) for s in shape)
    if len(shape) == 2:
        return shape + (1,)
    if len(shape) == 3:
        return shape
    raise ValueError(f"2-D context: a (H, W, C) or (H, W) array, not {len(shape)} dimensions")


def n_tiles2d(shape, th: int, tw: int) -> int:
    H, W, C = frame_dims(shape)
    return int(L.lib().vcf_cbaac2d_tiles(H, W, C, int(th), int(tw)))


def check_rows2d(priors, nclass: int) -> np.ndarray:
    """Version 4's nclass x 16 prior rows as a (nclass * 16, 256) uint16 array:
    every frequency >= 1, every row's total below the model's max_freq."""
    priors = np.ascontiguousarray(priors, np.uint16)
    if (not 1 <= int(nclass) <= 256 or priors.size != int(nclass) * NCTX_2D * 256 or int(priors.min()) < 1
            or int(priors.reshape(-1, 256).sum(axis=1, dtype=np.int64).max()) >= 16384):
        raise ValueError("bad prior table")
    return priors.reshape(-1, 256)


class FrameBatch2D(FrameBatch):
    """FrameBatch for container version 4: `n_frames` frames of one shape,
    each coded in tiles with the two-dimensional context, one launch per
    stage (vcf_cbaac_tiled2d_*_frames).  `ns` counts tiles, sizes() returns
    the tile byte counts and the (n_frames, nclass * 16, 256) prior rows."""

    def __init__(self, n_frames: int, shape, tile=TILE_2D, nclass: int = PRIOR_CLASSES, stream: Stream | None = None):
        lib = L.lib()
        self.n_frames = int(n_frames)
        self.shape = tuple(int(s) for s in shape)
        self.H, self.W, self.C = frame_dims(self.shape)
        self.n = self.H * self.W * self.C
        self.th, self.tw = int(tile[0]), int(tile[1])
        self.order, self.seg_len, self.prior, self.nclass = 0, self.th * self.tw, True, int(nclass)
        if self.th < 1 or self.tw < 1 or not 1 <= self.nclass <= 256:
            raise ValueError("tile sizes >= 1, 1 .. 256 prior classes")
        dims = (self.H, self.W, self.C, self.th, self.tw)
        self.ns = int(lib.vcf_cbaac_tiled2d_tiles(*dims))
        self.cap = int(lib.vcf_cbaac_tiled2d_bound(*dims))
        self.stream = stream if stream is not None else Stream()
        nf = max(self.n_frames, 1)
        self.ws = DeviceBuffer(max(int(lib.vcf_cbaac_tiled2d_workspace(nf, *dims)), 1))
        self.out = DeviceBuffer(max(self.cap * nf, 1))
        self.sizes_dev = DeviceBuffer(8 * (self.ns + 1) * nf)
        self.prior_dev = DeviceBuffer(512 * NCTX_2D * nf * self.nclass)
        self.hist = DeviceBuffer(1024 * NCTX_2D * nf * self.nclass)
        self._sizes = None
        self._priors = None

    def launch(self, sym: DeviceBuffer, offset: int = 0, after: Stream | None = None,
               frame_stride: int | None = None) -> None:
        from .device import Event
        if after is not None and after is not self.stream:
            ev = Event()
            ev.record(after)
            self.stream.wait_event(ev)
        self._sizes = None
        if not self.n_frames:
            return
        stride = self.n if frame_stride is None else int(frame_stride)
        base, h = sym.address(offset), self.stream.handle
        L.call("vcf_cbaac_tiled2d_prior_frames", base, self.n_frames, self.H, self.W, self.C, stride, self.th, self.tw,
               self.nclass, self.prior_dev.ptr, self.hist.ptr, h)
        L.call("vcf_cbaac_tiled2d_encode_frames", base, self.n_frames, self.H, self.W, self.C, stride,
               self.prior_dev.ptr, self.nclass, self.th, self.tw, self.out.ptr, self.cap, self.sizes_dev.ptr,
               self.ws.ptr, h)

    def _prior_shape(self):
        return (self.n_frames, self.nclass * NCTX_2D, 256)

    def header(self, f: int, shape=None) -> bytes:
        tiles, _, pri = self.sizes()
        return pack2d(self.shape if shape is None else tuple(shape), self.th, self.tw, self.nclass, pri[f], tiles[f], b"")

    def headers(self, shape=None) -> list:
        """Every frame's header (== header(f)), the sparse rows and varints of all frames at once."""
        tiles, _, pri = self.sizes()
        if not self.n_frames:
            return []
        shape = self.shape if shape is None else tuple(shape)
        for f in range(self.n_frames):
            check_rows2d(pri[f], self.nclass)
        fixed = _head2d(shape, self.th, self.tw, self.ns, self.nclass)
        rb, rend = _sparse_rows_batch(pri)
        vb, vend = _varints_rows(tiles)
        rst = np.concatenate([[0], rend[:-1]])
        vst = np.concatenate([[0], vend[:-1]])
        return [fixed + rb[rst[f] + 4:rend[f]] + vb[vst[f]:vend[f]] for f in range(self.n_frames)]


PLANE_DESC = np.dtype([("base", "<i8"), ("H", "<i4"), ("W", "<i4"), ("C", "<i4"), ("tile0", "<i4")])   # vcf_plane_desc


def plane_descriptors(arrays, tile=TILE_2D):
    """The descriptor table of a plane list (include/vcf_amd.h vcf_plane_desc)
    for `arrays` = (byte offset in the buffer, H, W, C) per coded array, in
    stream order -> (PLANE_DESC array, the list's tile count).  tile0 of array
    a is the tile count of the arrays before it; host arithmetic only."""
    th, tw = int(tile[0]), int(tile[1])
    if th < 1 or tw < 1:
        raise ValueError("tile sizes >= 1")
    desc = np.zeros(len(arrays), PLANE_DESC)
    tiles = 0
    for a, (base, H, W, C) in enumerate(arrays):
        if min(int(H), int(W), int(C)) < 1 or int(base) < 0:
            raise ValueError(f"array {a}: {(base, H, W, C)}: a plane list holds non-empty arrays at offsets >= 0")
        desc[a] = (int(base), int(H), int(W), int(C), tiles)
        tiles += int(C) * (-(-int(H) // th)) * (-(-int(W) // tw))
        if tiles > 0x7FFFFFFF:
            raise ValueError("too many tiles")
    return desc, tiles


class PlaneBatch2D:
    """Container version 4 over a plane list: arrays of different sizes
    anywhere in one device buffer (a batch of 2D-DWT frames' packed subbands),
    every tile of every array in one launch per stage
    (vcf_cbaac_tiled2d_*_planes).  Array a's stream is, byte for byte,
    TiledCBAACCodec(ctx2d=True).compress of that array alone.  launch()
    enqueues, streams(shapes) waits and returns the containers; decode()
    writes the arrays of parsed containers back to their places."""

    def __init__(self, tile=TILE_2D, nclass: int = PRIOR_CLASSES, stream: Stream | None = None):
        self.th, self.tw = int(tile[0]), int(tile[1])
        self.nclass = int(nclass)
        if self.th < 1 or self.tw < 1 or not 1 <= self.nclass <= 256:
            raise ValueError("tile sizes >= 1, 1 .. 256 prior classes")
        self.stream = stream if stream is not None else Stream()
        self.scratch = _Scratch()
        self.lock = threading.RLock()

    def _describe(self, arrays, buf: DeviceBuffer):
        desc, nt = plane_descriptors(arrays, (self.th, self.tw))
        if not len(desc):
            raise ValueError("empty plane list")
        ends = desc["base"] + desc["H"].astype(np.int64) * desc["W"] * desc["C"]
        if int(ends.max()) > buf.nbytes:
            raise ValueError(f"plane list: an array ends at byte {int(ends.max())} of a {buf.nbytes}-byte buffer")
        dd = self.scratch.get("desc", desc.nbytes)
        dd.upload(desc, self.stream)
        return desc, nt, dd

    def launch(self, buf: DeviceBuffer, arrays, after: Stream | None = None) -> None:
        """Enqueue the coding of `arrays` ((byte offset, H, W, C) each) of `buf`."""
        from .device import Event
        lib = L.lib()
        if after is not None and after is not self.stream:
            ev = Event()
            ev.record(after)
            self.stream.wait_event(ev)
        self.desc, self.nt, dd = self._describe(arrays, buf)
        na, K, h = len(self.desc), self.nclass, self.stream.handle
        self.cap = int(lib.vcf_cbaac_tiled2d_planes_bound(self.nt, self.th, self.tw))
        ws = self.scratch.get("ws", int(lib.vcf_cbaac_tiled2d_planes_workspace(self.nt, self.th, self.tw)))
        self.out = self.scratch.get("out", self.cap)
        self.sizes_dev = self.scratch.get("sizes", 8 * (self.nt + 1))
        self.prior_dev = self.scratch.get("prior", 512 * NCTX_2D * K * na)
        hist = self.scratch.get("hist", 1024 * NCTX_2D * K * na)
        L.call("vcf_cbaac_tiled2d_prior_planes", buf.ptr, buf.nbytes, self.desc.ctypes.data, dd.ptr, na, self.nt, self.th,
               self.tw, K, self.prior_dev.ptr, hist.ptr, h)
        L.call("vcf_cbaac_tiled2d_encode_planes", buf.ptr, buf.nbytes, self.desc.ctypes.data, dd.ptr, na, self.nt,
               self.prior_dev.ptr, K, self.th, self.tw, self.out.ptr, self.cap, self.sizes_dev.ptr, ws.ptr, h)

    def streams(self, shapes) -> list:
        """Wait for launch(); -> the version-4 container (bytes) of every
        array, written with shapes[a] (H * W * C symbols: the shape the
        single-array path would have been given)."""
        na = len(self.desc)
        sizes = np.empty(self.nt + 1, np.int64)
        pri = np.empty((na, self.nclass * NCTX_2D, 256), np.uint16)
        self.sizes_dev.download(sizes, self.stream)
        self.prior_dev.download(pri, self.stream)
        self.stream.synchronize()
        payload = np.empty(int(sizes[-1]), np.uint8)
        if payload.size:
            self.out.download(payload, self.stream)
            self.stream.synchronize()
        offs = np.zeros(self.nt + 1, np.int64)
        np.cumsum(sizes[:-1], out=offs[1:])
        t0 = np.append(self.desc["tile0"].astype(np.int64), self.nt)
        res = []
        for a in range(na):
            d = self.desc[a]
            shape = tuple(int(s) for s in shapes[a])
            if frame_dims(shape) != (int(d["H"]), int(d["W"]), int(d["C"])):
                raise ValueError(f"array {a}: shape {shape} is not the coded {(d['H'], d['W'], d['C'])}")
            res.append(pack2d(shape, self.th, self.tw, self.nclass, pri[a], sizes[t0[a]:t0[a + 1]],
                              payload[offs[t0[a]]:offs[t0[a + 1]]].tobytes()))
        return res

    def decode(self, parsed, buf: DeviceBuffer, arrays) -> None:
        """parsed[a] = _parse2d's fields of array a's container; its symbols
        are written to arrays[a] = (byte offset, H, W, C) of `buf`, enqueued on
        self.stream.  Every container is checked against its array, this
        coder's tile and class count and its own payload before anything is
        launched: ValueError otherwise."""
        if len(parsed) != len(arrays):
            raise ValueError("plane list: one container per array")
        for a, (f, arr) in enumerate(zip(parsed, arrays)):
            shape, th, tw, nclass, rows, tile_bytes, payload = f
            if frame_dims(shape) != tuple(int(v) for v in arr[1:]):
                raise ValueError(f"array {a}: a stream of shape {shape} where {tuple(arr[1:])} is expected")
            if (th, tw, nclass) != (self.th, self.tw, self.nclass):
                raise ValueError(f"array {a}: tile {th} x {tw}, {nclass} classes: not this coder's")
            check_rows2d(rows, nclass)
            if len(tile_bytes) != n_tiles2d(shape, th, tw) or int(np.sum(tile_bytes)) != len(payload):
                raise ValueError(f"array {a}: tile sizes do not match the array or the payload")
        desc, nt, dd = self._describe(arrays, buf)
        tile_bytes = np.concatenate([np.asarray(f[5], np.int64) for f in parsed])
        offs = np.zeros(nt + 1, np.int64)
        np.cumsum(tile_bytes, out=offs[1:])
        payload = np.frombuffer(b"".join(bytes(f[6]) for f in parsed), np.uint8)
        pri = np.concatenate([check_rows2d(f[4], self.nclass) for f in parsed])
        src = self.scratch.get("in", payload.size)
        if payload.size:
            src.upload(payload, self.stream)
        ob = self.scratch.get("offs", offs.nbytes)
        ob.upload(offs, self.stream)
        pr = self.scratch.get("prior_in", pri.nbytes)
        pr.upload(pri, self.stream)
        L.call("vcf_cbaac_tiled2d_decode_planes", src.ptr, ob.ptr, desc.ctypes.data, dd.ptr, len(desc), nt, pr.ptr,
               self.nclass, self.th, self.tw, buf.ptr, buf.nbytes, self.stream.handle)
        self.stream.synchronize()   # desc, offs and the payload were uploaded from temporaries


class Tiled2DCoder:
    """The version-4 GPU calls for one frame at a time, with a stream, a lock
    (as TiledCoder: the block codecs call the entropy codec from a thread
    pool) and the device state of the last shape kept for the next call."""

    def __init__(self, tile=TILE_2D, nclass: int = PRIOR_CLASSES, stream: Stream | None = None):
        self.tile, self.nclass = (int(tile[0]), int(tile[1])), int(nclass)
        self.stream = stream if stream is not None else Stream()
        self.scratch = _Scratch()
        self.last_prior = None
        self.lock = threading.RLock()
        self._fb = None

    def _batch(self, shape) -> FrameBatch2D:
        shape = tuple(int(s) for s in shape)
        if self._fb is None or self._fb.shape != shape:
            self._fb = FrameBatch2D(1, shape, self.tile, self.nclass, self.stream)
        return self._fb

    def encode_device(self, sym: DeviceBuffer, shape, offset: int = 0):
        """A frame already in HBM -> (tile byte counts, payload bytes); its
        prior rows are left in self.last_prior."""
        with self.lock:
            fb = self._batch(shape)
            fb.launch(sym, offset)
            tiles, payload, pri = fb.download()[0]
            self.last_prior = pri
            return tiles, payload

    def encode(self, img: np.ndarray):
        img = np.ascontiguousarray(img, np.uint8)
        with self.lock:
            buf = self.scratch.get("sym", img.size)
            if img.size:
                buf.upload(img, self.stream)
            return self.encode_device(buf, img.shape)

    def decode(self, payload: bytes, tile_bytes, shape, priors, nclass: int | None = None) -> np.ndarray:
        nclass = self.nclass if nclass is None else int(nclass)
        H, W, C = frame_dims(shape)
        th, tw = self.tile
        priors = check_rows2d(priors, nclass)
        tile_bytes = np.asarray(tile_bytes, np.int64)
        offs = np.zeros(tile_bytes.size + 1, np.int64)
        np.cumsum(tile_bytes, out=offs[1:])
        if tile_bytes.size != n_tiles2d(shape, th, tw) or int(offs[-1]) != len(payload):
            raise ValueError("tile sizes do not match the frame or the payload")
        n = H * W * C
        res = np.empty(tuple(int(s) for s in shape), np.uint8)
        with self.lock:
            src = self.scratch.get("in", len(payload))
            if len(payload):
                src.upload(np.frombuffer(payload, np.uint8), self.stream)
            ob = self.scratch.get("offs", offs.nbytes)
            ob.upload(offs, self.stream)
            pr = self.scratch.get("prior_in", priors.nbytes)
            pr.upload(priors, self.stream)
            out = self.scratch.get("dec", n)
            L.call("vcf_cbaac_tiled2d_decode_frames", src.ptr, ob.ptr, 1, H, W, C, pr.ptr, nclass, th, tw, out.ptr, n,
                   self.stream.handle)
            if n:
                out.download(res, self.stream)
            self.stream.synchronize()
        return res


def _head2d(shape, th: int, tw: int, n_tiles: int, nclass: int) -> bytes:
    return (np.array([len(shape), *shape], np.uint32).tobytes() + MAGIC +
            struct.pack("<IIIIII", VERSION_2D, th, tw, n_tiles, nclass, NCTX_2D))


def pack2d(shape, th: int, tw: int, nclass: int, priors, tile_bytes, payload: bytes) -> bytes:
    """The version-4 container."""
    tile_bytes = np.asarray(tile_bytes, np.int64)
    rows = check_rows2d(priors, nclass)
    return (_head2d(tuple(shape), th, tw, tile_bytes.size, nclass) + _sparse_rows(rows)[4:] + _varints(tile_bytes) +
            payload)


def container_version(data: bytes) -> int:
    """The version field of a `.tadpt_arith` container; ValueError if it is not one."""
    nd = struct.unpack_from("<I", data, 0)[0]
    if nd > 16:
        raise ValueError("ndims")
    p = 4 + 4 * nd
    if data[p:p + 4] != MAGIC:
        raise ValueError("not a tiled CBAAC stream")
    return struct.unpack_from("<I", data, p + 4)[0]


def _parse2d(data: bytes):
    """A version-4 container -> (shape, th, tw, nclass, prior rows, tile byte
    counts, payload); ValueError / struct.error if malformed (all checks on
    the host, before any device work)."""
    if container_version(data) != VERSION_2D:
        raise ValueError("not a version-4 stream")
    nd = struct.unpack_from("<I", data, 0)[0]
    shape = tuple(int(s) for s in struct.unpack_from(f"<{nd}I", data, 4))
    p = 4 + 4 * nd + 4
    _, th, tw, nt, nclass, nctx = struct.unpack_from("<IIIIII", data, p)
    p += 24
    if nd not in (2, 3):
        raise ValueError(f"{nd} dimensions")
    if th < 1 or tw < 1:
        raise ValueError(f"tile {th} x {tw}")
    if nctx != NCTX_2D:
        raise ValueError(f"{nctx} contexts")
    if not 1 <= nclass <= 256:
        raise ValueError(f"{nclass} prior classes")
    if nt != n_tiles2d(shape, th, tw):
        raise ValueError("tile count does not match the shape")
    rows, p = _parse_rows(data, p, nclass * NCTX_2D)
    rows = check_rows2d(rows, nclass)
    tile_bytes, p = _parse_varints(data, p, nt)
    payload = data[p:]
    if int(tile_bytes.sum()) != len(payload):
        raise ValueError("tile index does not match the payload")
    return shape, int(th), int(tw), int(nclass), rows, tile_bytes, payload


def _varints_rows(v: np.ndarray):
    """Unsigned LEB128 varints (7 bits per byte, high bit = more) of each row
    of a 2-D array (vcf_leb128_encode_rows) -> (bytes, end offset of each row)."""
    v = np.ascontiguousarray(v, np.int64)
    out = np.empty(max(5 * v.size, 1), np.uint8)
    ends = np.zeros(v.shape[0], np.int64)
    L.call("vcf_leb128_encode_rows", v.ctypes.data, v.shape[0], v.shape[1], out.ctypes.data, out.size,
           ends.ctypes.data)
    return out[:int(ends[-1]) if ends.size else 0].tobytes(), ends


def _varints(v: np.ndarray) -> bytes:
    return _varints_rows(np.asarray(v, np.int64).reshape(1, -1))[0]


def _sparse_rows_batch(pri: np.ndarray):
    """Version 3's sparse prior rows of every frame of an (F, K, 256) array
    (vcf_prior_rows_sparse) -> (bytes, end offset of each frame)."""
    pri = np.ascontiguousarray(pri, np.uint16)
    F, K = pri.shape[:2]
    out = np.empty(F * (4 + K * (2 + 3 * 256)), np.uint8)
    ends = np.zeros(F, np.int64)
    L.call("vcf_prior_rows_sparse", pri.ctypes.data, F, K, out.ctypes.data, out.size, ends.ctypes.data)
    return out[:int(ends[-1]) if F else 0].tobytes(), ends


def _parse_varints(data: bytes, p: int, count: int):
    """-> (count values, the offset after them); ValueError if the data end first."""
    if count == 0:
        return np.zeros(0, np.int64), p
    raw = np.frombuffer(data, np.uint8, min(len(data) - p, 5 * count), p)
    ends = np.flatnonzero(raw < 0x80)
    if ends.size < count:
        raise ValueError("segment index")
    stop = int(ends[count - 1]) + 1
    raw = raw[:stop].astype(np.uint64)
    grp = np.concatenate([[0], np.cumsum(raw[:-1] < 0x80)])
    start = np.concatenate([[0], ends[:count - 1] + 1])
    pos = np.arange(stop) - start[grp]
    if int(pos.max()) > 4:
        raise ValueError("segment index")
    vals = np.zeros(count, np.uint64)
    np.add.at(vals, grp, (raw & np.uint64(0x7F)) << (np.uint64(7) * pos.astype(np.uint64)))
    return vals.astype(np.int64), p + stop


def _sparse_rows(prior: np.ndarray) -> bytes:
    """Version 3's prior rows: per row uint16 m, m uint8 symbols, m uint16 frequencies (those != 1)."""
    return _sparse_rows_batch(np.asarray(prior)[None])[0]


def _parse_sparse_rows(data: bytes, p: int):
    (K,) = struct.unpack_from("<I", data, p)
    if not 1 <= K <= 256:
        raise ValueError(f"{K} prior classes")
    prior, p = _parse_rows(data, p + 4, K)
    return check_prior(prior), p


def _parse_rows(data: bytes, p: int, rows: int):
    """`rows` sparse prior rows at data[p:] -> ((rows, 256) uint16, the offset after them)."""
    prior = np.ones((rows, 256), np.uint16)
    for c in range(rows):
        (m,) = struct.unpack_from("<H", data, p)
        if m > 256 or p + 2 + 3 * m > len(data):
            raise ValueError("prior row")
        sy = np.frombuffer(data, np.uint8, m, p + 2)
        prior[c, sy] = np.frombuffer(data, "<u2", m, p + 2 + m)
        p += 2 + 3 * m
    return prior, p


def pack(shape, order: int, seg_len: int, seg_bytes, payload: bytes, prior=None) -> bytes:
    """The container: version 1 (prior None), 2 (one 256-entry prior) or 3 (nclass x 256 priors)."""
    seg_bytes = np.asarray(seg_bytes, np.int64)
    head = np.array([len(shape), *shape], np.uint32).tobytes()
    classes = prior is not None and np.ndim(prior) == 2
    version = VERSION if prior is None else (VERSION_CLASSES if classes else VERSION_PRIOR)
    head += MAGIC + struct.pack("<IIII", version, order, seg_len, seg_bytes.size)
    if classes:   # version 3: sparse prior rows, the segment sizes as LEB128 varints
        return head + _sparse_rows(check_prior(prior)) + _varints(seg_bytes) + payload
    if prior is not None:
        head += check_prior(prior).astype("<u2").tobytes()
    head += seg_bytes.astype(np.uint32).tobytes()
    return head + payload


def unpack(data: bytes):
    """-> (shape, order, seg_len, seg_bytes, payload); ValueError if malformed."""
    return _parse(data)[:5]


def _parse(data: bytes):
    """-> (shape, order, seg_len, seg_bytes, payload, prior or None)."""
    nd = struct.unpack_from("<I", data, 0)[0]
    if nd > 16:
        raise ValueError("ndims")
    shape = struct.unpack_from(f"<{nd}I", data, 4)
    p = 4 + 4 * nd
    if data[p:p + 4] != MAGIC:
        raise ValueError("not a tiled CBAAC stream")
    version, order, seg_len, ns = struct.unpack_from("<IIII", data, p + 4)
    if version not in (VERSION, VERSION_PRIOR, VERSION_CLASSES):
        raise ValueError(f"version {version}")
    if order > 1:                       # the GPU coder's orders (both versions)
        raise ValueError(f"order {order}")
    if seg_len <= 0 or seg_len % 256:   # vcf_cbaac_tiled_*: a positive multiple of 256
        raise ValueError(f"segment length {seg_len}")
    p += 20
    prior = None
    if version == VERSION_PRIOR:
        prior = check_prior(np.frombuffer(data, "<u2", 256, p))
        p += 512
    if version == VERSION_CLASSES:
        prior, p = _parse_sparse_rows(data, p)
        seg_bytes, p = _parse_varints(data, p, ns)
    else:
        seg_bytes = np.frombuffer(data, np.uint32, ns, p).astype(np.int64)
        p += 4 * ns
    payload = data[p:]
    n = int(np.prod(shape)) if nd else 1
    if n_segments(n, seg_len) != ns or int(seg_bytes.sum()) != len(payload):
        raise ValueError("segment index does not match the payload")
    return tuple(int(s) for s in shape), int(order), int(seg_len), seg_bytes, payload, prior


class _Container:
    """What the GPU codec and the host codec share: the parameters and the
    reader of the `.tadpt_arith` container, all four versions."""

    file_extension = FILE_EXTENSION

    def __init__(self, order: int = 0, seg_len: int = DEFAULT_SEG, prior: bool = False, nclass: int = 1,
                 ctx2d: bool = False, tile=TILE_2D):
        """ctx2d: write container version 4 (tiles of `tile` = (th, tw) with
        the two-dimensional context and `nclass` prior classes; order 0)."""
        self.ORDER = int(order)
        self.seg_len = int(seg_len)
        self.prior = bool(prior)
        self.nclass = int(nclass)
        self.ctx2d, self.tile = bool(ctx2d), (int(tile[0]), int(tile[1]))
        if self.ctx2d and self.ORDER != 0:
            raise NotImplementedError("the 2-D context takes the order's place: order 0")

    @staticmethod
    def _symbols(img) -> np.ndarray:
        img = np.asarray(img)
        if img.size and (img.min() < 0 or img.max() > 255):
            raise ValueError("CBAAC codes byte symbols (0..255)")
        return img

    def decompress(self, data, fn=None) -> np.ndarray:
        """One reader for versions 1-4, dispatched on the version field."""
        if isinstance(data, io.BytesIO):
            data = data.getvalue()
        data = bytes(data)
        try:
            tiles = container_version(data) == VERSION_2D
            fields = _parse2d(data) if tiles else _parse(data)
        except (ValueError, struct.error):
            return np.zeros((10, 10), np.uint8)      # CBAAC.py:101-102
        return self._decode_tiles(*fields) if tiles else self._decode_segments(*fields)


class HostTiledCBAACCodec(_Container):
    """TiledCBAACCodec on the CPU: the serial host coders run segment by
    segment (versions 1-3) or over the frame's tiles (version 4,
    vcf_cbaac2d_*), writing the bytes the GPU writes.  For machines without a
    GPU, and what the GPU coder is compared against."""

    def compress(self, img: np.ndarray, fn=None) -> io.BytesIO:
        img = self._symbols(img)
        k = np.ascontiguousarray(img, np.uint8)
        if self.ctx2d:
            th, tw = self.tile
            priors = prior2d_of(k, th, tw, self.nclass)
            tiles = host_tiles2d(k, priors, th, tw, self.nclass)
            data = pack2d(img.shape, th, tw, self.nclass, priors, [len(t) for t in tiles], b"".join(tiles))
        else:
            prior = prior_of(k, self.nclass, self.seg_len) if self.prior else None
            segs = (host_segments_prior(k, prior, self.seg_len, self.ORDER) if self.prior else
                    host_segments(k, self.ORDER, self.seg_len))
            data = pack(img.shape, self.ORDER, self.seg_len, [len(s) for s in segs], b"".join(segs), prior)
        b = io.BytesIO(data)
        b.seek(0)
        return b

    def _decode_tiles(self, shape, th, tw, nclass, priors, tile_bytes, payload):
        return host_decode2d(payload, tile_bytes, shape, priors, th, tw, nclass)

    def _decode_segments(self, shape, order, seg_len, seg_bytes, payload, prior):
        from .cbaac import decode_symbols
        n = int(np.prod(shape))
        out = np.empty(n, np.uint8)
        ends = np.cumsum(seg_bytes)
        for i, (nb, e) in enumerate(zip(seg_bytes, ends)):
            part = payload[int(e - nb):int(e)]
            m = min(seg_len, n - i * seg_len)
            if prior is None:
                out[i * seg_len:i * seg_len + m] = decode_symbols(part, m, order)
            else:
                row = prior[i * prior.shape[0] // len(seg_bytes)] if prior.ndim == 2 else prior
                out[i * seg_len:i * seg_len + m] = host_decode_prior(part, m, row, order)
        return out.reshape(shape)


class TiledCBAACCodec(_Container):
    """The entropy-codec surface of CBAAC.CoDec (compress/decompress,
    file_extension; CBAAC.py:72-156) over the tiled GPU coder."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self._coder = None
        self._make = threading.Lock()

    @property
    def coder(self):
        with self._make:
            if self._coder is None:
                if self.ctx2d:
                    self._coder = Tiled2DCoder(self.tile, self.nclass)
                else:
                    self._coder = TiledCoder(self.ORDER, self.seg_len, prior=self.prior, nclass=self.nclass)
            return self._coder

    def compress(self, img: np.ndarray, fn=None) -> io.BytesIO:
        img = self._symbols(img)
        flat = img.ravel()
        coder = self.coder
        if self.ctx2d:
            with coder.lock:    # last_prior belongs to this call's encode
                tiles, payload = coder.encode(img)
                b = io.BytesIO(pack2d(img.shape, *self.tile, self.nclass, coder.last_prior, tiles, payload))
            b.seek(0)
            return b
        with coder.lock:    # last_prior belongs to this call's encode
            sizes, payload = coder.encode(flat.astype(np.uint8))
            prior = coder.last_prior if self.prior else None
        b = io.BytesIO(pack(img.shape, self.ORDER, self.seg_len, sizes, payload, prior))
        b.seek(0)
        return b

    def compress_device(self, k: DeviceBuffer, shape, offset: int = 0) -> io.BytesIO:
        """Indices already in HBM (e.g. the DCT encode's output): only the
        compressed bytes cross PCIe."""
        n = int(np.prod(shape))
        coder = self.coder
        with coder.lock:
            if self.ctx2d:
                tiles, payload = coder.encode_device(k, shape, offset)
                data = pack2d(tuple(shape), *self.tile, self.nclass, coder.last_prior, tiles, payload)
            else:
                sizes, payload = coder.encode_device(k, n, offset)
                data = pack(tuple(shape), self.ORDER, self.seg_len, sizes, payload,
                            coder.last_prior if self.prior else None)
        b = io.BytesIO(data)
        b.seek(0)
        return b

    def _decode_segments(self, shape, order, seg_len, seg_bytes, payload, prior):
        mine = not self.ctx2d and (order, seg_len) == (self.ORDER, self.seg_len)
        coder = self.coder if mine else TiledCoder(order, seg_len)
        n = int(np.prod(shape))
        return coder.decode(payload, seg_bytes, n, prior).reshape(shape)

    def _decode_tiles(self, shape, th, tw, nclass, priors, tile_bytes, payload):
        coder = self.coder if self.ctx2d and (th, tw) == self.tile else Tiled2DCoder((th, tw), nclass)
        return coder.decode(payload, tile_bytes, shape, priors, nclass)


def host_segments(sym: np.ndarray, order: int = 0, seg_len: int = DEFAULT_SEG):
    """The host serial coder (vcf_cbaac_encode) run on every segment: what
    each segment of the tiled stream must equal (tests, rate reports)."""
    from .cbaac import encode_symbols
    sym = np.ascontiguousarray(sym, np.uint8).ravel()
    return [encode_symbols(sym[i:i + seg_len], order) for i in range(0, sym.size, seg_len)]


def prior_of(sym: np.ndarray, nclass: int = 1, seg_len: int | None = None) -> np.ndarray:
    """The version-2 prior of a frame's symbols (nclass = 1), or version 3's
    nclass rows for segments of seg_len, on the host (what
    vcf_cbaac_tiled_prior / _prior_classes compute on the GPU)."""
    sym = np.ascontiguousarray(sym, np.uint8).ravel()
    if nclass == 1:
        hist = np.bincount(sym, minlength=256).astype(np.uint64)
        n = max(sym.size, 1)
        return (1 + hist * 8192 // n).astype(np.uint16)
    ns = n_segments(sym.size, seg_len)
    rows = np.ones((nclass, 256), np.uint16)
    for c in range(nclass):
        segs = [s for s in range(ns) if s * nclass // ns == c]
        if not segs:
            continue
        part = sym[segs[0] * seg_len:(segs[-1] + 1) * seg_len]
        hist = np.bincount(part, minlength=256).astype(np.uint64)
        rows[c] = (1 + hist * 8192 // max(part.size, 1)).astype(np.uint16)
    return rows


def host_segments_prior(sym: np.ndarray, prior, seg_len: int = DEFAULT_SEG, order: int = 0):
    """vcf_cbaac_encode_prior on every segment: what each segment of a
    version-2 stream (one prior) or version-3 stream (prior rows: segment s of
    ns takes row s * nclass // ns) must equal."""
    import ctypes
    prior = check_prior(prior)
    sym = np.ascontiguousarray(sym, np.uint8).ravel()
    lib = L.lib()
    res = []
    ns = n_segments(sym.size, seg_len)
    for i in range(0, sym.size, seg_len):
        seg = np.ascontiguousarray(sym[i:i + seg_len])
        row = np.ascontiguousarray(prior[(i // seg_len) * prior.shape[0] // ns]) if prior.ndim == 2 else prior
        cap = int(lib.vcf_cbaac_bound(seg.size))
        out = np.empty(cap, np.uint8)
        nb, bits = ctypes.c_int64(), ctypes.c_int64()
        L.call("vcf_cbaac_encode_prior", seg.ctypes.data, seg.size, order, row.ctypes.data, out.ctypes.data, cap,
               ctypes.byref(nb), ctypes.byref(bits))
        res.append(out[:nb.value].tobytes())
    return res


def host_decode_prior(data: bytes, n: int, prior, order: int = 0) -> np.ndarray:
    prior = check_prior(prior)
    out = np.empty(n, np.uint8)
    buf = np.frombuffer(data, np.uint8)
    L.call("vcf_cbaac_decode_prior", buf.ctypes.data if buf.size else None, buf.size, n, order, prior.ctypes.data,
           out.ctypes.data)
    return out


def prior2d_of(img: np.ndarray, th: int = TILE_2D[0], tw: int = TILE_2D[1], nclass: int = PRIOR_CLASSES) -> np.ndarray:
    """Version 4's (nclass * 16, 256) prior rows of a frame on the host
    (vcf_cbaac2d_prior; what vcf_cbaac_tiled2d_prior_frames computes on the GPU)."""
    img = np.ascontiguousarray(img, np.uint8)
    H, W, C = frame_dims(img.shape)
    rows = np.empty((int(nclass) * NCTX_2D, 256), np.uint16)
    L.call("vcf_cbaac2d_prior", img.ctypes.data, H, W, C, int(th), int(tw), int(nclass), rows.ctypes.data)
    return rows


def host_tiles2d(img: np.ndarray, priors, th: int = TILE_2D[0], tw: int = TILE_2D[1],
                 nclass: int = PRIOR_CLASSES) -> list:
    """The host serial coder (vcf_cbaac2d_encode) over a frame -> its tiles'
    bytes, in tile order: what each tile of a version-4 stream must equal."""
    import ctypes
    img = np.ascontiguousarray(img, np.uint8)
    H, W, C = frame_dims(img.shape)
    priors = check_rows2d(priors, nclass)
    nt = n_tiles2d(img.shape, th, tw)
    cap = nt * int(L.lib().vcf_cbaac_bound(int(th) * int(tw)))
    out = np.empty(max(cap, 1), np.uint8)
    sizes = np.zeros(max(nt, 1), np.int64)
    total = ctypes.c_int64()
    L.call("vcf_cbaac2d_encode", img.ctypes.data, H, W, C, int(th), int(tw), int(nclass), priors.ctypes.data,
           out.ctypes.data, cap, sizes.ctypes.data, ctypes.byref(total))
    ends = np.cumsum(sizes[:nt])
    return [out[int(e - s):int(e)].tobytes() for s, e in zip(sizes[:nt], ends)]


def host_decode2d(payload: bytes, tile_bytes, shape, priors, th: int = TILE_2D[0], tw: int = TILE_2D[1],
                  nclass: int = PRIOR_CLASSES) -> np.ndarray:
    """vcf_cbaac2d_decode: a version-4 payload back to the frame, on the host."""
    H, W, C = frame_dims(shape)
    priors = check_rows2d(priors, nclass)
    tile_bytes = np.asarray(tile_bytes, np.int64)
    offs = np.zeros(tile_bytes.size + 1, np.int64)
    np.cumsum(tile_bytes, out=offs[1:])
    if tile_bytes.size != n_tiles2d(shape, th, tw) or int(offs[-1]) != len(payload):
        raise ValueError("tile sizes do not match the frame or the payload")
    buf = np.frombuffer(payload, np.uint8)
    out = np.empty(tuple(int(s) for s in shape), np.uint8)
    L.call("vcf_cbaac2d_decode", buf.ctypes.data if buf.size else None, offs.ctypes.data, H, W, C, int(th), int(tw),
           int(nclass), priors.ctypes.data, out.ctypes.data)
    return out

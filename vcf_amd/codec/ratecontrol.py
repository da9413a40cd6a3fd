"""Rate control for the 2D-DCT codec: the quantization step per frame that meets a byte budget.

choose_q() is the inverse of `-q`: given frames resident in HBM and a budget
(bytes per frame, or bits per pixel), it bisects the integer step Q of every
frame at once -- one DCT + deadzone encode per probe step and run of equal Q,
then either the index histograms and the zeroth-order estimate of
vcf_amd/rate.py (rate="estimate": nothing but counters leaves the GPU) or
the codec's own entropy stage (rate="coded") -- and always ends with a real
coding pass at the chosen steps, so the bytes it reports are the bytes of
ordinary `-q` files that the existing decoders read.

The search rule (bisect_q) is deterministic.  The rate of a frame is not
strictly monotone in Q, so the contract is the rule's outcome, with two
guarantees: the returned Q met the budget under the rate that was probed, and
q_max comes back with met = False where not even q_max did.

A frame's bytes are its code-stream ({out}{.tif, ...}) plus the 12 bytes of
{out}_shape.bin: what RDE.py sums for /tmp/encoded* and rd_curve reports.
"""
from __future__ import annotations

import io
from dataclasses import dataclass, field

import numpy as np

from .. import dct as D
from .. import distortion as DS
from .. import rate as R
from .._lib import VCF_DCT_NO_SUBBANDS, call
from ..device import DeviceBuffer, Stream
from .dct2d import CoDec as DCTCoDec

SIDE_BYTES = 12          # {out}_shape.bin: struct 'iii'
CORRECTIONS = 8          # exact passes after the first that may raise Q
UNIT_STEPS = 3           # of which the first raise it by one
RATES = ("estimate", "coded")
MAX_GRID = 16            # vcf_index_hist_u8's region grid


def probe_bound(q_min: int, q_max: int) -> int:
    """ceil(log2(q_max - q_min + 1)) + 2: the probes bisect_q may take."""
    return int(q_max - q_min).bit_length() + 2


def bisect_q(rate_fn, budgets, q_min: int = 1, q_max: int = 2048):
    """The search, for n frames at once.  rate_fn(q, active) -> the rate of every frame i with
    active[i] at step q[i] (entries of inactive frames are ignored); budgets: n rates.

    Per frame: probe q_max; a rate over the budget ends the search with (q_max, met = False).
    Probe q_min; a rate within the budget ends it with q_min.  Otherwise lo = q_min (over the
    budget) and hi = q_max (within it): probe (lo + hi) // 2, which becomes hi where it is within the
    budget and lo where not, until hi = lo + 1; the answer is hi.  One call of rate_fn per step
    serves every frame still searching.  -> (q int64[n], met bool[n], rates[n] at q, steps)."""
    budgets = np.asarray(budgets)
    n = len(budgets)
    q_min, q_max = int(q_min), int(q_max)
    if not 1 <= q_min <= q_max:
        raise ValueError(f"1 <= q_min <= q_max (got {q_min}, {q_max})")
    lo, hi = np.full(n, q_min, np.int64), np.full(n, q_max, np.int64)
    q, met = hi.copy(), np.zeros(n, bool)
    steps = 0
    if n == 0:
        return q, met, np.zeros(0, np.int64), steps
    active = np.ones(n, bool)
    r = np.asarray(rate_fn(hi.copy(), active.copy()))
    steps += 1
    got = r.copy()
    met = r <= budgets                       # the frames that do not fit at q_max are done: (q_max, False)
    active = met.copy()
    if q_min < q_max and active.any():
        r = np.asarray(rate_fn(lo.copy(), active.copy()))
        steps += 1
        fits = active & (r <= budgets)
        q[fits], got[fits] = q_min, r[fits]
        active &= ~fits
        while True:
            act = active & (hi > lo + 1)
            if not act.any():
                break
            mid = (lo + hi) // 2
            r = np.asarray(rate_fn(np.where(act, mid, q), act.copy()))
            steps += 1
            fits = act & (r <= budgets)
            over = act & ~fits
            hi[fits], got[fits] = mid[fits], r[fits]
            lo[over] = mid[over]
        q[active] = hi[active]
    assert steps <= probe_bound(q_min, q_max), (steps, q_min, q_max)
    return q, met, got, steps


@dataclass
class RateChoice:
    """choose_q's answer, per frame (arrays of n)."""
    q: np.ndarray                  # int64: the chosen quantization step
    bytes: np.ndarray              # int64: code-stream + SIDE_BYTES, of the real coding pass at q
    rmse: np.ndarray               # float64: against the resident originals (vcf_distortion_u8)
    probes: int                    # probe steps of the bisection (each serves every frame)
    met: np.ndarray = None         # bool: bytes <= budget
    budget: np.ndarray = None      # int64
    corrections: int = 0           # exact passes after the first (rate="estimate" only)
    estimate: np.ndarray = None    # int64: the probed rate at the bisection's Q
    payloads: list = field(default_factory=list, repr=False)   # the code-streams (bytes) of the final pass


def _runs(q, active):
    """(first frame, frames, Q) of every run of consecutive active frames with one Q."""
    out, i, n = [], 0, len(q)
    while i < n:
        if not active[i]:
            i += 1
            continue
        j = i + 1
        while j < n and active[j] and q[j] == q[i]:
            j += 1
        out.append((i, j - i, int(q[i])))
        i = j
    return out


def budgets_of(n, H, W, target_bytes=None, target_bpp=None) -> np.ndarray:
    """The byte budget of every frame: target_bytes (one number or n), or floor(target_bpp * H * W / 8)."""
    if (target_bytes is None) == (target_bpp is None):
        raise ValueError("give exactly one of target_bytes and target_bpp")
    if target_bytes is not None:
        b = np.broadcast_to(np.asarray(target_bytes, np.int64), (n,)).copy()
    else:
        b = np.floor(np.broadcast_to(np.asarray(target_bpp, np.float64), (n,)) * (H * W) / 8.0).astype(np.int64)
    if (b < 0).any():
        raise ValueError("a negative budget")
    return b


class _Session:
    """The buffers and launches of one choose_q call."""

    def __init__(self, frames_dev, n, H, W, codec):
        self.src, self.n, self.H, self.W, self.codec = frames_dev, n, H, W, codec
        self.B, self.flags = codec.block_size, codec.flags
        self.Hp, self.Wp = D.padded_shape(H, W, self.B)
        self.F, self.fb = H * W * 3, self.Hp * self.Wp * 3
        subbands = not (self.flags & VCF_DCT_NO_SUBBANDS) and self.B <= MAX_GRID
        self.regions = (self.B, self.B) if subbands else (1, 1)
        self.st = Stream()
        self.bufs = []
        self.k = self._buf(n * self.fb)
        self.counts = None

    def _buf(self, nbytes):
        b = DeviceBuffer(nbytes)
        self.bufs.append(b)
        return b

    def close(self):
        self.st.synchronize()
        for b in self.bufs:
            b.free()
        self.st.close()

    def encode(self, q, active):
        for s, cnt, Q in _runs(q, active):
            call("vcf_dct_dz_encode", self.src.address(s * self.F), cnt, self.H, self.W, self.B, Q, self.flags,
                 self.k.address(s * self.fb), self.st.handle)

    def estimate(self, q, active):
        """Probe with the histogram kernel: only the counters come back."""
        self.encode(q, active)
        nreg = self.regions[0] * self.regions[1]
        if self.counts is None:
            self.counts = self._buf(self.n * nreg * R.CHANNELS * R.BINS * 4)
        R.histogram_device(self.k, (self.n, self.Hp, self.Wp, 3), self.regions, self.counts, self.st)
        c = np.empty((self.n, nreg, R.CHANNELS, R.BINS), np.uint32)
        self.counts.download(c, self.st)
        self.st.synchronize()
        return R.estimate_bytes(c, "subband") + SIDE_BYTES

    def _tiff_on_gpu(self):
        from .. import zlib_gpu
        from .tiff import TIFFCodec
        return (isinstance(self.codec.entropy, TIFFCodec) and TIFFCodec.gpu_batches
                and zlib_gpu.covers((self.Hp, self.Wp, 3), 1))

    def coded(self, q, active):
        """Probe with the codec's entropy stage: the sizes of the real code-streams."""
        self.encode(q, active)
        if self._tiff_on_gpu():
            from .. import zlib_gpu
            return zlib_gpu.tiff_sizes_device(self.k, self.n, (self.Hp, self.Wp, 3), np.uint8, stream=self.st) + SIDE_BYTES
        sizes = np.zeros(self.n, np.int64)
        for i, p in self.payloads(q, active, encode=False).items():
            sizes[i] = len(p) + SIDE_BYTES
        return sizes

    def payloads(self, q, active, encode=True) -> dict:
        """frame -> the code-stream encode_fn writes at Q = q[frame], for the active frames."""
        if encode:
            self.encode(q, active)
        padded, ent, out = (self.Hp, self.Wp, 3), self.codec.entropy, {}
        if self._tiff_on_gpu():
            from .. import zlib_gpu
            for s, cnt, _ in _runs(np.zeros(self.n, np.int64), active):
                files = zlib_gpu.tiff_frames_device(self.k, cnt, padded, np.uint8, offset=s * self.fb, stream=self.st)
                out.update({s + i: f for i, f in enumerate(files)})
            return out
        self.st.synchronize()
        for i in np.flatnonzero(active):
            if hasattr(ent, "compress_device"):
                cs = ent.compress_device(self.k, padded, offset=int(i) * self.fb)
            else:
                cs = self.codec.compress(self.k.download(np.empty(padded, np.uint8), offset=int(i) * self.fb))
            cs.seek(0)
            out[int(i)] = cs.read()
        return out

    def rmse(self, q):
        rec = self._buf(self.n * self.F)
        dist = self._buf(self.n * 3 * DS.RECORD.itemsize)
        for s, cnt, Q in _runs(q, np.ones(self.n, bool)):
            call("vcf_dct_dz_decode", self.k.address(s * self.fb), cnt, self.H, self.W, self.B, Q, self.flags,
                 rec.address(s * self.F), self.st.handle)
        DS.sse_device(self.src, rec, self.n, self.H, self.W, 3, dist, self.st)
        return DS.records(dist, self.n, 3, self.H * self.W, self.st).rmse()


def _check_codec(codec):
    if not isinstance(codec, DCTCoDec):
        raise NotImplementedError(f"rate control runs on the 2D-DCT codec, not on {type(codec).__name__}")
    if codec.lm is not None:
        raise NotImplementedError("rate control with -a LloydMax: the search moves the deadzone step")


def choose_q(frames_dev: DeviceBuffer, shape, *, target_bytes=None, target_bpp=None, codec, rate: str = "estimate",
             q_min: int = 1, q_max: int = 2048) -> RateChoice:
    """The quantization step of every frame that meets the budget, and the coded result at it.

    frames_dev holds n x H x W x 3 u8 frames (`shape`); `codec` is a dct2d.CoDec, whose -B, -p, -x
    and -c are used and whose -q is ignored.  The budget is target_bytes (one number, or n) or
    target_bpp bits per pixel, counted as in this module's docstring.  rate = "coded" bisects on the
    sizes of the codec's real code-streams: the result is bisect_q's outcome under the true rate.
    rate = "estimate" bisects on rate.estimate_bytes(..., "subband") of the index histograms, then
    codes every frame once; a frame whose real bytes miss the budget has its Q raised -- by one in
    the first UNIT_STEPS passes, then to ceil(Q * bytes / budget) -- and is coded again, CORRECTIONS
    times at most.
    `bytes`, `met` and `payloads` always come from the last real coding pass, `rmse` from
    vcf_distortion_u8 against the frames still resident."""
    if rate not in RATES:
        raise ValueError(f"rate {rate!r}: one of {RATES}")
    _check_codec(codec)
    shape = tuple(int(s) for s in shape)
    if len(shape) == 3:
        shape = (1,) + shape
    if len(shape) != 4 or shape[3] != 3 or min(shape) < 1:
        raise ValueError(f"frames are n x H x W x 3 with n, H, W >= 1, got {shape}")
    n, H, W, _ = shape
    if frames_dev.nbytes < n * H * W * 3:
        raise ValueError("input buffer too small")
    budget = budgets_of(n, H, W, target_bytes, target_bpp)
    s = _Session(frames_dev, n, H, W, codec)
    try:
        q, _, est, probes = bisect_q(s.estimate if rate == "estimate" else s.coded, budget, q_min, q_max)
        everyone = np.ones(n, bool)
        payloads = s.payloads(q, everyone)
        size = np.array([len(payloads[i]) + SIDE_BYTES for i in range(n)], np.int64)
        corrections = 0
        while rate == "estimate" and corrections < CORRECTIONS:
            miss = (size > budget) & (q < q_max)
            if not miss.any():
                break
            # by one at first (the estimate is usually a step or two short); a frame that still misses after
            # UNIT_STEPS passes jumps as if rate were 1 / Q, to ceil(Q * bytes / budget), so that 8 passes suffice
            up = -(-q * size // np.maximum(budget, 1)) if corrections >= UNIT_STEPS else q + 1
            q = np.where(miss, np.minimum(q_max, np.maximum(q + 1, up)), q)
            for i, p in s.payloads(q, miss).items():
                payloads[i], size[i] = p, len(p) + SIDE_BYTES
            corrections += 1
        return RateChoice(q=q, bytes=size, rmse=s.rmse(q), probes=probes, met=size <= budget, budget=budget,
                          corrections=corrections, estimate=np.asarray(est, np.int64),
                          payloads=[payloads[i] for i in range(n)])
    finally:
        s.close()


def choose_q_frames(frames, **kw) -> RateChoice:
    """choose_q for host frames (H x W x 3 or n x H x W x 3 u8): uploaded once, freed afterwards."""
    from .._blockio import frames_u8
    f = frames_u8(frames, "frames")
    buf = DeviceBuffer.from_array(f)
    try:
        return choose_q(buf, f.shape, **kw)
    finally:
        buf.free()


def q_file(out_fn: str) -> str:
    return f"{out_fn}_q.txt"


def write_choice(codec, choice: RateChoice, out_fns, shape) -> list:
    """The files `2D-DCT.py encode -q <chosen> -e out_fn` writes for every frame -- {out_fn}{ext} and
    {out_fn}_shape.bin -- plus {out_fn}_q.txt with the chosen integer.  -> code-stream bytes per frame."""
    sizes = []
    for out_fn, payload, q in zip(out_fns, choice.payloads, choice.q):
        codec._write_side(out_fn, tuple(shape), None)
        sizes.append(codec.encode_write_fn(io.BytesIO(payload), out_fn))
        with open(q_file(out_fn), "w") as f:
            f.write(f"{int(q)}\n")
    return sizes


def read_q(in_fn: str) -> int:
    with open(q_file(in_fn)) as f:
        return int(f.read().strip())


def targets_of(args):
    """(target_bytes, target_bpp) of a parsed command line; both None where rate control is off."""
    return getattr(args, "target_bytes", None), getattr(args, "target_bpp", None)


def encode_files(codec, pairs, args, batch: int = 64) -> list:
    """encode_fns under rate control: (in_fn, out_fn) pairs read, grouped by shape in batches, every
    frame coded at its own chosen Q.  -> code-stream bytes written per frame."""
    tb, tbpp = targets_of(args)
    kw = dict(target_bytes=tb, target_bpp=tbpp, codec=codec, rate=getattr(args, "rate", "estimate"),
              q_min=int(getattr(args, "q_min", 1)), q_max=int(getattr(args, "q_max", 2048)))
    pairs = list(pairs)
    sizes = [0] * len(pairs)
    for b0 in range(0, len(pairs), max(1, int(batch))):
        chunk = list(range(b0, min(len(pairs), b0 + batch)))
        imgs = {i: codec.encode_read_fn(pairs[i][0]) for i in chunk}
        groups = {}
        for i in chunk:
            codec._check_frame(imgs[i])
            groups.setdefault(imgs[i].shape, []).append(i)
        for shape, idx in groups.items():
            choice = choose_q_frames(np.stack([imgs[i] for i in idx]), **kw)
            for i, sz in zip(idx, write_choice(codec, choice, [pairs[i][1] for i in idx], shape)):
                sizes[i] = sz
            codec.original_shape = tuple(shape)
    return sizes


def decode_files(codec, pairs, batch: int = 64) -> list:
    """decode_fns with every frame's Q read from its {in_fn}_q.txt: one decode_fns call per Q."""
    pairs = list(pairs)
    qs = [read_q(p[0]) for p in pairs]
    sizes = [0] * len(pairs)
    kept = codec.QSS
    try:
        for Q in sorted(set(qs)):
            idx = [i for i, q in enumerate(qs) if q == Q]
            codec.QSS = Q
            for i, sz in zip(idx, codec.decode_fns([pairs[i] for i in idx], batch=batch)):
                sizes[i] = sz
    finally:
        codec.QSS = kept
    return sizes


def refuse_unless_dct(args, transform: str) -> None:
    """The new flags on a codec other than 2D-DCT."""
    tb, tbpp = targets_of(args)
    if (tb is not None or tbpp is not None or getattr(args, "q_from_files", False)) and transform != "2D-DCT":
        raise NotImplementedError(f"--target_bpp, --target_bytes and --q_from_files with {transform}: "
                                  "rate control is on the 2D-DCT path only")


class CoDec(DCTCoDec):
    """`rate-control.py`: 2D-DCT.py's encode under a budget; its decode, with --q_from_files at the chosen Q."""

    def encode(self, in_fn=None, out_fn=None):
        in_fn = str(self.args.original) if in_fn is None else in_fn
        out_fn = str(self.args.encoded) if out_fn is None else out_fn
        if targets_of(self.args) == (None, None):
            raise ValueError("rate-control.py encode needs --target_bpp or --target_bytes")
        return encode_files(self, [(in_fn, out_fn)], self.args)[0]

    def decode(self, in_fn=None, out_fn=None):
        in_fn = str(self.args.encoded) if in_fn is None else in_fn
        out_fn = str(self.args.decoded) if out_fn is None else out_fn
        if getattr(self.args, "q_from_files", False):
            self.QSS = read_q(in_fn)
        return self.decode_fn(in_fn, out_fn)

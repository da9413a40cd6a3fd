"""Rate-distortion optimised quantization of the 2D-DCT encode (vcf_dct_rdoq.hip; not in the reference).

vcf_dct_dz_encode_rdoq is vcf_dct_dz_encode with a decision per coefficient: where the extra
distortion is worth less than the bits saved, the index drops by one, or to zero.  The rule is
stated in include/vcf_amd.h; the rate term is a table of costs in bits per (position in the block,
channel, index byte), built here from the exact counts of rate.histogram on the (8, 8) subband grid.
The output is an ordinary index frame: no decoder knows about it.

    cost_table            counts -> add-one smoothed order-0 costs in bits (host, numpy)
    encode_device         the bare call, table in HBM
    encode_frames_device  plain encode -> histogram -> table -> RDOQ encode, one table per frame
    encode                host convenience

There is no CPU path for the encode."""
from __future__ import annotations

import numpy as np

from . import dct as D
from . import rate
from ._blockio import check_input, frames_u8 as _frames, output, round_trip
from ._lib import VCF_DCT_NO_SUBBANDS, call
from .device import DeviceBuffer, _h, synchronize

REGIONS = 64
TABLE = REGIONS * rate.CHANNELS * rate.BINS       # doubles of one frame's table
MAX_ITERATIONS = 4


def cost_table(counts) -> np.ndarray:
    """bits[v] = log2((N + 256) / (c_v + 1)), N the sum of the 256 counts of a frame, region and
    channel: float64 of the counts' shape (n x 64 x 3 x 256 from rate.histogram(..., regions=(8, 8))).
    Add-one smoothing, so a symbol never seen still has a finite cost; one float64 division and
    one np.log2 per entry, so equal counts give equal bits."""
    c = np.asarray(counts)
    if c.ndim < 1 or c.shape[-1] != rate.BINS:
        raise ValueError(f"counts end in {rate.BINS} bins, got shape {c.shape}")
    if c.dtype.kind not in "ui":
        raise TypeError(f"counts are integers, got {c.dtype}")
    total = c.sum(axis=-1, dtype=np.uint64, keepdims=True).astype(np.float64) + float(rate.BINS)
    return np.log2(total / (c.astype(np.float64) + 1.0))


def lambda_of(mu: float, Q: int) -> float:
    """--rdoq MU: the distortion is in squared coefficient units, so lambda scales with Q * Q."""
    mu = float(mu)
    if not np.isfinite(mu) or mu < 0:
        raise ValueError(f"--rdoq {mu}: a finite value >= 0")
    return mu * int(Q) * int(Q)


def encode_device(rgb: DeviceBuffer, n: int, H: int, W: int, Q: int, lam: float, cost: DeviceBuffer,
                  cost_frames: int, flags: int = 0, out: DeviceBuffer | None = None, stream=None) -> DeviceBuffer:
    """n frames resident in HBM -> index frames in HBM (asynchronous on `stream`), the costs read
    from `cost`: float64 cost_frames x 64 x 3 x 256, cost_frames 1 or n."""
    Hp, Wp = D.padded_shape(H, W, 8)
    check_input(rgb, n * H * W * 3)
    out = output(out, n * Hp * Wp * 3)
    call("vcf_dct_dz_encode_rdoq", rgb.ptr, n, H, W, 8, int(Q), flags, cost.ptr, int(cost_frames), cost.nbytes // 8,
         float(lam), out.ptr, _h(stream))
    return out


def encode_frames_device(rgb: DeviceBuffer, n: int, H: int, W: int, Q: int, lam: float, flags: int = 0,
                         iterations: int = 1, out: DeviceBuffer | None = None) -> DeviceBuffer:
    """The two-pass pipeline on the null stream: the plain encode in subband layout (whatever
    `flags` says: the counts per subband do not depend on the layout), its histogram on the (8, 8)
    grid, the counts downloaded, cost_table, the table uploaded, then the RDOQ encode with the
    caller's flags.  Every further iteration (up to 4 in all) rebuilds the table from the RDOQ
    indices in subband layout and codes again."""
    iterations = int(iterations)
    if not 1 <= iterations <= MAX_ITERATIONS:
        raise ValueError(f"iterations = {iterations}: 1 to {MAX_ITERATIONS}")
    Hp, Wp = D.padded_shape(H, W, 8)
    check_input(rgb, n * H * W * 3)
    out = output(out, n * Hp * Wp * 3)
    sub_flags = flags & ~VCF_DCT_NO_SUBBANDS
    # the subband-layout indices the counts are taken from: `out` itself unless the caller wants -x
    scratch = DeviceBuffer(n * Hp * Wp * 3) if flags != sub_flags else None
    idx = out if scratch is None else scratch
    hist = table = None
    counts = np.empty((n, REGIONS, rate.CHANNELS, rate.BINS), np.uint32)
    try:
        D.encode_device(rgb, n, H, W, Q, sub_flags, out=idx)
        for it in range(iterations):
            hist = rate.histogram_device(idx, (n, Hp, Wp, 3), (8, 8), out=hist)
            hist.download(counts)
            bits = np.ascontiguousarray(cost_table(counts))
            if table is None:
                table = DeviceBuffer(bits.nbytes)
            table.upload(bits)
            last = it == iterations - 1
            encode_device(rgb, n, H, W, Q, lam, table, n, flags if last else sub_flags, out=out if last else idx)
        synchronize()     # the table and the scratch are freed below
    finally:
        for b in (scratch, hist, table):
            if b is not None:
                b.free()
    return out


def encode(rgb: np.ndarray, Q: int, lam: float, flags: int = 0, iterations: int = 1) -> np.ndarray:
    """Host convenience, like dct.encode: HxWx3 (or NxHxWx3) u8 -> HpxWpx3 (NxHpxWpx3) u8 indices
    of the two-pass pipeline."""
    f = _frames(rgb, "rgb")
    n, H, W, _ = f.shape
    return round_trip(f, np.asarray(rgb).ndim == 3,
                      lambda din: encode_frames_device(din, n, H, W, Q, lam, flags, iterations),
                      D.padded_shape(H, W, 8) + (3,))

"""Deblocking post-filter of the block-transform decoders on the GPU (-f deblock;
vcf_deblock.hip).  Not in the reference.

vcf_deblock_u8 filters decoded u8 RGB frames across the edges of a B x B block
grid: pass V across the vertical edges, then pass H across the horizontal ones,
per line HEVC's normal filter with the strengths beta and tc; the rule is stated
in include/vcf_amd.h.  (top, left) are the rows and columns of centred padding
the decoder cropped, so the grid is the codec's own.  deblock_device takes and
returns DeviceBuffers, deblock host arrays; default_strength is the rule the
codecs use when --deblock_beta / --deblock_tc are absent.  There is no CPU path.
"""
from __future__ import annotations

import numpy as np

from ._blockio import check_input, frames_u8, output, round_trip
from ._lib import call
from .device import DeviceBuffer, _h

__all__ = ["MIN_BLOCK_SIZE", "default_strength", "strength", "crop_offsets", "deblock_device", "deblock"]

MIN_BLOCK_SIZE = 4      # below it the lines of two edges would overlap


def default_strength(Q: int):
    """(beta, tc) for the quantization step Q: beta = Q, tc = max(1, Q // 8).  An orthonormal
    transform puts Q on HEVC's Qstep scale, whose tables give about these values at Qstep 32."""
    Q = int(Q)
    return Q, max(1, Q // 8)


def strength(Q: int, beta=None, tc=None):
    """(beta, tc): the given values, default_strength(Q) for those that are None."""
    b, t = default_strength(Q)
    beta, tc = (b if beta is None else int(beta)), (t if tc is None else int(tc))
    if beta < 0 or tc < 0:
        raise ValueError(f"--deblock_beta {beta} / --deblock_tc {tc}: values >= 0")
    return beta, tc


def crop_offsets(H: int, W: int, B: int):
    """(top, left) of the centred padding to multiples of B (2D-DCT.py:187-266), which decode crops."""
    return ((-H) % B) // 2, ((-W) % B) // 2


def deblock_device(src: DeviceBuffer, n_frames: int, H: int, W: int, B: int, top: int, left: int, beta: int,
                   tc: int, out: DeviceBuffer | None = None, stream=None, frame_stride: int | None = None,
                   src_offset: int = 0, out_offset: int = 0) -> DeviceBuffer:
    """n frames of H x W x 3 u8 in `src` -> the filtered frames in `out` (a new buffer if None),
    enqueued on `stream`.  Frame f lies frame_stride bytes (default H * W * 3) after frame f - 1,
    the first one src_offset / out_offset bytes into its buffer; the bytes between frames are not
    written.  Out of place: `out` must not be `src`."""
    n, H, W = int(n_frames), int(H), int(W)
    F = H * W * 3
    stride = F if frame_stride is None else int(frame_stride)
    extent = (n - 1) * stride + F if n > 0 else 0
    if min(n, H, W) >= 0 and stride >= F and src_offset >= 0 and out_offset >= 0:
        check_input(src, src_offset + extent)
        out = output(out, out_offset + extent)
    elif out is None:
        out = DeviceBuffer(1)
    call("vcf_deblock_u8", src.address(src_offset), out.address(out_offset), n, H, W, stride, int(B), int(top),
         int(left), int(beta), int(tc), _h(stream))
    return out


def deblock(img, B: int, top: int, left: int, beta: int, tc: int) -> np.ndarray:
    """Host convenience: H x W x 3 (or N x H x W x 3) u8 -> the filtered frame(s)."""
    f = frames_u8(img, "img")
    n, H, W, _ = f.shape
    return round_trip(f, np.asarray(img).ndim == 3,
                      lambda din: deblock_device(din, n, H, W, B, top, left, beta, tc), (H, W, 3))

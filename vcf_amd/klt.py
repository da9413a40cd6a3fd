"""2D-KLT + deadzone hot path on the GPU (include/vcf_amd.h vcf_klt_*).

The reference's src/2D-KLT.py learns, per frame and colour channel, an
eigen-basis of the B x B blocks and codes the coefficients with the deadzone
chain.  On the GPU: the exact second moments of the blocks (vcf_klt_moments),
the fused encode with a given basis (pad, -128, YCoCg, the dense D x D float64
transform, deadzone, +128, wrap, subbands) and the fused decode (down to the
cropped RGB frame).  The D x D eigenproblem runs on the host (numpy.linalg.eigh
on the covariance formed from the integer moments).  2 <= B <= 16.
"""
from __future__ import annotations

import ctypes
import struct

import numpy as np

from ._blockio import check_input, flags_from, frames_u8, output, round_trip
from ._lib import VCF_DCT_NO_SUBBANDS, call
from .device import DeviceBuffer, _h

__all__ = ["padded_shape", "check_blocks", "shape_bin", "flags_from", "moments_device", "encode_device", "decode_device",
           "moments", "covariance", "basis", "train", "encode", "decode", "VCF_DCT_NO_SUBBANDS"]


def padded_shape(H: int, W: int, block_size: int = 8):
    """(Hp, Wp, pad_top, pad_left) of 2D-KLT.py:393-411."""
    v = [ctypes.c_int32() for _ in range(4)]
    call("vcf_klt_padded_shape", H, W, block_size, *[ctypes.byref(x) for x in v])
    return tuple(x.value for x in v)


def check_blocks(H: int, W: int, block_size: int = 8) -> int:
    """The number of blocks N; ValueError where the reference's np.cov gives no D x D matrix (B = 1,
    or a frame of one block), NotImplementedError above B = 16.  Host only."""
    Hp, Wp = padded_shape(H, W, block_size)[:2]
    N = (Hp // block_size) * (Wp // block_size)
    if N < 2:
        raise ValueError(f"{H}x{W} at block size {block_size} is one block: no covariance to learn a basis from")
    return N


def shape_bin(H: int, W: int) -> bytes:
    """The 12 bytes of {out}_shape.bin: 'iii' original shape."""
    return struct.pack("iii", H, W, 3)


def moments_device(rgb: DeviceBuffer, n_frames: int, H: int, W: int, block_size: int = 8,
                   s1: DeviceBuffer | None = None, s2: DeviceBuffer | None = None, stream=None):
    """Frames in HBM -> (S1, S2) in HBM: int64 n x 3 x D and n x 3 x D x D (asynchronous on `stream`)."""
    D = block_size * block_size
    check_input(rgb, n_frames * H * W * 3)
    s1 = output(s1, n_frames * 3 * D * 8)
    s2 = output(s2, n_frames * 3 * D * D * 8)
    call("vcf_klt_moments", rgb.ptr, n_frames, H, W, block_size, s1.ptr, s2.ptr, _h(stream))
    return s1, s2


def encode_device(rgb: DeviceBuffer, n_frames: int, H: int, W: int, weights: DeviceBuffer, Q: int = 32,
                  flags: int = 0, out: DeviceBuffer | None = None, stream=None, block_size: int = 8) -> DeviceBuffer:
    """Frames and float64 weights (n x 3 x D x D) in HBM -> coefficient frames in HBM."""
    Hp, Wp = padded_shape(H, W, block_size)[:2]
    D = block_size * block_size
    check_input(rgb, n_frames * H * W * 3)
    check_input(weights, n_frames * 3 * D * D * 8)
    out = output(out, n_frames * Hp * Wp * 3)
    call("vcf_klt_dz_encode", rgb.ptr, n_frames, H, W, block_size, int(Q), flags, weights.ptr, out.ptr, _h(stream))
    return out


def decode_device(k: DeviceBuffer, n_frames: int, H: int, W: int, weights: DeviceBuffer, Q: int = 32,
                  flags: int = 0, out: DeviceBuffer | None = None, stream=None, block_size: int = 8) -> DeviceBuffer:
    """Coefficient frames and float32 weights (n x 3 x D x D) in HBM -> RGB frames in HBM."""
    Hp, Wp = padded_shape(H, W, block_size)[:2]
    D = block_size * block_size
    check_input(k, n_frames * Hp * Wp * 3)
    check_input(weights, n_frames * 3 * D * D * 4)
    out = output(out, n_frames * H * W * 3)
    call("vcf_klt_dz_decode", k.ptr, n_frames, H, W, block_size, int(Q), flags, weights.ptr, out.ptr, _h(stream))
    return out


def _moments(din: DeviceBuffer, n: int, H: int, W: int, B: int):
    D = B * B
    d1, d2 = moments_device(din, n, H, W, B)
    S1 = d1.download(np.empty((n, 3, D), np.int64))
    S2 = d2.download(np.empty((n, 3, D, D), np.int64))
    d1.free()
    d2.free()
    return S1, S2


def moments(frames: np.ndarray, B: int = 8):
    """HxWx3 (or NxHxWx3) u8 -> (S1 int64 (3, D), S2 int64 (3, D, D)) (or with a leading N): the
    sums over the frame's padded blocks of s = 4 x and s s^T, exact."""
    single = np.asarray(frames).ndim == 3
    f = frames_u8(frames, "rgb")
    n, H, W, _ = f.shape
    check_blocks(H, W, B)
    din = DeviceBuffer.from_array(f)
    S1, S2 = _moments(din, n, H, W, B)
    din.free()
    return (S1[0], S2[0]) if single else (S1, S2)


def covariance(S1: np.ndarray, S2: np.ndarray, N: int) -> np.ndarray:
    """The blocks' covariance (np.cov's N - 1 normalisation) from the integer moments, float64."""
    S1 = S1.astype(np.float64)
    return (S2.astype(np.float64) - S1[..., :, None] * S1[..., None, :] / N) / (16.0 * (N - 1))


def basis(C: np.ndarray) -> np.ndarray:
    """2D-KLT.py:158-167: eigh, rows = eigenvectors by descending eigenvalue."""
    w, v = np.linalg.eigh(C)
    return v[:, np.argsort(w)[::-1]].T


def _train(din: DeviceBuffer, n: int, H: int, W: int, B: int) -> np.ndarray:
    N = check_blocks(H, W, B)
    S1, S2 = _moments(din, n, H, W, B)
    C = covariance(S1, S2, N)
    return np.stack([np.stack([basis(C[i, c]) for c in range(3)]) for i in range(n)])


def train(frames: np.ndarray, B: int = 8) -> np.ndarray:
    """The learned bases, float64 (3, D, D) (or (N, 3, D, D)): moments on the GPU, eigh on the host."""
    single = np.asarray(frames).ndim == 3
    f = frames_u8(frames, "rgb")
    n, H, W, _ = f.shape
    check_blocks(H, W, B)
    din = DeviceBuffer.from_array(f)
    w = _train(din, n, H, W, B)
    din.free()
    return w[0] if single else w


def _weights(w, n: int, B: int, dtype) -> np.ndarray:
    D = B * B
    w = np.asarray(w)
    if w.dtype != dtype:
        raise TypeError(f"weights must be {np.dtype(dtype).name}, got {w.dtype}")
    if w.shape == (3, D, D):
        w = np.broadcast_to(w, (n, 3, D, D))
    if w.shape != (n, 3, D, D):
        raise ValueError(f"weights {w.shape} do not match {(n, 3, D, D)}")
    return np.ascontiguousarray(w)


def encode(frames: np.ndarray, Q: int = 32, flags: int = 0, B: int = 8, weights: np.ndarray | None = None):
    """Host convenience: HxWx3 (or NxHxWx3) u8 -> (HpxWpx3 u8 indices, float64 weights).  The basis is
    trained per frame when `weights` (float64 (3, D, D), or one per frame) is not given."""
    single = np.asarray(frames).ndim == 3
    f = frames_u8(frames, "rgb")
    n, H, W, _ = f.shape
    check_blocks(H, W, B)
    w = None

    def launch(din):
        nonlocal w
        w = _train(din, n, H, W, B) if weights is None else _weights(weights, n, B, np.float64)
        dw = DeviceBuffer.from_array(w)
        return encode_device(din, n, H, W, dw, Q, flags, block_size=B), dw

    res = round_trip(f, single, launch, padded_shape(H, W, B)[:2] + (3,))
    return res, (w[0] if single else w)


def decode(k: np.ndarray, H: int, W: int, Q: int = 32, flags: int = 0, B: int = 8,
           weights32: np.ndarray | None = None, post=None) -> np.ndarray:
    """Host convenience: HpxWpx3 (or N...) u8 indices and the float32 weights of
    {out}_weights.npz -> HxWx3 u8 reconstruction.  post(d, n, H, W) -> (buffer to download, *buffers to
    free) runs on the decoded frames d before the download (-f deblock)."""
    if weights32 is None:
        raise ValueError("decode needs the float32 weights the encoder stored")
    f = frames_u8(k, "k")
    n = f.shape[0]
    check_blocks(H, W, B)
    Hp, Wp = padded_shape(H, W, B)[:2]
    if f.shape[1:3] != (Hp, Wp):
        raise ValueError(f"index frames {f.shape[1:3]} do not match {(Hp, Wp)} for {H}x{W}")
    def launch(din, dw):
        d = decode_device(din, n, H, W, dw, Q, flags, block_size=B)
        return d if post is None else post(d, n, H, W)

    return round_trip(f, np.asarray(k).ndim == 3, launch, (H, W, 3), extra=[_weights(weights32, n, B, np.float32)])

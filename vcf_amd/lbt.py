"""2D-LBT + deadzone hot path on the GPU (include/vcf_amd.h vcf_lbt_*).

The reference's src/2D-LBT.py trains, per frame, a linear autoencoder of the
B x B blocks of all three YCoCg channels (1000 Adam epochs by default) and
codes y = We (x - mean) with the deadzone chain; the decoder matrix Wd and the
scalar mean travel as side information.  On the GPU: the second moments of
the blocks (vcf_lbt_moments, the frame is read once), the whole training from
those moments in one launch with one workgroup per frame (vcf_lbt_train), the
fused encode (pad, -128, YCoCg, - mean, the D x D float32 transform, -p,
deadzone, +128, clip, subbands) and the fused decode (down to the cropped RGB
frame).  2 <= B <= 8.

The reference draws its initial weights (normal, std 0.02) unseeded; here
they come from numpy's PCG64 seeded with 0, the same for every frame, so equal
runs write equal files.
"""
from __future__ import annotations

import ctypes

import numpy as np

from ._blockio import check_input, flags_from, frames_u8, output, round_trip
from ._lib import VCF_DCT_NO_SUBBANDS, VCF_DCT_PERCEPTUAL, call
from .device import DeviceBuffer, _h
from .klt import shape_bin

__all__ = ["padded_shape", "tile_plan", "check_block_size", "shape_bin", "flags_from", "initial_weights", "moments_device",
           "train_device", "encode_device", "decode_device", "moments", "train", "encode", "decode",
           "VCF_DCT_NO_SUBBANDS", "VCF_DCT_PERCEPTUAL"]

EPOCHS = 1000       # 2D-LBT.py:40
LR = 1e-3           # :41
LAMBDA = 1e-6       # :259
INIT_STD = 0.02     # :68-69
INIT_SEED = 0


def check_block_size(B: int) -> None:
    if not 2 <= B <= 8:
        raise NotImplementedError(f"block size {B}: the LBT kernels cover 2 <= B <= 8")


def padded_shape(H: int, W: int, block_size: int = 8):
    """(Hp, Wp, pad_top, pad_left) of 2D-LBT.py:275-317 (the 2D-KLT codec's)."""
    from . import klt
    check_block_size(block_size)
    return klt.padded_shape(H, W, block_size)


def tile_plan(H: int, W: int, block_size: int = 8, decode: bool = False):
    """(TB, lds_class, tiles, moment_chunks, moment_stage_blocks): the blocks of one encode (or
    decode) workgroup, its LDS class 0..2 and the workgroups per frame; the moments kernel's
    workgroups per frame and channel and the blocks one of them stages at a time.  Host only."""
    v = [ctypes.c_int32() for _ in range(5)]
    call("vcf_lbt_tile_plan", H, W, block_size, int(bool(decode)), *[ctypes.byref(x) for x in v])
    return tuple(x.value for x in v)


def rows(H: int, W: int, B: int) -> int:
    """The rows of the training matrix: the blocks of the three channels."""
    Hp, Wp = padded_shape(H, W, B)[:2]
    return 3 * (Hp // B) * (Wp // B)


def initial_weights(B: int, seed: int = INIT_SEED):
    """(We, Wd) float32 (D, D): normal, std 0.02, the encoder drawn first (2D-LBT.py:67-69)."""
    D = B * B
    rng = np.random.Generator(np.random.PCG64(seed))
    we = (rng.standard_normal((D, D)) * INIT_STD).astype(np.float32)
    wd = (rng.standard_normal((D, D)) * INIT_STD).astype(np.float32)
    return we, wd


def moments_device(rgb: DeviceBuffer, n_frames: int, H: int, W: int, block_size: int = 8,
                   s1: DeviceBuffer | None = None, s2: DeviceBuffer | None = None, stream=None):
    """Frames in HBM -> (S1, S2) in HBM: float64 n x D and n x D x D (asynchronous on `stream`)."""
    check_block_size(block_size)
    D = block_size * block_size
    check_input(rgb, n_frames * H * W * 3)
    s1 = output(s1, n_frames * D * 8)
    s2 = output(s2, n_frames * D * D * 8)
    call("vcf_lbt_moments", rgb.ptr, n_frames, H, W, block_size, s1.ptr, s2.ptr, _h(stream))
    return s1, s2


def train_device(s1: DeviceBuffer, s2: DeviceBuffer, n_frames: int, block_size: int, n_rows: int, we: DeviceBuffer,
                 wd: DeviceBuffer, epochs: int = EPOCHS, lr: float = LR, lam: float = LAMBDA,
                 mean: DeviceBuffer | None = None, loss: DeviceBuffer | None = None, stream=None):
    """Moments and initial weights (float32 n x D x D each, updated in place) in HBM -> (mean, loss)
    in HBM: float32 n and n x 3 (loss, MSE, mean log variance at the final weights)."""
    check_block_size(block_size)
    D = block_size * block_size
    check_input(s1, n_frames * D * 8)
    check_input(s2, n_frames * D * D * 8)
    check_input(we, n_frames * D * D * 4)
    check_input(wd, n_frames * D * D * 4)
    mean = output(mean, n_frames * 4)
    loss = output(loss, n_frames * 12)
    call("vcf_lbt_train", s1.ptr, s2.ptr, n_frames, block_size, int(n_rows), int(epochs), float(lr), float(lam),
         we.ptr, wd.ptr, mean.ptr, loss.ptr, _h(stream))
    return mean, loss


def encode_device(rgb: DeviceBuffer, n_frames: int, H: int, W: int, we: DeviceBuffer, mean: DeviceBuffer, Q: int = 32,
                  flags: int = 0, out: DeviceBuffer | None = None, stream=None, block_size: int = 8) -> DeviceBuffer:
    """Frames, float32 encoder matrices (n x D x D) and means (n) in HBM -> coefficient frames in HBM."""
    Hp, Wp = padded_shape(H, W, block_size)[:2]
    D = block_size * block_size
    check_input(rgb, n_frames * H * W * 3)
    check_input(we, n_frames * D * D * 4)
    check_input(mean, n_frames * 4)
    out = output(out, n_frames * Hp * Wp * 3)
    call("vcf_lbt_dz_encode", rgb.ptr, n_frames, H, W, block_size, int(Q), flags, we.ptr, mean.ptr, out.ptr, _h(stream))
    return out


def decode_device(k: DeviceBuffer, n_frames: int, H: int, W: int, wd: DeviceBuffer, mean: DeviceBuffer, Q: int = 32,
                  flags: int = 0, out: DeviceBuffer | None = None, stream=None, block_size: int = 8) -> DeviceBuffer:
    """Coefficient frames, float32 decoder matrices (n x D x D) and means (n) in HBM -> RGB frames in HBM."""
    Hp, Wp = padded_shape(H, W, block_size)[:2]
    D = block_size * block_size
    check_input(k, n_frames * Hp * Wp * 3)
    check_input(wd, n_frames * D * D * 4)
    check_input(mean, n_frames * 4)
    out = output(out, n_frames * H * W * 3)
    call("vcf_lbt_dz_decode", k.ptr, n_frames, H, W, block_size, int(Q), flags, wd.ptr, mean.ptr, out.ptr, _h(stream))
    return out


def moments(frames: np.ndarray, B: int = 8):
    """HxWx3 (or NxHxWx3) u8 -> (S1 float64 (D,), S2 float64 (D, D)) (or with a leading N): the sums of
    x and x x^T over the blocks of the three channels, exact."""
    check_block_size(B)
    single = np.asarray(frames).ndim == 3
    f = frames_u8(frames, "rgb")
    n, H, W, _ = f.shape
    D = B * B
    bufs = [DeviceBuffer.from_array(f)]
    try:
        bufs.extend(moments_device(bufs[0], n, H, W, B))
        S1 = bufs[1].download(np.empty((n, D), np.float64))
        S2 = bufs[2].download(np.empty((n, D, D), np.float64))
    finally:
        for b in bufs:
            b.free()
    return (S1[0], S2[0]) if single else (S1, S2)


def _per_frame(a, n: int, D: int, what: str) -> np.ndarray:
    a = np.asarray(a)
    if a.dtype != np.float32:
        raise TypeError(f"{what} must be float32, got {a.dtype}")
    if a.shape == (D, D):
        a = np.broadcast_to(a, (n, D, D))
    if a.shape != (n, D, D):
        raise ValueError(f"{what} {a.shape} do not match {(n, D, D)}")
    return np.ascontiguousarray(a)


def _means(m, n: int) -> np.ndarray:
    m = np.asarray(m, np.float32).reshape(-1)
    if m.size == 1:
        m = np.broadcast_to(m, (n,))
    if m.shape != (n,):
        raise ValueError(f"{m.size} means for {n} frames")
    return np.ascontiguousarray(m)


def _train(din: DeviceBuffer, n: int, H: int, W: int, B: int, epochs: int = EPOCHS, lr: float = LR,
           lam: float = LAMBDA, init=None):
    """Frames in HBM -> (dWe, dWd, dmean, dloss) in HBM: one moments launch, one train launch.  The
    caller frees the four buffers."""
    D = B * B
    we0, wd0 = initial_weights(B) if init is None else init
    bufs = []
    try:
        s1, s2 = moments_device(din, n, H, W, B)
        bufs += [s1, s2]
        dwe = DeviceBuffer.from_array(_per_frame(we0, n, D, "encoder weights"))
        bufs.append(dwe)
        dwd = DeviceBuffer.from_array(_per_frame(wd0, n, D, "decoder weights"))
        bufs.append(dwd)
        dmean, dloss = train_device(s1, s2, n, B, rows(H, W, B), dwe, dwd, epochs, lr, lam)
    except BaseException:
        for b in bufs:
            b.free()
        raise
    s1.free()
    s2.free()
    return dwe, dwd, dmean, dloss


def train(frames: np.ndarray, B: int = 8, epochs: int = EPOCHS, lr: float = LR, lam: float = LAMBDA, init=None):
    """HxWx3 (or NxHxWx3) u8 -> dict(we, wd float32 (D, D), mean float32, loss float32 (3,)) (or with
    a leading N).  `init` = (We, Wd) float32, one pair or one per frame; default initial_weights(B)."""
    check_block_size(B)
    single = np.asarray(frames).ndim == 3
    f = frames_u8(frames, "rgb")
    n, H, W, _ = f.shape
    D = B * B
    bufs = [DeviceBuffer.from_array(f)]
    try:
        bufs.extend(_train(bufs[0], n, H, W, B, epochs, lr, lam, init))
        res = dict(we=bufs[1].download(np.empty((n, D, D), np.float32)),
                   wd=bufs[2].download(np.empty((n, D, D), np.float32)),
                   mean=bufs[3].download(np.empty(n, np.float32)),
                   loss=bufs[4].download(np.empty((n, 3), np.float32)))
    finally:
        for b in bufs:
            b.free()
    return {k: v[0] for k, v in res.items()} if single else res


def encode(frames: np.ndarray, Q: int = 32, flags: int = 0, B: int = 8, weights=None, mean=None, epochs: int = EPOCHS,
           lr: float = LR, lam: float = LAMBDA, init=None):
    """Host convenience: HxWx3 (or NxHxWx3) u8 -> (HpxWpx3 u8 indices, decoder weights float32 (D, D),
    mean float32).  The model is trained per frame unless the encoder matrix `weights` (float32
    (D, D), or one per frame) and `mean` are given; then they come back as they are."""
    check_block_size(B)
    single = np.asarray(frames).ndim == 3
    f = frames_u8(frames, "rgb")
    n, H, W, _ = f.shape
    D = B * B
    side = {}

    def launch(din):
        if weights is None:
            dwe, dwd, dmean, dloss = made = _train(din, n, H, W, B, epochs, lr, lam, init)
        else:
            if mean is None:
                raise ValueError("an encoder matrix needs the mean it was trained with")
            dwe = DeviceBuffer.from_array(_per_frame(weights, n, D, "encoder weights"))
            made = (dwe,)
            dmean = DeviceBuffer.from_array(_means(mean, n))
            made += (dmean,)
            dwd = dwe
        try:
            dk = encode_device(din, n, H, W, dwe, dmean, Q, flags, block_size=B)
            side["w"] = dwd.download(np.empty((n, D, D), np.float32))
            side["m"] = dmean.download(np.empty(n, np.float32))
        except BaseException:
            for b in made:
                b.free()
            raise
        return (dk,) + tuple(made)

    res = round_trip(f, single, launch, padded_shape(H, W, B)[:2] + (3,))
    return (res, side["w"][0], side["m"][0]) if single else (res, side["w"], side["m"])


def decode(k: np.ndarray, H: int, W: int, Q: int = 32, flags: int = 0, B: int = 8, weights=None, mean=None,
           post=None):
    """Host convenience: HpxWpx3 (or N...) u8 indices, the float32 decoder matrix and the mean of
    {out}.weights.pth -> HxWx3 u8 reconstruction.  post(d, n, H, W) -> (buffer to download, *buffers to
    free) runs on the decoded frames d before the download (-f deblock)."""
    check_block_size(B)
    if weights is None or mean is None:
        raise ValueError("decode needs the decoder matrix and the mean the encoder stored")
    f = frames_u8(k, "k")
    n = f.shape[0]
    Hp, Wp = padded_shape(H, W, B)[:2]
    if f.shape[1:3] != (Hp, Wp):
        raise ValueError(f"index frames {f.shape[1:3]} do not match {(Hp, Wp)} for {H}x{W}")
    def launch(din, dw, dm):
        d = decode_device(din, n, H, W, dw, dm, Q, flags, block_size=B)
        return d if post is None else post(d, n, H, W)

    return round_trip(f, np.asarray(k).ndim == 3, launch, (H, W, 3),
                      extra=[_per_frame(weights, n, B * B, "decoder weights"), _means(mean, n)])

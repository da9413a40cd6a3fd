"""The 2D-KLT codec restated in numpy, for the tests.

Written from the arithmetic of the reference's 2D-KLT encode_fn/decode_fn (a
Karhunen-Loeve basis of the B x B blocks learned per colour channel, over
YCoCg, deadzone, uint8 indices):

  encode  u8 RGB -> float32 -> centred zero pad to multiples of B (the smaller
          half above and left) -> -128 (pad pixels become -128) -> YCoCg
          (float32, every value a multiple of 1/4) -> per channel X = the N x D
          matrix of blocks (raster order, row-major inside a block, D = B^2)
          -> coef = X W^T in float64 (row k of W = basis vector k) -> subbands
          -> int32(coef / Q) (float64 division, truncated) + 128 -> u8, WRAPPED
  train   C = np.cov(X, rowvar=False) (float64), eigh, rows by descending
          eigenvalue
  decode  u8 -> int16 - 128 -> Q k (int16) -> blocks -> rec = Y W with the
          float32 weights of {out}_weights.npz -> crop -> RGB -> +128 -> clip
          -> u8 (truncated)

The reference multiplies through BLAS, whose order is unspecified; `order`
picks the accumulation order of the sums here ("fwd": ascending, "rev":
descending).  The decode runs in float64 (weights widened: what the GPU does)
or in float32 (what the reference does); the fixtures are the cases where all
of these agree.  moments() restates the integer second-moment reduction of the
product's training path.
"""
import struct

import numpy as np

NO_SUBBANDS = 1


def padded_shape(H, W, B):
    """(Hp, Wp, pad_top, pad_left)."""
    Hp = (H + B - 1) // B * B
    Wp = (W + B - 1) // B * B
    return Hp, Wp, (Hp - H) // 2, (Wp - W) // 2


def shape_bin(H, W):
    """The 12 bytes of {out}_shape.bin."""
    return struct.pack("iii", H, W, 3)


def n_blocks(H, W, B):
    Hp, Wp = padded_shape(H, W, B)[:2]
    return (Hp // B) * (Wp // B)


def check(H, W, B):
    """The two cases in which the reference's np.cov gives no D x D matrix."""
    if B < 2:
        raise ValueError("block size 1: the covariance of one-sample blocks is a scalar")
    if n_blocks(H, W, B) < 2:
        raise ValueError("a frame of one block has no covariance")


def to_patches(img, B):
    """(Hp, Wp, 3) -> (3, N, D)."""
    Hp, Wp = img.shape[:2]
    return img.reshape(Hp // B, B, Wp // B, B, 3).transpose(4, 0, 2, 1, 3).reshape(3, -1, B * B)


def from_patches(p, Hp, Wp, B):
    """(3, N, D) -> (Hp, Wp, 3)."""
    return p.reshape(3, Hp // B, Wp // B, B, B).transpose(1, 3, 2, 4, 0).reshape(Hp, Wp, 3)


def blocks(rgb, B):
    """The float32 YCoCg blocks X, (3, N, D)."""
    H, W = rgb.shape[:2]
    check(H, W, B)
    Hp, Wp, top, left = padded_shape(H, W, B)
    img = np.pad(rgb.astype(np.float32), ((top, Hp - H - top), (left, Wp - W - left), (0, 0)))
    img -= 128
    R, G, Bl = img[..., 0], img[..., 1], img[..., 2]
    ct = np.empty_like(img)
    ct[..., 0] = R / 4 + G / 2 + Bl / 4
    ct[..., 1] = R / 2 - Bl / 2
    ct[..., 2] = -R / 4 + G / 2 - Bl / 4
    return to_patches(ct, B)


def moments(rgb, B):
    """(S1 int64 (3, D), S2 int64 (3, D, D)): sums over the blocks of s = 4 x and s s^T."""
    X = blocks(rgb, B)
    S = (X * 4).astype(np.int64)
    assert np.array_equal(S, X.astype(np.float64) * 4)
    return S.sum(1), np.einsum("cni,cnj->cij", S, S)


def covariance(rgb, B):
    """np.cov of the blocks, as the reference forms it: float64 (3, D, D)."""
    return np.stack([np.cov(x, rowvar=False) for x in blocks(rgb, B)])


def covariance_from_moments(S1, S2, N):
    """The product's host formula, float64."""
    S1 = S1.astype(np.float64)
    return (S2.astype(np.float64) - S1[..., :, None] * S1[..., None, :] / N) / (16.0 * (N - 1))


def basis(C):
    """eigh of one covariance matrix; rows = eigenvectors, largest eigenvalue first."""
    w, v = np.linalg.eigh(C)
    return v[:, np.argsort(w)[::-1]].T


def train(rgb, B):
    """float64 (3, D, D), as the reference trains."""
    return np.stack([basis(c) for c in covariance(rgb, B)])


def to_subbands(a, B):
    Hp, Wp = a.shape[:2]
    return a.reshape(Hp // B, B, Wp // B, B, -1).transpose(1, 0, 3, 2, 4).reshape(a.shape)


def to_blocks(a, B):
    Hp, Wp = a.shape[:2]
    return a.reshape(B, Hp // B, B, Wp // B, -1).transpose(1, 0, 3, 2, 4).reshape(a.shape)


def _order(n, order):
    return range(n) if order == "fwd" else range(n - 1, -1, -1)


def encode(rgb, weights64, B=8, Q=32, flags=0, order="fwd"):
    """dict(k, pre): the u8 indices in their final layout and the float64 coefficients
    before the division (final layout)."""
    H, W = rgb.shape[:2]
    Hp, Wp = padded_shape(H, W, B)[:2]
    X = blocks(rgb, B).astype(np.float64)
    Wt = np.asarray(weights64, np.float64)
    D = B * B
    assert Wt.shape == (3, D, D)
    acc = np.zeros_like(X)
    for j in _order(D, order):
        acc = acc + X[:, :, j, None] * Wt[:, None, :, j]
    pre = from_patches(acc, Hp, Wp, B)
    if not flags & NO_SUBBANDS:
        pre = to_subbands(pre, B)
    k = (pre / Q).astype(np.int32) + 128
    return dict(k=k.astype(np.uint8), k32=k, pre=pre)


def decode(k, H, W, weights32, B=8, Q=32, flags=0, order="fwd", dtype=np.float64):
    """dict(rgb, pre): the decoded u8 frame and the pixel values before clip and truncation,
    both in `dtype` arithmetic (float64: weights widened; float32: the reference's)."""
    Hp, Wp, top, left = padded_shape(H, W, B)
    assert k.shape == (Hp, Wp, 3) and k.dtype == np.uint8
    w = np.asarray(weights32)
    assert w.dtype == np.float32
    y = (Q * (k.astype(np.int32) - 128)).astype(np.int16)    # int16 arithmetic wraps
    if not flags & NO_SUBBANDS:
        y = to_blocks(y, B)
    Y = to_patches(y, B).astype(dtype)
    Wt = w.astype(dtype)
    acc = np.zeros(Y.shape, dtype)
    for kk in _order(B * B, order):
        acc = acc + Y[:, :, kk, None] * Wt[:, None, kk, :]
    c = from_patches(acc, Hp, Wp, B)[top:top + H, left:left + W]
    Yc, Co, Cg = c[..., 0], c[..., 1], c[..., 2]
    pre = np.stack([Yc + Co - Cg, Yc + Cg, Yc - Co - Cg], -1) + dtype(128)
    return dict(rgb=np.clip(pre, 0, 255).astype(np.uint8), pre=pre)


def synth_frame(H, W, seed):
    """A deterministic frame with smooth content, texture and a few saturated pixels."""
    rng = np.random.Generator(np.random.PCG64(seed))
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    ch = [128 + 70 * np.sin(x / 23 + c) + 60 * np.cos(y / 17 - c) + rng.normal(0, 12, (H, W)) for c in range(3)]
    return np.clip(np.rint(np.stack(ch, -1)), 0, 255).astype(np.uint8)


def midsize_frame():
    """256 x 320: many tiles in both directions."""
    return synth_frame(256, 320, 77)


def index_margin(pre, Q):
    """Distance of pre / Q (float64, before truncation) to the nearest nonzero integer, the
    deadzone quantizer's thresholds (the wrap to u8 adds none), per position."""
    t = np.abs(pre / Q)
    r = np.maximum(np.rint(t), 1.0)
    return np.abs(t - r)


def pixel_margin(pre):
    """Distance of the float64 pixel values to the nearest of 1, 2, ..., 255: the values at which
    clip-then-truncate steps (below 1 everything gives 0)."""
    pre = pre.astype(np.float64)
    return np.abs(pre - np.clip(np.rint(pre), 1, 255))

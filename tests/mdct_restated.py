"""The lapped 2D-MDCT codec restated in numpy, for the tests.

Written from the arithmetic of the reference's 2D-MDCT encode_fn/decode_fn
(Malvar's lapped transform over YCoCg, deadzone, uint8 indices), vectorised
over blocks instead of looping over rows, columns and blocks:

  encode  u8 RGB -> float32 -> centred symmetric pad to ceil((dim + 2B)/B)*B
          -> -128 -> YCoCg (float32) -> float64 -> every row, then every
          column: extend the line by N = B samples (symmetric), 2N samples at
          hop N, times the sine window, X[k] = sum_n cos(pi/N (n + (N+1)/2)
          (k + 1/2)) x[n] -> float32 -> / scale -> -p weights -> subbands
          -> (x / Q) truncated -> +128 -> clip to [0, 255] -> u8
  decode  u8 -> int16 - 128 -> Q k (int16) -> blocks -> -p -> float64 ->
          every column, then every row: per block dot * 2 / N, times the
          window, overlap-added into a zero line of L + 2N, [N : N + L] kept
          -> float32 -> * scale -> RGB (float32) -> crop -> +128 -> clip ->
          u8 (truncated)

The reference sums through BLAS, whose order is unspecified; `order` picks
the accumulation order of the float64 sums here ("fwd": n ascending, "rev":
n descending), so a test can tell which outputs depend on it.  Besides the
indices and the decoded frame, the float64 and float32 coefficients before
the quantizer and the pixel values before the truncation are returned.
"""
import struct

import numpy as np

NO_SUBBANDS = 1
PERCEPTUAL = 2

Y_QSS = np.array([[16, 11, 10, 16, 24, 40, 51, 61], [12, 12, 14, 19, 26, 58, 60, 55],
                  [14, 13, 16, 24, 40, 57, 69, 56], [14, 17, 22, 29, 51, 87, 80, 62],
                  [18, 22, 37, 56, 68, 109, 103, 77], [24, 35, 55, 64, 81, 104, 113, 92],
                  [49, 64, 78, 87, 103, 121, 120, 101], [72, 92, 95, 98, 112, 100, 103, 99]], np.float32)
C_QSS = np.array([[17, 18, 24, 47, 99, 99, 99, 99], [18, 21, 26, 66, 99, 99, 99, 99],
                  [24, 26, 56, 99, 99, 99, 99, 99], [47, 66, 99, 99, 99, 99, 99, 99]] + [[99] * 8] * 4, np.float32)


def padded_shape(H, W, B):
    """(Hp, Wp, pad_top, pad_left): one extra block of context on every side."""
    Hp = (H + 2 * B + B - 1) // B * B
    Wp = (W + 2 * B + B - 1) // B * B
    return Hp, Wp, (Hp - H) // 2, (Wp - W) // 2


def shape_bin(H, W, B):
    """The 20 bytes of {out}_shape.bin."""
    _, _, top, left = padded_shape(H, W, B)
    return struct.pack("iii", H, W, 3) + struct.pack("ii", top, left)


def scale_factor(B):
    if B <= 8:
        return B / 2.0
    if B >= 32:
        return B / 4.0
    return 4.0 + (B - 8) / 24 * 4.0


def tables(N):
    """(window[2N], cos[N, 2N]) in float64."""
    n = np.arange(2 * N)
    k = np.arange(N)
    win = np.sin(np.pi * (n + 0.5) / (2 * N))
    cos = np.cos(np.pi / N * (n + (N + 1) / 2) * (k[:, None] + 0.5))
    return win, cos


def weights():
    """-p at B = 8: (3, 8, 8) float32 QSS / max per channel."""
    wy = Y_QSS / np.max(Y_QSS)
    wc = C_QSS / np.max(C_QSS)
    return np.stack([wy, wc, wc]).astype(np.float32)


def _order(n, order):
    return range(n) if order == "fwd" else range(n - 1, -1, -1)


def analyze_last(x, N, order="fwd"):
    """MDCT analysis along the last axis of a float64 array."""
    win, cos = tables(N)
    L = x.shape[-1]
    nb = L // N
    ext = np.pad(x, [(0, 0)] * (x.ndim - 1) + [(N, N)], mode="symmetric")
    idx = np.arange(nb)[:, None] * N + np.arange(2 * N)[None, :]
    blk = ext[..., idx] * win                      # (..., nb, 2N): the window product first
    acc = np.zeros(x.shape[:-1] + (nb, N))
    for n in _order(2 * N, order):
        acc = acc + blk[..., n, None] * cos[:, n]
    return acc.reshape(x.shape[:-1] + (L,))


def synthesize_last(X, N, order="fwd"):
    """MDCT synthesis along the last axis: no boundary extension; the first N
    samples get blocks 0 and 1, the last N only the last block."""
    win, cos = tables(N)
    L = X.shape[-1]
    nb = L // N
    Xb = X.reshape(X.shape[:-1] + (nb, N))
    acc = np.zeros(X.shape[:-1] + (nb, 2 * N))
    for k in _order(N, order):
        acc = acc + Xb[..., k, None] * cos[k, :]
    blk = acc * 2 / N
    blk = blk * win
    out = np.zeros(X.shape[:-1] + (nb, N))
    out += blk[..., N:]                             # block s: its second half
    out[..., :-1, :] += blk[..., 1:, :N]            # block s + 1: its first half
    return out.reshape(X.shape[:-1] + (L,))


def to_subbands(a, B):
    Hp, Wp = a.shape[:2]
    return a.reshape(Hp // B, B, Wp // B, B, -1).transpose(1, 0, 3, 2, 4).reshape(a.shape)


def to_blocks(a, B):
    Hp, Wp = a.shape[:2]
    return a.reshape(B, Hp // B, B, Wp // B, -1).transpose(1, 0, 3, 2, 4).reshape(a.shape)


def _tile_weights(Hp, Wp):
    return np.tile(weights().transpose(1, 2, 0), (Hp // 8, Wp // 8, 1))


def encode(rgb, B=8, Q=32, flags=0, order="fwd"):
    """dict(k, coef64, coef32, pre): the u8 indices in their final layout, the
    float64 MDCT coefficients (block layout), the float32 values handed to the
    quantizer (final layout) and coef64 carried through the same steps in
    float64 (final layout), for threshold distances."""
    if (flags & PERCEPTUAL) and B != 8:
        raise NotImplementedError("-p is pinned at B = 8 only")
    H, W = rgb.shape[:2]
    Hp, Wp, top, left = padded_shape(H, W, B)
    img = np.pad(rgb.astype(np.float32), ((top, Hp - H - top), (left, Wp - W - left), (0, 0)), mode="symmetric")
    img -= 128
    R, G, Bl = img[..., 0], img[..., 1], img[..., 2]
    ct = np.empty_like(img)
    ct[..., 0] = R / 4 + G / 2 + Bl / 4
    ct[..., 1] = R / 2 - Bl / 2
    ct[..., 2] = -R / 4 + G / 2 - Bl / 4
    x = ct.astype(np.float64).transpose(2, 0, 1)             # (3, Hp, Wp)
    x = analyze_last(x, B, order)                              # rows
    x = analyze_last(x.transpose(0, 2, 1), B, order).transpose(0, 2, 1)   # columns
    coef64 = x.transpose(1, 2, 0)
    scale = np.float32(scale_factor(B))
    c32 = coef64.astype(np.float32) / scale
    c64 = coef64 / np.float64(scale)
    if flags & PERCEPTUAL:
        w = _tile_weights(Hp, Wp)
        c32 = c32 * w
        c64 = c64 * w.astype(np.float64)
    if not flags & NO_SUBBANDS:
        c32, c64 = to_subbands(c32, B), to_subbands(c64, B)
    k = (c32 / np.float32(Q)).astype(np.int32) + 128
    return dict(k=np.clip(k, 0, 255).astype(np.uint8), coef64=coef64, coef32=c32, pre=c64)


def decode(k, H, W, B=8, Q=32, flags=0, order="fwd"):
    """dict(rgb, pix64, pre32, pre): the decoded u8 frame, the float64 synthesis
    output (padded frame, YCoCg), the float32 pixel values before clip and
    truncation, and the same carried in float64."""
    if (flags & PERCEPTUAL) and B != 8:
        raise NotImplementedError("-p is pinned at B = 8 only")
    Hp, Wp, top, left = padded_shape(H, W, B)
    assert k.shape == (Hp, Wp, 3) and k.dtype == np.uint8
    y = (Q * (k.astype(np.int32) - 128)).astype(np.int16)    # int16 arithmetic wraps
    if not flags & NO_SUBBANDS:
        y = to_blocks(y, B)
    if flags & PERCEPTUAL:
        y = y.astype(np.float32) / _tile_weights(Hp, Wp)
    x = y.astype(np.float64).transpose(2, 0, 1)
    x = synthesize_last(x.transpose(0, 2, 1), B, order).transpose(0, 2, 1)   # columns first
    x = synthesize_last(x, B, order)                                          # then rows
    pix64 = x.transpose(1, 2, 0)
    scale = np.float32(scale_factor(B))
    out = []
    for t, off in ((np.float32, np.float32(128)), (np.float64, np.float64(128))):
        c = pix64.astype(t) * t(scale)
        Y, Co, Cg = c[..., 0], c[..., 1], c[..., 2]
        p = np.stack([Y + Co - Cg, Y + Cg, Y - Co - Cg], -1)
        out.append(p[top:top + H, left:left + W] + off)
    pre32, pre = out
    return dict(rgb=np.clip(pre32, 0, 255).astype(np.uint8), pix64=pix64, pre32=pre32, pre=pre)


def synth_frame(H, W, seed):
    """A deterministic frame with smooth content, texture and a few saturated pixels."""
    rng = np.random.Generator(np.random.PCG64(seed))
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    ch = [128 + 70 * np.sin(x / 23 + c) + 60 * np.cos(y / 17 - c) + rng.normal(0, 12, (H, W)) for c in range(3)]
    return np.clip(np.rint(np.stack(ch, -1)), 0, 255).astype(np.uint8)


def midsize_frame():
    """256 x 320: crosses tile boundaries in both directions, with a partial last tile."""
    return synth_frame(256, 320, 77)


def index_margin(pre, Q):
    """Distance of pre / Q (float64, before truncation) to the nearest nonzero
    integer, the deadzone quantizer's thresholds, per position."""
    t = np.abs(pre / Q)
    r = np.maximum(np.rint(t), 1.0)
    return np.abs(t - r)


def pixel_margin(pre):
    """Distance of the float64 pixel values to the nearest of 1, 2, ..., 255: the
    values at which clip-then-truncate steps (below 1 everything gives 0)."""
    return np.abs(pre - np.clip(np.rint(pre), 1, 255))

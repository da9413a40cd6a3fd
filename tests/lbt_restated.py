"""The 2D-LBT codec restated in numpy, for the tests.

Written from the arithmetic of the reference's 2D-LBT.py (a linear
autoencoder of the B x B blocks, trained per image with Adam, over YCoCg,
deadzone, uint8 indices), in its own ROW-WISE form: the N x D forward pass,
the loss, the gradients by the chain rule through the rows, and torch's Adam.
The product trains from the D x D second moments instead; nothing here uses
that algebra, so the two check each other.

  blocks  u8 RGB -> centred zero pad to multiples of B -> -128 -> YCoCg ->
          the blocks of channel 0, then 1, then 2 (raster order, row-major
          inside a block) as one N x D matrix, N = 3 x blocks, D = B^2 ->
          minus ONE scalar mean over all of it
  train   x^ = (X We^T) Wd^T;  loss = mean((x^ - X)^2) + lambda mean_j
          log(var_j(X We^T) + 1e-6), var biased over the N rows;  `epochs`
          steps of Adam (beta 0.9 / 0.999, eps 1e-8, torch's bias correction)
          over both matrices
  encode  y = X We^T in float32 -> [-p: float32(float64(y) QSSs / 121 or 99)]
          -> subbands unless -x -> int32(y / Q) (float32 division, truncated)
          + 128 -> clip 0..255 -> u8
  decode  u8 -> int16 - 128 -> Q k (int16) -> blocks -> [-p: int16(float64 /
          weight)] -> float32 -> Y Wd^T + mean -> crop -> RGB, + 128 (float32)
          -> clip -> u8 (truncated)

Training runs in float64 here (`dtype` float32 gives torch's arithmetic up to
the order of the sums); encode and decode return the float64 value of the
quantity that is rounded last, for the tests' boundary sets.
"""
import struct

import numpy as np

NO_SUBBANDS = 1
PERCEPTUAL = 2

Y_QSS = np.array([[16, 11, 10, 16, 24, 40, 51, 61], [12, 12, 14, 19, 26, 58, 60, 55],
                  [14, 13, 16, 24, 40, 57, 69, 56], [14, 17, 22, 29, 51, 87, 80, 62],
                  [18, 22, 37, 56, 68, 109, 103, 77], [24, 35, 55, 64, 81, 104, 113, 92],
                  [49, 64, 78, 87, 103, 121, 120, 101], [72, 92, 95, 98, 112, 100, 103, 99]], np.uint8)
C_QSS = np.full((8, 8), 99, np.uint8)
C_QSS[:4, :4] = [[17, 18, 24, 47], [18, 21, 26, 66], [24, 26, 56, 99], [47, 66, 99, 99]]


def padded_shape(H, W, B):
    """(Hp, Wp, pad_top, pad_left)."""
    Hp = (H + B - 1) // B * B
    Wp = (W + B - 1) // B * B
    return Hp, Wp, (Hp - H) // 2, (Wp - W) // 2


def shape_bin(H, W):
    return struct.pack("iii", H, W, 3)


def to_patches(img, B):
    """(Hp, Wp, 3) -> (3 n, D), channel-major."""
    Hp, Wp = img.shape[:2]
    return img.reshape(Hp // B, B, Wp // B, B, 3).transpose(4, 0, 2, 1, 3).reshape(-1, B * B)


def from_patches(p, Hp, Wp, B):
    """(3 n, D) -> (Hp, Wp, 3)."""
    return p.reshape(3, Hp // B, Wp // B, B, B).transpose(1, 3, 2, 4, 0).reshape(Hp, Wp, 3)


def blocks(rgb, B):
    """The float32 YCoCg blocks before the mean is taken off, (N, D)."""
    H, W = rgb.shape[:2]
    Hp, Wp, top, left = padded_shape(H, W, B)
    img = np.pad(rgb.astype(np.float64), ((top, Hp - H - top), (left, Wp - W - left), (0, 0)))
    img -= 128
    R, G, Bl = img[..., 0], img[..., 1], img[..., 2]
    ct = np.stack([R / 4 + G / 2 + Bl / 4, R / 2 - Bl / 2, -R / 4 + G / 2 - Bl / 4], -1)
    return to_patches(ct, B).astype(np.float32)


def mean_of(rgb, B):
    """The scalar mean as a float32 value (the exact mean, rounded once)."""
    return np.float32(blocks(rgb, B).astype(np.float64).mean())


def centred(rgb, B, mean):
    """X = blocks - mean, in float32 as the reference forms it."""
    return blocks(rgb, B) - np.float32(mean)


# ---- training, row-wise -------------------------------------------------------
def loss_terms(X, We, Wd, lam=1e-6):
    """(loss, mse, mean log variance) of the rows X under the two matrices, in X's dtype."""
    Y = X @ We.T
    diff = Y @ Wd.T - X
    mse = np.mean(diff * diff)
    gain = np.mean(np.log(np.var(Y, axis=0) + 1e-6))
    return mse + lam * gain, mse, gain


def gradients(X, We, Wd, lam=1e-6):
    """d loss / d We, d loss / d Wd by the chain rule through the N rows."""
    N, D = X.shape
    Y = X @ We.T
    diff = Y @ Wd.T - X
    dXh = diff * (2.0 / (N * D))
    gWd = dXh.T @ Y
    dY = dXh @ Wd
    if lam > 0:
        Yc = Y - Y.mean(axis=0)
        var = np.mean(Yc * Yc, axis=0) + 1e-6
        dY = dY + Yc * (2.0 * lam / (N * D)) / var
    return dY.T @ X, gWd


def train(X, We0, Wd0, epochs, lr=1e-3, lam=1e-6, dtype=np.float64):
    """`epochs` Adam steps from (We0, Wd0) -> (We, Wd) in `dtype`."""
    X = np.asarray(X, dtype)
    W = [np.array(We0, dtype), np.array(Wd0, dtype)]
    m = [np.zeros_like(w) for w in W]
    v = [np.zeros_like(w) for w in W]
    b1, b2, eps = 0.9, 0.999, 1e-8
    for t in range(1, epochs + 1):
        g = gradients(X, W[0], W[1], lam)
        step = dtype(lr / (1 - b1 ** t))
        bc2 = dtype((1 - b2 ** t) ** 0.5)
        for i in range(2):
            m[i] = m[i] + (g[i] - m[i]) * dtype(1 - b1)
            v[i] = v[i] * dtype(b2) + dtype(1 - b2) * g[i] * g[i]
            W[i] = W[i] - step * (m[i] / (np.sqrt(v[i]) / bc2 + dtype(eps)))
    return W[0], W[1]


# ---- the -p tables ----------------------------------------------------------
def perceptual_weights(B, tables=None):
    """(2, D) float64: Y_QSSs / 121 and C_QSSs / 99.  B = 8 needs no resize; for another B pass the
    resized uint8 tables (the reference resizes with OpenCV)."""
    if tables is None:
        if B != 8:
            raise ValueError("the resized tables of B != 8 must be given")
        tables = (Y_QSS, C_QSS)
    return np.stack([np.asarray(tables[0], np.uint8).reshape(-1) / 121, np.asarray(tables[1], np.uint8).reshape(-1) / 99])


def to_subbands(a, B):
    Hp, Wp = a.shape[:2]
    return a.reshape(Hp // B, B, Wp // B, B, -1).transpose(1, 0, 3, 2, 4).reshape(a.shape)


def to_blocks(a, B):
    Hp, Wp = a.shape[:2]
    return a.reshape(B, Hp // B, B, Wp // B, -1).transpose(1, 0, 3, 2, 4).reshape(a.shape)


def _channel_weights(pw, n_rows):
    """(N, D): row r belongs to channel r // (N / 3); luma rows get pw[0], chroma rows pw[1]."""
    n = n_rows // 3
    return np.concatenate([np.broadcast_to(pw[0], (n, pw.shape[1])), np.broadcast_to(pw[1], (2 * n, pw.shape[1]))])


# ---- encode / decode --------------------------------------------------------
def encode(rgb, We, mean, B=8, Q=32, flags=0, tables=None):
    """dict(k, pre, mag): the u8 indices in their final layout, the float64 value of y / Q before the
    truncation (from a float64 product) and sum_j |We[k][j] x[j]| / Q per position, the magnitude
    a float32 product's rounding error scales with."""
    H, W = rgb.shape[:2]
    Hp, Wp = padded_shape(H, W, B)[:2]
    X = centred(rgb, B, mean)
    We = np.asarray(We, np.float32)
    y32 = X @ We.T
    y64 = X.astype(np.float64) @ We.astype(np.float64).T
    mag = np.abs(X).astype(np.float64) @ np.abs(We).astype(np.float64).T
    if flags & PERCEPTUAL:
        cw = _channel_weights(perceptual_weights(B, tables), X.shape[0])
        y32 = (y32.astype(np.float64) * cw).astype(np.float32)
        y64, mag = y64 * cw, mag * cw
    out = []
    for a in (y32, y64, mag):
        a = from_patches(a, Hp, Wp, B)
        out.append(a if flags & NO_SUBBANDS else to_subbands(a, B))
    k = (out[0] / np.float32(Q)).astype(np.int32) + 128
    return dict(k=np.clip(k, 0, 255).astype(np.uint8), pre=out[1] / Q, mag=out[2] / Q)


def decode(k, H, W, Wd, mean, B=8, Q=32, flags=0, tables=None):
    """dict(rgb, pre, mag): the decoded u8 frame, the float64 pixel values before clip and truncation
    and, per pixel, the magnitude of the terms summed (for a float32 error bound)."""
    Hp, Wp, top, left = padded_shape(H, W, B)
    assert k.shape == (Hp, Wp, 3) and k.dtype == np.uint8
    Wd = np.asarray(Wd, np.float32)
    y = (Q * (k.astype(np.int32) - 128)).astype(np.int16)    # int16 arithmetic wraps
    if not flags & NO_SUBBANDS:
        y = to_blocks(y, B)
    Y = to_patches(y, B)
    if flags & PERCEPTUAL:
        cw = _channel_weights(perceptual_weights(B, tables), Y.shape[0])
        Y = (Y.astype(np.float64) / cw).astype(np.int16)
    m32 = np.float32(mean)
    x32 = Y.astype(np.float32) @ Wd.T + m32
    x64 = Y.astype(np.float64) @ Wd.astype(np.float64).T + float(m32)
    mag = np.abs(Y).astype(np.float64) @ np.abs(Wd).astype(np.float64).T + abs(float(m32))

    def rgb_of(x):
        c = from_patches(x, Hp, Wp, B)[top:top + H, left:left + W]
        Yc, Co, Cg = c[..., 0], c[..., 1], c[..., 2]
        return np.stack([Yc + Co - Cg, Yc + Cg, Yc - Co - Cg], -1) + x.dtype.type(128)

    m = from_patches(mag, Hp, Wp, B)[top:top + H, left:left + W]
    pmag = np.stack([m.sum(-1), m[..., 0] + m[..., 2], m.sum(-1)], -1) + 128
    return dict(rgb=np.clip(rgb_of(x32), 0, 255).astype(np.uint8), pre=rgb_of(x64), mag=pmag)


# ---- boundary sets ----------------------------------------------------------
EPS32 = 2.0 ** -24


def tau(mag, D):
    """The float32 error bound of a D-term product (and the few additions after it) whose terms have
    total magnitude `mag`: (D + 4) unit roundoffs of it."""
    return (D + 4) * EPS32 * mag


def index_boundary(pre, mag, D):
    """Positions whose y / Q lies within tau of a quantizer threshold: the nonzero integers."""
    t = np.abs(pre)
    return np.abs(t - np.maximum(np.rint(t), 1.0)) <= tau(mag, D)


def pixel_boundary(pre, mag, D):
    """Positions whose pixel value lies within tau of one of 1, 2, ..., 255."""
    return np.abs(pre - np.clip(np.rint(pre), 1, 255)) <= tau(mag, D)


def synth_frame(H, W, seed):
    """A deterministic frame with smooth content, texture and a few saturated pixels."""
    rng = np.random.Generator(np.random.PCG64(seed))
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    ch = [128 + 70 * np.sin(x / 23 + c) + 60 * np.cos(y / 17 - c) + rng.normal(0, 12, (H, W)) for c in range(3)]
    return np.clip(np.rint(np.stack(ch, -1)), 0, 255).astype(np.uint8)

"""The overlapped compensation rule of include/vcf_amd.h ("Overlapped block
motion compensation") in numpy: the reference for
vcf_ipp_motion_compensate_obmc.  Validity is subpel_ref.valid; everything is
integer arithmetic.  Nothing here calls the library."""
import numpy as np

import subpel_ref as R

BLOCK_SIZES = (4, 8, 16, 32, 64)
LIMIT = 1 << 28


def quarter(mv, bs, H, W):
    """Step 1: (H//bs, W//bs, 2) int64 (qx, qy), rint(4 m) half to even clamped to +-2^28 (a NaN
    gives -2^28), an invalid vector replaced by (0, 0)."""
    mv = np.asarray(mv, np.float32).reshape(H // bs, W // bs, 2)
    with np.errstate(over="ignore", invalid="ignore"):
        f = np.float32(4) * mv
    nan = np.isnan(f)
    f = np.rint(np.where(nan, np.float32(0), f))
    # +-inf and huge values are decided by comparison, never converted
    big, small = f >= LIMIT, f <= -LIMIT
    q = np.where(big | small | nan, 0, f).astype(np.int64)
    q = np.where(big, LIMIT, np.where(small | nan, -LIMIT, q))
    for by in range(q.shape[0]):
        for bx in range(q.shape[1]):
            if not R.valid(4 * bx * bs + int(q[by, bx, 0]), 4 * by * bs + int(q[by, bx, 1]), bs, H, W):
                q[by, bx] = 0
    return q


def sample(frame, qx, qy, y, x):
    """Step 2: P(q; y, x) for arrays of pixels (y, x) and their vectors (qx, qy) -> (..., 3) int64;
    the four taps clamped to the frame."""
    H, W = frame.shape[:2]
    r = frame.astype(np.int64)
    X, Y = 4 * x + qx, 4 * y + qy
    ix, fx, iy, fy = X >> 2, (X & 3)[..., None], Y >> 2, (Y & 3)[..., None]
    x0, x1 = np.clip(ix, 0, W - 1), np.clip(ix + 1, 0, W - 1)
    y0, y1 = np.clip(iy, 0, H - 1), np.clip(iy + 1, 0, H - 1)
    acc = (4 - fx) * (4 - fy) * r[y0, x0] + fx * (4 - fy) * r[y0, x1] + (4 - fx) * fy * r[y1, x0] + fx * fy * r[y1, x1]
    return (acc + 8) >> 4


def _axis(n, bs, nb):
    """Steps 3 and 4 along one axis for positions 0 .. n-1: (own block, neighbour block, own weight)."""
    p = np.arange(n)
    b = p // bs
    u = p - b * bs
    low = u < bs // 2
    return b, np.clip(np.where(low, b - 1, b + 1), 0, nb - 1), np.where(low, bs + 2 * u + 1, 3 * bs - 2 * u - 1)


def motion_compensate(frame, mv, bs=16):
    """The overlapped prediction of frame (H x W x 3 u8) under the float field mv."""
    if bs not in BLOCK_SIZES:
        raise ValueError("bs must be 4, 8, 16, 32 or 64")
    frame = np.ascontiguousarray(frame, np.uint8)
    H, W = frame.shape[:2]
    nby, nbx = H // bs, W // bs
    out = np.zeros_like(frame)
    if nby == 0 or nbx == 0:
        return out
    q = quarter(mv, bs, H, W)
    by, ny, wy = _axis(nby * bs, bs, nby)
    bx, nx, wx = _axis(nbx * bs, bs, nbx)
    y, x = np.meshgrid(np.arange(nby * bs), np.arange(nbx * bs), indexing="ij")
    acc = np.zeros((nby * bs, nbx * bs, 3), np.int64)
    for rows, w_r in ((by, wy), (ny, 2 * bs - wy)):
        for cols, w_c in ((bx, wx), (nx, 2 * bs - wx)):
            v = q[rows[:, None], cols[None, :]]
            acc += (w_r[:, None] * w_c[None, :])[..., None] * sample(frame, v[..., 0], v[..., 1], y, x)
    shift = 2 * (bs.bit_length() - 1) + 2
    out[:nby * bs, :nbx * bs] = (acc + 2 * bs * bs) >> shift
    return out

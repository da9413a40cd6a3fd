"""The sub-pel motion rule of include/vcf_amd.h ("Sub-pel motion") in numpy:
the reference for vcf_ipp_block_match_subpel and vcf_ipp_motion_compensate_qpel,
and the synthetic sequence with true quarter-pel motion the tests and
scripts/bench_subpel.py use.  The integer stage is the oracle's
(oracle.ipp_block_matching); everything after it is integer arithmetic."""
import numpy as np

from oracle import oracle as O


def split(X):
    """X = 4 * origin + q -> (integer origin, fraction 0..3)."""
    return X >> 2, X & 3


def valid(X, Y, bs, H, W):
    """Every sample the vector reads lies in the frame."""
    ix, fx = split(X)
    iy, fy = split(Y)
    return ix >= 0 and ix + bs + (1 if fx else 0) <= W and iy >= 0 and iy + bs + (1 if fy else 0) <= H


def predict(r, X, Y, bs):
    """The bs x bs (x channels) prediction from plane or frame r at quarter-pel (X, Y); the vector is valid."""
    ix, fx = split(X)
    iy, fy = split(Y)
    r = r.astype(np.int64)
    acc = (4 - fx) * (4 - fy) * r[iy:iy + bs, ix:ix + bs]
    if fx:                                  # a tap whose weight is 0 is not read
        acc = acc + fx * (4 - fy) * r[iy:iy + bs, ix + 1:ix + 1 + bs]
    if fy:
        acc = acc + (4 - fx) * fy * r[iy + 1:iy + 1 + bs, ix:ix + bs]
    if fx and fy:
        acc = acc + fx * fy * r[iy + 1:iy + 1 + bs, ix + 1:ix + 1 + bs]
    return ((acc + 8) >> 4).astype(np.uint8)


def block_sad(rg, cg, i, j, X, Y, bs):
    return int(np.abs(predict(rg, X, Y, bs).astype(np.int64) - cg[i:i + bs, j:j + bs].astype(np.int64)).sum())


def block_matching(ref, cur, bs=16, sr=8, fast=False, subpel=1):
    """(H//bs, W//bs, 2) float32 (dx, dy) in pixels, multiples of 1/subpel."""
    if subpel not in (1, 2, 4):
        raise ValueError("subpel must be 1, 2 or 4")
    mv = O.ipp_block_matching(ref, cur, bs, sr, fast)
    if subpel == 1 or mv.size == 0:
        return mv
    H, W = ref.shape[:2]
    rg, cg = O.ipp_gray(ref), O.ipp_gray(cur)
    out = np.empty_like(mv)
    for by in range(H // bs):
        for bx in range(W // bs):
            i, j = by * bs, bx * bs
            qx, qy = 4 * int(mv[by, bx, 0]), 4 * int(mv[by, bx, 1])
            best = block_sad(rg, cg, i, j, 4 * j + qx, 4 * i + qy, bs)
            for step in ((2,) if subpel == 2 else (2, 1)):
                cx, cy = qx, qy
                for ddy in (-step, 0, step):
                    for ddx in (-step, 0, step):
                        if ddx == 0 and ddy == 0:
                            continue
                        X, Y = 4 * j + cx + ddx, 4 * i + cy + ddy
                        if not valid(X, Y, bs, H, W):
                            continue
                        s = block_sad(rg, cg, i, j, X, Y, bs)
                        if s < best:            # the first strict minimum: argmin of (SAD, index)
                            best, qx, qy = s, cx + ddx, cy + ddy
            out[by, bx] = (qx / 4.0, qy / 4.0)
    return out


def field_sad(ref, cur, mv, bs):
    """Per-block luma SAD of a (valid) field: (H//bs, W//bs) int64."""
    H, W = ref.shape[:2]
    rg, cg = O.ipp_gray(ref), O.ipp_gray(cur)
    out = np.zeros(mv.shape[:2], np.int64)
    for by in range(H // bs):
        for bx in range(W // bs):
            i, j = by * bs, bx * bs
            qx, qy = (int(v) for v in np.rint(4 * mv[by, bx].astype(np.float32)))
            out[by, bx] = block_sad(rg, cg, i, j, 4 * j + qx, 4 * i + qy, bs)
    return out


def motion_compensate(frame, mv, bs=16):
    """Compensation of an arbitrary float field: q = rint(4 m) (half to even, as lrintf),
    invalid vectors -> the co-located block, outside the full-block area zeros."""
    frame = np.ascontiguousarray(frame, np.uint8)
    H, W = frame.shape[:2]
    mv = np.asarray(mv, np.float32)
    out = np.zeros_like(frame)
    for by in range(H // bs):
        for bx in range(W // bs):
            i, j = by * bs, bx * bs
            q = np.rint(np.float32(4) * mv[by, bx])
            X, Y = 4 * j + int(q[0]), 4 * i + int(q[1])
            if not valid(X, Y, bs, H, W):
                X, Y = 4 * j, 4 * i
            out[i:i + bs, j:j + bs] = predict(frame, X, Y, bs)
    return out


def subpel_sequence(H, W, n, seed=0, sigma=2.0):
    """n frames H x W x 3 u8 with true quarter-pel motion: a random texture in
    2-pixel cells held at 4x resolution; frame t is cropped at quarter-pel
    offsets (5t, 7t) plus a 12-pixel margin, box-downsampled by 4, given
    Gaussian noise (sigma) and rounded and clipped."""
    rng = np.random.Generator(np.random.PCG64(seed))
    m = 12
    need_h, need_w = H + 2 * m + (7 * n) // 4 + 2, W + 2 * m + (5 * n) // 4 + 2
    cells = rng.integers(0, 256, ((need_h + 1) // 2, (need_w + 1) // 2, 3)).astype(np.uint8)
    hi = np.kron(cells, np.ones((8, 8, 1), np.uint8))   # 2-pixel cells at 4x resolution
    out = []
    for t in range(n):
        y0, x0 = 4 * m + 7 * t, 4 * m + 5 * t
        f = hi[y0:y0 + 4 * H, x0:x0 + 4 * W].reshape(H, 4, W, 4, 3).mean(axis=(1, 3))
        f = f + rng.normal(0, sigma, f.shape)
        out.append(np.clip(np.rint(f), 0, 255).astype(np.uint8))
    return out

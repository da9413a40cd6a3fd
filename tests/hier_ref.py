"""The hierarchical motion search of include/vcf_amd.h ("Hierarchical motion
search") in numpy: the reference for vcf_ipp_block_match_hier, and the
synthetic sequence with fast motion that the tests and scripts/bench_hier.py
use.  Level 0 is the oracle's luma (oracle.ipp_gray); everything after it is
integer arithmetic.  The top level is stated twice: plane_search in numpy, and
through the oracle's own full search on the plane as a gray frame (its luma of
(g, g, g) is g: (16384 g + 8192) >> 14), which the tests hold equal."""
import numpy as np

from oracle import oracle as O

MAX_LEVELS = 3


def halve(g):
    """One pyramid step: rounded 2 x 2 means, an odd last row or column dropped."""
    h, w = g.shape[0] >> 1, g.shape[1] >> 1
    a = g[:2 * h, :2 * w].astype(np.int64)
    return ((a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2] + 2) >> 2).astype(np.uint8)


def pyramid(g, levels):
    """[g_0 .. g_levels]."""
    out = [np.ascontiguousarray(g, np.uint8)]
    for _ in range(levels):
        out.append(halve(out[-1]))
    return out


def check(bs, levels):
    if levels not in range(MAX_LEVELS + 1):
        raise ValueError("levels must be 0 .. 3")
    if levels and (bs % (1 << levels) or (bs >> levels) < 2):
        raise ValueError("bs must be a multiple of 2^levels and at least 2^(levels + 1)")


def inside(y, x, b, H, W):
    return y >= 0 and y + b <= H and x >= 0 and x + b <= W


def sad(rg, cg, i, j, y, x, b):
    return int(np.abs(rg[y:y + b, x:x + b].astype(np.int64) - cg[i:i + b, j:j + b].astype(np.int64)).sum())


def plane_search(rg, cg, b, sr, shape=None):
    """The full search on two luma planes: dy outer, dx inner from -sr, in-plane candidates only,
    the first strict minimum -> (rows, cols, 2) int (dx, dy)."""
    H, W = rg.shape
    nby, nbx = shape if shape is not None else (H // b, W // b)
    out = np.zeros((nby, nbx, 2), np.int64)
    for by in range(nby):
        for bx in range(nbx):
            i, j = by * b, bx * b
            best = None
            for dy in range(-sr, sr + 1):
                for dx in range(-sr, sr + 1):
                    if not inside(i + dy, j + dx, b, H, W):
                        continue
                    s = sad(rg, cg, i, j, i + dy, j + dx, b)
                    if best is None or s < best:
                        best, out[by, bx] = s, (dx, dy)
    return out


def plane_search_oracle(rg, cg, b, sr):
    """The same through the oracle's full search, the planes as gray frames."""
    mv = O.ipp_block_matching(np.repeat(rg[:, :, None], 3, 2), np.repeat(cg[:, :, None], 3, 2), b, sr, False)
    return mv.astype(np.int64)


def refine(rg, cg, b, v):
    """One refinement level on planes rg, cg with block side b: v holds the level above's field."""
    H, W = rg.shape
    out = np.empty_like(v)
    for by in range(v.shape[0]):
        for bx in range(v.shape[1]):
            i, j = by * b, bx * b
            cx, cy = 2 * int(v[by, bx, 0]), 2 * int(v[by, bx, 1])
            assert inside(i + cy, j + cx, b, H, W)            # the centre is always valid
            best, win = sad(rg, cg, i, j, i + cy, j + cx, b), (cx, cy)
            for ddy in (-1, 0, 1):
                for ddx in (-1, 0, 1):
                    if (ddx == 0 and ddy == 0) or not inside(i + cy + ddy, j + cx + ddx, b, H, W):
                        continue
                    s = sad(rg, cg, i, j, i + cy + ddy, j + cx + ddx, b)
                    if s < best:                              # the first strict minimum after the centre
                        best, win = s, (cx + ddx, cy + ddy)
            out[by, bx] = win
    return out


def chain(rg, cg, bs, sr, levels, top=plane_search_oracle):
    """[v_levels .. v_0] of two luma planes, each (H // bs, W // bs, 2) int (dx, dy)."""
    check(bs, levels)
    H, W = rg.shape
    pr, pc = pyramid(rg, levels), pyramid(cg, levels)
    v = top(pr[levels], pc[levels], bs >> levels, sr)
    assert v.shape[:2] == (H // bs, W // bs)
    out = [v]
    for l in range(levels - 1, -1, -1):
        v = refine(pr[l], pc[l], bs >> l, v)
        out.append(v)
    return out


def integer_field(ref, cur, bs=16, sr=8, levels=0):
    H, W = ref.shape[:2]
    if H // bs == 0 or W // bs == 0:
        check(bs, levels)
        return np.zeros((H // bs, W // bs, 2), np.float32)
    return chain(O.ipp_gray(ref), O.ipp_gray(cur), bs, sr, levels)[-1].astype(np.float32)


def block_matching(ref, cur, bs=16, sr=8, levels=0, subpel=1):
    """(H//bs, W//bs, 2) float32 (dx, dy): the hierarchical integer search, then the sub-pel stages
    of subpel_ref around 4 v_0."""
    import subpel_ref as S
    mv = integer_field(ref, cur, bs, sr, levels)
    if subpel == 1 or mv.size == 0:
        return mv
    H, W = ref.shape[:2]
    rg, cg = O.ipp_gray(ref), O.ipp_gray(cur)
    out = np.empty_like(mv)
    for by in range(H // bs):
        for bx in range(W // bs):
            i, j = by * bs, bx * bs
            qx, qy = 4 * int(mv[by, bx, 0]), 4 * int(mv[by, bx, 1])
            best = S.block_sad(rg, cg, i, j, 4 * j + qx, 4 * i + qy, bs)
            for step in ((2,) if subpel == 2 else (2, 1)):
                cx, cy = qx, qy
                for ddy in (-step, 0, step):
                    for ddx in (-step, 0, step):
                        if ddx == 0 and ddy == 0:
                            continue
                        X, Y = 4 * j + cx + ddx, 4 * i + cy + ddy
                        if not S.valid(X, Y, bs, H, W):
                            continue
                        s = S.block_sad(rg, cg, i, j, X, Y, bs)
                        if s < best:
                            best, qx, qy = s, cx + ddx, cy + ddy
            out[by, bx] = (qx / 4.0, qy / 4.0)
    return out


def workspace(ref, cur, levels):
    """The bytes vcf_ipp_block_match_hier leaves in its workspace: level by level, ref's plane then cur's."""
    pr, pc = pyramid(O.ipp_gray(ref), levels), pyramid(O.ipp_gray(cur), levels)
    return np.concatenate([p.reshape(-1) for l in range(levels + 1) for p in (pr[l], pc[l])])


def _box(a, k):
    """Box filter of odd width k along the first two axes (edges replicated)."""
    for ax in (0, 1):
        pad = [(0, 0)] * a.ndim
        pad[ax] = (k // 2 + 1, k // 2)
        c = np.cumsum(np.pad(a, pad, mode="edge"), axis=ax)
        n = a.shape[ax]
        a = (np.take(c, range(k, k + n), axis=ax) - np.take(c, range(0, n), axis=ax)) / k
    return a


def fast_sequence(n, H, W, shift, seed=0, sigma=2.0, periods=(23.0, 37.0, 61.0, 97.0), amp=14.0, blur=9,
                  noise_amp=30.0):
    """n frames H x W x 3 u8 of one texture moving by shift = (dx, dy) pixels per frame, so that the
    true vector of frame t + 1 against frame t is shift: frame t shows the canvas at t * shift.
    The texture has most of its energy below 1/8 cycle per pixel: per channel a sum of sinusoids
    (periods of 23 .. 97 pixels along seeded directions, amplitude amp each) plus uniform noise
    blurred twice by a box of `blur` pixels (scaled to a standard deviation of noise_amp); a
    fractional offset is taken by bilinear interpolation of the blurred canvas.  Every frame gets
    fresh white Gaussian noise of standard deviation sigma, then is rounded and clipped."""
    rng = np.random.Generator(np.random.PCG64(seed))
    dx, dy = float(shift[0]), float(shift[1])
    ox, oy = max(0.0, -dx * (n - 1)), max(0.0, -dy * (n - 1))
    ch, cw = H + int(np.ceil(abs(dy) * (n - 1))) + 2, W + int(np.ceil(abs(dx) * (n - 1))) + 2
    canvas = _box(_box(rng.uniform(-1, 1, (ch, cw, 3)), blur), blur)
    canvas *= noise_amp / canvas.std()
    waves = [(p, rng.uniform(0, 2 * np.pi), rng.uniform(0, 2 * np.pi, 3), rng.uniform(0.5, 1.0, 3)) for p in periods]
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    out = []
    for t in range(n):
        y0, x0 = oy + t * dy, ox + t * dx
        iy, ix = int(np.floor(y0)), int(np.floor(x0))
        fy, fx = y0 - iy, x0 - ix
        c = canvas[iy:iy + H + 1, ix:ix + W + 1]
        f = ((1 - fy) * (1 - fx) * c[:H, :W] + (1 - fy) * fx * c[:H, 1:W + 1] + fy * (1 - fx) * c[1:H + 1, :W]
             + fy * fx * c[1:H + 1, 1:W + 1]) + 128.0
        for p, th, ph, a in waves:
            arg = 2 * np.pi / p * ((xx + x0) * np.cos(th) + (yy + y0) * np.sin(th))
            f = f + amp * a * np.sin(arg[:, :, None] + ph)
        f = f + rng.normal(0, sigma, f.shape)
        out.append(np.clip(np.rint(f), 0, 255).astype(np.uint8))
    return out

"""The deblocking rule of include/vcf_amd.h (vcf_deblock_u8) restated in
vectorised numpy, int32 throughout.  deblock_ref is what the GPU tests compare with;
deblock_masks also returns, per pass, which branch every line took, so that a test can count
the paths its inputs reach."""
import numpy as np


def edges(n, phase, B):
    """The edge positions x of an axis of n samples: 0 < x < n and (x + phase) % B == 0."""
    x = np.arange(1, max(n, 1))
    return x[(x + phase) % B == 0]


def _pass(img, axis_edges, beta, tc):
    """One pass whose lines run along axis 1 of img (rows x n x C), across the edges axis_edges.
    -> (out uint8, masks): a dict of bool arrays, rows x (the edges at least 3 and 2 samples
    from the borders) x C, one per name in MASKS."""
    a = img.astype(np.int32)
    n = a.shape[1]
    x = axis_edges[(axis_edges - 3 >= 0) & (axis_edges + 2 <= n - 1)]
    out = a.copy()
    if x.size == 0:
        z = np.zeros((a.shape[0], 0, a.shape[2]), bool)
        return out.astype(np.uint8), {k: z for k in MASKS}
    p2, p1, p0 = a[:, x - 3], a[:, x - 2], a[:, x - 1]
    q0, q1, q2 = a[:, x], a[:, x + 1], a[:, x + 2]
    dp = np.abs(p2 - 2 * p1 + p0)
    dq = np.abs(q2 - 2 * q1 + q0)
    off_beta = dp + dq >= beta
    delta = (9 * (q0 - p0) - 3 * (q1 - p1) + 8) >> 4
    off_tc = ~off_beta & (np.abs(delta) >= 10 * tc)
    on = ~off_beta & ~off_tc
    dc = np.clip(delta, -tc, tc)
    side = (beta + (beta >> 1)) >> 3
    h = tc >> 1
    p0n, q0n = p0 + dc, q0 - dc
    p1n = p1 + np.clip((((p2 + p0 + 1) >> 1) - p1 + dc) >> 1, -h, h)
    q1n = q1 + np.clip((((q2 + q0 + 1) >> 1) - q1 - dc) >> 1, -h, h)
    wp1, wq1 = on & (dp < side), on & (dq < side)
    out[:, x - 1] = np.where(on, np.clip(p0n, 0, 255), p0)
    out[:, x] = np.where(on, np.clip(q0n, 0, 255), q0)
    out[:, x - 2] = np.where(wp1, np.clip(p1n, 0, 255), p1)
    out[:, x + 1] = np.where(wq1, np.clip(q1n, 0, 255), q1)
    sat_lo = (on & ((p0n < 0) | (q0n < 0))) | (wp1 & (p1n < 0)) | (wq1 & (q1n < 0))
    sat_hi = (on & ((p0n > 255) | (q0n > 255))) | (wp1 & (p1n > 255)) | (wq1 & (q1n > 255))
    masks = {"off_beta": off_beta, "off_tc": off_tc, "on": on, "clipped": on & (dc != delta),
             "unclipped": on & (dc == delta), "p1_written": wp1, "p1_kept": on & ~wp1, "q1_written": wq1,
             "q1_kept": on & ~wq1, "sat_lo": sat_lo, "sat_hi": sat_hi}
    return out.astype(np.uint8), masks


MASKS = ("off_beta", "off_tc", "on", "clipped", "unclipped", "p1_written", "p1_kept", "q1_written", "q1_kept",
         "sat_lo", "sat_hi")


def pass_v(img, B, left, beta, tc):
    """Pass V of one H x W x C frame: vertical edges, lines along the rows."""
    return _pass(img, edges(img.shape[1], left, B), int(beta), int(tc))


def pass_h(img, B, top, beta, tc):
    """Pass H: horizontal edges, lines down the columns."""
    out, m = _pass(np.swapaxes(img, 0, 1), edges(img.shape[0], top, B), int(beta), int(tc))
    return np.ascontiguousarray(np.swapaxes(out, 0, 1)), m


def deblock_masks(img, B, top, left, beta, tc):
    """One H x W x C uint8 frame -> (filtered frame, pass V's result, pass V's masks, pass H's masks)."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3 and B >= 4 and 0 <= top < B and 0 <= left < B
    v, mv = pass_v(img, B, left, beta, tc)
    out, mh = pass_h(v, B, top, beta, tc)
    return out, v, mv, mh


def deblock_ref(img, B, top, left, beta, tc):
    """H x W x C or N x H x W x C uint8 -> the filtered frame(s)."""
    img = np.asarray(img)
    if img.ndim == 4:
        return np.stack([deblock_masks(f, B, top, left, beta, tc)[0] for f in img]) if len(img) else img.copy()
    return deblock_masks(img, B, top, left, beta, tc)[0]


def crop_offsets(H, W, B):
    """(top, left) of the centred padding to multiples of B that the block decoders crop."""
    return ((-H) % B) // 2, ((-W) % B) // 2


def blocky_frames(seed, n, H, W, B, top, left, amp=3):
    """n seeded blocky frames: a constant per block of the (B, top, left) grid and channel, plus noise of
    +-amp, with about one block in eight pinned near 0 and one in eight near 255."""
    rng = np.random.Generator(np.random.PCG64(seed))
    by, bx = (np.arange(H) + top) // B, (np.arange(W) + left) // B
    nby, nbx = int(by.max()) + 1, int(bx.max()) + 1
    level = rng.integers(0, 256, (n, nby, nbx, 3))
    pin = rng.integers(0, 8, (n, nby, nbx, 1))
    level = np.where(pin == 0, rng.integers(0, 4, level.shape), level)
    level = np.where(pin == 1, rng.integers(252, 256, level.shape), level)
    # neighbours a small step apart too, so that filtered lines are common
    level = np.where(pin >= 5, 120 + rng.integers(-12, 13, level.shape), level)
    img = level[:, by][:, :, bx] + rng.integers(-amp, amp + 1, (n, H, W, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


# ---- the cases of the GPU comparison (tests/test_deblock_gpu.py), whose inputs the host test
# ---- (tests/test_deblock.py) checks for branch coverage: (H, W, B, top, left)
GPU_CASES = [
    (1, 1, 8, 0, 0),
    (16, 16, 4, 0, 0),
    (13, 29, 4, 1, 2),          # 87 bytes a row
    (24, 40, 8, 0, 0),
    (61, 77, 8, 1, 1),
    (9, 200, 8, 7, 6),          # edges at y = 1 and x = 2
    (9, 200, 8, 6, 2),          # y = 2, x = 198 = W - 2
    (9, 200, 8, 0, 1),          # y = 8 = H - 1, x = 199 = W - 1
    (70, 9, 8, 4, 7),           # y = 68 = H - 2, x = 1
    (70, 9, 8, 3, 0),           # y = 69 = H - 1, x = 8 = W - 1
    (70, 9, 8, 6, 6),           # y = 2, x = 2
    (70, 9, 8, 7, 1),           # y = 1, x = 7 = W - 2
    (48, 80, 16, 0, 0),
    (210, 405, 200, 95, 97),    # a block larger than any tile
    (8, 8, 4096, 0, 0),         # no edge
]
GPU_STRENGTHS = [(16, 4), (64, 8), (1, 1), (0, 5), (40, 0), (4096, 255)]
GPU_FRAMES = 3


def case_id(case):
    H, W, B, top, left = case
    return f"{H}x{W}-B{B}-{top}-{left}"


def case_frames(case):
    """The GPU_FRAMES seeded blocky frames of a case."""
    H, W, B, top, left = case
    return blocky_frames(1000 + GPU_CASES.index(case), GPU_FRAMES, H, W, B, top, left)

"""GPU parity of the encode's provable-zero row skipping: the product kernel
(wave-uniform skip of row pairs 1..3, rows 2..7 of the LDS image zeroed
beforehand) is bit-exact against the oracle, against the scalar kernel that
knows no skipping (A/B variant 1) and against the A/B library's packed kernels
without the test (20) and with it but without the zeroed image (21), on frames
built to reach every path: all waves skip, none skips, one lane vetoes its
wave, only some pairs can skip, coefficients right at the quantizer's steps."""
import functools

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

D = pytest.importorskip("vcf_amd.dct")

# two full tiles with the full-tile copy-out; 18 tiles and a last one of 9 blocks (a wave with 9 active lanes,
# byte copy-out); the same grid from a frame that needs padding
SHAPES = [(16, 2048), (72, 4104), (70, 4100)]
KINDS = ["smooth", "noise", "mixed", "band3", "band23", "sweep"]
QS = [1, 32, 64]


def _basis():
    n = np.arange(8)
    return np.array([[np.sqrt((1 if k == 0 else 2) / 8) * np.cos(np.pi * (2 * m + 1) * k / 16) for m in n] for k in n])


def _from_coefs(coefs):
    """[nby, nbx, 8, 8] orthonormal 2-D DCT coefficients of Y - 128 -> gray u8 frame (R = G = B)."""
    C = _basis()
    px = np.einsum("iy,abij,jx->aybx", C, coefs, C)
    nby, _, nbx, _ = px.shape
    g = np.clip(np.rint(px.reshape(nby * 8, nbx * 8) + 128), 0, 255).astype(np.uint8)
    return np.repeat(g[:, :, None], 3, 2)


@functools.lru_cache(maxsize=None)
def frame(shape, kind):
    H, W = shape
    Hp, Wp = (H + 7) // 8 * 8, (W + 7) // 8 * 8
    nby, nbx = Hp // 8, Wp // 8
    rng = np.random.Generator(np.random.PCG64(H * 7919 + W + len(kind)))
    y, x = np.mgrid[0:Hp, 0:Wp]
    smooth = np.stack([128 + 40 * np.sin(x / 300 + c) + 30 * np.cos(y / 200 - c) for c in range(3)], -1)
    smooth = np.clip(np.rint(smooth), 0, 255).astype(np.uint8)
    noise = rng.integers(0, 256, (Hp, Wp, 3), dtype=np.uint8)
    if kind == "smooth":
        f = smooth
    elif kind == "noise":
        f = noise
    elif kind == "mixed":      # one textured block per wave of 64 raster blocks, at lane 0, 31 or 63
        f = smooth.copy()
        for w in range((nby * nbx + 63) // 64):
            n = w * 64 + (0, 31, 63)[w % 3]
            if n < nby * nbx:
                by, bx = divmod(n, nbx)
                f[by * 8:by * 8 + 8, bx * 8:bx * 8 + 8] = noise[by * 8:by * 8 + 8, bx * 8:bx * 8 + 8]
    elif kind in ("band3", "band23"):   # vertical frequencies up to row 5 (only pair 3 can skip) or 3 (pairs 2, 3)
        top = 5 if kind == "band3" else 3
        co = np.zeros((nby, nbx, 8, 8))
        co[:, :, 0, 0] = rng.uniform(-300, 300, (nby, nbx))
        for i in range(1, top + 1):
            co[:, :, i, 0] = rng.choice([-80.0, 80.0], (nby, nbx))
            co[:, :, i, 1] = rng.uniform(-20, 20, (nby, nbx))
        f = _from_coefs(co)
    else:                      # sweep: one cosine per block at (i, j), its coefficient stepped through +-Q
        # (Q = 1 has no room between pixel steps; it still encodes these frames.)  Row i is the same for a
        # whole wave, so the other pairs of that wave do skip.  Even waves: the blocks step through the index
        # change at |coefficient| = Q.  Odd waves: all 64 blocks at one amplitude, stepped from wave to wave
        # through the bound's own threshold (0.5 * sum|u| = Q at 0.71 Q for j = 0, 0.78-0.8 Q for j = 3, 7);
        # pixel rounding spreads the blocks of such a wave to both sides of it.
        co = np.zeros((nby, nbx, 8, 8)).reshape(-1, 8, 8)
        nw = (nby * nbx + 63) // 64
        for w in range(nw):
            lanes = np.arange(w * 64, min(w * 64 + 64, nby * nbx))
            i, Q = (2, 4, 7)[w % 3], (32, 64)[(w // 6) % 2]
            j = np.array((0, 3, 7))[(lanes + w) % 3]
            if w % 2 == 0:
                amp = np.linspace(0.8, 1.2, len(lanes))
            else:
                amp = np.full(len(lanes), 0.55 + 0.4 * ((w // 2) % 12) / 11)
                j[:] = (0, 3, 7)[(w // 2) % 3]
            co[lanes, i, j] = Q * amp * rng.choice([-1.0, 1.0], len(lanes))
        f = _from_coefs(co.reshape(nby, nbx, 8, 8))
    top, left = (Hp - H) // 2, (Wp - W) // 2
    return np.ascontiguousarray(f[top:top + H, left:left + W])


@functools.lru_cache(maxsize=None)
def want(shape, kind, Q, flags):
    return O.encode_frame(frame(shape, kind), Q, flags)


def test_sweep_reaches_the_quantizer_steps():
    """The sweep frame does put indices 0 and +-1 next to each other in rows 2, 4 and 7."""
    k = want((16, 2048), "sweep", 32, 1).astype(np.int16) - 128   # -x: pixel-domain layout, Y in channel 0
    for i in (2, 4, 7):
        vals = set(np.unique(k[i::8, :, 0]).tolist())
        assert {-1, 0, 1} <= vals, (i, vals)


@pytest.mark.parametrize("flags", [0, 1])
@pytest.mark.parametrize("Q", QS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_encode_skip_bit_exact(shape, kind, Q, flags):
    rgb = frame(shape, kind)
    ref = want(shape, kind, Q, flags)
    assert np.array_equal(D.encode(rgb, Q, flags), ref), "product kernel vs oracle"
    assert np.array_equal(D.encode(rgb, Q, flags, variant=1), ref), "scalar kernel vs oracle"
    for v in (20, 21):
        assert np.array_equal(D.encode(rgb, Q, flags, variant=v), ref), v


@pytest.mark.parametrize("flags", [0, 1])
@pytest.mark.parametrize("shape", SHAPES)
def test_encode_skip_batch_of_three(shape, flags):
    kinds = ("mixed", "noise", "smooth")
    frames = np.stack([frame(shape, k) for k in kinds])
    got = D.encode(frames, 32, flags)
    for f, k in enumerate(kinds):
        assert np.array_equal(got[f], want(shape, k, 32, flags)), k
    assert np.array_equal(D.encode(frames, 32, flags, variant=21), got)

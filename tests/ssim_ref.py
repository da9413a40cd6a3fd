"""The integer-window SSIM of DESIGN.md §4.15, restated in numpy/scipy, and the float64 form it
approximates.  Nothing here imports vcf_amd: ssim_ref is what vcf_ssim_u8 must equal bit for bit,
float_ssim is Wang et al.'s SSIM with the unrounded Gaussian, for comparison only."""
import numpy as np
from scipy.ndimage import correlate1d

# the 11-tap Gaussian (sigma 1.5) scaled to sum 256 and rounded: the outer taps round to 0
TAPS = np.array([0, 2, 9, 28, 55, 68, 55, 28, 9, 2, 0], np.int64)
S = 1 << 16                              # the 2-D weight sum
C1 = 27928024842                         # round(6.5025 * 2^32): (0.01 * 255)^2 in units of S^2
C2 = 251352223580                        # round(58.5225 * 2^32): (0.03 * 255)^2
ONE = 1 << 30                            # k = rint(q * 2^30)
WIN = 11


def _frames(a):
    a = np.asarray(a)
    assert a.dtype == np.uint8
    if a.ndim == 2:
        a = a[None, :, :, None]
    elif a.ndim == 3:
        a = a[None]
    assert a.ndim == 4 and a.shape[1] >= WIN and a.shape[2] >= WIN
    return a


def _window_sums(p):
    """int64 n x H x W x C -> the weighted sum of every window wholly inside the frame:
    n x (H - 10) x (W - 10) x C, exact."""
    v = correlate1d(p, TAPS, axis=1, mode="constant", cval=0)
    v = correlate1d(v, TAPS, axis=2, mode="constant", cval=0)
    return v[:, 5:-5, 5:-5, :]


def factors(a, b):
    """(f1, f2, f3, f4), int64, per window and channel."""
    x, y = _frames(a).astype(np.int64), _frames(b).astype(np.int64)
    assert x.shape == y.shape
    A, B = _window_sums(x), _window_sums(y)
    XX, YY, XY = _window_sums(x * x), _window_sums(y * y), _window_sums(x * y)
    f1 = 2 * A * B + C1
    f2 = 2 * (S * XY - A * B) + C2
    f3 = A * A + B * B + C1
    f4 = S * XX - A * A + S * YY - B * B + C2
    return f1, f2, f3, f4


def k_map(a, b):
    """k = rint(q * 2^30) per window and channel (n x (H - 10) x (W - 10) x C, int64):
    q = (double(f1) * double(f2)) / (double(f3) * double(f4)), two products and one division."""
    f1, f2, f3, f4 = (f.astype(np.float64) for f in factors(a, b))
    q = (f1 * f2) / (f3 * f4)
    return np.rint(q * float(ONE)).astype(np.int64)


def ssim_ref(a, b):
    """(sum_k int64 n x C, windows int, min_k int64 n x C) of u8 frames H x W, H x W x C or n x H x W x C."""
    k = k_map(a, b)
    n, h, w, C = k.shape
    k = k.reshape(n, h * w, C)
    return k.sum(axis=1), h * w, k.min(axis=1)


def per_channel(sum_k, windows):
    return np.asarray(sum_k, np.int64).astype(np.float64) / float(windows * ONE)


def per_frame(sum_k, windows):
    sum_k = np.asarray(sum_k, np.int64)
    return sum_k.sum(axis=1).astype(np.float64) / float(sum_k.shape[1] * windows * ONE)


def float_ssim(a, b):
    """Per frame and channel (n x C float64): the mean over the valid windows of Wang et al.'s SSIM
    with the unrounded 11 x 11 Gaussian (sigma 1.5, normalised to sum 1), all in float64."""
    x, y = _frames(a).astype(np.float64), _frames(b).astype(np.float64)
    g = np.exp(-((np.arange(WIN) - 5) ** 2) / (2 * 1.5 ** 2))
    g /= g.sum()

    def blur(p):
        v = correlate1d(p, g, axis=1, mode="constant", cval=0.0)
        v = correlate1d(v, g, axis=2, mode="constant", cval=0.0)
        return v[:, 5:-5, 5:-5, :]

    mx, my = blur(x), blur(y)
    sxx, syy, sxy = blur(x * x) - mx * mx, blur(y * y) - my * my, blur(x * y) - mx * my
    c1, c2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    s = ((2 * mx * my + c1) * (2 * sxy + c2)) / ((mx * mx + my * my + c1) * (sxx + syy + c2))
    n, h, w, C = s.shape
    return s.reshape(n, h * w, C).mean(axis=1)

"""The integer-window SSIM without a GPU: the window table and constants, the 2^53 bound on the
factors, what the restatement (tests/ssim_ref.py) gives on the cases that can be worked out by hand,
its distance from the float64 SSIM, the argument checks of vcf_ssim_u8 (they answer before any
device work), the host wrappers' refusals and the parsers' --ssim flag.

Integer form against float_ssim (test_integer_form_against_the_float_form), per frame and channel
over the three RDE fixtures and twelve synthetic pairs: largest |difference| 3.035e-3 (the textured
frame at noise sigma 25, integer form below); the integer form is lower by 2e-7 to 3.0e-3 on every
pair but for a few channels where it is higher by at most 5.9e-5."""
import ctypes
import functools
import os
from fractions import Fraction

import numpy as np
import pytest

from conftest import GOLDEN

import ssim_ref as R
import vcf_amd._lib as L
from vcf_amd import distortion as DS
from vcf_amd.codec import parser as P
from vcf_amd.codec import rde

# the largest |integer form - float form| over pairs() below, measured once and recorded here; the
# test allows twice as much because the set is small
RECORDED_MAX_DIFFERENCE = 3.035e-3


def test_table_and_constants():
    assert R.TAPS.tolist() == [0, 2, 9, 28, 55, 68, 55, 28, 9, 2, 0] and int(R.TAPS.sum()) == 256
    g = np.exp(-((np.arange(11) - 5) ** 2) / (2 * 1.5 ** 2))
    assert np.array_equal(np.rint(g / g.sum() * 256).astype(np.int64), R.TAPS)      # rounded, no correction needed
    assert R.S == 256 * 256 == 2 ** 16
    assert R.C1 == 27928024842 == round(Fraction(255, 100) ** 2 * 2 ** 32) == round(6.5025 * 2 ** 32)
    assert R.C2 == 251352223580 == round(Fraction(3 * 255, 100) ** 2 * 2 ** 32) == round(58.5225 * 2 ** 32)
    assert (DS.SSIM_WINDOW, DS.SSIM_ONE) == (11, 2 ** 30) and R.ONE == DS.SSIM_ONE


def checker(H, W, C=1):
    y, x = np.mgrid[0:H, 0:W]
    return np.repeat((((x + y) & 1) * 255).astype(np.uint8)[:, :, None], C, axis=2)


def test_factors_stay_below_2_to_the_53():
    """The extreme inputs: every factor converts to float64 exactly, with three bits to spare."""
    H, W = 14, 15
    zero, full, grey = np.zeros((H, W, 1), np.uint8), np.full((H, W, 1), 255, np.uint8), np.full((H, W, 1), 128, np.uint8)
    ck = checker(H, W)
    largest = 0
    for a, b in ((zero, full), (full, zero), (full, full), (ck, 255 - ck), (255 - ck, ck), (ck, grey), (grey, ck),
                 (ck, ck), (ck, full)):
        for f in R.factors(a, b):
            assert f.dtype == np.int64
            largest = max(largest, int(np.abs(f).max()))
            assert np.array_equal(f.astype(np.float64).astype(np.int64), f)
    assert largest < 2 ** 53
    assert largest < 2 ** 50
    # the bound's terms: A <= 255 * 2^16, S * XX <= 65025 * 2^32, S * (XX + YY) < 2^49
    assert 255 * 2 ** 16 < 2 ** 24 and 65025 * 2 ** 16 < 2 ** 32 and 2 * 65025 * 2 ** 32 + R.C2 < 2 ** 50


def test_identical_frames_give_exactly_one():
    rng = np.random.Generator(np.random.PCG64(1))
    a = rng.integers(0, 256, (2, 19, 23, 3), dtype=np.uint8)
    assert (R.k_map(a, a) == 2 ** 30).all()
    s, w, m = R.ssim_ref(a, a)
    assert w == 9 * 13 and (s == w * 2 ** 30).all() and (m == 2 ** 30).all()
    assert (R.per_channel(s, w) == 1.0).all() and (R.per_frame(s, w) == 1.0).all()
    assert (DS.Ssim(s, m, w).per_channel() == 1.0).all() and (DS.Ssim(s, m, w).per_frame() == 1.0).all()


def test_black_against_white_one_window():
    a, b = np.zeros((11, 11), np.uint8), np.full((11, 11), 255, np.uint8)
    s, w, m = R.ssim_ref(a, b)
    # A = XX = XY = 0, B = 255 * 2^16, S * YY = B^2: f1 = C1, f2 = f4 = C2, f3 = B^2 + C1
    B = 255 * 2 ** 16
    q = (float(R.C1) * float(R.C2)) / (float(B * B + R.C1) * float(R.C2))
    assert w == 1 and s.shape == (1, 1) and int(s[0, 0]) == int(m[0, 0]) == int(np.rint(q * 2 ** 30)) == 107363
    assert abs(R.per_channel(s, w)[0, 0] - 1.0e-4) < 1e-6


def test_negative_k_and_min_k():
    rng = np.random.Generator(np.random.PCG64(2))
    a = rng.integers(0, 256, (1, 24, 31, 3), dtype=np.uint8)
    b = 255 - a                                                    # anti-correlated content
    k = R.k_map(a, b)
    s, w, m = R.ssim_ref(a, b)
    assert (k < 0).any() and (m < 0).all()
    assert np.array_equal(m, k.reshape(1, -1, 3).min(axis=1)) and np.array_equal(s, k.reshape(1, -1, 3).sum(axis=1))
    assert (R.per_channel(s, w) < 0).all()


def test_host_record_arithmetic():
    s = np.array([[3 << 28, 1 << 29, -(1 << 28)], [5, 6, 7]], np.int64)
    r = DS.Ssim(s, s.copy(), 4)
    assert np.array_equal(r.per_channel(), s.astype(np.float64) / float(4 * 2 ** 30))
    assert np.array_equal(r.per_frame(), np.array([float(s[0].sum()) / (3 * 4 * 2 ** 30), 18.0 / (3 * 4 * 2 ** 30)]))
    assert np.array_equal(r.per_frame(), R.per_frame(s, 4))
    assert r.per_channel().dtype == np.float64 and r.per_frame().shape == (2,)


@functools.lru_cache(maxsize=None)
def pairs():
    """(name, a, b): the RDE fixtures, and smooth, textured and noisy 96 x 128 x 3 frames against themselves plus
    Gaussian noise of sigma 2, 5, 10 and 25."""
    out = []
    for name in ("grey_16x16", "rgb_37x53", "rgb_64x96_two"):
        z = np.load(os.path.join(GOLDEN, f"rde_{name}.npz"))
        out.append((name, z["original"], z["decoded"]))
    H, W = 96, 128
    y, x = np.mgrid[0:H, 0:W]
    rng = np.random.Generator(np.random.PCG64(3))
    smooth = np.stack([128 + 100 * np.sin(x / 31.0) * np.cos(y / 23.0), 1.6 * x + 0.4 * y, 250 - 2.2 * y], -1)
    textured = np.stack([128 + 70 * np.sin(x * 1.3) * np.sin(y * 0.9), 128 + 110 * np.sign(np.sin(x * 0.8 + y * 0.5)),
                         40 + 25.0 * ((x // 3 + y // 2) % 7)], -1)
    noisy = rng.uniform(0, 255, (H, W, 3))
    for name, base in (("smooth", smooth), ("textured", textured), ("noisy", noisy)):
        a = np.clip(np.rint(base), 0, 255).astype(np.uint8)
        for sigma in (2, 5, 10, 25):
            b = np.clip(np.rint(a + rng.normal(0, sigma, a.shape)), 0, 255).astype(np.uint8)
            out.append((f"{name}_{sigma}", a, b))
    return tuple(out)


def test_integer_form_against_the_float_form():
    """Both sides are references: the weight rounding (and the 2^-30 steps of k) is all that separates them.
    The figures are printed (pytest -s shows them) before the assertion."""
    largest, where = 0.0, None
    for name, a, b in pairs():
        s, w, _ = R.ssim_ref(a, b)
        d = R.per_channel(s, w) - R.float_ssim(a, b)
        print(f"ssim integer - float, {name}: min {d.min():+.3e} max {d.max():+.3e}")
        if np.abs(d).max() > largest:
            largest, where = float(np.abs(d).max()), name
    print(f"largest |difference| {largest:.3e} ({where})")
    assert largest <= 2 * RECORDED_MAX_DIFFERENCE


@pytest.mark.parametrize("args", [dict(H=10), dict(W=10), dict(C=2), dict(C=4), dict(C=0), dict(n=0), dict(n=-3),
                                  dict(a=None), dict(b=None), dict(out=None), dict(out=ctypes.c_void_p(20))])
def test_argument_errors_before_any_device_work(args):
    dummy = ctypes.c_void_p(16)    # never dereferenced: validation fails first
    a = dict(a=dummy, b=dummy, n=1, H=11, W=11, C=3, out=dummy)
    a.update(args)
    rc = L.lib().vcf_ssim_u8(a["a"], a["b"], a["n"], a["H"], a["W"], a["C"], a["out"], None)
    assert rc == L.VCF_ERR_INVALID
    assert L.lib().vcf_last_error()
    if "H" in args or "W" in args:
        assert b"11 x 11" in L.lib().vcf_last_error()


def test_symbol_record_and_tile():
    assert hasattr(L.lib(), "vcf_ssim_u8") and "vcf_ssim_u8" in L.SIGNATURES
    assert DS.SSIM_RECORD.itemsize == 24 == 3 * ctypes.sizeof(ctypes.c_int64)
    assert DS.SSIM_RECORD.names == ("sum_k", "windows", "min_k")
    assert [DS.SSIM_RECORD.fields[n][1] for n in DS.SSIM_RECORD.names] == [0, 8, 16]
    assert L.lib().vcf_ssim_tile() >= 1


def test_parsers_accept_the_flag():
    assert P.rde_parser().parse_args([]).ssim is False and P.rde_parser().parse_args(["--ssim"]).ssim is True
    assert P.rd_curve_parser().parse_args([]).ssim is False and P.rd_curve_parser().parse_args(["--ssim"]).ssim is True
    a = P.rde_parser().parse_args(["-o", "a.png", "--ssim", "-N", "3"])
    assert (a.original, a.number_of_frames, a.ssim) == ("a.png", 3, True)


def test_small_frames_are_refused_by_name(tmp_path, capsys):
    """ValueError naming the window, before anything is uploaded; --ssim exits with it and prints no RDE line."""
    small = np.zeros((10, 40, 3), np.uint8)
    for a in (small, np.zeros((40, 10), np.uint8), np.zeros((2, 12, 10, 3), np.uint8)):
        with pytest.raises(ValueError, match="11 x 11"):
            DS.ssim(a, a)
    with pytest.raises(ValueError, match="1 or 3 channels"):
        DS.ssim(np.zeros((12, 12, 2), np.uint8), np.zeros((12, 12, 2), np.uint8))
    with pytest.raises(ValueError, match="shapes differ"):
        DS.ssim(np.zeros((12, 12), np.uint8), np.zeros((12, 13), np.uint8))
    with pytest.raises(TypeError):
        DS.ssim(np.zeros((12, 12), np.int16), np.zeros((12, 12), np.int16))
    with pytest.raises(ValueError, match="11 x 11"):
        rde.rd_curve(np.zeros((8, 64, 3), np.uint8), [8], ssim=True)
    from PIL import Image
    Image.fromarray(small).save(tmp_path / "a.png")
    Image.fromarray(small).save(tmp_path / "b.png")
    argv = ["-o", str(tmp_path / "a.png"), "-c", str(tmp_path / "enc"), "-d", str(tmp_path / "b.png"), "--ssim"]
    assert rde.main(argv) == 1
    cap = capsys.readouterr()
    assert cap.out == "" and "11 x 11" in cap.err


def test_lines_with_and_without_ssim():
    r = rde.Result("o.png", "d.png", ["e.tif"], [100], 1000, 900, (16, 16, 3), 2.5)
    plain = r.lines()
    assert plain[-1] == "RDE: J = R + D = 5.62" and not any("SSIM" in ln for ln in plain)
    assert "ssim" not in repr(r)
    r.ssim = 0.98765
    assert r.lines() == plain + ["RDE: SSIM: 0.9877"]

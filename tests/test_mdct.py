"""The lapped 2D-MDCT codec without a GPU: the numpy restatement
(tests/mdct_restated.py) against the reference's own fixtures
(tests/golden/mdct_*.npz, make_golden_mdct.py), the host-only ABI, argument
validation before any device work, and the command-line surface."""
import ctypes
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

import mdct_restated as M
import vcf_amd._lib as L

CAP = 1e-5   # positions that may depend on the float64 summation order, per case


def mdct_manifest():
    with open(os.path.join(GOLDEN, "manifest_mdct.json")) as f:
        return json.load(f)


def mdct_cases():
    return mdct_manifest()["cases"]


def load(case):
    return np.load(os.path.join(GOLDEN, f"mdct_{case['name']}.npz"))


def params(case):
    B, Q, fl = 8, 32, 0
    it = iter(case["flags"])
    for f in it:
        if f == "-B":
            B = int(next(it))
        elif f == "-q":
            Q = int(next(it))
        elif f == "-x":
            fl |= M.NO_SUBBANDS
        elif f == "-p":
            fl |= M.PERCEPTUAL
    return B, Q, fl


CASES = mdct_cases()
IDS = [c["name"] for c in CASES]


def test_fixture_set_is_the_one_the_codec_needs():
    names = set(IDS)
    for need in ("rand_1x1", "rand_3x17_q3", "smooth_37x45", "smooth_37x45_b12", "rand_40x48_x", "smooth_64x64_p",
                 "flat_48x56_b32", "smooth_33x35_b4", "extreme_32x40_q1", "rand_24x24_b64_q7"):
        assert need in names
    assert any(params(c)[0] == 2 for c in CASES)
    for c in CASES:
        assert os.path.getsize(os.path.join(GOLDEN, f"mdct_{c['name']}.npz")) < 256 * 1024


@pytest.mark.parametrize("case", CASES, ids=IDS)
@pytest.mark.parametrize("order", ["fwd", "rev"])
def test_restatement_equals_the_reference(case, order):
    """Indices, _shape.bin and decoded frame, in both accumulation orders: the fixtures do not
    depend on the order of the float64 sums (the reference's is BLAS's)."""
    z = load(case)
    B, Q, fl = params(case)
    H, W = z["rgb"].shape[:2]
    assert bytes(z["shape_bin"]) == M.shape_bin(H, W, B) and len(bytes(z["shape_bin"])) == 20
    assert np.array_equal(M.encode(z["rgb"], B, Q, fl, order)["k"], z["k"])
    assert np.array_equal(M.decode(z["k"], H, W, B, Q, fl, order)["rgb"], z["decoded"])


def test_extreme_case_clips_instead_of_wrapping():
    case = [c for c in CASES if c["name"] == "extreme_32x40_q1"][0]
    z = load(case)
    B, Q, fl = params(case)
    raw = (M.encode(z["rgb"], B, Q, fl)["coef32"] / np.float32(Q)).astype(np.int32) + 128
    assert np.count_nonzero(raw < 0) and np.count_nonzero(raw > 255)
    assert np.array_equal(z["k"], np.clip(raw, 0, 255).astype(np.uint8))
    assert not np.array_equal(z["k"], raw.astype(np.uint8))   # the DCT path's modulo-256 wrap differs


def test_robustness_manifest():
    """The generator verified both summation orders against the reference and recorded each case's
    distance to the nearest quantizer / truncation threshold."""
    m = mdct_manifest()
    assert m["generator"] == "tests/golden/make_golden_mdct.py"
    assert len(m["cases"]) >= 11
    for c in m["cases"]:
        assert c["min_index_margin"] >= 0 and c["min_pixel_margin"] >= 0
        z = load(c)
        assert list(z["k"].shape) == c["k_shape"]


@pytest.mark.parametrize("B", [8, 16])
def test_summation_orders_stay_within_the_cap(B):
    """The mid-size frame of the GPU test: the restatement's two accumulation orders differ in at
    most CAP of the positions, so the cap on left-out positions cannot hide a failure."""
    rgb = M.midsize_frame()
    a, b = M.encode(rgb, B, 32, 0, "fwd"), M.encode(rgb, B, 32, 0, "rev")
    assert np.count_nonzero(a["k"] != b["k"]) <= CAP * a["k"].size
    assert np.max(np.abs(a["coef64"] - b["coef64"])) <= 1e-12 * np.max(np.abs(a["coef64"]))
    H, W = rgb.shape[:2]
    da, db = M.decode(a["k"], H, W, B, 32, 0, "fwd"), M.decode(a["k"], H, W, B, 32, 0, "rev")
    assert np.count_nonzero(da["rgb"] != db["rgb"]) <= CAP * da["rgb"].size


# ---- host-only ABI ---------------------------------------------------------
def _padded(H, W, B):
    v = [ctypes.c_int32() for _ in range(4)]
    rc = L.lib().vcf_mdct_padded_shape(H, W, B, *[ctypes.byref(x) for x in v])
    return rc, tuple(x.value for x in v)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_padded_shape_equals_the_fixtures(case):
    z = load(case)
    B = params(case)[0]
    H, W = z["rgb"].shape[:2]
    rc, (Hp, Wp, top, left) = _padded(H, W, B)
    assert rc == 0
    assert (Hp, Wp) == z["k"].shape[:2]
    assert bytes(z["shape_bin"]) == np.array([H, W, 3, top, left], np.int32).tobytes()


def test_padded_shape_errors():
    assert _padded(0, 8, 8)[0] == L.VCF_ERR_INVALID
    assert _padded(8, 8, 1)[0] == L.VCF_ERR_UNSUPPORTED
    assert _padded(8, 8, 65)[0] == L.VCF_ERR_UNSUPPORTED
    assert L.lib().vcf_mdct_padded_shape(8, 8, 8, None, None, None, None) == L.VCF_ERR_INVALID


@pytest.mark.parametrize("fn", ["vcf_mdct_dz_encode", "vcf_mdct_dz_decode"])
@pytest.mark.parametrize("args,status", [
    (dict(block_size=1), L.VCF_ERR_UNSUPPORTED),
    (dict(block_size=65), L.VCF_ERR_UNSUPPORTED),
    (dict(Q=0), L.VCF_ERR_INVALID),
    (dict(Q=32768), L.VCF_ERR_INVALID),
    (dict(H=0), L.VCF_ERR_INVALID),
    (dict(flags=8), L.VCF_ERR_INVALID),
    (dict(n_frames=-1), L.VCF_ERR_INVALID),
    (dict(block_size=16, flags=2), L.VCF_ERR_UNSUPPORTED),   # -p away from B = 8: unpinned
])
def test_argument_errors_before_any_device_work(fn, args, status):
    a = dict(n_frames=1, H=8, W=8, block_size=8, Q=32, flags=0)
    a.update(args)
    dummy = ctypes.c_void_p(16)   # never dereferenced: validation fails first
    rc = getattr(L.lib(), fn)(dummy, a["n_frames"], a["H"], a["W"], a["block_size"], a["Q"], a["flags"], dummy, None)
    assert rc == status
    assert L.lib().vcf_last_error()


@pytest.mark.parametrize("fn", ["vcf_mdct_dz_encode", "vcf_mdct_dz_decode"])
def test_null_buffers_rejected(fn):
    assert getattr(L.lib(), fn)(None, 1, 8, 8, 8, 32, 0, None, None) == L.VCF_ERR_INVALID


# ---- command line ------------------------------------------------------------
def test_parser_accepts_the_reference_flags():
    from vcf_amd.codec import parser as P
    e = P.parse(P.mdct_parser(), ["encode", "-B", "12", "-t", "YCoCg", "-p", "-x", "-q", "7", "-c", "TIFF",
                                  "-o", "/tmp/a.png", "-e", "/tmp/b"])
    assert (e.block_size_MDCT, e.color_transform, e.perceptual_quantization, e.disable_subbands, e.QSS,
            e.entropy_image_codec, e.original, e.encoded) == (12, "YCoCg", True, True, 7, "TIFF", "/tmp/a.png", "/tmp/b")
    d = P.parse(P.mdct_parser(), ["decode"])
    assert (d.block_size_MDCT, d.color_transform, d.perceptual_quantization, d.disable_subbands, d.QSS,
            d.quantizer, d.filter, d.encoded, d.decoded) == (8, "YCoCg", False, False, 32, "deadzone", "no_filter",
                                                              "/tmp/encoded", "/tmp/decoded.png")
    i = P.parse(P.iii_parser(transform="2D-MDCT"), ["encode", "-T", "2D-MDCT", "-B", "16", "-N", "3"])
    assert (i.transform, i.block_size_MDCT, i.number_of_frames) == ("2D-MDCT", 16, 3)


def test_transform_codec_returns_the_mdct_codec():
    from vcf_amd.codec import parser as P
    from vcf_amd.codec.iii import transform_codec
    from vcf_amd.codec.mdct2d import CoDec
    c = transform_codec(P.parse(P.iii_parser(transform="2D-MDCT"), ["encode", "-T", "2D-MDCT", "-B", "12"]))
    assert isinstance(c, CoDec) and c.block_size == 12 and c.file_extension == ".tif"
    assert c.mdct_scale_factor == pytest.approx(4.0 + 4 / 24 * 4)


def test_options_outside_the_hip_path_are_refused():
    from vcf_amd.codec import parser as P
    from vcf_amd.codec.mdct2d import CoDec
    for argv in (["encode", "-a", "LloydMax"], ["encode", "-B", "65"], ["encode", "-B", "1"],
                 ["encode", "-p", "-B", "16"]):
        with pytest.raises(NotImplementedError):
            CoDec(P.parse(P.mdct_parser(), argv))

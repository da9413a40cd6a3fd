"""The 2D-KLT codec without a GPU: the numpy restatement (tests/klt_restated.py)
against the reference's own fixtures (tests/golden/klt_*.npz,
make_golden_klt.py), the host-only ABI, argument validation before any device
work, the refusals, the command-line surface, and the conditions under which
the block-size sweep of tests/test_klt_sweep_gpu.py means something
(tests/klt_sweep_cases.py)."""
import ctypes
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

import klt_restated as K
import klt_sweep_cases as S
import vcf_amd._lib as L
from test_mdct import CAP


def klt_manifest():
    with open(os.path.join(GOLDEN, "manifest_klt.json")) as f:
        return json.load(f)


def load(case):
    return np.load(os.path.join(GOLDEN, f"klt_{case['name']}.npz"))


def params(case):
    B, Q, fl = 8, 32, 0
    it = iter(case["flags"])
    for f in it:
        if f == "-B":
            B = int(next(it))
        elif f == "-q":
            Q = int(next(it))
        elif f == "-x":
            fl |= K.NO_SUBBANDS
    return B, Q, fl


CASES = klt_manifest()["cases"]
IDS = [c["name"] for c in CASES]
SEPARATED = ("smooth_61x77", "rand_40x48_b4_q8", "rand_64x72_q1")   # well-separated spectra


def test_fixture_set_is_the_one_the_codec_needs():
    assert set(IDS) == {"smooth_61x77", "rand_40x48_b4_q8", "rand_64x72_q1", "flat_48x56", "rand_40x48_x",
                        "smooth_37x45_b12", "rand_17x9_b2", "smooth_9x9_b8"}
    by = {c["name"]: c for c in CASES}
    assert params(by["smooth_61x77"]) == (8, 32, 0) and by["smooth_61x77"]["k_shape"] == [64, 80, 3]
    assert params(by["rand_40x48_b4_q8"]) == (4, 8, 0)
    assert params(by["rand_64x72_q1"]) == (8, 1, 0) and by["rand_64x72_q1"]["wrapped_indices"] > 0
    assert params(by["rand_40x48_x"]) == (8, 32, K.NO_SUBBANDS)
    assert params(by["smooth_37x45_b12"])[0] == 12 and by["smooth_37x45_b12"]["n_blocks"] == 16
    assert params(by["rand_17x9_b2"])[0] == 2
    assert by["smooth_9x9_b8"]["n_blocks"] == 4
    for c in CASES:
        assert os.path.getsize(os.path.join(GOLDEN, f"klt_{c['name']}.npz")) < 1024 * 1024
        assert c["name"] == "flat_48x56" or min(c["min_index_margin"], c["min_pixel_margin"]) >= 1e-9


def test_flat_case_has_no_covariance_at_all():
    """One colour all over: C = 0 exactly, every eigenvalue equal, the basis a permutation of the unit
    vectors -- every product and sum is exact, whatever the order."""
    case = [c for c in CASES if c["name"] == "flat_48x56"][0]
    z = load(case)
    assert len(np.unique(z["rgb"].reshape(-1, 3), axis=0)) == 1
    assert not np.any(K.covariance(z["rgb"], 8))
    w = z["weights64"]
    assert np.all((w == 0) | (np.abs(w) == 1)) and np.all(np.abs(w).sum(2) == 1) and np.all(np.abs(w).sum(1) == 1)


@pytest.mark.parametrize("case", CASES, ids=IDS)
@pytest.mark.parametrize("order", ["fwd", "rev"])
def test_restatement_equals_the_reference(case, order):
    """Indices given the reference's float64 weights, _shape.bin, and the decoded frame in float64
    (what the GPU does) and in float32 (what the reference does), in both accumulation orders."""
    z = load(case)
    B, Q, fl = params(case)
    H, W = z["rgb"].shape[:2]
    w64 = z["weights64"]
    w32 = w64.astype(np.float32)
    assert bytes(z["shape_bin"]) == K.shape_bin(H, W) and len(bytes(z["shape_bin"])) == 12
    assert z["k"].shape == tuple(K.padded_shape(H, W, B)[:2]) + (3,)
    assert np.array_equal(K.encode(z["rgb"], w64, B, Q, fl, order)["k"], z["k"])
    assert np.array_equal(K.decode(z["k"], H, W, w32, B, Q, fl, order, np.float64)["rgb"], z["decoded"])
    assert np.array_equal(K.decode(z["k"], H, W, w32, B, Q, fl, order, np.float32)["rgb"], z["decoded"])


def test_wrapping_case_wraps_instead_of_clipping():
    case = [c for c in CASES if c["name"] == "rand_64x72_q1"][0]
    z = load(case)
    B, Q, fl = params(case)
    raw = K.encode(z["rgb"], z["weights64"], B, Q, fl)["k32"]
    assert np.count_nonzero((raw < 0) | (raw > 255)) == case["wrapped_indices"] > 0
    assert np.array_equal(z["k"], raw.astype(np.uint8))
    assert not np.array_equal(z["k"], np.clip(raw, 0, 255).astype(np.uint8))


@pytest.mark.parametrize("name", SEPARATED)
def test_restated_training_finds_the_reference_basis(name):
    """Where the eigenvalues are distinct the basis is determined up to the sign of each row."""
    z = load([c for c in CASES if c["name"] == name][0])
    B = params([c for c in CASES if c["name"] == name][0])[0]
    w = K.train(z["rgb"], B)
    dots = np.einsum("ckj,ckj->ck", w, z["weights64"])
    assert np.max(np.abs(np.abs(dots) - 1)) <= 1e-9
    assert np.max(np.abs(w * np.sign(dots)[..., None] - z["weights64"])) <= 1e-9


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_covariance_from_integer_moments(case):
    """The product forms C from exact integer sums; np.cov of the float32 blocks is the reference's."""
    z = load(case)
    B = params(case)[0]
    H, W = z["rgb"].shape[:2]
    S1, S2 = K.moments(z["rgb"], B)
    assert S1.dtype == np.int64 and S2.dtype == np.int64 and np.array_equal(S2, S2.transpose(0, 2, 1))
    C = K.covariance(z["rgb"], B)
    Cm = K.covariance_from_moments(S1, S2, K.n_blocks(H, W, B))
    assert np.max(np.abs(C - Cm)) <= 1e-12 * max(np.max(np.abs(C)), 1.0)


@pytest.mark.parametrize("B", [8, 16])
def test_summation_orders_stay_within_the_cap(B):
    """The mid-size frame of the GPU test: the restatement's two accumulation orders differ in at
    most CAP of the positions, so the cap on left-out positions cannot hide a failure."""
    rgb = K.midsize_frame()
    H, W = rgb.shape[:2]
    w64 = K.train(rgb, B)
    a, b = K.encode(rgb, w64, B, 32, 0, "fwd"), K.encode(rgb, w64, B, 32, 0, "rev")
    assert np.count_nonzero(a["k"] != b["k"]) <= CAP * a["k"].size
    assert np.max(np.abs(a["pre"] - b["pre"])) <= 1e-12 * np.max(np.abs(a["pre"]))
    w32 = w64.astype(np.float32)
    da, db = K.decode(a["k"], H, W, w32, B, 32, 0, "fwd"), K.decode(a["k"], H, W, w32, B, 32, 0, "rev")
    assert np.count_nonzero(da["rgb"] != db["rgb"]) <= CAP * da["rgb"].size


# ---- the block-size sweep (tests/klt_sweep_cases.py): what keeps it honest ----------
@pytest.mark.parametrize("name", S.ENCODE_IDS)
def test_sweep_encode_cases_do_not_depend_on_the_summation_order(name):
    """On the sweep's frame CAP * size is about 1 position, so the reference alone must be exact:
    both accumulation orders give the same indices and the same pixels.  At Q = 1 the case is there
    for the encoder's wrap to u8: at least 1 % of the indices leave 0..255."""
    case = S.by_name(name)
    a = S.encoded(name)
    assert np.array_equal(a["k"], S.encode(case, "rev")["k"])
    assert np.array_equal(S.decoded(name)["rgb"], S.decode(case, a["k"], "rev")["rgb"])
    wrapped = np.mean((a["k32"] < 0) | (a["k32"] > 255))
    print(f"{name}: {wrapped:.4f} of the indices wrap")
    if case["Q"] == 1:
        assert wrapped >= 0.01
        assert not np.array_equal(a["k"], np.clip(a["k32"], 0, 255).astype(np.uint8))


@pytest.mark.parametrize("name", S.RAW_IDS)
def test_sweep_raw_cases_are_fit_to_decode(name):
    """Index frames no encoder writes: the decode does not depend on the summation order and at most
    half of the pixels are clipped."""
    case = S.by_name(name)
    k = S.raw_k(name)
    d = S.decoded(name)
    assert np.array_equal(d["rgb"], S.decode(case, k, "rev")["rgb"])
    saturated = np.mean((d["rgb"] == 0) | (d["rgb"] == 255))
    wrapping = np.count_nonzero(np.abs(case["Q"] * (k.astype(np.int64) - 128)) > 32767)
    print(f"{name}: {saturated:.4f} of the pixels at 0 or 255, {wrapping} indices wrap in int16")
    assert saturated <= 0.5
    if case["Q"] == 1:
        assert len(np.unique(k)) == 256
    else:
        assert wrapping >= 1


def test_sweep_weights_are_orthonormal():
    for B in S.SWEEP_B:
        w = S.weights(B)
        assert w.shape == (3, B * B, B * B) and w.dtype == np.float64
        assert np.max(np.abs(w @ w.transpose(0, 2, 1) - np.eye(B * B))) <= 1e-12
        assert S.weights32(B).dtype == np.float32


def test_restatement_refuses_what_the_reference_cannot_do():
    rgb = np.zeros((8, 8, 3), np.uint8)
    with pytest.raises(ValueError):
        K.blocks(rgb, 1)
    with pytest.raises(ValueError):
        K.blocks(rgb, 8)       # one block


# ---- host-only ABI ---------------------------------------------------------
def _padded(H, W, B):
    v = [ctypes.c_int32() for _ in range(4)]
    rc = L.lib().vcf_klt_padded_shape(H, W, B, *[ctypes.byref(x) for x in v])
    return rc, tuple(x.value for x in v)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_padded_shape_equals_the_fixtures(case):
    z = load(case)
    B = params(case)[0]
    H, W = z["rgb"].shape[:2]
    rc, got = _padded(H, W, B)
    assert rc == 0 and got == K.padded_shape(H, W, B) and got[:2] == z["k"].shape[:2]


def test_padded_shape_errors():
    assert _padded(0, 8, 8)[0] == L.VCF_ERR_INVALID
    assert _padded(8, 8, 1)[0] == L.VCF_ERR_INVALID
    assert _padded(8, 8, 17)[0] == L.VCF_ERR_UNSUPPORTED
    assert L.lib().vcf_klt_padded_shape(8, 8, 8, None, None, None, None) == L.VCF_ERR_INVALID
    assert _padded(61, 77, 8) == (0, (64, 80, 1, 1))
    assert _padded(9, 9, 8) == (0, (16, 16, 3, 3))


BAD_ARGS = [
    (dict(block_size=1), L.VCF_ERR_INVALID),
    (dict(block_size=0), L.VCF_ERR_INVALID),
    (dict(block_size=17), L.VCF_ERR_UNSUPPORTED),
    (dict(block_size=64), L.VCF_ERR_UNSUPPORTED),
    (dict(H=8, W=8), L.VCF_ERR_INVALID),          # one block
    (dict(H=3, W=5), L.VCF_ERR_INVALID),          # one block after the pad
    (dict(H=0), L.VCF_ERR_INVALID),
    (dict(W=-1), L.VCF_ERR_INVALID),
    (dict(n_frames=0), L.VCF_ERR_INVALID),
    (dict(n_frames=-1), L.VCF_ERR_INVALID),
]


@pytest.mark.parametrize("fn", ["vcf_klt_dz_encode", "vcf_klt_dz_decode"])
@pytest.mark.parametrize("args,status", BAD_ARGS + [
    (dict(Q=0), L.VCF_ERR_INVALID),
    (dict(Q=32768), L.VCF_ERR_INVALID),
    (dict(flags=2), L.VCF_ERR_INVALID),           # -p is not an option of this codec
    (dict(flags=8), L.VCF_ERR_INVALID),
])
def test_argument_errors_before_any_device_work(fn, args, status):
    a = dict(n_frames=1, H=16, W=16, block_size=8, Q=32, flags=0)
    a.update(args)
    dummy = ctypes.c_void_p(16)   # never dereferenced: validation fails first
    rc = getattr(L.lib(), fn)(dummy, a["n_frames"], a["H"], a["W"], a["block_size"], a["Q"], a["flags"], dummy,
                              dummy, None)
    assert rc == status
    assert L.lib().vcf_last_error()


@pytest.mark.parametrize("args,status", BAD_ARGS)
def test_moments_argument_errors_before_any_device_work(args, status):
    a = dict(n_frames=1, H=16, W=16, block_size=8)
    a.update(args)
    dummy = ctypes.c_void_p(16)
    assert L.lib().vcf_klt_moments(dummy, a["n_frames"], a["H"], a["W"], a["block_size"], dummy, dummy, None) == status
    assert L.lib().vcf_last_error()


def test_null_buffers_rejected():
    d = ctypes.c_void_p(16)
    for bufs in ((None, d, d), (d, None, d), (d, d, None)):
        assert L.lib().vcf_klt_dz_encode(bufs[0], 1, 16, 16, 8, 32, 0, bufs[1], bufs[2], None) == L.VCF_ERR_INVALID
        assert L.lib().vcf_klt_dz_decode(bufs[0], 1, 16, 16, 8, 32, 0, bufs[1], bufs[2], None) == L.VCF_ERR_INVALID
        assert L.lib().vcf_klt_moments(bufs[0], 1, 16, 16, 8, bufs[1], bufs[2], None) == L.VCF_ERR_INVALID


# ---- the wrapper's refusals (host only: nothing is allocated first) ----------
def test_wrapper_refusals():
    import vcf_amd.klt as G
    rgb = np.zeros((16, 16, 3), np.uint8)
    with pytest.raises(ValueError):
        G.encode(rgb, B=1)
    with pytest.raises(NotImplementedError):
        G.encode(rgb, B=17)
    with pytest.raises(ValueError):
        G.encode(rgb, B=16)                        # one block
    with pytest.raises(ValueError):
        G.train(np.zeros((5, 7, 3), np.uint8), 8)   # one block after the pad
    with pytest.raises(ValueError):
        G.moments(rgb, 16)
    with pytest.raises(ValueError):
        G.decode(np.zeros((16, 16, 3), np.uint8), 16, 16, B=16, weights32=np.zeros((3, 256, 256), np.float32))
    assert G.shape_bin(61, 77) == K.shape_bin(61, 77)


# ---- command line ------------------------------------------------------------
def test_parser_accepts_the_reference_flags():
    from vcf_amd.codec import parser as P
    e = P.parse(P.klt_parser(), ["encode", "-B", "12", "-t", "YCoCg", "-x", "-q", "7", "-c", "TIFF",
                                 "-o", "/tmp/a.png", "-e", "/tmp/b"])
    assert (e.block_size, e.color_transform, e.disable_subbands, e.QSS, e.entropy_image_codec, e.original,
            e.encoded) == (12, "YCoCg", True, 7, "TIFF", "/tmp/a.png", "/tmp/b")
    assert not hasattr(e, "block_size_DCT") and not hasattr(e, "perceptual_quantization") and not hasattr(e, "Lambda")
    d = P.parse(P.klt_parser(), ["decode"])
    assert (d.block_size, d.color_transform, d.disable_subbands, d.QSS, d.quantizer, d.filter, d.encoded,
            d.decoded) == (8, "YCoCg", False, 32, "deadzone", "no_filter", "/tmp/encoded", "/tmp/decoded.png")
    i = P.parse(P.iii_parser(transform="2D-KLT"), ["encode", "-T", "2D-KLT", "-B", "16", "-N", "3"])
    assert (i.transform, i.block_size, i.number_of_frames) == ("2D-KLT", 16, 3)


def test_transform_codec_returns_the_klt_codec():
    from vcf_amd.codec import parser as P
    from vcf_amd.codec.iii import transform_codec
    from vcf_amd.codec.klt2d import CoDec
    c = transform_codec(P.parse(P.iii_parser(transform="2D-KLT"), ["encode", "-T", "2D-KLT", "-B", "12", "-x"]))
    assert isinstance(c, CoDec) and c.block_size == 12 and c.file_extension == ".tif" and c.flags == 1
    with pytest.raises(NotImplementedError, match="2D-KLT"):
        transform_codec(P.parse(P.iii_parser(), ["encode", "-T", "LBT"]))


def test_options_outside_the_hip_path_are_refused():
    from vcf_amd.codec import parser as P
    from vcf_amd.codec.klt2d import CoDec
    for argv in (["encode", "-a", "LloydMax"], ["encode", "-t", "YCrCb"], ["decode", "-f", "gaussian_blur"],
                 ["encode", "-B", "17"]):
        with pytest.raises(NotImplementedError):
            CoDec(P.parse(P.klt_parser(), argv))
    with pytest.raises(ValueError):
        CoDec(P.parse(P.klt_parser(), ["encode", "-B", "1"]))
    CoDec(P.parse(P.klt_parser(), ["encode", "-B", "2"]))
    CoDec(P.parse(P.klt_parser(), ["decode", "-B", "16"]))


def test_codec_refuses_a_one_block_frame(tmp_path):
    from PIL import Image
    from vcf_amd.codec import parser as P
    from vcf_amd.codec.klt2d import CoDec
    src = str(tmp_path / "in.png")
    Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(src)
    with pytest.raises(ValueError):
        CoDec(P.parse(P.klt_parser(), ["encode"])).encode_fn(src, str(tmp_path / "enc"))

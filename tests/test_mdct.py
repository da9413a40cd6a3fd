"""The lapped 2D-MDCT codec without a GPU: the numpy restatement
(tests/mdct_restated.py) against the reference's own fixtures
(tests/golden/mdct_*.npz, make_golden_mdct.py), the host-only ABI, argument
validation before any device work, the command-line surface, and the
conditions under which the block-size sweep of tests/test_mdct_sweep_gpu.py
means something (tests/mdct_sweep_cases.py)."""
import ctypes
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

import mdct_restated as M
import mdct_sweep_cases as S
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


# ---- the block-size sweep (tests/mdct_sweep_cases.py): what keeps it honest --------
def _plan(case, decode):
    """(TX, TY, lds_class, tiles_x, tiles_y) of the launch, from the library itself."""
    import vcf_amd.mdct as G
    H, W = case["shape"]
    return G.tile_plan(H, W, case["B"], case["flags"], decode)


@pytest.mark.parametrize("name", S.ENCODE_IDS)
def test_sweep_encode_cases_do_not_depend_on_the_summation_order(name):
    """At these sizes CAP * size is 1 to 4 positions, so the GPU comparison is all but exact and the
    reference alone must be exact: both accumulation orders give the same indices and pixels."""
    case = S.by_name(name)
    a = S.encoded(name)
    assert np.array_equal(a["k"], S.encode(case, "rev")["k"])
    assert np.array_equal(S.decoded(name)["rgb"], S.decode(case, a["k"], "rev")["rgb"])


@pytest.mark.parametrize("name", S.RAW_IDS)
def test_sweep_raw_cases_are_fit_to_decode(name):
    """Conditions on the inputs no encoder writes: the decode does not depend on the summation order,
    at most half of the pixels are clipped, and a wrap case does wrap."""
    case = S.by_name(name)
    k = S.raw_k(name)
    d = S.decoded(name)
    assert np.array_equal(d["rgb"], S.decode(case, k, "rev")["rgb"])
    saturated = np.mean((d["rgb"] == 0) | (d["rgb"] == 255))
    wrapping = np.count_nonzero(np.abs(case["Q"] * (k.astype(np.int64) - 128)) > 32767)
    print(f"{name}: {saturated:.4f} of the pixels at 0 or 255, {wrapping} wrapping coefficients")
    assert saturated <= 0.5
    if case["kind"] == "wrap":
        assert wrapping >= 100
        y = (case["Q"] * (k.astype(np.int32) - 128)).astype(np.int16)
        assert np.max(np.abs(y.astype(np.int32))) <= case["bound"]
    else:
        assert case["Q"] == 1 and len(np.unique(k)) == case["hi"] - case["lo"] + 1


def _reachable(flags, decode):
    """The LDS classes the launch can pick at all: over every block size the flags allow and frames
    from one block to 4K."""
    import vcf_amd.mdct as G
    sizes = (1, 9, 24, 61, 97, 150, 256, 480, 1080, 2160, 3840)
    return {G.tile_plan(H, W, B, flags, decode)[2]
            for B in ((8,) if flags & M.PERCEPTUAL else range(2, 65)) for H in sizes for W in sizes}


def test_sweep_reaches_every_lds_class():
    """What the sweep launches, from vcf_mdct_tile_plan: encode, decode and decode with -p (float
    coefficients in LDS) each meet every LDS class they can reach; class 2 runs with tiles of more
    than one block, at least 2 each way; every class, and every case whose tiles can be, has a
    partial last tile.  Retuning pick_tile so that the sweep stops reaching a class fails here."""
    met = {("encode", 0): {}, ("decode", 0): {}, ("decode", M.PERCEPTUAL): {}}
    for case in S.ENCODE + S.RAW:
        partial, one_block = False, True
        for decode in (False, True):
            if not decode and "kind" in case:
                continue
            TX, TY, cls, tx, ty = _plan(case, decode)
            ex, ey = S.extents(case, decode)
            part = "x" * bool(ex % TX) + "y" * bool(ey % TY)
            print(f"{case['name']:>22} {'decode' if decode else 'encode'}: tile {TX}x{TY}, class {cls}, {tx}x{ty} tiles"
                  f" of {ex}x{ey}" + (f", last one partial in {part}" if part else ""))
            assert (tx, ty) == ((ex + TX - 1) // TX, (ey + TY - 1) // TY)
            assert tx * ty > 1 or case["shape"] != S.FRAME
            partial, one_block = partial or bool(part), one_block and TX * TY == 1
            key = ("decode", case["flags"] & M.PERCEPTUAL) if decode else ("encode", 0)
            met[key].setdefault(cls, []).append((TX, TY, tx, ty, part))
        # a tile of one block is never partial (B = 63, 64); the 1 x 2 and 2 x 1 tiles of B = 40
        # divide its 8 x 6 blocks and 6 x 4 segments
        assert partial or one_block or case["name"] in S.WHOLE_TILES, case["name"]
    for (what, perc), by_class in met.items():
        assert set(by_class) == _reachable(perc, what == "decode"), (what, perc, sorted(by_class))
        for cls, plans in by_class.items():
            assert any(p[4] for p in plans), (what, perc, cls, "no partial last tile")
    for key, by_class in met.items():
        assert any(TX * TY > 1 and tx >= 2 and ty >= 2 for TX, TY, tx, ty, _ in by_class[2]), key
    # the -p decoder, in each of its classes: a seam in y and a partial last tile in y
    for cls, plans in met[("decode", M.PERCEPTUAL)].items():
        assert any(ty >= 2 and "y" in part for _, _, _, ty, part in plans), cls


def test_tile_plan_errors():
    v = [ctypes.c_int32() for _ in range(5)]
    p = [ctypes.byref(x) for x in v]
    f = L.lib().vcf_mdct_tile_plan
    assert f(150, 210, 8, 0, 0, *p) == 0 and all(x.value >= 0 for x in v)
    assert f(0, 210, 8, 0, 0, *p) == L.VCF_ERR_INVALID
    assert f(150, 210, 65, 0, 1, *p) == L.VCF_ERR_UNSUPPORTED
    assert f(150, 210, 16, 2, 1, *p) == L.VCF_ERR_UNSUPPORTED   # -p away from B = 8, as the launches
    assert f(150, 210, 8, 8, 0, *p) == L.VCF_ERR_INVALID
    assert f(150, 210, 8, 0, 0, None, None, None, None, None) == L.VCF_ERR_INVALID


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

"""The lapped 2D-MDCT kernels on the GPU.

On the reference's own fixtures (tests/golden/mdct_*.npz, robust against the
order of the float64 sums by construction) the GPU must equal the reference
exactly: indices, .tif bytes, _shape.bin bytes, decoded pixels.  For inputs
without a fixture the numpy restatement (tests/mdct_restated.py) is the
reference; a position may be left out only if the restatement's own float64
value lies within 1e-9 of a quantizer / truncation threshold and the GPU value
is exactly one step away, at most 1 in 10^5 positions per case."""
import os

import numpy as np
import pytest

import mdct_restated as M
from test_mdct import CAP, CASES, IDS, load, params

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    import vcf_amd.mdct as G
    return G


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fixtures_through_the_c_abi(G, case):
    z = load(case)
    B, Q, fl = params(case)
    H, W = z["rgb"].shape[:2]
    assert G.shape_bin(H, W, B) == bytes(z["shape_bin"])
    assert np.array_equal(G.encode(z["rgb"], Q, fl, B), z["k"])
    assert np.array_equal(G.decode(z["k"], H, W, Q, fl, B), z["decoded"])


def test_batch_equals_single_frames(G):
    frames = np.stack([M.synth_frame(61, 77, s) for s in (1, 2, 3)])
    for B in (8, 12):
        k = G.encode(frames, 32, 0, B)
        y = G.decode(k, 61, 77, 32, 0, B)
        for i in range(3):
            ki = G.encode(frames[i], 32, 0, B)
            assert np.array_equal(k[i], ki)
            assert np.array_equal(y[i], G.decode(ki, 61, 77, 32, 0, B))
        assert not np.array_equal(k[0], k[1])


def _args(sub, case, extra=()):
    from vcf_amd.codec import parser as P
    return P.parse(P.mdct_parser(), [sub] + list(case["flags"]) + list(extra))


@pytest.mark.parametrize("name", ["smooth_37x45_b12", "smooth_64x64_p"])
def test_codec_files_are_byte_equal(tmp_path, name):
    from PIL import Image
    from vcf_amd.codec.mdct2d import CoDec
    case = [c for c in CASES if c["name"] == name][0]
    z = load(case)
    src, enc, dec = str(tmp_path / "in.png"), str(tmp_path / "enc"), str(tmp_path / "dec.png")
    Image.fromarray(z["rgb"]).save(src)
    n = CoDec(_args("encode", case)).encode_fn(src, enc)
    assert open(enc + ".tif", "rb").read() == bytes(z["tif"]) and n == len(bytes(z["tif"]))
    assert open(enc + "_shape.bin", "rb").read() == bytes(z["shape_bin"])
    CoDec(_args("decode", case)).decode_fn(enc, dec)
    assert np.array_equal(np.array(Image.open(dec)), z["decoded"])


def test_iii_with_the_mdct_transform(tmp_path):
    from PIL import Image
    from vcf_amd.codec import parser as P
    from vcf_amd.codec.iii import CoDec
    frames = [M.synth_frame(37, 45, s) for s in (4, 5, 6)]
    for i, f in enumerate(frames):
        Image.fromarray(f).save(str(tmp_path / ("orig_%04d.png" % i)))
    kw = dict(encode_prefix=str(tmp_path / "enc"), decode_prefix=str(tmp_path / "dec"))
    common = ["-T", "2D-MDCT", "-N", "3", "-B", "8", "-q", "16"]
    e = CoDec(P.parse(P.iii_parser(transform="2D-MDCT"),
                      ["encode"] + common + ["-o", str(tmp_path / "orig_%04d.png")]), **kw)
    total = e.encode()
    assert total == sum(os.path.getsize(str(tmp_path / ("enc_%04d.tif" % i))) for i in range(3))
    CoDec(P.parse(P.iii_parser(transform="2D-MDCT"), ["decode"] + common), **kw).decode()
    from vcf_amd.codec.tiff import imread_bytes
    for i, f in enumerate(frames):
        want = M.encode(f, 8, 16)
        k = imread_bytes(open(str(tmp_path / ("enc_%04d.tif" % i)), "rb").read())
        _compare("III indices", k, want["k"], M.index_margin(want["pre"], 16))
        assert open(str(tmp_path / ("enc_%04d_shape.bin" % i)), "rb").read() == M.shape_bin(37, 45, 8)
        d = M.decode(k, 37, 45, 8, 16)
        _compare("III pixels", np.array(Image.open(str(tmp_path / ("dec_%04d.png" % i)))), d["rgb"],
                 M.pixel_margin(d["pre"]))


def _compare(what, got, want, margin):
    """Exact, but for positions within 1e-9 of a threshold where the GPU is one step away; at most
    CAP of the positions."""
    diff = got.astype(np.int32) - want.astype(np.int32)
    bad = diff != 0
    excused = bad & (margin < 1e-9) & (np.abs(diff) == 1)
    print(f"{what}: {np.count_nonzero(bad)} differing, {np.count_nonzero(excused)} at a threshold, of {bad.size}")
    assert not np.any(bad & ~excused), f"{what}: {np.count_nonzero(bad & ~excused)} positions differ"
    assert np.count_nonzero(excused) <= CAP * bad.size


@pytest.fixture(scope="module")
def midsize():
    rgb = M.midsize_frame()
    return rgb, {B: M.encode(rgb, B, 32, 0) for B in (8, 16)}


@pytest.mark.parametrize("B", [8, 16])
def test_midsize_against_the_restatement(G, midsize, B):
    rgb, ref = midsize
    H, W = rgb.shape[:2]
    want = ref[B]
    _compare("indices", G.encode(rgb, 32, 0, B), want["k"], M.index_margin(want["pre"], 32))
    d = M.decode(want["k"], H, W, B, 32, 0)
    _compare("pixels", G.decode(want["k"], H, W, 32, 0, B), d["rgb"], M.pixel_margin(d["pre"]))

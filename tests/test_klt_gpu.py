"""The 2D-KLT kernels on the GPU.

The moments are integer sums: they must equal the numpy int64 restatement bit
for bit.  On the reference's own fixtures (tests/golden/klt_*.npz, robust
against the order of the sums by construction) the transforms, given the
reference's weights, must equal the reference exactly: indices, _shape.bin
bytes, decoded pixels.  For inputs without a fixture the numpy restatement
(tests/klt_restated.py) is the reference; a position may be left out only if
the restatement's own float64 value lies within 1e-9 of a quantizer /
truncation threshold and the GPU value is exactly one step away, at most 1 in
10^5 positions per case.  Training is pinned by properties, and to the
reference's basis where the spectrum determines it."""
import os

import numpy as np
import pytest

import klt_restated as K
from test_klt import CASES, IDS, SEPARATED, load, params
from test_mdct import CAP

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    import vcf_amd.klt as G
    return G


def _compare(what, got, want, margin):
    """Exact, but for positions within 1e-9 of a threshold where the GPU is one step away (modulo
    256 for the wrapped indices); at most CAP of the positions."""
    diff = got.astype(np.int32) - want.astype(np.int32)
    bad = diff != 0
    step = (np.abs(diff) == 1) | (np.abs(diff) == 255)
    excused = bad & (margin < 1e-9) & step
    print(f"{what}: {np.count_nonzero(bad)} differing, {np.count_nonzero(excused)} at a threshold, of {bad.size}")
    assert not np.any(bad & ~excused), f"{what}: {np.count_nonzero(bad & ~excused)} positions differ"
    assert np.count_nonzero(excused) <= CAP * bad.size


# ---- 1. moments --------------------------------------------------------------
def _moments_equal(G, rgb, B):
    S1, S2 = G.moments(rgb, B)
    R1, R2 = K.moments(rgb, B)
    assert S1.dtype == np.int64 and S2.dtype == np.int64
    assert np.array_equal(S1, R1) and np.array_equal(S2, R2)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_moments_are_exact_on_the_fixtures(G, case):
    _moments_equal(G, load(case)["rgb"], params(case)[0])


@pytest.mark.parametrize("B", [8, 16])
def test_moments_are_exact_midsize(G, B):
    _moments_equal(G, K.midsize_frame(), B)


@pytest.mark.parametrize("B", [2, 8, 16])
def test_moments_are_exact_on_a_checkerboard(G, B):
    """0 / 255 pixel by pixel: the extreme |s|."""
    y, x = np.mgrid[0:64, 0:64]
    rgb = np.repeat((((x + y) & 1) * 255).astype(np.uint8)[..., None], 3, 2)
    rgb[..., 1] = 255 - rgb[..., 1]
    _moments_equal(G, rgb, B)


def test_moments_batch_equals_single_frames(G):
    frames = np.stack([K.synth_frame(61, 77, s) for s in (1, 2, 3)])
    S1, S2 = G.moments(frames, 8)
    assert S1.shape == (3, 3, 64) and S2.shape == (3, 3, 64, 64)
    for i in range(3):
        R1, R2 = K.moments(frames[i], 8)
        assert np.array_equal(S1[i], R1) and np.array_equal(S2[i], R2)
        a1, a2 = G.moments(frames[i], 8)
        assert np.array_equal(S1[i], a1) and np.array_equal(S2[i], a2)
    assert not np.array_equal(S2[0], S2[1])


# ---- 2. fixtures through the C ABI ---------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fixtures_through_the_c_abi(G, case):
    z = load(case)
    B, Q, fl = params(case)
    H, W = z["rgb"].shape[:2]
    w64 = z["weights64"]
    assert G.shape_bin(H, W) == bytes(z["shape_bin"])
    k, w = G.encode(z["rgb"], Q, fl, B, weights=w64)
    assert np.array_equal(k, z["k"]) and np.array_equal(w, w64)
    assert np.array_equal(G.decode(z["k"], H, W, Q, fl, B, w64.astype(np.float32)), z["decoded"])


# ---- 3. mid-size, no fixture -----------------------------------------------------
@pytest.fixture(scope="module")
def midsize():
    rgb = K.midsize_frame()
    out = {}
    for B in (8, 16):
        w64 = K.train(rgb, B)
        out[B] = (w64, K.encode(rgb, w64, B, 32, 0))
    return rgb, out


@pytest.mark.parametrize("B", [8, 16])
def test_midsize_against_the_restatement(G, midsize, B):
    rgb, ref = midsize
    H, W = rgb.shape[:2]
    w64, want = ref[B]
    w32 = w64.astype(np.float32)
    _compare("indices", G.encode(rgb, 32, 0, B, weights=w64)[0], want["k"], K.index_margin(want["pre"], 32))
    d = K.decode(want["k"], H, W, w32, B, 32, 0)
    _compare("pixels", G.decode(want["k"], H, W, 32, 0, B, w32), d["rgb"], K.pixel_margin(d["pre"]))


def test_batch_equals_single_frames(G):
    """Every frame of a batch with its own weights; no result depends on the batch position."""
    frames = np.stack([K.synth_frame(61, 77, s) for s in (1, 2, 3)])
    for B in (8, 5):
        k, w = G.encode(frames, 32, 0, B)
        assert w.shape == (3, 3, B * B, B * B) and w.dtype == np.float64
        y = G.decode(k, 61, 77, 32, 0, B, w.astype(np.float32))
        for i in range(3):
            ki, _ = G.encode(frames[i], 32, 0, B, weights=w[i])
            assert np.array_equal(k[i], ki)
            assert np.array_equal(y[i], G.decode(ki, 61, 77, 32, 0, B, w[i].astype(np.float32)))
        assert not np.array_equal(k[0], k[1])


# ---- 4. training -------------------------------------------------------------------
@pytest.mark.parametrize("name", SEPARATED)
def test_training_finds_the_reference_basis(G, name):
    case = [c for c in CASES if c["name"] == name][0]
    z = load(case)
    w = G.train(z["rgb"], params(case)[0])
    ref = z["weights64"]
    sign = np.sign(np.einsum("ckj,ckj->ck", w, ref))[..., None]
    err = np.max(np.abs(w * sign - ref))
    print(f"{name}: rows equal the reference's up to sign within {err:.3g}")
    assert err <= 1e-9


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_training_properties(G, case):
    z = load(case)
    B = params(case)[0]
    D = B * B
    w = G.train(z["rgb"], B)
    assert w.shape == (3, D, D) and w.dtype == np.float64
    C = K.covariance(z["rgb"], B)
    for c in range(3):
        lam = np.linalg.eigvalsh(C[c])[::-1]
        lmax = max(lam[0], 0.0)
        orth = np.max(np.abs(w[c] @ w[c].T - np.eye(D)))
        M = w[c] @ C[c] @ w[c].T
        off = np.max(np.abs(M - np.diag(np.diag(M))))
        dg = np.diag(M)
        print(f"{case['name']} ch {c}: |W W^T - I| {orth:.3g}, off-diagonal {off:.3g}, "
              f"diagonal - eigenvalues {np.max(np.abs(dg - lam)):.3g}, lambda_max {lmax:.6g}")
        assert orth <= 1e-12
        assert off <= 1e-12 * lmax
        assert np.all(np.diff(dg) <= 1e-9 * lmax)
        assert np.max(np.abs(dg - lam)) <= 1e-9 * lmax


# ---- 5. codec files ------------------------------------------------------------------
def _args(sub, case, extra=()):
    from vcf_amd.codec import parser as P
    return P.parse(P.klt_parser(), [sub] + list(case["flags"]) + list(extra))


@pytest.mark.parametrize("name", ["smooth_61x77", "rand_40x48_x", "smooth_37x45_b12"])
def test_decode_fn_reads_the_reference_files(tmp_path, name):
    from PIL import Image
    from vcf_amd.codec.klt2d import CoDec
    case = [c for c in CASES if c["name"] == name][0]
    z = load(case)
    enc, dec = str(tmp_path / "enc"), str(tmp_path / "dec.png")
    open(enc + ".tif", "wb").write(bytes(z["tif"]))
    open(enc + "_shape.bin", "wb").write(bytes(z["shape_bin"]))
    np.savez_compressed(enc + "_weights.npz", weights=z["weights64"].astype(np.float32))
    CoDec(_args("decode", case)).decode_fn(enc, dec)
    assert np.array_equal(np.array(Image.open(dec)), z["decoded"])


@pytest.mark.parametrize("name", ["smooth_61x77", "rand_40x48_b4_q8"])
def test_encode_fn_writes_the_three_files(tmp_path, name):
    from PIL import Image
    from vcf_amd.codec.klt2d import CoDec
    from vcf_amd.codec.tiff import imread_bytes
    case = [c for c in CASES if c["name"] == name][0]
    z = load(case)
    B, Q, fl = params(case)
    H, W = z["rgb"].shape[:2]
    src, enc, dec = str(tmp_path / "in.png"), str(tmp_path / "enc"), str(tmp_path / "dec.png")
    Image.fromarray(z["rgb"]).save(src)
    n = CoDec(_args("encode", case)).encode_fn(src, enc)
    assert n == os.path.getsize(enc + ".tif")
    assert open(enc + "_shape.bin", "rb").read() == bytes(z["shape_bin"])
    with np.load(enc + "_weights.npz") as f:
        assert list(f.keys()) == ["weights"]
        w32 = f["weights"]
    assert w32.dtype == np.float32 and w32.shape == (3, B * B, B * B)
    k = imread_bytes(open(enc + ".tif", "rb").read())
    assert k.shape == z["k"].shape and k.dtype == np.uint8
    CoDec(_args("decode", case)).decode_fn(enc, dec)
    d = K.decode(k, H, W, w32, B, Q, fl)
    _compare("pixels of our own files", np.array(Image.open(dec)), d["rgb"], K.pixel_margin(d["pre"]))


# ---- 6. III -------------------------------------------------------------------------------
def test_iii_with_the_klt_transform(tmp_path):
    from PIL import Image
    from vcf_amd.codec import parser as P
    from vcf_amd.codec.iii import CoDec
    from vcf_amd.codec.klt2d import CoDec as KLT
    from vcf_amd.codec.tiff import imread_bytes
    frames = [K.synth_frame(37, 45, s) for s in (4, 5, 6)]
    for i, f in enumerate(frames):
        Image.fromarray(f).save(str(tmp_path / ("orig_%04d.png" % i)))
    kw = dict(encode_prefix=str(tmp_path / "enc"), decode_prefix=str(tmp_path / "dec"))
    common = ["-T", "2D-KLT", "-N", "3", "-B", "8", "-q", "16"]
    e = CoDec(P.parse(P.iii_parser(transform="2D-KLT"),
                      ["encode"] + common + ["-o", str(tmp_path / "orig_%04d.png")]), **kw)
    total = e.encode()
    assert total == sum(os.path.getsize(str(tmp_path / ("enc_%04d.tif" % i))) for i in range(3))
    CoDec(P.parse(P.iii_parser(transform="2D-KLT"), ["decode"] + common), **kw).decode()
    single = KLT(P.parse(P.klt_parser(), ["encode", "-B", "8", "-q", "16"]))
    for i, f in enumerate(frames):
        for ext in (".tif", "_shape.bin", "_weights.npz"):
            assert os.path.exists(str(tmp_path / ("enc_%04d" % i)) + ext)
        assert open(str(tmp_path / ("enc_%04d_shape.bin" % i)), "rb").read() == K.shape_bin(37, 45)
        k = imread_bytes(open(str(tmp_path / ("enc_%04d.tif" % i)), "rb").read())
        with np.load(str(tmp_path / ("enc_%04d_weights.npz" % i))) as z:
            w32 = z["weights"]
        assert w32.dtype == np.float32 and w32.shape == (3, 64, 64)
        d = K.decode(k, 37, 45, w32, 8, 16)
        _compare("III pixels", np.array(Image.open(str(tmp_path / ("dec_%04d.png" % i)))), d["rgb"],
                 K.pixel_margin(d["pre"]))
        # the batch equals the frame coded alone
        one = str(tmp_path / ("one_%04d" % i))
        single.encode_fn(str(tmp_path / ("orig_%04d.png" % i)), one)
        assert np.array_equal(imread_bytes(open(one + ".tif", "rb").read()), k)
        with np.load(one + "_weights.npz") as z:
            assert np.array_equal(z["weights"], w32)

"""The 2D-LBT codec on the GPU against the reference's fixtures (tests/golden/lbt_*.npz) and the
row-wise float64 restatement (tests/lbt_restated.py): encode and decode with given weights, the
training from the moments, batch independence, determinism and the files end to end.

Measured on an MI355X (printed by the tests before they assert): 20 epochs end within 0.83-1.46 x
d_ref of the restatement (bound 4 x); after 1000 epochs the float64 loss is 1.1e-8 (relative) below the
reference's (allowed: its spread, 1.8e-7, above); no index or pixel differs, on the boundary sets or
off them.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

import lbt_restated as R
from test_lbt import CASES, FULL, IDS, SHORT, flags_of, load, restated

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    import vcf_amd.lbt as G
    return G


def _check_indices(k, e, D, ref=None):
    """Equal to the restatement's off the boundary set, one step on it; the set holds <= 1 %."""
    ref = e["k"] if ref is None else ref
    ib = R.index_boundary(e["pre"], e["mag"], D)
    diff = np.abs(k.astype(int) - ref.astype(int))
    print(f"index boundary {ib.mean():.5f}, differing {np.count_nonzero(diff)} (on the set {np.count_nonzero(diff[ib])})")
    assert ib.mean() <= 0.01
    assert not np.any(diff[~ib]) and diff.max(initial=0) <= 1


def _check_pixels(rgb, d, D, ref):
    pb = R.pixel_boundary(d["pre"], d["mag"], D)
    diff = np.abs(rgb.astype(int) - ref.astype(int))
    print(f"pixel boundary {pb.mean():.5f}, differing {np.count_nonzero(diff)} (on the set {np.count_nonzero(diff[pb])})")
    assert pb.mean() <= 0.01
    assert not np.any(diff[~pb]) and diff.max(initial=0) <= 1


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_decode_of_the_reference_indices(G, case):
    """The reference's decoder matrix, mean and indices -> the reference's pixels off the boundary set."""
    z = load(case)
    B, Q, fl = case["B"], case["Q"], flags_of(case)
    H, W = z["rgb"].shape[:2]
    got = G.decode(z["k"], H, W, Q, fl, B, z["wd_ref"], float(z["mean_ref"]))
    d = R.decode(z["k"], H, W, z["wd_ref"], float(z["mean_ref"]), B, Q, fl)
    assert got.shape == (H, W, 3) and got.dtype == np.uint8
    _check_pixels(got, d, B * B, z["decoded"])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_encode_with_given_weights(G, case):
    """The restatement's trained encoder (float32) and the fixture's mean -> the restatement's indices;
    with the reference's encoder -> the reference's indices."""
    z = load(case)
    B, Q, fl = case["B"], case["Q"], flags_of(case)
    for we, ref in ((restated(case)[0].astype(np.float32), None), (z["we_ref"], z["k"])):
        k, w_back, m_back = G.encode(z["rgb"], Q, fl, B, weights=we, mean=float(z["mean_ref"]))
        assert k.shape == tuple(case["k_shape"]) and k.dtype == np.uint8
        assert np.array_equal(w_back, we) and m_back == np.float32(z["mean_ref"])
        _check_indices(k, R.encode(z["rgb"], we, float(z["mean_ref"]), B, Q, fl), B * B, ref)


def test_batched_launches_equal_single_ones(G):
    """Three frames of one shape, each with its own matrices and mean, in one launch."""
    for name in ("rand_40x48_x", "rand_40x48_p"):
        case = [c for c in CASES if c["name"] == name][0]
        z = load(case)
        B, Q, fl = case["B"], case["Q"], flags_of(case)
        H, W = z["rgb"].shape[:2]
        rng = np.random.Generator(np.random.PCG64(11))
        frames = np.stack([z["rgb"], R.synth_frame(H, W, 5), R.synth_frame(H, W, 6)])
        wes = np.stack([z["we_ref"], z["we_ref"][::-1].copy(), rng.normal(0, 0.05, (64, 64)).astype(np.float32)])
        wds = np.stack([z["wd_ref"], z["wd_ref"][:, ::-1].copy(), rng.normal(0, 0.05, (64, 64)).astype(np.float32)])
        means = np.array([float(z["mean_ref"]), 3.5, -20.25], np.float32)
        ks = G.encode(frames, Q, fl, B, weights=wes, mean=means)[0]
        for i in range(3):
            assert np.array_equal(ks[i], G.encode(frames[i], Q, fl, B, weights=wes[i], mean=means[i])[0])
        out = G.decode(ks, H, W, Q, fl, B, wds, means)
        for i in range(3):
            assert np.array_equal(out[i], G.decode(ks[i], H, W, Q, fl, B, wds[i], means[i]))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_moments_are_exact(G, case):
    z = load(case)
    X = R.blocks(z["rgb"], case["B"]).astype(np.float64)
    S1, S2 = G.moments(z["rgb"], case["B"])
    assert np.array_equal(S1, X.sum(0)) and np.array_equal(S2, X.T @ X)


@pytest.mark.parametrize("case", SHORT, ids=[c["name"] for c in SHORT])
def test_short_training_follows_the_restatement(G, case):
    """20 epochs from the fixture's initial weights: both matrices within 4 x d_ref of the float64
    row-wise restatement's (d_ref: what torch's float32 run differs from it by)."""
    z = load(case)
    B = case["B"]
    we, wd = restated(case)
    t = G.train(z["rgb"], B, case["epochs"], init=(z["we0"], z["wd0"]))
    X = R.centred(z["rgb"], B, float(t["mean"])).astype(np.float64)
    dE, dD = float(np.max(np.abs(t["we"] - we))), float(np.max(np.abs(t["wd"] - wd)))
    print(f"{case['name']}: |We - restated| {dE:.3e}, |Wd - restated| {dD:.3e}, d_ref {case['d_ref']:.3e}, "
          f"ratio {max(dE, dD) / case['d_ref']:.2f}")
    assert abs(float(t["mean"]) - float(z["mean_ref"])) <= 2.0 ** -17
    loss = R.loss_terms(X, t["we"].astype(np.float64), t["wd"].astype(np.float64))
    assert np.allclose(t["loss"], loss, rtol=1e-3, atol=1e-6)      # the kernel's own float32 report
    assert max(dE, dD) <= 4 * case["d_ref"]


@pytest.mark.parametrize("case", FULL, ids=[c["name"] for c in FULL])
def test_full_training_reaches_the_reference_loss(G, case):
    """1000 epochs: the float64 loss at the GPU's final weights is no greater than at the reference's,
    plus the relative spread between torch's float32 run and the float64 restatement."""
    z = load(case)
    B = case["B"]
    t = G.train(z["rgb"], B, case["epochs"], init=(z["we0"], z["wd0"]))
    X = R.centred(z["rgb"], B, float(z["mean_ref"])).astype(np.float64)
    got = R.loss_terms(X, t["we"].astype(np.float64), t["wd"].astype(np.float64))[0]
    ref = R.loss_terms(X, z["we_ref"].astype(np.float64), z["wd_ref"].astype(np.float64))[0]
    print(f"{case['name']}: loss GPU {got:.9g}, reference {ref:.9g}, relative {(got - ref) / ref:.3e}, "
          f"spread {case['spread']:.3e}")
    assert got <= ref * (1 + case["spread"])


def test_frames_of_a_batch_train_independently(G):
    a, b = load(SHORT[0])["rgb"], R.synth_frame(37, 45, 9)
    both = G.train(np.stack([a, b]), 8, 20)
    for i, f in enumerate((a, b)):
        one = G.train(f, 8, 20)
        for key in ("we", "wd", "mean", "loss"):
            assert np.array_equal(both[key][i], one[key], equal_nan=True), key
    assert not np.array_equal(both["wd"][0], both["wd"][1])


def _png(path, rgb):
    from PIL import Image
    Image.fromarray(rgb).save(path)


def _cli(name, *argv):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "vcf_amd", "cli", name), *argv], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr


def test_equal_runs_write_equal_files(tmp_path):
    from vcf_amd.codec import parser as P
    from vcf_amd.codec.lbt2d import CoDec
    src = str(tmp_path / "in.png")
    _png(src, R.synth_frame(37, 45, 2))
    c = CoDec(P.parse(P.lbt_parser(), ["encode", "--epochs", "20"]))
    for o in ("a", "b"):
        c.encode_fn(src, str(tmp_path / o))
    for ext in (".weights.pth", ".tif", "_shape.bin"):
        assert open(str(tmp_path / "a") + ext, "rb").read() == open(str(tmp_path / "b") + ext, "rb").read()


def test_cli_round_trip_through_the_three_files(tmp_path):
    """The program's encode and decode of a 37 x 45 PNG, with --side_info and without, on the
    reference's fixed files (its encode() and decode() ignore -o, -e and -d, 2D-LBT.py:465, 566); the
    decoded frame is what the restatement decodes from the files."""
    from PIL import Image
    from vcf_amd import pth
    from vcf_amd.codec.tiff import TIFFCodec
    rgb = R.synth_frame(37, 45, 2)
    enc, dec = "/tmp/encoded", "/tmp/decoded.png"
    for side in (None, str(tmp_path / "side.pth")):
        for fn in (dec, enc + ".tif", enc + "_shape.bin", enc + ".weights.pth"):
            if os.path.exists(fn):
                os.remove(fn)
        _png("/tmp/original.png", rgb)
        extra = ["--side_info", side] if side else []
        _cli("2D-LBT.py", "encode", "--epochs", "20", *extra)
        wfile = side or enc + ".weights.pth"
        assert os.path.getsize(enc + "_shape.bin") == 12 and os.path.exists(wfile) and os.path.exists(enc + ".tif")
        assert side is None or not os.path.exists(enc + ".weights.pth")
        _cli("2D-LBT.py", "decode", *extra)
        got = np.array(Image.open(dec))
        wd, mean = pth.load(wfile, 64)
        k = TIFFCodec().decompress(open(enc + ".tif", "rb").read())
        assert k.shape == (40, 48, 3) and k.dtype == np.uint8
        d = R.decode(k, 37, 45, wd, mean)
        _check_pixels(got, d, 64, d["rgb"])
        assert np.mean(np.abs(got.astype(float) - rgb)) < 64     # 20 epochs: far from converged, but an image


def test_iii_equals_frame_by_frame(tmp_path):
    """III -T 2D-LBT over 3 frames of two shapes equals encode_fn frame by frame."""
    from vcf_amd.codec import parser as P
    from vcf_amd.codec.iii import CoDec as III
    from vcf_amd.codec.lbt2d import CoDec
    shapes = [(37, 45), (24, 32), (37, 45)]
    for i, (H, W) in enumerate(shapes):
        _png(str(tmp_path / f"original_{i:04d}.png"), R.synth_frame(H, W, 20 + i))
    flags = ["-T", "2D-LBT", "-N", "3", "--epochs", "10", "-B", "4"]
    e = P.parse(P.iii_parser(transform="2D-LBT"), ["encode", "-o", str(tmp_path / "original_%04d.png")] + flags)
    III(e, encode_prefix=str(tmp_path / "enc"), decode_prefix=str(tmp_path / "dec")).encode()
    one = CoDec(P.parse(P.lbt_parser(), ["encode", "--epochs", "10", "-B", "4"]))
    for i in range(3):
        one.encode_fn(str(tmp_path / f"original_{i:04d}.png"), str(tmp_path / f"one_{i:04d}"))
        for ext in (".tif", "_shape.bin", ".weights.pth"):
            assert open(str(tmp_path / f"enc_{i:04d}") + ext, "rb").read() == \
                open(str(tmp_path / f"one_{i:04d}") + ext, "rb").read(), (i, ext)
    d = P.parse(P.iii_parser(transform="2D-LBT"), ["decode", "-T", "2D-LBT", "-N", "3", "-B", "4"])
    III(d, encode_prefix=str(tmp_path / "enc"), decode_prefix=str(tmp_path / "dec")).decode()
    dec1 = CoDec(P.parse(P.lbt_parser(), ["decode", "-B", "4"]))
    from PIL import Image
    for i in range(3):
        dec1.decode_fn(str(tmp_path / f"one_{i:04d}"), str(tmp_path / f"one_{i:04d}.png"))
        assert np.array_equal(np.array(Image.open(str(tmp_path / f"dec_{i:04d}.png"))),
                              np.array(Image.open(str(tmp_path / f"one_{i:04d}.png"))))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_decoder_reads_the_reference_files(tmp_path, case):
    """The fixture's three files as the reference wrote them (-c z_lib) -> the reference's pixels."""
    from PIL import Image
    from vcf_amd.codec import parser as P
    from vcf_amd.codec.lbt2d import CoDec
    z = load(case)
    enc = str(tmp_path / "encoded")
    for ext, key in ((".npz", "npz"), ("_shape.bin", "shape_bin"), (".weights.pth", "pth")):
        with open(enc + ext, "wb") as f:
            f.write(bytes(z[key]))
    c = CoDec(P.parse(P.lbt_parser(entropy="z_lib"), ["decode", "-c", "z_lib"] + case["flags"]))
    c.decode_fn(enc, str(tmp_path / "dec.png"))
    got = np.array(Image.open(str(tmp_path / "dec.png")))
    H, W = z["rgb"].shape[:2]
    d = R.decode(z["k"], H, W, z["wd_ref"], float(z["mean_ref"]), case["B"], case["Q"], flags_of(case))
    _check_pixels(got, d, case["B"] ** 2, z["decoded"])

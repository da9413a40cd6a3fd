"""The vector quantizer on the GPU (vcf_vq.hip through vcf_amd.vq, the codecs and
the two CLIs) against the restatement (tests/vq_restated.py) and what sklearn
and the reference recorded (tests/golden/vq_*.npz)."""
import functools
import os
import subprocess
import sys
from argparse import Namespace

import numpy as np
import pytest
from PIL import Image

import vq_restated as R
from test_vq import GOLDEN, cases, load, restated_fit

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [c["name"] for c in cases()]


def _rand(shape, seed):
    return np.random.Generator(np.random.PCG64(seed)).integers(0, 256, shape, dtype=np.uint8)


def _checkerboard():
    y, x = np.mgrid[0:32, 0:48]
    return np.repeat((((y + x) & 1) * 255).astype(np.uint8)[:, :, None], 3, 2)


# further shapes, with a seeded codebook each: a constant image, N < K reduced to K = N, a checkerboard, one
# channel, four channels with the largest vector (D = 1024: the 64 KiB tile), more vectors than one block of the
# assign and accumulate kernels, and the accumulate kernel's global-atomic path (K * (D + 1) * 4 > 48 KiB)
@functools.lru_cache(maxsize=None)
def extra(name):
    if name == "constant":
        img, BS, K = np.full((32, 32, 3), 77, np.uint8), 4, 8
    elif name == "n_lt_k":
        img, BS, K = _rand((16, 16, 3), 11), 4, 16
    elif name == "checkerboard":
        img, BS, K = _checkerboard(), 2, 4
    elif name == "gray":
        img, BS, K = _rand((20, 28, 1), 12), 4, 5
    elif name == "rgba_b16":
        img, BS, K = _rand((32, 48, 4), 13), 16, 6
    elif name == "many":
        img, BS, K = _rand((96, 132, 3), 14), 1, 33        # N = 12672: 25 assign blocks, 7 accumulate blocks
    else:
        raise KeyError(name)
    X = R.blocks(img, BS)
    rng = np.random.Generator(np.random.PCG64(99))
    cent = rng.uniform(0, 255, (K, X.shape[1]))
    return img, BS, K, X, cent


EXTRA = ["constant", "n_lt_k", "checkerboard", "gray", "rgba_b16", "many"]


def shape(name):
    """(img, BS, K, X, a codebook) of a fixture or an extra shape."""
    if name in EXTRA:
        return extra(name)
    z = load(name)
    BS, K = int(z["BS"]), int(z["K"])
    return z["img"], BS, K, R.blocks(z["img"], BS), restated_fit(name, False)[0]


@pytest.mark.parametrize("name", NAMES + EXTRA)
def test_accumulate_is_exact(name):
    from vcf_amd import vq
    img, BS, K, X, _ = shape(name)
    labels = np.random.Generator(np.random.PCG64(3)).integers(0, K, X.shape[0]).astype(np.uint16)
    labels[: min(K, 3)] = K - 1                      # the last cluster is never empty
    sums, counts = vq.accumulate(img, BS, labels, K)
    rs, rc = R.accumulate(X, labels, K)
    assert np.array_equal(sums, rs) and np.array_equal(counts, rc)
    assert counts.sum() == X.shape[0]


@pytest.mark.parametrize("name", NAMES + EXTRA)
def test_assign(name):
    from vcf_amd import vq
    img, BS, K, X, cent = shape(name)
    labels, dist = vq.assign(img, BS, cent, want_dist=True)
    ref = R.distances(X, cent)
    n = np.arange(X.shape[0])
    g = R.gamma(X.shape[1])
    print(f"{name}: gamma {g:.3g}, worst excess over the minimum {np.max(ref[n, labels] - ref.min(axis=1)):.3g}")
    assert labels.max() < K
    assert np.all(ref[n, labels] - ref.min(axis=1) <= g)
    assert np.all(np.abs(dist - ref[n, labels]) <= g)
    # the arithmetic is restated bit for bit: labels (ties included) and distances are equal
    rl, rb, _ = R.assign(X, cent)
    assert np.array_equal(labels, rl)
    assert np.array_equal(dist, rb)


def test_assign_ties_take_the_lowest_index():
    from vcf_amd import vq
    img = _checkerboard()
    X = R.blocks(img, 2)
    cent = np.stack([X[0], X[0], X[1], X[1], X[0] + 0.5]).astype(np.float64)   # duplicated centroids
    labels = vq.assign(img, 2, cent)
    assert set(labels.tolist()) <= {0, 2}
    assert np.array_equal(labels, R.assign(X, cent)[0])


@pytest.mark.parametrize("name", NAMES + ["constant", "n_lt_k", "many"])
@pytest.mark.parametrize("seed", [0, 1])
def test_init_pp_is_the_integer_restatement(name, seed):
    from vcf_amd import vq
    img, BS, K, X, _ = shape(name)
    cent, ids = vq.init_pp(img, BS, K, seed)
    rcent, rids = R.init_pp(X, K, seed)
    assert np.array_equal(ids, rids)
    assert np.array_equal(cent, rcent)
    cent2, ids2 = vq.init_pp(img, BS, K, seed)
    assert np.array_equal(ids2, ids) and np.array_equal(cent2, cent)


@pytest.mark.parametrize("name", NAMES)
def test_fit_from_the_fixture_codebook(name):
    from vcf_amd import vq
    z = load(name)
    BS, K = int(z["BS"]), int(z["K"])
    X = R.blocks(z["img"], BS)
    cent, labels, rep = vq.fit(z["img"], BS, K, init=z["init"].astype(np.float64))
    assert np.array_equal(labels, z["sk_labels"])
    assert rep.n_iter == int(z["sk_n_iter"])
    assert rep.stop_reason == "strict"
    sums, counts = R.accumulate(X, labels, K)
    assert counts.min() > 0
    assert np.array_equal(cent, sums.astype(np.float64) / counts.astype(np.float64)[:, None])
    rcent, rlabels, rrep, _ = restated_fit(name, False)
    assert np.array_equal(cent, rcent)
    assert rep.inertia == rrep["inertia"] and rep.tol_abs == rrep["tol_abs"]
    assert abs(rep.inertia - float(z["sk_inertia"])) <= 1e-9 * float(z["sk_inertia"])


@pytest.mark.parametrize("name", NAMES)
def test_fit_from_its_own_init(name):
    from vcf_amd import vq
    z = load(name)
    BS, K = int(z["BS"]), int(z["K"])
    X = R.blocks(z["img"], BS)
    cent, labels, rep = vq.fit(z["img"], BS, K, seed=0)
    rcent, rlabels, rrep, _ = restated_fit(name, True)
    assert np.array_equal(labels, rlabels) and np.array_equal(cent, rcent)
    assert (rep.n_iter, rep.stop_reason, rep.relocations) == (rrep["n_iter"], rrep["stop_reason"], rrep["relocations"])
    assert rep.inertia == rrep["inertia"]
    print(f"{name}: inertia {rep.inertia:.6g}, sklearn k-means++ worst {z['sk_pp_inertias'].max():.6g}, "
          f"median {np.median(z['sk_pp_inertias']):.6g}")
    assert rep.inertia <= z["sk_pp_inertias"].max()
    if rep.stop_reason == "strict":
        sums, counts = R.accumulate(X, labels, K)
        assert counts.min() > 0 or len(np.unique(X, axis=0)) < K
        live = counts > 0
        assert np.array_equal(cent[live], sums[live].astype(np.float64) / counts[live].astype(np.float64)[:, None])


def test_fit_relocates_empty_clusters():
    """A codebook with far-away entries leaves clusters empty: they take the farthest vectors, as restated."""
    from vcf_amd import vq
    img, BS, _, X, _ = shape("rand_24x40_b2_k32")
    K = 6
    init = np.concatenate([X[:3].astype(np.float64), np.full((3, X.shape[1]), 1e4) + np.arange(3)[:, None]])
    cent, labels, rep = vq.fit(img, BS, K, init=init)
    rcent, rlabels, rrep = R.fit(X, K, init=init)
    assert rrep["relocations"] >= 3
    assert rep.relocations == rrep["relocations"]
    assert np.array_equal(labels, rlabels) and np.array_equal(cent, rcent)
    assert (rep.n_iter, rep.stop_reason, rep.inertia) == (rrep["n_iter"], rrep["stop_reason"], rrep["inertia"])


def test_fit_stops_by_tol_and_by_max_iter():
    from vcf_amd import vq
    img, BS, K, X, _ = shape("rand_16x16_b1_k8")
    for kw in (dict(max_iter=2), dict(tol=0.05)):
        cent, labels, rep = vq.fit(img, BS, K, seed=0, **kw)
        rcent, rlabels, rrep = R.fit(X, K, seed=0, **kw)
        assert rep.stop_reason == rrep["stop_reason"] == ("max_iter" if "max_iter" in kw else "tol")
        assert rep.n_iter == rrep["n_iter"]
        assert np.array_equal(labels, rlabels) and np.array_equal(cent, rcent)
        assert np.array_equal(labels, R.assign(X, cent)[0])      # the labels match the returned centroids


@pytest.mark.parametrize("name", ["constant", "n_lt_k"])
def test_degenerate_images(name):
    from vcf_amd import vq
    img, BS, K, X, _ = shape(name)
    cent, labels, rep = vq.fit(img, BS, K, seed=0)
    assert rep.inertia == 0.0 and rep.n_iter >= 1
    H, W, C = img.shape
    out = vq.decode(labels.reshape(H // BS, W // BS), cent, BS, C)
    assert np.array_equal(out, img)
    rcent, rlabels, rrep = R.fit(X, K, seed=0)
    assert np.array_equal(labels, rlabels) and np.array_equal(cent, rcent)
    assert (rep.n_iter, rep.stop_reason) == (rrep["n_iter"], rrep["stop_reason"])


def test_decode_truncates_and_checks_labels():
    from vcf_amd import vq
    rng = np.random.Generator(np.random.PCG64(21))
    for BS, C, shp in ((4, 3, (5, 7)), (1, 3, (9, 11)), (16, 4, (2, 3)), (3, 1, (70, 90))):
        K = 9
        cent = rng.uniform(0, 255.99, (K, BS * BS * C))
        cent[0, 0], cent[1, 0] = 255.999, 0.999
        labels = rng.integers(0, K, shp).astype(np.uint16)
        assert np.array_equal(vq.decode(labels, cent, BS, C), R.decode(labels, cent, BS, C))
        bad = labels.copy()
        bad[-1, -1] = K
        with pytest.raises(IndexError):
            vq.decode(bad, cent, BS, C)


def _args(sub, **kw):
    base = dict(subparser_name=sub, entropy_image_codec="TIFF", filter="no_filter", original="/tmp/original.png",
                encoded="/tmp/encoded", decoded="/tmp/decoded.png", debug=False)
    return Namespace(**{**base, **kw})


@pytest.mark.parametrize("module", ["VQ", "color-VQ"])
def test_decode_fn_reproduces_the_reference(module, tmp_path):
    """The reference's own label file and codebook file give its decoded PNG pixel for pixel."""
    from vcf_amd.codec.vq import ColorVQCoDec, VQCoDec
    z = np.load(os.path.join(GOLDEN, f"vq_ref_{module}.npz"))
    enc = str(tmp_path / "enc")
    with open(enc + ".tif", "wb") as f:
        f.write(z["enc"].tobytes())
    with open(enc + "_centroids.npz", "wb") as f:
        f.write(z["codebook_file"].tobytes())
    if module == "VQ":
        codec = VQCoDec(_args("decode", block_size_VQ=4, N_clusters=16))
    else:
        codec = ColorVQCoDec(_args("decode", N_color_clusters=8))
    codec.decode_fn(enc, str(tmp_path / "dec.png"))
    assert np.array_equal(np.array(Image.open(tmp_path / "dec.png")), z["decoded"])
    assert codec.total_input_size == z["enc"].size + z["codebook_file"].size
    with pytest.raises(NotImplementedError):
        VQCoDec(_args("decode", filter="gaussian_blur", block_size_VQ=4, N_clusters=16))


def _rmse(a, b):
    return float(np.sqrt(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))


def test_encode_fn_then_decode_fn_vq(tmp_path):
    from vcf_amd.codec.tiff import imread_bytes
    from vcf_amd.codec.vq import VQCoDec
    z = load("smooth_32x48_b4_k16")
    img = z["img"]
    Image.fromarray(img).save(tmp_path / "in.png")
    enc = str(tmp_path / "enc")
    codec = VQCoDec(_args("encode", block_size_VQ=4, N_clusters=16))
    codec.encode_fn(str(tmp_path / "in.png"), enc)
    labels = imread_bytes(open(enc + ".tif", "rb").read())
    book = np.load(enc + "_centroids.npz")
    assert book.files == ["a"]
    a = book["a"]
    assert labels.dtype == np.uint16 and labels.shape == (8, 12)
    assert a.dtype == np.float64 and a.shape == (16, 16, 3)
    assert np.all(np.diff(np.sum(a.reshape(16, -1) ** 2, axis=1)) >= 0)
    assert codec.total_output_size == os.path.getsize(enc + ".tif") + os.path.getsize(enc + "_centroids.npz")
    rl, rbook, _ = R.vq_encode(img, 4, 16)
    assert np.array_equal(labels, rl) and np.array_equal(a, rbook)
    VQCoDec(_args("decode", block_size_VQ=4, N_clusters=16)).decode_fn(enc, str(tmp_path / "dec.png"))
    out = np.array(Image.open(tmp_path / "dec.png"))
    restated = R.decode(rl, rbook.reshape(16, -1), 4, 3)
    assert np.array_equal(out, restated)
    assert _rmse(out, img) == _rmse(restated, img)


def test_encode_fn_reduces_k(tmp_path):
    from vcf_amd.codec.vq import VQCoDec
    img = _rand((16, 16, 3), 11)
    Image.fromarray(img).save(tmp_path / "in.png")
    enc = str(tmp_path / "enc")
    codec = VQCoDec(_args("encode", block_size_VQ=4, N_clusters=256))
    codec.encode_fn(str(tmp_path / "in.png"), enc)
    assert codec.N_clusters == 16 and codec.report.inertia == 0.0
    assert np.load(enc + "_centroids.npz")["a"].shape == (16, 16, 3)
    VQCoDec(_args("decode", block_size_VQ=4, N_clusters=256)).decode_fn(enc, str(tmp_path / "dec.png"))
    assert np.array_equal(np.array(Image.open(tmp_path / "dec.png")), img)
    Image.fromarray(img[:15]).save(tmp_path / "odd.png")
    with pytest.raises(ValueError):
        VQCoDec(_args("encode", block_size_VQ=4, N_clusters=4)).encode_fn(str(tmp_path / "odd.png"), enc)


def test_encode_fn_then_decode_fn_color_vq(tmp_path):
    from vcf_amd.codec.tiff import imread_bytes
    from vcf_amd.codec.vq import ColorVQCoDec
    img = load("rand_16x16_b1_k8")["img"]
    Image.fromarray(img).save(tmp_path / "in.png")
    enc = str(tmp_path / "enc")
    codec = ColorVQCoDec(_args("encode", N_color_clusters=8))
    codec.encode_fn(str(tmp_path / "in.png"), enc)
    labels = imread_bytes(open(enc + ".tif", "rb").read())
    a = np.load(enc + "_centroids.npz")["a"]
    assert labels.dtype == np.uint16 and labels.shape == (16, 16)
    assert a.dtype == np.uint8 and a.shape == (8, 3)
    rl, rbook, _ = R.color_vq_encode(img, 8)
    assert np.array_equal(labels, rl) and np.array_equal(a, rbook)
    ColorVQCoDec(_args("decode", N_color_clusters=8)).decode_fn(enc, str(tmp_path / "dec.png"))
    out = np.array(Image.open(tmp_path / "dec.png"))
    restated = R.decode(rl, rbook, 1, 3)
    assert np.array_equal(out, restated)
    assert _rmse(out, img) == _rmse(restated, img)


@pytest.mark.parametrize("module,flags", [("VQ", ["-b", "4", "-q", "16"]), ("color-VQ", ["-q", "8"])])
def test_cli_end_to_end(module, flags):
    """`python <module>.py encode|decode [flags]` over the reference's hard-wired /tmp files."""
    img = load("smooth_32x48_b4_k16")["img"]
    for fn in ("/tmp/decoded.png", "/tmp/encoded.tif", "/tmp/encoded_centroids.npz"):
        if os.path.exists(fn):
            os.remove(fn)
    Image.fromarray(img).save("/tmp/original.png")
    for sub in ("encode", "decode"):
        r = subprocess.run([sys.executable, f"vcf_amd/cli/{module}.py", sub] + flags, cwd=ROOT, capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
    if module == "VQ":
        rl, rbook, _ = R.vq_encode(img, 4, 16)
        want = R.decode(rl, rbook.reshape(16, -1), 4, 3)
    else:
        rl, rbook, _ = R.color_vq_encode(img, 8)
        want = R.decode(rl, rbook, 1, 3)
    assert np.array_equal(np.load("/tmp/encoded_centroids.npz")["a"], rbook)
    assert np.array_equal(np.array(Image.open("/tmp/decoded.png")), want)

"""The vector quantizer without a GPU: the restatement (tests/vq_restated.py)
against what sklearn recorded (tests/golden/vq_*.npz), the parsers, the
reference's side-file layout, the K reduction, and the argument checks of the
C ABI, which answer before any device work."""
import ctypes
import functools
import io
import json
import os

import numpy as np
import pytest

import vq_restated as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def cases():
    with open(os.path.join(GOLDEN, "manifest_vq.json")) as f:
        return json.load(f)["cases"]


@functools.lru_cache(maxsize=None)
def load(name):
    z = np.load(os.path.join(GOLDEN, f"vq_{name}.npz"))
    return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def restated_fit(name, own_init):
    """The restated fit of a fixture, from its codebook or from the restated k-means++ (seed 0); computed once."""
    z = load(name)
    X = R.blocks(z["img"], int(z["BS"]))
    gaps = []
    if own_init:
        out = R.fit(X, int(z["K"]), seed=0, gaps=gaps)
    else:
        out = R.fit(X, int(z["K"]), init=z["init"], gaps=gaps)
    return out + (min(gaps),)


@pytest.mark.parametrize("c", cases(), ids=lambda c: c["name"])
def test_restatement_reproduces_sklearn(c):
    z = load(c["name"])
    cent, labels, rep, gap = restated_fit(c["name"], False)
    assert np.array_equal(labels, z["sk_labels"])
    assert rep["n_iter"] == int(z["sk_n_iter"])
    # sklearn works on centred data: a few ulp of 256 apart
    assert np.abs(cent - z["sk_centers"]).max() <= 1e-10
    assert abs(rep["inertia"] - float(z["sk_inertia"])) <= 1e-9 * float(z["sk_inertia"])
    assert gap > R.gamma(cent.shape[1])          # the fixture is robust to the rounding of a distance


@pytest.mark.parametrize("c", cases(), ids=lambda c: c["name"])
def test_restated_own_init_is_no_worse_than_sklearn(c):
    z = load(c["name"])
    _, _, rep, gap = restated_fit(c["name"], True)
    assert rep["inertia"] <= z["sk_pp_inertias"].max()
    assert gap > R.gamma(int(z["BS"]) ** 2 * 3)


def test_draw_is_splitmix64():
    # splitmix64 from state 0: the published first outputs
    assert R.draw(0, 0, 0) == 0xE220A8397B1DCDAF
    assert R.draw(0, 0, 1) == 0x6E789E6AA1B965F4
    assert R.mulhi64(1 << 63, 10) == 5


def test_parser_defaults():
    from vcf_amd.codec import parser as P
    e = P.parse(P.build_vq_parser(), ["encode"])
    assert (e.block_size_VQ, e.N_clusters, e.entropy_image_codec) == (4, 256, "TIFF")
    assert (e.original, e.encoded) == ("/tmp/original.png", "/tmp/encoded")
    assert not hasattr(e, "filter") and not hasattr(e, "seed")
    d = P.parse(P.build_vq_parser(), ["decode", "-b", "8", "-q", "64"])
    assert (d.block_size_VQ, d.N_clusters, d.filter, d.decoded) == (8, 64, "no_filter", "/tmp/decoded.png")
    e = P.parse(P.build_color_vq_parser(), ["encode"])
    assert e.N_color_clusters == 32 and not hasattr(e, "block_size_VQ")
    d = P.parse(P.build_color_vq_parser(entropy="CBAHC"), ["decode", "-c", "CBAHC"])
    assert (d.N_color_clusters, d.filter, d.order) == (32, "no_filter", 0)


def test_make_quantizer_still_refuses_vq():
    from argparse import Namespace
    from vcf_amd.codec.quantizers import make_quantizer
    with pytest.raises(NotImplementedError):
        make_quantizer(Namespace(quantizer="VQ"))


@pytest.mark.parametrize("module", ["VQ", "color-VQ"])
def test_side_file_layout_of_the_reference(module):
    """What src/VQ.py and src/color-VQ.py wrote: the layout the codecs keep, and the restated decode."""
    z = np.load(os.path.join(GOLDEN, f"vq_ref_{module}.npz"))
    book = np.load(io.BytesIO(z["codebook_file"].tobytes()))
    assert book.files == ["a"]
    a = book["a"]
    assert z["labels"].dtype == np.uint16
    if module == "VQ":
        assert a.dtype == np.float64 and a.shape == (16, 16, 3)
        assert z["labels"].shape == (8, 12)
        e = np.array([np.sum(c * c) for c in a])
        assert np.all(np.diff(e) >= 0)             # ascending energy (A14)
        out = R.decode(z["labels"], a.reshape(16, -1), 4, 3)
    else:
        assert a.dtype == np.uint8 and a.shape == (8, 3)
        assert z["labels"].shape == (32, 48)
        out = R.decode(z["labels"], a, 1, 3)
    assert np.array_equal(out, z["decoded"])


def test_restated_energy_reorder():
    rng = np.random.Generator(np.random.PCG64(5))
    cent = rng.uniform(0, 255, (9, 12))
    labels = rng.integers(0, 9, 50)
    out, lab = R.sort_by_energy(cent, labels)
    assert np.all(np.diff(np.sum(out * out, axis=1)) > 0)
    assert np.array_equal(out[lab], cent[labels])
    from vcf_amd.codec.vq import sort_by_energy
    out2, lab2 = sort_by_energy(cent, labels)
    assert np.array_equal(out2, out) and np.array_equal(lab2, lab)


def test_k_reduction_restated():
    rng = np.random.Generator(np.random.PCG64(6))
    img = rng.integers(0, 256, (16, 16, 3), dtype=np.uint8)
    labels, book, rep = R.vq_encode(img, 4, 256)
    assert book.shape == (16, 16, 3) and labels.shape == (4, 4)
    assert rep["inertia"] == 0.0
    assert np.array_equal(R.decode(labels, book.reshape(16, -1), 4, 3), img)


# ---- the C ABI's argument checks -------------------------------------------------
_P = ctypes.c_void_p


def _status(name, *args):
    from vcf_amd import _lib
    return getattr(_lib.lib(), name)(*args)


def test_abi_argument_errors():
    """Each returns VCF_ERR_INVALID from host code: the pointers are never used."""
    from vcf_amd import _lib
    from vcf_amd.vq import _Report
    buf = np.zeros(1 << 16, np.uint8)
    p = buf.ctypes.data_as(_P)
    rep = _Report()
    INV = _lib.VCF_ERR_INVALID
    geo_bad = [(32, 48, 3, 0), (32, 48, 3, 17), (30, 48, 3, 4), (32, 46, 3, 4), (32, 48, 0, 4), (32, 48, 5, 4),
               (0, 48, 3, 4)]
    for H, W, C, BS in geo_bad:
        assert _status("vcf_vq_assign", p, H, W, C, BS, p, 4, p, None, None) == INV
        assert _status("vcf_vq_accumulate", p, H, W, C, BS, p, 4, p, p, None) == INV
        assert _status("vcf_vq_init_pp", p, H, W, C, BS, 4, 0, p, None, None) == INV
        assert _status("vcf_vq_fit", p, H, W, C, BS, 4, 0, 300, 1e-4, None, p, p, ctypes.byref(rep), None) == INV
    for K in (0, 97, 4097, -1):          # N = 96
        assert _status("vcf_vq_assign", p, 32, 48, 3, 4, p, K, p, None, None) == INV
        assert _status("vcf_vq_accumulate", p, 32, 48, 3, 4, p, K, p, p, None) == INV
        assert _status("vcf_vq_init_pp", p, 32, 48, 3, 4, K, 0, p, None, None) == INV
        assert _status("vcf_vq_fit", p, 32, 48, 3, 4, K, 0, 300, 1e-4, None, p, p, ctypes.byref(rep), None) == INV
    assert "K" in _lib.lib().vcf_last_error().decode()
    # NULL buffers
    assert _status("vcf_vq_assign", None, 32, 48, 3, 4, p, 4, p, None, None) == INV
    assert _status("vcf_vq_assign", p, 32, 48, 3, 4, None, 4, p, None, None) == INV
    assert _status("vcf_vq_assign", p, 32, 48, 3, 4, p, 4, None, None, None) == INV
    assert _status("vcf_vq_accumulate", p, 32, 48, 3, 4, p, 4, None, p, None) == INV
    assert _status("vcf_vq_accumulate", p, 32, 48, 3, 4, p, 4, p, None, None) == INV
    assert _status("vcf_vq_init_pp", p, 32, 48, 3, 4, 4, 0, None, None, None) == INV
    assert _status("vcf_vq_fit", p, 32, 48, 3, 4, 4, 0, 300, 1e-4, None, None, p, ctypes.byref(rep), None) == INV
    assert _status("vcf_vq_fit", p, 32, 48, 3, 4, 4, 0, 300, 1e-4, None, p, p, None, None) == INV
    assert _status("vcf_vq_fit", p, 32, 48, 3, 4, 4, 0, 0, 1e-4, None, p, p, ctypes.byref(rep), None) == INV
    assert _status("vcf_vq_fit", p, 32, 48, 3, 4, 4, 0, 300, -1.0, None, p, p, ctypes.byref(rep), None) == INV
    assert _status("vcf_vq_decode", p, 8, 12, 3, 4, p, 4, p, None, None) == INV
    assert _status("vcf_vq_decode", None, 8, 12, 3, 4, p, 4, p, p, None) == INV
    assert _status("vcf_vq_decode", p, 0, 12, 3, 4, p, 4, p, p, None) == INV
    assert _status("vcf_vq_decode", p, 8, 12, 3, 17, p, 4, p, p, None) == INV
    assert _status("vcf_vq_decode", p, 8, 12, 3, 4, p, 0, p, p, None) == INV


def test_signatures_cover_the_exports():
    from vcf_amd import _lib
    for name in ("vcf_vq_assign", "vcf_vq_accumulate", "vcf_vq_init_pp", "vcf_vq_fit", "vcf_vq_decode"):
        assert name in _lib.SIGNATURES
        assert getattr(_lib.lib(), name).argtypes == _lib.SIGNATURES[name]

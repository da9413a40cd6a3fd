"""The 2D-LBT codec without a GPU: the row-wise numpy restatement (tests/lbt_restated.py) against
the reference's own fixtures (tests/golden/lbt_*.npz, make_golden_lbt.py), the torch-free .pth
reader and writer, the command-line surface and the refusals."""
import io
import json
import os
import pickle
import zipfile

import numpy as np
import pytest

from conftest import GOLDEN

import lbt_restated as R


def lbt_manifest():
    with open(os.path.join(GOLDEN, "manifest_lbt.json")) as f:
        return json.load(f)


def load(case):
    return np.load(os.path.join(GOLDEN, f"lbt_{case['name']}.npz"))


CASES = lbt_manifest()["cases"]
IDS = [c["name"] for c in CASES]
SHORT = [c for c in CASES if c["epochs"] == 20]
FULL = [c for c in CASES if c["epochs"] == 1000]
_trained = {}


def flags_of(case):
    return (R.NO_SUBBANDS if "-x" in case["flags"] else 0) | (R.PERCEPTUAL if "-p" in case["flags"] else 0)


def restated(case):
    """The float64 restatement's (We, Wd) from the fixture's initial weights, computed once."""
    if case["name"] not in _trained:
        z = load(case)
        X = R.centred(z["rgb"], case["B"], float(z["mean_ref"])).astype(np.float64)
        _trained[case["name"]] = R.train(X, z["we0"], z["wd0"], case["epochs"])
    return _trained[case["name"]]


def test_fixture_set_is_the_one_the_issue_names():
    by = {c["name"]: c for c in CASES}
    assert set(by) == {"rand_37x45", "rand_16x24_b4_q8", "rand_9x9", "rand_15x21_b3", "rand_40x48_x", "rand_40x48_p",
                       "rand_32x32_b4_q1", "rand_24x32_b4_full"}
    assert by["rand_37x45"]["k_shape"] == [40, 48, 3] and by["rand_37x45"]["epochs"] == 20
    assert (by["rand_16x24_b4_q8"]["B"], by["rand_16x24_b4_q8"]["Q"]) == (4, 8)
    assert by["rand_9x9"]["k_shape"] == [16, 16, 3] and by["rand_9x9"]["rows"] == 12 < 64
    assert by["rand_15x21_b3"]["B"] == 3
    assert flags_of(by["rand_40x48_x"]) == R.NO_SUBBANDS and flags_of(by["rand_40x48_p"]) == R.PERCEPTUAL
    assert (by["rand_32x32_b4_q1"]["B"], by["rand_32x32_b4_q1"]["Q"]) == (4, 1)
    assert by["rand_24x32_b4_full"]["epochs"] == 1000 and by["rand_24x32_b4_full"]["encode_flags"] == []
    for c in CASES:
        assert os.path.getsize(os.path.join(GOLDEN, f"lbt_{c['name']}.npz")) < 1024 * 1024
        assert c["index_boundary"] <= 0.01 and c["pixel_boundary"] <= 0.01 and c["d_ref"] > 0


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_restatement_reproduces_the_fixture(case):
    """Trained weights within d_ref (by construction of d_ref: this pins the fixture to the
    restatement as it stands), indices and pixels equal off the boundary sets, one step on them."""
    z = load(case)
    B, Q, fl, D = case["B"], case["Q"], flags_of(case), case["B"] ** 2
    H, W = z["rgb"].shape[:2]
    we, wd = restated(case)
    assert np.max(np.abs(wd - z["wd_ref"])) <= case["d_ref"] and np.max(np.abs(we - z["we_ref"])) <= case["d_ref"]
    assert abs(float(R.mean_of(z["rgb"], B)) - float(z["mean_ref"])) <= 2.0 ** -17
    assert bytes(z["shape_bin"]) == R.shape_bin(H, W)
    e = R.encode(z["rgb"], z["we_ref"], float(z["mean_ref"]), B, Q, fl)
    ib = R.index_boundary(e["pre"], e["mag"], D)
    assert ib.mean() <= 0.01 and np.array_equal(e["k"][~ib], z["k"][~ib])
    assert np.max(np.abs(e["k"].astype(int) - z["k"])) <= 1
    d = R.decode(z["k"], H, W, z["wd_ref"], float(z["mean_ref"]), B, Q, fl)
    pb = R.pixel_boundary(d["pre"], d["mag"], D)
    assert pb.mean() <= 0.01 and np.array_equal(d["rgb"][~pb], z["decoded"][~pb])
    assert np.max(np.abs(d["rgb"].astype(int) - z["decoded"])) <= 1


def test_gradients_are_the_derivative_of_the_loss():
    """The restatement's chain rule against central differences of its own loss."""
    rng = np.random.Generator(np.random.PCG64(3))
    X = rng.normal(0, 30, (50, 9))
    X -= X.mean()
    We, Wd = rng.normal(0, 0.3, (9, 9)), rng.normal(0, 0.3, (9, 9))
    lam = 0.5
    gE, gD = R.gradients(X, We, Wd, lam)
    for g, which in ((gE, 0), (gD, 1)):
        for i, j in ((0, 0), (3, 7), (8, 2)):
            Ws = [We.copy(), Wd.copy()], [We.copy(), Wd.copy()]
            h = 1e-6
            Ws[0][which][i, j] += h
            Ws[1][which][i, j] -= h
            num = (R.loss_terms(X, *Ws[0], lam)[0] - R.loss_terms(X, *Ws[1], lam)[0]) / (2 * h)
            assert abs(num - g[i, j]) <= 1e-6 * max(1.0, abs(num))


# ---- the .pth payload ---------------------------------------------------------
def test_pth_writer_loads_in_torch():
    torch = pytest.importorskip("torch")
    from vcf_amd import pth
    rng = np.random.Generator(np.random.PCG64(5))
    for D in (4, 9, 64):
        w = rng.normal(0, 1, (D, D)).astype(np.float32)
        data = pth.dumps(w, -12.3456789)
        ck = torch.load(io.BytesIO(data), weights_only=True)
        assert set(ck) == {"decoder_state", "mean_val"} and list(ck["decoder_state"]) == ["weight"]
        t = ck["decoder_state"]["weight"]
        assert t.dtype == torch.float32 and np.array_equal(t.numpy(), w) and ck["mean_val"] == -12.3456789
        torch.nn.Linear(D, D, bias=False).load_state_dict(ck["decoder_state"])
        assert pth.dumps(w, -12.3456789) == data
        w2, m2 = pth.loads(data, D)
        assert np.array_equal(w2, w) and w2.dtype == np.float32 and m2 == -12.3456789


def test_pth_layout_is_torch_saves():
    from vcf_amd import pth
    data = pth.dumps(np.eye(8, dtype=np.float32), 1.5)
    with zipfile.ZipFile(io.BytesIO(data)) as z:
        names = [i.filename for i in z.infolist()]
        assert names == ["archive/data.pkl", "archive/.format_version", "archive/.storage_alignment", "archive/byteorder",
                         "archive/data/0", "archive/version"]
        assert all(i.compress_type == zipfile.ZIP_STORED for i in z.infolist())
        info = z.getinfo("archive/data/0")
        assert (info.header_offset + 30 + len(info.filename) + len(info.extra)) % 64 == 0
        assert z.read("archive/byteorder") == b"little" and z.read("archive/version") == b"3\n"


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_pth_reader_reads_the_reference_files(case):
    from vcf_amd import pth
    z = load(case)
    w, m = pth.loads(bytes(z["pth"]), case["B"] ** 2)
    assert w.dtype == np.float32 and np.array_equal(w, z["wd_ref"]) and m == float(z["mean_ref"])


def test_pth_reader_agrees_with_torch_on_the_reference_files():
    torch = pytest.importorskip("torch")
    from vcf_amd import pth
    z = load(CASES[0])
    ck = torch.load(io.BytesIO(bytes(z["pth"])), weights_only=True)
    w, m = pth.loads(bytes(z["pth"]))
    assert np.array_equal(ck["decoder_state"]["weight"].numpy(), w) and ck["mean_val"] == m


def _archive(pkl: bytes, storage: bytes = b"\0" * 64) -> bytes:
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w") as z:
        z.writestr("archive/data.pkl", pkl)
        z.writestr("archive/data/0", storage)
    return buf.getvalue()


def test_pth_reader_refuses_other_globals():
    from vcf_amd import pth
    for evil in (b"cos\nsystem\n(X\x04\x00\x00\x00truetR.", b"cbuiltins\neval\n(X\x01\x00\x00\x001tR.",
                 b"ctorch._utils\n_rebuild_tensor\n."):
        with pytest.raises(pickle.UnpicklingError):
            pth.loads(_archive(evil))
    good = pth.dumps(np.zeros((4, 4), np.float32), 0.0)
    with zipfile.ZipFile(io.BytesIO(good)) as z:
        pkl = z.read("archive/data.pkl")
    with pytest.raises(ValueError):
        pth.loads(_archive(pkl.replace(b"FloatStorage", b"DoubleStorage"), b"\0" * 128))
    with pytest.raises(pickle.UnpicklingError):
        pth.loads(_archive(pkl.replace(b"ccollections\nOrderedDict", b"ccollections\ndefaultdict")))


def test_pth_reader_rejects_the_wrong_matrix():
    from vcf_amd import pth
    good = pth.dumps(np.zeros((4, 4), np.float32), 0.0)
    with pytest.raises(ValueError):
        pth.loads(good, 16)
    with pytest.raises(ValueError):
        pth.dumps(np.zeros((4, 4), np.float64), 0.0)
    with pytest.raises(ValueError):
        pth.dumps(np.zeros((4, 5), np.float32), 0.0)
    with zipfile.ZipFile(io.BytesIO(good)) as z:
        pkl = z.read("archive/data.pkl")
    with pytest.raises(ValueError):
        pth.loads(_archive(pkl, b"\0" * 60))      # the storage is short


# ---- command line ------------------------------------------------------------
def test_parser_defaults_and_flag_names_are_the_references():
    from vcf_amd.codec import parser as P
    e = P.parse(P.lbt_parser(), ["encode"])
    assert (e.block_size_DCT, e.side_info, e.epochs, e.lr, e.color_transform, e.perceptual_quantization, e.Lambda,
            e.disable_subbands, e.QSS, e.quantizer, e.entropy_image_codec) == \
        (8, None, 1000, 1e-3, "YCoCg", False, None, False, 32, "deadzone", "TIFF")
    d = P.parse(P.lbt_parser(), ["decode"])
    assert (d.block_size_DCT, d.side_info, d.color_transform, d.perceptual_quantization, d.disable_subbands, d.QSS,
            d.filter) == (8, None, "YCoCg", False, False, 32, "no_filter")
    assert not hasattr(d, "epochs") and not hasattr(d, "lr") and not hasattr(d, "Lambda")
    e = P.parse(P.lbt_parser(), ["encode", "-B", "4", "--side_info", "/tmp/w.pth", "--epochs", "20", "--lr", "0.01",
                                 "-L", "0.5", "-t", "YCoCg", "-p", "-x", "-q", "7"])
    assert (e.block_size_DCT, e.side_info, e.epochs, e.lr, e.Lambda, e.perceptual_quantization, e.disable_subbands,
            e.QSS) == (4, "/tmp/w.pth", 20, 0.01, "0.5", True, True, 7)
    i = P.parse(P.iii_parser(transform="2D-LBT"), ["encode", "-T", "2D-LBT", "-B", "4", "--epochs", "5", "-N", "3"])
    assert (i.transform, i.block_size_DCT, i.epochs, i.number_of_frames) == ("2D-LBT", 4, 5, 3)


def test_codec_takes_the_training_options():
    from vcf_amd.codec import parser as P
    from vcf_amd.codec.iii import transform_codec
    from vcf_amd.codec.lbt2d import CoDec
    c = transform_codec(P.parse(P.iii_parser(transform="2D-LBT"), ["encode", "-T", "2D-LBT", "-B", "4", "-x", "-p"]))
    assert isinstance(c, CoDec) and (c.block_size, c.flags, c.epochs, c.lr, c.lambda_gain) == (4, 3, 1000, 1e-3, 1e-6)
    c = CoDec(P.parse(P.lbt_parser(), ["encode", "-L", "0.25", "--epochs", "7", "--lr", "0.5"]))
    assert (c.lambda_gain, c.epochs, c.lr, c.block_size) == (0.25, 7, 0.5, 8)   # -L starts no block-size search
    assert CoDec(P.parse(P.lbt_parser(entropy="z_lib"), ["decode", "-c", "z_lib"])).file_extension == ".npz"
    c = CoDec(P.parse(P.lbt_parser(), ["decode", "--side_info", "/tmp/x.pth"]))
    assert c._side_path("/tmp/enc") == "/tmp/x.pth"
    assert CoDec(P.parse(P.lbt_parser(), ["decode"]))._side_path("/tmp/enc") == "/tmp/enc.weights.pth"


def test_options_outside_the_hip_path_are_refused():
    from vcf_amd.codec import parser as P
    from vcf_amd.codec.ipp import codec_class
    from vcf_amd.codec.lbt2d import CoDec
    for argv in (["encode", "-B", "1"], ["encode", "-B", "9"], ["encode", "-a", "LloydMax"], ["decode", "-f", "NLM"],
                 ["encode", "-t", "YCrCb"]):
        with pytest.raises(NotImplementedError):
            CoDec(P.parse(P.lbt_parser(), argv))
    CoDec(P.parse(P.lbt_parser(), ["encode", "-B", "2"]))
    CoDec(P.parse(P.lbt_parser(), ["decode", "-B", "8"]))
    with pytest.raises(NotImplementedError):
        codec_class("2D-LBT")


def test_argument_errors_before_any_device_work():
    import ctypes

    import vcf_amd._lib as L
    d = ctypes.c_void_p(16)   # never dereferenced: validation fails first
    lib = L.lib()
    assert lib.vcf_lbt_moments(d, 1, 16, 16, 9, d, d, None) == L.VCF_ERR_UNSUPPORTED
    assert lib.vcf_lbt_moments(d, 1, 16, 16, 1, d, d, None) == L.VCF_ERR_UNSUPPORTED
    assert lib.vcf_lbt_moments(d, 0, 16, 16, 8, d, d, None) == L.VCF_ERR_INVALID
    assert lib.vcf_lbt_moments(None, 1, 16, 16, 8, d, d, None) == L.VCF_ERR_INVALID
    assert lib.vcf_lbt_train(d, d, 1, 8, 12, -1, 1e-3, 1e-6, d, d, d, d, None) == L.VCF_ERR_INVALID
    assert lib.vcf_lbt_train(d, d, 1, 8, 0, 5, 1e-3, 1e-6, d, d, d, d, None) == L.VCF_ERR_INVALID
    assert lib.vcf_lbt_train(d, d, 1, 9, 12, 5, 1e-3, 1e-6, d, d, d, d, None) == L.VCF_ERR_UNSUPPORTED
    assert lib.vcf_lbt_train(d, d, 1, 8, 12, 5, 0.0, 1e-6, d, d, d, d, None) == L.VCF_ERR_INVALID
    assert lib.vcf_lbt_train(d, d, 1, 8, 12, 5, 1e-3, 1e-6, d, None, d, d, None) == L.VCF_ERR_INVALID
    for fn in (lib.vcf_lbt_dz_encode, lib.vcf_lbt_dz_decode):
        assert fn(d, 1, 16, 16, 8, 0, 0, d, d, d, None) == L.VCF_ERR_INVALID
        assert fn(d, 1, 16, 16, 8, 32, 4, d, d, d, None) == L.VCF_ERR_INVALID
        assert fn(d, 1, 16, 16, 9, 32, 0, d, d, d, None) == L.VCF_ERR_UNSUPPORTED
        assert fn(d, 1, 16, 16, 8, 32, 0, d, None, d, None) == L.VCF_ERR_INVALID
        assert fn(d, 1, 0, 16, 8, 32, 0, d, d, d, None) == L.VCF_ERR_INVALID
    assert lib.vcf_last_error()

"""RDE without a GPU: the parser, the code-stream prefix rule, the printed lines
from recorded numbers (tests/golden/rde_*.npz: the reference's RDE.py run as a
program), the dimension-mismatch branch, the readers' refusals, and the
argument checks of vcf_distortion_u8, which answer before any device work."""
import ctypes
import json
import os

import numpy as np
import pytest
from PIL import Image

from conftest import GOLDEN

import vcf_amd._lib as L
from vcf_amd.codec import parser as P
from vcf_amd.codec import rde


def cases():
    with open(os.path.join(GOLDEN, "manifest_rde.json")) as f:
        return json.load(f)["cases"]


NAMES = [c["name"] for c in cases()]


def load(name):
    return np.load(os.path.join(GOLDEN, f"rde_{name}.npz"))


def lay_out(z, d):
    """Write a fixture's files into directory d; -> (original, -c argument, decoded, expected lines) with names
    relative to d, for a caller whose working directory it is: the prefix rule cuts at the first dot of the whole
    path, so the result must not depend on where the temporary directory lives."""
    d = str(d)
    with open(os.path.join(d, "original.png"), "wb") as f:
        f.write(z["original_png"].tobytes())
    with open(os.path.join(d, "decoded.png"), "wb") as f:
        f.write(z["decoded_png"].tobytes())
    for fn, n in zip(z["cs_names"], z["cs_lengths"]):
        with open(os.path.join(d, str(fn)), "wb") as f:
            f.write(bytes(int(n)))
    return "original.png", str(z["cflag"]), "decoded.png", [str(ln).replace("{D}/", "") for ln in z["lines"]]


def canon(lines):
    """glob's order is the directory's: the per-file lines and the list in the summary line are
    compared sorted; everything else in place."""
    import ast
    files = sorted(ln for ln in lines if ln.startswith("RDE: Code-stream file:"))
    rest = []
    for ln in lines:
        if ln.startswith("RDE: Code-stream file:"):
            continue
        if ln.startswith("RDE: Code-stream: ["):
            end = ln.index("]") + 1
            ln = "RDE: Code-stream: " + repr(sorted(ast.literal_eval(ln[len("RDE: Code-stream: "):end]))) + ln[end:]
        rest.append(ln)
    n_files = sum(1 for ln in lines if ln.startswith("RDE: Code-stream file:"))
    assert [ln.startswith("RDE: Code-stream file:") for ln in lines[:n_files]] == [True] * n_files   # they come first
    return files + rest


def test_parser_flags_and_defaults():
    a = P.rde_parser().parse_args([])
    assert (a.original, a.codestream, a.decoded, a.number_of_frames) == \
        ("/tmp/original.png", "/tmp/encoded*", "/tmp/decoded.png", None)
    a = P.rde_parser().parse_args(["-o", "a.png", "-c", "b", "-d", "c.png", "-N", "7"])
    assert (a.original, a.codestream, a.decoded, a.number_of_frames) == ("a.png", "b", "c.png", 7)
    a = P.rde_parser().parse_args(["--original", "a.png", "--codestream", "b", "--decoded", "c.png"])
    assert (a.original, a.codestream, a.decoded) == ("a.png", "b", "c.png")
    with pytest.raises(SystemExit):      # RDE.py uses parse_args: unknown options are errors
        P.rde_parser().parse_args(["-q", "3"])
    c = P.rd_curve_parser().parse_args([])
    assert (c.original, c.QSS, c.block_size_DCT, c.perceptual_quantization, c.disable_subbands, c.json,
            c.number_of_frames) == ("/tmp/original.png", "8,16,32,64", 8, False, False, False, None)
    assert "no counterpart in the reference" in " ".join(P.rd_curve_parser().format_help().split())


def test_prefix_rule():
    assert rde.codestream_prefix("/tmp/encoded*") == "/tmp/encoded**"
    assert rde.codestream_prefix("/tmp/encoded.tif") == "/tmp/encoded*"
    assert rde.codestream_prefix("/tmp/encoded.v2.tif") == "/tmp/encoded*"
    assert rde.codestream_prefix("/data/run.1/encoded") == "/data/run*"      # the first dot, wherever it is


def test_glob_rule(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)     # relative paths: no dot but the ones written here
    for fn, n in (("encoded.tif", 10), ("encoded_shape.bin", 12), ("encoded.v2.tif", 5), ("other.tif", 99)):
        (tmp_path / fn).write_bytes(bytes(n))
    for flag in ("encoded", "encoded*", "encoded.tif", "encoded.v2.tif"):
        assert sorted(rde.codestream_files(flag)) == ["encoded.tif", "encoded.v2.tif", "encoded_shape.bin"], flag
    # a dot in a directory name cuts the pattern there, as in the reference: the directory itself matches
    os.mkdir("run.1")
    (tmp_path / "run.1" / "encoded.tif").write_bytes(bytes(3))
    assert rde.codestream_files(os.path.join("run.1", "encoded")) == ["run.1"]


@pytest.mark.parametrize("name", NAMES)
def test_lines_from_recorded_numbers(name, tmp_path, monkeypatch):
    """Result.lines() prints what RDE.py printed, given the exact RMSE (no GPU: the numbers are the manifest's)."""
    z, case = load(name), next(c for c in cases() if c["name"] == name)
    o, c, d, want = lay_out(z, tmp_path)
    monkeypatch.chdir(tmp_path)
    files = rde.codestream_files(c)
    r = rde.Result(o, d, files, [os.path.getsize(f) for f in files], os.path.getsize(o), os.path.getsize(d),
                   tuple(z["original"].shape), case["exact_rmse"])
    assert canon(r.lines()) == canon(want)


@pytest.mark.parametrize("name", NAMES)
def test_fixtures_are_off_the_rounding_boundary(name):
    """Exact RMSE * 100 at least 0.01 from a half-integer, and RDE.py's float32 arithmetic (restated) prints the same."""
    z = load(name)
    a, b = z["original"], z["decoded"]
    d = a.astype(np.int64) - b.astype(np.int64)
    exact = float(np.sqrt(float((d * d).sum()) / d.size))
    assert abs((exact * 100) % 1.0 - 0.5) >= 0.01
    f32 = np.sqrt(((a.astype(np.float32) - b.astype(np.float32)) ** 2).mean())
    assert f"{f32:.2f}" == f"{exact:.2f}"
    assert any(str(ln) == f"RDE: Distortion (RMSE): {exact:.2f}" for ln in z["lines"])
    assert np.array_equal(np.array(Image.open(__import__("io").BytesIO(z["original_png"].tobytes()))), a)


def test_readers(tmp_path, monkeypatch):
    z = load("rgb_37x53")
    o, _, _, _ = lay_out(z, tmp_path)
    monkeypatch.chdir(tmp_path)
    assert np.array_equal(rde.read_image(o), z["original"])                   # the library's PNG reader
    g = load("grey_16x16")
    Image.fromarray(g["original"]).save(tmp_path / "g.png")
    assert np.array_equal(rde.read_image(str(tmp_path / "g.png")), g["original"])   # PIL: H x W
    rgba = np.random.Generator(np.random.PCG64(5)).integers(0, 256, (9, 7, 4), dtype=np.uint8)
    Image.fromarray(rgba).save(tmp_path / "rgba.png")
    assert np.array_equal(rde.read_image(str(tmp_path / "rgba.png")), rgba)   # alpha kept, as np.array(Image.open())
    Image.fromarray(np.arange(64, dtype=np.uint16).reshape(8, 8) * 900).save(tmp_path / "deep.png")
    with pytest.raises(NotImplementedError):
        rde.read_image(str(tmp_path / "deep.png"))
    with pytest.raises(FileNotFoundError, match="no such image file"):
        rde.read_image(str(tmp_path / "absent.png"))
    with pytest.raises(FileNotFoundError):
        rde.evaluate(str(tmp_path / "absent.png"), str(tmp_path / "encoded"), o)


def test_mismatch_branch(tmp_path, capsys):
    """RDE.py:34-38's three lines, then a non-zero status instead of the reference's TypeError."""
    Image.fromarray(np.zeros((8, 10, 3), np.uint8)).save(tmp_path / "a.png")
    Image.fromarray(np.zeros((8, 12, 3), np.uint8)).save(tmp_path / "b.png")
    rc = rde.main(["-o", str(tmp_path / "a.png"), "-c", str(tmp_path / "enc"), "-d", str(tmp_path / "b.png")])
    assert rc == 1
    assert capsys.readouterr().out.splitlines() == ["Error: Image dimensions do not match.",
                                                    "Image 1 shape: (8, 10, 3)", "Image 2 shape: (8, 12, 3)"]
    with pytest.raises(rde.ShapeMismatch):
        rde.evaluate(str(tmp_path / "a.png"), str(tmp_path / "enc"), str(tmp_path / "b.png"))


@pytest.mark.parametrize("args", [dict(C=0), dict(C=5), dict(n=-1), dict(H=-1), dict(W=-3), dict(a=None), dict(b=None),
                                  dict(out=None), dict(out=ctypes.c_void_p(20))])
def test_argument_errors_before_any_device_work(args):
    dummy = ctypes.c_void_p(16)    # never dereferenced: validation fails first
    a = dict(a=dummy, b=dummy, n=1, H=8, W=8, C=3, out=dummy)
    a.update(args)
    rc = L.lib().vcf_distortion_u8(a["a"], a["b"], a["n"], a["H"], a["W"], a["C"], a["out"], None)
    assert rc == L.VCF_ERR_INVALID
    assert L.lib().vcf_last_error()


def test_empty_calls_are_no_ops():
    dummy = ctypes.c_void_p(16)    # nothing is enqueued, so nothing is dereferenced
    assert L.lib().vcf_distortion_u8(dummy, dummy, 0, 8, 8, 3, dummy, None) == L.VCF_OK
    assert L.lib().vcf_distortion_u8(dummy, dummy, 4, 0, 8, 3, dummy, None) == L.VCF_OK
    assert L.lib().vcf_distortion_u8(dummy, dummy, 4, 8, 0, 1, dummy, None) == L.VCF_OK


def test_host_conveniences_check_their_inputs():
    """dtype and shape errors are raised before anything is uploaded."""
    from vcf_amd import distortion as DS
    u8 = np.zeros((4, 4, 3), np.uint8)
    with pytest.raises(TypeError):
        DS.measure(u8.astype(np.int16), u8)
    with pytest.raises(TypeError):
        DS.rmse(u8, u8.astype(np.float32))
    with pytest.raises(ValueError):
        DS.measure(u8, np.zeros((4, 5, 3), np.uint8))
    with pytest.raises(ValueError):
        DS.measure(np.zeros((4, 4, 5), np.uint8), np.zeros((4, 4, 5), np.uint8))
    with pytest.raises(ValueError):
        DS.psnr(np.zeros(7, np.uint8), np.zeros(7, np.uint8))
    assert DS.RECORD.itemsize == 24
    assert np.isinf(DS.psnr_of_mse(0.0)) and abs(float(DS.psnr_of_mse(255.0 ** 2))) == 0.0

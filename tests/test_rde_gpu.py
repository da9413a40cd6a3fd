"""RDE on the GPU: the RDE.py drop-in against what the reference's RDE.py printed
(tests/golden/rde_*.npz), evaluate_sequence against per-frame evaluate, rd_curve against the
chain it replaces run through files (encode_fn, decode_fn, RDE on the files), and the -L
search's J values against numpy on the downloaded reconstructions."""
import os
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

from test_rde import NAMES, canon, lay_out, load

import vcf_amd.dct as D
from vcf_amd.codec import parser as P
from vcf_amd.codec import rde
from vcf_amd.codec.dct2d import CoDec

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _frames(n, H, W, seed):
    """Smooth frames with some noise: every Q leaves a distortion and a compressible index frame."""
    rng = np.random.Generator(np.random.PCG64(seed))
    y, x = np.mgrid[0:H, 0:W]
    out = []
    for i in range(n):
        base = np.stack([128 + 90 * np.sin((x + 3 * i) / 9.0) * np.cos(y / 7.0), 2.0 * x + y, 255 - 1.5 * y + 5 * i], -1)
        out.append(np.clip(base + rng.normal(0, 6, (H, W, 3)), 0, 255).astype(np.uint8))
    return np.stack(out)


@pytest.mark.parametrize("name", NAMES)
def test_cli_reproduces_the_reference_lines(name, tmp_path):
    o, c, d, want = lay_out(load(name), tmp_path)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "vcf_amd", "cli", "RDE.py"), "-o", o, "-c", c, "-d", d],
                       cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-1500:]
    assert canon(p.stdout.splitlines()) == canon(want)


def test_cli_defaults_in_process(tmp_path, monkeypatch, capsys):
    """main() in this process prints the same lines (and evaluate() returns the numbers behind them)."""
    z = load("rgb_64x96_two")
    o, c, d, want = lay_out(z, tmp_path)
    monkeypatch.chdir(tmp_path)
    assert rde.main(["-o", o, "-c", c, "-d", d]) == 0
    assert canon(capsys.readouterr().out.splitlines()) == canon(want)
    r = rde.evaluate(o, c, d)
    dd = z["original"].astype(np.int64) - z["decoded"].astype(np.int64)
    assert r.rmse == float(np.sqrt(float((dd * dd).sum()) / dd.size))
    assert r.codestream_bytes == int(z["cs_lengths"].sum()) and r.shape == (64, 96, 3)


def test_sequence_equals_per_frame(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    n = 5
    a = _frames(n, 48, 64, 21)
    rng = np.random.Generator(np.random.PCG64(22))
    b = np.clip(a.astype(np.int64) + rng.integers(-9, 10, a.shape), 0, 255).astype(np.uint8)
    for i in range(n):
        Image.fromarray(a[i]).save(f"original_{i:04d}.png")
        Image.fromarray(b[i]).save(f"decoded_{i:04d}.png")
        with open(f"encoded_{i:04d}.tif", "wb") as f:
            f.write(bytes(500 + 37 * i))
        with open(f"encoded_{i:04d}_shape.bin", "wb") as f:
            f.write(bytes(12))
    seq = rde.evaluate_sequence("original_%04d.png", "decoded_%04d.png", "encoded_%04d", n, batch=3)
    assert seq.launches == 2        # 5 frames of one shape in batches of 3
    for i in range(n):
        one = rde.evaluate(f"original_{i:04d}.png", f"encoded_{i:04d}", f"decoded_{i:04d}.png")
        assert seq.bytes[i] == one.codestream_bytes == 512 + 37 * i
        assert seq.bpp[i] == one.codestream_bpp and seq.rmse[i] == one.rmse and seq.psnr[i] == one.psnr
        assert sorted(seq.frames[i].codestream_files) == sorted(one.codestream_files)
    assert seq.means["rmse"] == float(seq.rmse.mean()) and seq.means["bytes"] == float(seq.bytes.mean())
    assert rde.main(["-o", "original_%04d.png", "-c", "encoded_%04d", "-d", "decoded_%04d.png", "-N", str(n)]) == 0
    out = capsys.readouterr().out.splitlines()
    assert len(out) == n + 1 and all(ln.startswith("RDE: ") for ln in out)
    assert out[0].startswith(f"RDE: Frame 0: 512 bytes ({512 * 8 / (48 * 64):.2f}) bits/pixel, RMSE {seq.rmse[0]:.2f},")
    assert out[-1].startswith("RDE: Mean of 5 frames:")


@pytest.mark.parametrize("H,W", [(64, 96), (61, 77)])
def test_rd_curve_equals_the_file_chain(H, W, tmp_path, monkeypatch):
    """bytes and RMSE, exactly: encode_fn, decode_fn and RDE through temporary files, per frame and Q."""
    monkeypatch.chdir(tmp_path)
    frames, Qs = _frames(3, H, W, 31), [8, 32]
    curve = rde.rd_curve(frames, Qs, block_size=8)
    assert [c["Q"] for c in curve] == Qs
    for c in curve:
        for i in range(3):
            Image.fromarray(frames[i]).save("original.png")
            for fn in ("encoded.tif", "encoded_shape.bin", "decoded.png"):
                if os.path.exists(fn):
                    os.remove(fn)
            CoDec(P.parse(P.dct_parser(), ["encode", "-q", str(c["Q"])])).encode_fn("original.png", "encoded")
            CoDec(P.parse(P.dct_parser(), ["decode", "-q", str(c["Q"])])).decode_fn("encoded", "decoded.png")
            r = rde.evaluate("original.png", "encoded", "decoded.png")
            assert sorted(r.codestream_files) == ["encoded.tif", "encoded_shape.bin"]
            assert int(c["bytes"][i]) == r.codestream_bytes == os.path.getsize("encoded.tif") + 12
            assert c["rmse"][i] == r.rmse and c["rmse"][i] > 0
            assert c["bpp"][i] == r.codestream_bpp and c["J"][i] == r.J and c["psnr"][i] == r.psnr
    assert (curve[0]["bytes"] > curve[1]["bytes"]).all() and (curve[0]["rmse"] < curve[1]["rmse"]).all()


def test_rd_curve_refuses_what_it_does_not_cover():
    with pytest.raises(TypeError):
        rde.rd_curve(np.zeros((8, 8, 3), np.float32), [8])
    with pytest.raises(ValueError):
        rde.rd_curve(np.zeros((8, 8), np.uint8), [8])


def test_L_candidates_unchanged():
    """optimize_block_size's J per candidate = bytes + Lambda * np.sqrt(np.mean(...)) of the reconstruction
    downloaded here, to the last bit."""
    img = _frames(1, 128, 128, 41)[0]
    codec = CoDec(P.parse(P.dct_parser(), ["encode", "-q", "16"]))
    codec.Lambda = 25.0
    chosen = codec.optimize_block_size(img)
    x64 = img.astype(np.float32).astype(np.float64)
    want = {}
    for B in [2 ** i for i in range(1, 8)]:
        k = D.encode_k32(img, 16, 0, B)
        cs = codec.compress(k.astype(np.uint8))
        cs.seek(0)
        y = D.decode_k32(k, 128, 128, 16, 0, B)
        assert y.dtype == np.uint8
        want[B] = len(cs.read()) + 25.0 * float(np.sqrt(np.mean((x64 - y) ** 2)))
    assert codec.J == want
    assert chosen == min(want, key=lambda B: (want[B], B)) == codec.block_size

"""vcf_ssim_u8 on the GPU (vcf_ssim.hip through vcf_amd.distortion): sum_k, windows and min_k must
equal the numpy restatement (tests/ssim_ref.py) exactly -- at one window, one row and one column of
windows, odd sizes, every size around the kernel's tile edge, many tiles, batches whose frames start
at every byte alignment, and contents that reach the extremes of the factors -- and must not depend
on the batch split or on the run; then rd_curve(ssim=True) and RDE.py --ssim on top of it."""
import os
import subprocess
import sys

import numpy as np
import pytest

import ssim_ref as R
from test_rde import canon, lay_out, load

import vcf_amd.dct as D
from vcf_amd import distortion as DS
from vcf_amd._lib import call, lib
from vcf_amd.codec import rde
from vcf_amd.device import DeviceBuffer, Stream

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = lib().vcf_ssim_tile()        # the tile edge in windows: a frame of T + 10 rows is exactly one tile high

CONTENTS = ("identical", "black_white", "random", "checker", "gradient")


def content(kind, shape, seed):
    """(a, b) of n x H x W x C u8."""
    n, H, W, C = shape
    rng = np.random.Generator(np.random.PCG64(seed))
    if kind == "identical":
        a = rng.integers(0, 256, shape, dtype=np.uint8)
        return a, a.copy()
    if kind == "black_white":
        return np.zeros(shape, np.uint8), np.full(shape, 255, np.uint8)
    if kind == "random":                 # independent: negative k
        return rng.integers(0, 256, shape, dtype=np.uint8), rng.integers(0, 256, shape, dtype=np.uint8)
    y, x = np.mgrid[0:H, 0:W]
    if kind == "checker":                # against its inverse: the extremes of f2 and f4
        ck = np.broadcast_to(((((x + y) & 1) * 255).astype(np.uint8))[None, :, :, None], shape).copy()
        return ck, 255 - ck
    base = np.stack([(2.0 * x + 1.5 * y + 40 * c) % 256 for c in range(C)], -1)[None] + np.zeros((n, 1, 1, 1))
    a = np.clip(base, 0, 255).astype(np.uint8)
    b = np.clip(base + rng.normal(0, 7, shape), 0, 255).astype(np.uint8)
    return a, b


def check(m, a, b):
    s, w, mn = R.ssim_ref(a, b)
    assert m.sum_k.dtype == np.int64 and m.min_k.dtype == np.int64
    assert m.windows == w
    assert np.array_equal(m.sum_k, s)
    assert np.array_equal(m.min_k, mn)
    assert np.array_equal(m.per_channel(), R.per_channel(s, w)) and np.array_equal(m.per_frame(), R.per_frame(s, w))
    return s, w, mn


AROUND_TILE = [(T + dy, T + dx, 3) for dy in (9, 10, 11) for dx in (9, 10, 11)]
SHAPES = [(11, 11, 1), (11, 11, 3), (11, 40, 3), (40, 11, 1), (12, 27, 3), (37, 53, 3)] + AROUND_TILE + [(270, 480, 3)]


@pytest.mark.parametrize("H,W,C", SHAPES)
def test_shapes_and_contents(H, W, C):
    for i, kind in enumerate(CONTENTS):
        a, b = content(kind, (1, H, W, C), 100 * H + W + 7 * i + C)
        s, w, mn = check(DS.ssim(a, b), a, b)
        if kind == "identical":
            assert (s == w * 2 ** 30).all() and (mn == 2 ** 30).all()
        if kind == "random" and H * W > 400:
            assert (mn < 0).all()
    g = DS.ssim(a[0, :, :, 0], b[0, :, :, 0])                     # H x W: one grey frame
    assert g.sum_k.shape == (1, 1) and int(g.sum_k[0, 0]) == int(s[0, 0])


def test_batch_of_different_frames():
    """Five frames of 37 x 53 x 3 (5883 bytes: every frame starts at another alignment), each with its own
    content and its own distortion per channel: a frame or channel mix-up cannot cancel."""
    n, H, W = 5, 37, 53
    rng = np.random.Generator(np.random.PCG64(11))
    a = np.concatenate([content(kind, (1, H, W, 3), 50 + i)[0] for i, kind in enumerate(CONTENTS)])
    b = a.astype(np.int64)
    for f in range(n):
        for c in range(3):
            b[f, :, :, c] += rng.integers(-(2 + 3 * f + 5 * c), 3 + 3 * f + 5 * c, (H, W))
    b = np.clip(b, 0, 255).astype(np.uint8)
    s, w, _ = check(DS.ssim(a, b), a, b)
    assert len({int(v) for v in s.ravel()}) == n * 3


def test_repeatable_and_independent_of_the_batch():
    H, W = 270, 480
    a, b = content("gradient", (4, H, W, 3), 21)
    b[1] = content("random", (1, H, W, 3), 22)[1][0]
    st = Stream()
    da, db = DeviceBuffer.from_array(a, st), DeviceBuffer.from_array(b, st)
    out = DeviceBuffer(4 * 3 * DS.SSIM_RECORD.itemsize)
    out.fill(0xFF, st)                   # the call sets the records itself
    try:
        DS.ssim_device(da, db, 4, H, W, 3, out, st)
        first = DS.ssim_records(out, 4, 3, st)
        check(first, a, b)
        DS.ssim_device(da, db, 4, H, W, 3, out, st)
        second = DS.ssim_records(out, 4, 3, st)
        assert np.array_equal(first.sum_k, second.sum_k) and np.array_equal(first.min_k, second.min_k)
        assert first.windows == second.windows == 260 * 470
        F = H * W * 3
        for f in range(4):
            call("vcf_ssim_u8", da.address(f * F), db.address(f * F), 1, H, W, 3, out.ptr, st.handle)
            one = DS.ssim_records(out, 1, 3, st)
            assert np.array_equal(one.sum_k[0], first.sum_k[f]) and np.array_equal(one.min_k[0], first.min_k[f])
    finally:
        st.synchronize()
        for buf in (da, db, out):
            buf.free()
        st.close()


def test_frame_sets_at_any_offset():
    """Frame sets that start off a 16-byte boundary, and at different offsets from it: the staging's 16-byte pieces
    are cut per frame set, and the pieces across a set's first and last bytes are read bytewise."""
    n, H, W, C = 2, 29, 45, 3
    a, b = content("random", (n, H, W, C), 31)
    F = n * H * W * C
    da, db = DeviceBuffer(F + 16), DeviceBuffer(F + 16)
    out = DeviceBuffer(n * C * DS.SSIM_RECORD.itemsize)
    try:
        for oa, ob in ((3, 3), (0, 5), (7, 2), (15, 0)):
            da.fill(0xAA)
            db.fill(0x55)
            da.upload(a, offset=oa)
            db.upload(b, offset=ob)
            call("vcf_ssim_u8", da.address(oa), db.address(ob), n, H, W, C, out.ptr, None)
            check(DS.ssim_records(out, n, C), a, b)
    finally:
        for buf in (da, db, out):
            buf.free()


def test_default_out_and_small_buffers():
    a, b = content("gradient", (1, 16, 16, 3), 41)
    da, db = DeviceBuffer.from_array(a), DeviceBuffer.from_array(b)
    out = DS.ssim_device(da, db, 1, 16, 16, 3)
    check(DS.ssim_records(out, 1, 3), a, b)
    with pytest.raises(ValueError):
        DS.ssim_device(da, db, 2, 16, 16, 3)                  # the inputs hold one frame
    with pytest.raises(ValueError):
        DS.ssim_device(da, db, 1, 16, 16, 3, out=DeviceBuffer(8))
    with pytest.raises(ValueError, match="11 x 11"):
        DS.ssim_device(da, db, 1, 10, 16, 3)
    for buf in (da, db, out):
        buf.free()


def _frames(n, H, W, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    y, x = np.mgrid[0:H, 0:W]
    out = []
    for i in range(n):
        base = np.stack([128 + 90 * np.sin((x + 3 * i) / 9.0) * np.cos(y / 7.0), 2.0 * x + y, 255 - 1.5 * y + 5 * i], -1)
        out.append(np.clip(base + rng.normal(0, 6, (H, W, 3)), 0, 255).astype(np.uint8))
    return np.stack(out)


def test_rd_curve_with_ssim():
    """ssim is the restatement's value for the frames dct.decode returns for dct.encode's indices, per frame,
    exactly; every other key equals the ssim=False call's."""
    H, W, Qs = 64, 96, (8, 64)
    frames = _frames(2, H, W, 51)
    plain = rde.rd_curve(frames, Qs)
    curve = rde.rd_curve(frames, Qs, ssim=True)
    assert [sorted(c) for c in plain] == [["J", "Q", "bpp", "bytes", "psnr", "rmse"]] * 2
    for c, p, Q in zip(curve, plain, Qs):
        assert sorted(c) == ["J", "Q", "bpp", "bytes", "psnr", "rmse", "ssim"] and c["Q"] == p["Q"] == Q
        for key in ("bytes", "bpp", "rmse", "psnr", "J"):
            assert np.array_equal(c[key], p[key]), key
        assert c["ssim"].shape == (2,) and c["ssim"].dtype == np.float64
        for i in range(2):
            rec = D.decode(D.encode(frames[i], Q), H, W, Q)
            s, w, _ = R.ssim_ref(frames[i], rec)
            assert c["ssim"][i] == R.per_frame(s, w)[0]
    assert (curve[0]["ssim"] > curve[1]["ssim"]).all() and (curve[1]["ssim"] < 1).all()


def test_cli_prints_the_extra_line(tmp_path, monkeypatch, capsys):
    """RDE.py --ssim: today's lines, then the SSIM line with the restatement's value; without the flag, today's."""
    z = load("rgb_37x53")
    o, c, d, want = lay_out(z, tmp_path)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "vcf_amd", "cli", "RDE.py"), "-o", o, "-c", c, "-d", d,
                        "--ssim"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-1500:]
    got = p.stdout.splitlines()
    s, w, _ = R.ssim_ref(z["original"], z["decoded"])
    assert got[-1] == f"RDE: SSIM: {R.per_frame(s, w)[0]:.4f}"
    assert canon(got[:-1]) == canon(want)
    monkeypatch.chdir(tmp_path)
    assert rde.main(["-o", o, "-c", c, "-d", d]) == 0
    assert canon(capsys.readouterr().out.splitlines()) == canon(want)
    r = rde.evaluate(o, c, d, ssim=True)
    assert r.ssim == R.per_frame(s, w)[0] and rde.evaluate(o, c, d).ssim is None


def test_sequence_with_ssim(tmp_path, monkeypatch):
    from PIL import Image
    monkeypatch.chdir(tmp_path)
    a = _frames(3, 24, 32, 61)
    b = np.clip(a.astype(np.int64) + np.random.Generator(np.random.PCG64(62)).integers(-9, 10, a.shape), 0, 255)
    b = b.astype(np.uint8)
    for i in range(3):
        Image.fromarray(a[i]).save(f"original_{i:04d}.png")
        Image.fromarray(b[i]).save(f"decoded_{i:04d}.png")
        with open(f"encoded_{i:04d}.tif", "wb") as f:
            f.write(bytes(100 + i))
    seq = rde.evaluate_sequence("original_%04d.png", "decoded_%04d.png", "encoded_%04d", 3, batch=2, ssim=True)
    s, w, _ = R.ssim_ref(a, b)
    assert np.array_equal(seq.ssim, R.per_frame(s, w)) and seq.means["ssim"] == float(seq.ssim.mean())
    assert all(ln.endswith(f", SSIM {v:.4f}") for ln, v in zip(seq.lines(), list(seq.ssim) + [seq.means["ssim"]]))
    plain = rde.evaluate_sequence("original_%04d.png", "decoded_%04d.png", "encoded_%04d", 3, batch=2)
    assert plain.ssim is None and "ssim" not in plain.means and not any("SSIM" in ln for ln in plain.lines())
    assert np.array_equal(plain.rmse, seq.rmse) and np.array_equal(plain.bytes, seq.bytes)

"""The index-histogram kernel against np.bincount, its ABI, and choose_q end to end.

Counts are integers, so every comparison is equality.  The shapes are the smallest that reach each
path of vcf_index_hist.hip: frames under one 48-byte span and with unaligned heads and tails
(8 x 8, 61 x 77, 33 x 35 in a batch, whose frames start at every alignment), row segments per
region (the 8 x 8 and 16 x 16 grids), one value in every lane, and a batch across the 65535-frame
launch split.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import batch_split_cases as S
from abi_buffers import Guarded
from vcf_amd import _lib as L
from vcf_amd import rate as R
from vcf_amd.codec import parser as P
from vcf_amd.codec import ratecontrol as RC
from vcf_amd.device import DeviceBuffer, synchronize
from vcf_amd.synthetic import synth_frame

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL = ctypes.c_void_p(0)


def bincounts(frames, rows, cols):
    """n x rows * cols x 3 x 256 by np.bincount, region by region."""
    n, H, W, _ = frames.shape
    rh, cw = H // rows, W // cols
    out = np.zeros((n, rows * cols, 3, 256), np.uint32)
    for f in range(n):
        for i in range(rows):
            for j in range(cols):
                cell = frames[f, i * rh:(i + 1) * rh, j * cw:(j + 1) * cw]
                for c in range(3):
                    out[f, i * cols + j, c] = np.bincount(cell[..., c].ravel(), minlength=256)
    return out


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _index_like(seed, shape):
    """Bytes peaked at the zero index 128, as index planes are, with every value present."""
    rng = _rng(seed)
    a = np.clip(np.rint(rng.laplace(128, 3, shape)), 0, 255).astype(np.uint8)
    noise = rng.integers(0, 256, shape, dtype=np.uint8)
    return np.where(rng.random(shape) < 0.1, noise, a)


CASES = {
    "8x8_plane": ((1, 8, 8, 3), (1, 1)),
    "61x77_plane": ((1, 61, 77, 3), (1, 1)),
    "64x96_grid8": ((1, 64, 96, 3), (8, 8)),
    "48x64_grid16": ((1, 48, 64, 3), (16, 16)),
    "3_frames_33x35": ((3, 33, 35, 3), (1, 1)),
    "2_frames_66x35_grid2x5": ((2, 66, 35, 3), (2, 5)),
    "400x128_plane_sliced": ((2, 400, 128, 3), (1, 1)),        # 150 KiB a frame: several slices a region
    "400x128_grid1x2": ((1, 400, 128, 3), (1, 2)),
}


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("content", ["index_like", "uniform"])
def test_counts_equal_bincount(name, content):
    shape, regions = CASES[name]
    seed = 100 + sorted(CASES).index(name)
    frames = _index_like(seed, shape) if content == "index_like" else _rng(seed).integers(0, 256, shape, dtype=np.uint8)
    if shape[0] > 1:
        assert len({f.tobytes() for f in frames}) == shape[0]
    got = R.histogram(frames, regions=regions)
    want = bincounts(frames, *regions)
    assert got.dtype == np.uint32 and got.shape == want.shape
    assert np.array_equal(got, want)
    assert int(got.sum()) == frames.size


@pytest.mark.parametrize("value", [128, 7])
def test_a_plane_of_one_value(value):
    """Every lane adds to one bin: the zero index (counted in registers) and another value (64 lanes on one counter)."""
    frames = np.full((1, 61, 77, 3), value, np.uint8)
    got = R.histogram(frames)
    want = np.zeros((1, 1, 3, 256), np.uint32)
    want[..., value] = 61 * 77
    assert np.array_equal(got, want)
    assert np.array_equal(R.histogram(frames[:, :60, :70], regions=(4, 7)), bincounts(frames[:, :60, :70], 4, 7))


def test_a_second_call_does_not_accumulate_and_device_buffers_are_reused():
    frames = _index_like(7, (2, 24, 40, 3))
    idx = DeviceBuffer.from_array(frames)
    out = DeviceBuffer(2 * 4 * 768 * 4)
    out.fill(0xFF)
    for _ in range(2):
        assert R.histogram_device(idx, frames.shape, (2, 2), out) is out
    got = out.download(np.empty((2, 4, 3, 256), np.uint32))
    assert np.array_equal(got, bincounts(frames, 2, 2))
    assert np.array_equal(R.histogram(idx, frames.shape, (2, 2)), got)
    with pytest.raises(ValueError):
        R.histogram_device(idx, frames.shape, (2, 2), DeviceBuffer(100))
    idx.free()
    out.free()


def test_batch_across_the_launch_split():
    """N = 65562 frames of 3 x 5 x 3 repeating a pool of 251 (tests/batch_split_cases.py): 45 bytes a frame, so
    the frames start at every alignment and every one is head and tail bytes only."""
    pool = S.distortion()["a"]
    assert pool.shape[1:] == S.DIST_SHAPE and S.pairwise_distinct(pool)
    want_pool = bincounts(pool, 1, 1)
    got = R.histogram(S.batch(pool), regions=(1, 1))
    assert got.shape == (S.N, 1, 3, 256)
    entry = S.entry_of()
    for f in S.PROBES:
        assert np.array_equal(got[f], want_pool[entry[f]]), f
    assert np.array_equal(got, want_pool[entry])


# ---- ABI: pointer alignment and output extent ---------------------------------------------------
def _call(idx, n, H, W, rows, cols, counts, capacity):
    return L.call("vcf_index_hist_u8", idx, n, H, W, rows, cols, counts, capacity, NULL)


@pytest.mark.parametrize("in_off,out_off", [(0, 0), (1, 0), (3, 4), (5, 8), (8, 12), (15, 4), (16, 0)])
def test_any_input_address_and_only_the_stated_extent_is_written(in_off, out_off):
    frames = _index_like(40 + in_off, (2, 20, 26, 3))
    want = bincounts(frames, 2, 2)
    gi = Guarded(frames.nbytes, in_off, frames)
    go = Guarded(want.nbytes + 64, out_off)
    _call(gi.ptr, 2, 20, 26, 2, 2, go.ptr, (want.nbytes + 64) // 4)
    synchronize()
    assert np.array_equal(go.download(np.uint32, want.size).reshape(want.shape), want)
    go.check_outside([(0, want.nbytes)], "counts")
    go.check("counts")
    gi.check_untouched("indices")


def test_rejected_calls_write_nothing():
    frames = _index_like(50, (2, 20, 26, 3))
    need = 2 * 4 * 768
    gi = Guarded(frames.nbytes, 0, frames)
    go = Guarded(need * 4, 0)
    odd = Guarded(need * 4 + 4, 1)
    cases = [
        ("a short output buffer", (gi.ptr, 2, 20, 26, 2, 2, go.ptr, need - 1), L.VCFInvalidArgument),
        ("a misaligned counts pointer", (gi.ptr, 2, 20, 26, 2, 2, odd.ptr, need), L.VCFInvalidArgument),
        ("a grid that does not divide the rows", (gi.ptr, 2, 20, 26, 3, 2, go.ptr, need * 2), L.VCFInvalidArgument),
        ("a grid that does not divide the columns", (gi.ptr, 2, 20, 26, 2, 4, go.ptr, need * 2), L.VCFInvalidArgument),
        ("an empty grid", (gi.ptr, 2, 20, 26, 0, 1, go.ptr, need), L.VCFInvalidArgument),
        ("a negative batch", (gi.ptr, -1, 20, 26, 2, 2, go.ptr, need), L.VCFInvalidArgument),
        ("a null input", (NULL, 2, 20, 26, 2, 2, go.ptr, need), L.VCFInvalidArgument),
        ("a grid over 16", (gi.ptr, 2, 20, 26, 20, 1, go.ptr, need * 8), L.VCFUnsupported),
    ]
    for what, args, exc in cases:
        with pytest.raises(exc) as e:
            _call(*args)
        assert e.value.status == (L.VCF_ERR_INVALID if exc is L.VCFInvalidArgument else L.VCF_ERR_UNSUPPORTED), what
        synchronize()
        for g in (gi, go, odd):
            g.check_untouched(what)
    with pytest.raises(ValueError):
        R.histogram(frames, regions=(3, 2))
    with pytest.raises(NotImplementedError):
        R.histogram(np.zeros((1, 34, 34, 3), np.uint8), regions=(17, 17))
    # no frames: nothing is enqueued; an empty frame: the counters are zeroed
    _call(gi.ptr, 0, 20, 26, 2, 2, go.ptr, need)
    synchronize()
    go.check_untouched("n_frames = 0")
    _call(gi.ptr, 2, 0, 26, 2, 2, go.ptr, need)
    synchronize()
    assert not go.download(np.uint32, need).any()
    go.check("H = 0")


# ---- choose_q ------------------------------------------------------------------------------------
H, W = 64, 96
BPPS = (0.5, 1.0, 2.0)


@pytest.fixture(scope="module")
def clip():
    frames = np.stack([synth_frame(H, W, seed) for seed in (1, 2, 3)])
    frames.setflags(write=False)
    return frames


def _codec(argv):
    from vcf_amd.codec.dct2d import CoDec
    return CoDec(P.parse(P.dct_parser(), argv))


def _decode_at(q, prefix, out_png):
    """`2D-DCT.py decode -q q -e prefix -d out_png`, in this process."""
    from vcf_amd.codec.eic import read_image
    c = _codec(["decode", "-q", str(q), "-e", prefix, "-d", out_png])
    c.decode_fn(prefix, out_png)
    return read_image(out_png)[0]


@pytest.mark.parametrize("rate", RC.RATES)
@pytest.mark.parametrize("bpp", BPPS)
def test_choose_q_writes_ordinary_q_files(clip, tmp_path, rate, bpp):
    from vcf_amd.codec.eic import write_image
    codec = _codec(["encode"])
    choice = RC.choose_q_frames(clip, target_bpp=bpp, codec=codec, rate=rate)
    budget = int(bpp * H * W / 8)
    print(f"{rate} {bpp} bpp: budget {budget} q {choice.q.tolist()} bytes {choice.bytes.tolist()} "
          f"estimate {choice.estimate.tolist()} probes {choice.probes} corrections {choice.corrections} "
          f"rmse {np.round(choice.rmse, 3).tolist()}")
    assert choice.budget.tolist() == [budget] * 3
    assert choice.probes <= RC.probe_bound(1, 2048) and choice.corrections <= RC.CORRECTIONS
    assert choice.met.all() and (choice.bytes <= budget).all()
    assert ((1 <= choice.q) & (choice.q <= 2048)).all()
    outs = [str(tmp_path / f"rc_{i:04d}") for i in range(3)]
    sizes = RC.write_choice(codec, choice, outs, (H, W, 3))
    for i, out in enumerate(outs):
        q = RC.read_q(out)
        assert q == choice.q[i]
        assert sizes[i] == os.path.getsize(out + ".tif")
        assert choice.bytes[i] == os.path.getsize(out + ".tif") + os.path.getsize(out + "_shape.bin")
        # the same frame through `2D-DCT.py encode -q q`, and both decoded by `2D-DCT.py decode -q q`
        png, fixed = str(tmp_path / f"orig_{i}.png"), str(tmp_path / f"fixed_{i:04d}")
        write_image(png, clip[i])
        _codec(["encode", "-q", str(q)]).encode_fn(png, fixed)
        a = _decode_at(q, out, str(tmp_path / f"dec_rc_{i}.png"))
        b = _decode_at(q, fixed, str(tmp_path / f"dec_fixed_{i}.png"))
        assert a.shape == (H, W, 3) and np.array_equal(a, b)
        d = a.astype(np.float64) - clip[i]
        assert choice.rmse[i] == np.sqrt((d * d).sum() / d.size)


Q_SCAN = (1, 20)        # sizes of the -c TIFF files of synth_frame(32, 32, 13) fall monotonically over these steps


def test_coded_search_against_a_scan_of_every_q():
    """rate = "coded" on one 32 x 32 frame against every Q of the range coded one by one.  The frame and the
    range are chosen so that the sizes are monotone (checked on the host with the oracle encoder and zlib
    when this test was written, and asserted here): the bisection's outcome is then the smallest Q that fits."""
    from vcf_amd import dct as D
    from vcf_amd.codec.tiff import imwrite_bytes
    frame = synth_frame(32, 32, 13)
    codec = _codec(["encode"])
    qs = list(range(Q_SCAN[0], Q_SCAN[1] + 1))
    scan = np.array([len(imwrite_bytes(D.encode(frame, q))) + RC.SIDE_BYTES for q in qs])
    monotone = bool((np.diff(scan) <= 0).all())
    print("scan", scan.tolist())
    assert monotone
    for budget in sorted({int(scan[0]), int(scan[3]) + 1, int(scan[7]), int(scan[12]) - 1, int(scan[-1]), int(scan[-1]) - 1}):
        c = RC.choose_q_frames(frame, target_bytes=budget, codec=codec, rate="coded", q_min=Q_SCAN[0], q_max=Q_SCAN[1])
        fits = [q for q, s in zip(qs, scan) if s <= budget]
        assert c.probes <= RC.probe_bound(*Q_SCAN)
        if fits:
            assert c.met[0] and c.bytes[0] <= budget
            assert c.bytes[0] == scan[int(c.q[0]) - Q_SCAN[0]]
            assert c.q[0] == fits[0]
        else:
            assert not c.met[0] and c.q[0] == Q_SCAN[1]


@pytest.mark.parametrize("entropy", ["TCBAAC2D", "z_lib"])
def test_other_entropy_codecs(clip, entropy):
    """The device coder (compress_device) and a host-only codec, both rates."""
    codec = _codec(["encode", "-c", entropy])
    for rate in RC.RATES:
        c = RC.choose_q_frames(clip[:2], target_bpp=2.0, codec=codec, rate=rate, q_max=256)
        assert c.met.all()
        for i in range(2):
            k = codec.decompress(c.payloads[i])
            from vcf_amd import dct as D
            assert np.array_equal(k, D.encode(clip[i], int(c.q[i])))


def test_rate_control_cli_and_iii(clip, tmp_path):
    """rate-control.py encode + 2D-DCT.py decode -q <chosen>, and III encode --target_bpp + decode --q_from_files."""
    from vcf_amd.codec.eic import read_image, write_image
    from vcf_amd.codec.iii import CoDec as III
    for i in range(3):
        write_image(str(tmp_path / f"original_{i:04d}.png"), clip[i])
    out = "/tmp/encoded"       # 2D-DCT.py's decode() reads the reference's hard-wired paths, whatever -e and -d say
    env = dict(os.environ, PYTHONPATH=ROOT)
    subprocess.run([sys.executable, os.path.join(ROOT, "vcf_amd/cli/rate-control.py"), "encode", "-o",
                    str(tmp_path / "original_0000.png"), "--target_bpp", "1.0", "--rate", "coded"],
                   check=True, env=env, timeout=120)
    q = RC.read_q(out)
    assert os.path.getsize(out + ".tif") + 12 <= 768
    want = RC.choose_q_frames(clip[0], target_bpp=1.0, codec=_codec(["encode"]), rate="coded")
    assert q == want.q[0] and open(out + ".tif", "rb").read() == want.payloads[0]
    subprocess.run([sys.executable, os.path.join(ROOT, "vcf_amd/cli/2D-DCT.py"), "decode", "-q", str(q)],
                   check=True, env=env, timeout=120)
    from vcf_amd import dct as D
    assert np.array_equal(read_image("/tmp/decoded.png")[0], D.decode(D.encode(clip[0], q), H, W, q))

    kw = dict(encode_prefix=str(tmp_path / "encoded"), decode_prefix=str(tmp_path / "decoded"))
    e = III(P.parse(P.iii_parser(rate_control=True), ["encode", "-N", "3", "--target_bytes", "1000", "-o",
                                                      str(tmp_path / "original_%04d.png")]), **kw)
    total = e.encode()
    assert total == sum(os.path.getsize(str(tmp_path / f"encoded_{i:04d}.tif")) for i in range(3))
    qs = [RC.read_q(str(tmp_path / f"encoded_{i:04d}")) for i in range(3)]
    assert all(os.path.getsize(str(tmp_path / f"encoded_{i:04d}.tif")) + 12 <= 1000 for i in range(3))
    III(P.parse(P.iii_parser(rate_control=True), ["decode", "-N", "3", "--q_from_files"]), **kw).decode()
    for i in range(3):
        got = read_image(str(tmp_path / f"decoded_{i:04d}.png"))[0]
        assert np.array_equal(got, D.decode(D.encode(clip[i], qs[i]), H, W, qs[i]))
    with pytest.raises(NotImplementedError):
        III(P.parse(P.iii_parser(transform="2D-DWT", rate_control=True), ["encode", "-T", "2D-DWT", "--target_bpp", "1"]))

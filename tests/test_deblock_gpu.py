"""-f deblock on the GPU: vcf_deblock_u8 bit for bit against tests/deblock_ref.py over the cases
tests/test_deblock.py checks for branch coverage, the entry's argument errors and stream order, and
the filter behind the decoders of 2D-DCT, 2D-KLT and 2D-LBT, III and rd_curve."""
import numpy as np
import pytest

import deblock_ref as R

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 0xA5
OFFSETS = [(0, 0), (1, 1), (3, 3), (1, 3)]     # (in, out) bytes off a 16-byte aligned base


def _run(frames, B, top, left, beta, tc, in_off, out_off, stride_pad=7, stream=None):
    """frames through vcf_deblock_u8 from bases in_off / out_off bytes off alignment, a frame every
    F + stride_pad bytes, the output inside guard bytes -> (filtered frames, whether every byte
    outside them came back untouched)."""
    from vcf_amd import deblock as DB
    from vcf_amd.device import DeviceBuffer
    n, H, W, _ = frames.shape
    F = H * W * 3
    stride = F + stride_pad
    extent = (n - 1) * stride + F
    host_in = np.zeros(in_off + n * stride, np.uint8)
    for i in range(n):
        host_in[in_off + i * stride:in_off + i * stride + F] = frames[i].ravel()
    base = 16 * ((GUARD + 15) // 16)
    total = base + out_off + extent + GUARD
    din, dout = DeviceBuffer.from_array(host_in), DeviceBuffer(total)
    try:
        assert din.ptr.value % 16 == 0 and dout.ptr.value % 16 == 0
        dout.upload(np.full(total, FILL, np.uint8))
        DB.deblock_device(din, n, H, W, B, top, left, beta, tc, out=dout, stream=stream, frame_stride=stride,
                          src_offset=in_off, out_offset=base + out_off)
        if stream is not None:
            stream.synchronize()
        got = dout.download(np.empty(total, np.uint8))
    finally:
        din.free()
        dout.free()
    res = np.empty_like(frames)
    inside = np.zeros(total, bool)
    for i in range(n):
        lo = base + out_off + i * stride
        res[i] = got[lo:lo + F].reshape(H, W, 3)
        inside[lo:lo + F] = True
    return res, bool(np.all(got[~inside] == FILL))


@pytest.mark.parametrize("case", R.GPU_CASES, ids=R.case_id)
def test_kernel_equals_the_restatement(case):
    H, W, B, top, left = case
    frames = R.case_frames(case)
    for beta, tc in R.GPU_STRENGTHS:
        want = R.deblock_ref(frames, B, top, left, beta, tc)
        for in_off, out_off in OFFSETS:
            got, clean = _run(frames, B, top, left, beta, tc, in_off, out_off)
            assert clean, (beta, tc, in_off, out_off, "bytes outside the frames were written")
            assert np.array_equal(got, want), (beta, tc, in_off, out_off, int((got != want).sum()))
    if B > max(H, W):
        assert np.array_equal(want, frames)


def test_contiguous_frames_and_host_wrapper():
    """frame_stride_bytes = H * W * 3 (the codecs' call), many tiles in both directions."""
    from vcf_amd import deblock as DB
    frames = R.blocky_frames(77, 2, 130, 350, 8, 3, 5)
    want = R.deblock_ref(frames, 8, 3, 5, 32, 4)
    assert np.array_equal(DB.deblock(frames, 8, 3, 5, 32, 4), want)
    assert np.array_equal(DB.deblock(frames[0], 8, 3, 5, 32, 4), want[0])
    got, clean = _run(frames, 8, 3, 5, 32, 4, 0, 0, stride_pad=0)
    assert clean and np.array_equal(got, want)
    b4 = R.blocky_frames(78, 1, 70, 200, 4, 1, 3)
    assert np.array_equal(DB.deblock(b4, 4, 1, 3, 4096, 255), R.deblock_ref(b4, 4, 1, 3, 4096, 255))


def test_argument_errors():
    from vcf_amd import _lib
    from vcf_amd.device import DeviceBuffer
    H, W = 16, 16
    F = H * W * 3
    a, b = DeviceBuffer(4 * F), DeviceBuffer(4 * F)
    try:
        b.fill(FILL)
        f = _lib.lib().vcf_deblock_u8

        def rc(pin, pout, n=1, stride=F, B=8, top=0, left=0, beta=16, tc=4):
            return f(pin, pout, n, H, W, stride, B, top, left, beta, tc, None)

        A, Bp = a.ptr, b.ptr
        assert rc(A, Bp) == _lib.VCF_OK
        assert rc(A, A) == _lib.VCF_ERR_INVALID                                  # in place
        assert rc(A, a.address(F - 1)) == _lib.VCF_ERR_INVALID                   # overlapping by a byte
        assert rc(A, a.address(2 * F), n=3) == _lib.VCF_ERR_INVALID              # overlapping batches
        assert rc(A, a.address(2 * F), n=2) == _lib.VCF_OK                       # adjacent, not overlapping
        assert rc(A, Bp, B=3) == _lib.VCF_ERR_INVALID
        assert rc(A, Bp, top=8) == _lib.VCF_ERR_INVALID
        assert rc(A, Bp, left=-1) == _lib.VCF_ERR_INVALID
        assert rc(A, Bp, beta=-1) == _lib.VCF_ERR_INVALID
        assert rc(A, Bp, tc=-1) == _lib.VCF_ERR_INVALID
        assert rc(A, Bp, n=2, stride=F - 1) == _lib.VCF_ERR_INVALID
        assert rc(None, Bp) == _lib.VCF_ERR_INVALID
        b.fill(FILL)
        for bad in (dict(B=3), dict(top=8), dict(pout=None)):
            kw = dict(pin=A, pout=Bp)
            kw.update(bad)
            assert rc(**kw) == _lib.VCF_ERR_INVALID
        assert np.all(b.download(np.empty(4 * F, np.uint8)) == FILL)             # nothing was written
    finally:
        a.free()
        b.free()


def test_call_is_ordered_on_the_callers_stream():
    """A memset of the input on the caller's stream, then the filter on that stream: it reads the memset's bytes."""
    from vcf_amd import deblock as DB
    from vcf_amd.device import DeviceBuffer, Stream
    n, H, W = 2, 300, 400
    frames = R.blocky_frames(9, n, H, W, 8, 0, 0)
    st = Stream()
    din, dout = DeviceBuffer.from_array(frames), DeviceBuffer(frames.nbytes)
    try:
        din.fill(200, st)
        DB.deblock_device(din, n, H, W, 8, 0, 0, 64, 8, out=dout, stream=st)
        got = dout.download(np.empty_like(frames), st)
        st.synchronize()
        assert np.all(got == 200)
    finally:
        din.free()
        dout.free()
        st.close()


# ---- behind the decoders ----------------------------------------------------------------
def _png(fn, img):
    from PIL import Image
    Image.fromarray(img).save(fn)


def _read(fn):
    from PIL import Image
    return np.array(Image.open(fn))


def _natural(H, W, seed):
    """A smooth frame with texture, so that -q 32 leaves visible block edges."""
    rng = np.random.Generator(np.random.PCG64(seed))
    y, x = np.mgrid[0:H, 0:W]
    base = np.stack([128 + 90 * np.sin(x / 11.0 + c) * np.cos(y / 17.0 - c) for c in range(3)], axis=2)
    return np.clip(base + rng.normal(0, 6, (H, W, 3)), 0, 255).astype(np.uint8)


CODECS = [("2D-DCT", ["-B", "8"], (64, 96)), ("2D-DCT", ["-B", "4"], (32, 40)), ("2D-DCT", ["-B", "16", "-x"], (48, 64)),
          ("2D-DCT", ["-B", "8", "-p"], (45, 61)), ("2D-DCT", ["-B", "8", "-a", "LloydMax"], (40, 48)),
          ("2D-KLT", ["-B", "4"], (24, 32)), ("2D-LBT", ["-B", "4"], (26, 30))]


def _codec(name, sub, flags, deblock=None):
    from vcf_amd.codec import parser as P
    mod = {"2D-DCT": "dct2d", "2D-KLT": "klt2d", "2D-LBT": "lbt2d"}[name]
    C = __import__(f"vcf_amd.codec.{mod}", fromlist=["CoDec"]).CoDec
    kw = {"filter": "deblock"} if deblock is not None else {}
    flags = list(flags)
    if name == "2D-DCT":
        make = lambda: P.dct_parser(quantizer="LloydMax" if "LloydMax" in flags else "deadzone", **kw)  # noqa: E731
    else:
        make = {"2D-KLT": P.klt_parser, "2D-LBT": P.lbt_parser}[name]
        make = (lambda m: (lambda: m(**kw)))(make)
    if name == "2D-LBT" and sub == "encode":
        flags += ["--epochs", "10"]
    return C(P.parse(make(), [sub, "-q", "32"] + flags + (list(deblock) if deblock is not None else [])))


@pytest.mark.parametrize("name,flags,shape", CODECS, ids=[c[0] + "".join(c[1]) for c in CODECS])
def test_decode_fn_applies_the_filter(tmp_path, name, flags, shape):
    from vcf_amd import deblock as DB
    H, W = shape
    B = int(flags[flags.index("-B") + 1])
    _png(str(tmp_path / "o.png"), _natural(H, W, 3))
    enc = str(tmp_path / "enc")
    if "LloydMax" in flags:
        enc = "/tmp/encoded"        # LloydMax keeps its side files at the reference's default path
    _codec(name, "encode", flags).encode_fn(str(tmp_path / "o.png"), enc)
    _codec(name, "decode", flags).decode_fn(enc, str(tmp_path / "plain.png"))
    plain = _read(str(tmp_path / "plain.png"))
    c = _codec(name, "decode", flags, deblock=["-f", "deblock"])
    c.decode_fn(enc, str(tmp_path / "fil.png"))
    top, left = c._crop_offsets(H, W)
    assert (top, left) == R.crop_offsets(H, W, B)
    want = R.deblock_ref(plain, B, top, left, *DB.default_strength(32))
    assert np.array_equal(_read(str(tmp_path / "fil.png")), want)
    assert not np.array_equal(want, plain)
    _codec(name, "decode", flags, deblock=["-f", "deblock", "--deblock_beta", "50", "--deblock_tc", "2"]) \
        .decode_fn(enc, str(tmp_path / "fil2.png"))
    assert np.array_equal(_read(str(tmp_path / "fil2.png")), R.deblock_ref(plain, B, top, left, 50, 2))


@pytest.mark.parametrize("name,flags", [("2D-DCT", ["-B", "8"]), ("2D-KLT", ["-B", "4"]), ("2D-LBT", ["-B", "4"])],
                         ids=["2D-DCT", "2D-KLT", "2D-LBT"])
def test_batched_decode_and_iii(tmp_path, name, flags):
    """decode_fns of a mixed-shape batch and III decode -f deblock write what decode_fn writes."""
    from vcf_amd.codec import parser as P
    from vcf_amd.codec.iii import CoDec as III
    shapes = [(37, 45), (24, 32), (37, 45)]
    for i, (H, W) in enumerate(shapes):
        _png(str(tmp_path / f"original_{i:04d}.png"), _natural(H, W, 30 + i))
    enc = _codec(name, "encode", flags)
    for i in range(3):
        enc.encode_fn(str(tmp_path / f"original_{i:04d}.png"), str(tmp_path / f"enc_{i:04d}"))
    one = _codec(name, "decode", flags, deblock=["-f", "deblock"])
    for i in range(3):
        one.decode_fn(str(tmp_path / f"enc_{i:04d}"), str(tmp_path / f"one_{i:04d}.png"))
    many = _codec(name, "decode", flags, deblock=["-f", "deblock"])
    many.decode_fns([(str(tmp_path / f"enc_{i:04d}"), str(tmp_path / f"many_{i:04d}.png")) for i in range(3)])
    d = P.parse(P.iii_parser(transform=name, filter="deblock"),
                ["decode", "-T", name, "-N", "3", "-q", "32", "-f", "deblock"] + flags)
    III(d, encode_prefix=str(tmp_path / "enc"), decode_prefix=str(tmp_path / "dec")).decode()
    plain = _codec(name, "decode", flags)
    changed = 0
    for i in range(3):
        a = _read(str(tmp_path / f"one_{i:04d}.png"))
        assert np.array_equal(_read(str(tmp_path / f"many_{i:04d}.png")), a), i
        assert np.array_equal(_read(str(tmp_path / f"dec_{i:04d}.png")), a), i
        plain.decode_fn(str(tmp_path / f"enc_{i:04d}"), str(tmp_path / f"plain_{i:04d}.png"))
        changed += not np.array_equal(_read(str(tmp_path / f"plain_{i:04d}.png")), a)
    assert changed, "the filter changed no frame: the comparison above would say nothing"


def test_rd_curve_measures_the_filtered_frames():
    from vcf_amd import dct as D
    from vcf_amd import deblock as DB
    from vcf_amd import distortion as DS
    from vcf_amd.codec.rde import rd_curve
    frames = np.stack([_natural(61, 77, 50 + i) for i in range(2)])
    Qs = [16, 64]
    plain = rd_curve(frames, Qs, ssim=True)
    fil = rd_curve(frames, Qs, ssim=True, filter="deblock")
    fil2 = rd_curve(frames, Qs, ssim=True, filter="deblock", deblock_beta=30, deblock_tc=3)
    top, left = R.crop_offsets(61, 77, 8)
    for Q, p, f, f2 in zip(Qs, plain, fil, fil2):
        assert np.array_equal(p["bytes"], f["bytes"]) and np.array_equal(p["bytes"], f2["bytes"])
        rec = D.decode(D.encode(frames, Q), 61, 77, Q)
        for curve, (beta, tc) in ((f, DB.default_strength(Q)), (f2, (30, 3))):
            want = R.deblock_ref(rec, 8, top, left, beta, tc)
            diff = frames.astype(np.int64) - want
            rmse = np.sqrt((diff ** 2).sum(axis=(1, 2, 3)).astype(np.float64) / (61 * 77 * 3))
            assert np.array_equal(curve["rmse"], rmse)
            assert np.array_equal(curve["ssim"], DS.ssim(frames, want).per_frame())
        assert not np.array_equal(p["rmse"], f["rmse"])

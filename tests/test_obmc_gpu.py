"""Overlapped block motion compensation on the GPU (vcf_amd/csrc/vcf_ipp_obmc.hip)
against the numpy restatement of the rule (tests/obmc_ref.py): the kernel bit
for bit, pointer alignment and written extents, a caller's stream, and --obmc
through the IPP codecs end to end against the numpy loop of tests/test_obmc.py."""
import ctypes
import filecmp
import json
import os

import numpy as np
import pytest
from PIL import Image

import obmc_ref as OB
import subpel_ref as R
import test_obmc as T
from abi_buffers import Guarded
from oracle import oracle as O

pytestmark = pytest.mark.gpu

NULL = ctypes.c_void_p(0)
ENTRY = "vcf_ipp_motion_compensate_obmc"
SHAPES = [(48, 80, 16),
          (21, 43, 4),        # rows that are no multiple of 4 bytes, a border outside the blocks
          (37, 50, 8),
          (64, 128, 64),
          (64, 64, 32),
          (16, 16, 16),       # one block
          (10, 12, 16)]       # an empty field


@pytest.fixture(scope="module")
def K():
    from vcf_amd import ipp
    return ipp


@pytest.fixture(scope="module")
def L():
    from vcf_amd import _lib
    from vcf_amd.device import set_device
    set_device(0)
    return _lib


def _frame(rng, H, W):
    return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)


def _fields(rng, shape):
    """Multiples of 1/4 within +-40 pixels (many invalid), within +-2.75 pixels (most valid), and
    the latter with NaN, +-inf and 1e30 entries."""
    wide = (rng.integers(-160, 161, shape) / 4.0).astype(np.float32)
    near = (rng.integers(-11, 12, shape) / 4.0).astype(np.float32)
    odd = (rng.integers(-11, 12, shape) / 4.0).astype(np.float32)
    flat = odd.reshape(-1)
    for i, v in enumerate((np.nan, np.inf, -np.inf, 1e30, -1e30, np.nan)):
        if flat.size:
            flat[(5 * i + 1) % flat.size] = v
    return {"wide": wide, "near": near, "non-finite": odd}


@pytest.mark.parametrize("H,W,bs", SHAPES)
def test_kernel_equals_the_rule(K, H, W, bs):
    rng = np.random.Generator(np.random.PCG64(1000 * H + W))
    f = _frame(rng, H, W)
    for name, mv in _fields(rng, (H // bs, W // bs, 2)).items():
        got = K.motion_compensate(f, mv, bs, subpel=4, obmc=True)
        assert np.array_equal(got, OB.motion_compensate(f, mv, bs)), name
        assert np.array_equal(K.motion_compensate(f, mv, bs, obmc=True), got), name      # every subpel: one entry


@pytest.mark.parametrize("bs", [4, 8, 16, 32, 64])
def test_uniform_valid_field_and_one_block_equal_the_plain_compensator(K, bs):
    rng = np.random.Generator(np.random.PCG64(bs))
    H, W = 2 * bs + 3, 3 * bs + 3
    f = _frame(rng, H, W)
    for v in ((0.0, 0.0), (0.75, 1.25), (2.75, 2.5), (2.0, 1.0)):
        mv = np.tile(np.float32(v), (2, 3, 1))
        assert np.array_equal(K.motion_compensate(f, mv, bs, obmc=True), K.motion_compensate(f, mv, bs, subpel=4)), v
    f = _frame(rng, bs + 2, bs + 3)
    for v in ((1.25, 0.5), (0.0, 1.75), (9.0, 0.0)):                 # the last one is invalid
        mv = np.float32(v).reshape(1, 1, 2)
        assert np.array_equal(K.motion_compensate(f, mv, bs, obmc=True), K.motion_compensate(f, mv, bs, subpel=4)), v


def _guarded_call(L, f, mv, H, W, bs, in_off, out_off, mv_off=0, reject=False, null=None):
    """One call on Guarded buffers at the given byte offsets -> the output bytes; guards checked."""
    from vcf_amd.device import synchronize
    n = H * W * 3
    gf, gm, go = Guarded(f.nbytes, in_off, f), Guarded(max(mv.nbytes, 8) + 4, mv_off, mv), Guarded(n + 64, out_off)
    ptr = {"ref": gf.ptr, "mv": gm.ptr, "out": go.ptr}
    if null:
        ptr[null] = NULL
    what = f"{ENTRY} {H}x{W} bs {bs} in+{in_off} out+{out_off} mv+{mv_off} null {null}"
    if reject:
        with pytest.raises(L.VCFInvalidArgument) as e:
            L.call(ENTRY, ptr["ref"], ptr["mv"], H, W, bs, ptr["out"], NULL)
        assert e.value.status == L.VCF_ERR_INVALID, what
        synchronize()
        for g in (gf, gm, go):
            g.check_untouched(what)
        return None
    L.call(ENTRY, ptr["ref"], ptr["mv"], H, W, bs, ptr["out"], NULL)
    synchronize()
    got = go.download()[:n].copy()
    go.check_outside([(0, n)], what)
    go.check(what)
    gf.check_untouched(what)
    gm.check_untouched(what)
    return got


@pytest.mark.parametrize("H,W,bs", [(48, 80, 16), (21, 43, 4), (37, 50, 8)])
def test_pointers_and_extents(L, H, W, bs):
    rng = np.random.Generator(np.random.PCG64(H))
    f = _frame(rng, H, W)
    mv = (rng.integers(-11, 12, (H // bs, W // bs, 2)) / 4.0).astype(np.float32)
    want = OB.motion_compensate(f, mv, bs).reshape(-1)
    for oi in range(4):
        for oo in range(4):
            assert np.array_equal(_guarded_call(L, f, mv, H, W, bs, oi, oo), want), (oi, oo)
    assert np.array_equal(_guarded_call(L, f, mv, H, W, bs, 0, 0, mv_off=4), want)
    for bad in (0, 2, 12, 128):
        _guarded_call(L, f, mv, H, W, bad, 0, 0, reject=True)
    for null in ("ref", "mv", "out"):
        _guarded_call(L, f, mv, H, W, bs, 0, 0, reject=True, null=null)
    for off in (1, 2, 3):
        _guarded_call(L, f, mv, H, W, bs, 0, 0, mv_off=off, reject=True)


def test_two_calls_on_a_caller_stream(L):
    from vcf_amd.device import DeviceBuffer, Stream
    H, W, bs = 48, 80, 16
    rng = np.random.Generator(np.random.PCG64(77))
    f = _frame(rng, H, W)
    fields = [(rng.integers(-11, 12, (3, 5, 2)) / 4.0).astype(np.float32) for _ in range(2)]
    df = DeviceBuffer.from_array(f)
    dm = [DeviceBuffer.from_array(m) for m in fields]
    do = [DeviceBuffer(f.nbytes) for _ in range(2)]
    s = Stream()
    try:
        for m, o in zip(dm, do):
            L.call(ENTRY, df.ptr, m.ptr, H, W, bs, o.ptr, s.handle)
        s.synchronize()
        got = [o.download(np.empty_like(f)) for o in do]
    finally:
        for b in [df] + dm + do:
            b.free()
        s.close()
    assert not np.array_equal(got[0], got[1])
    for g, m in zip(got, fields):
        assert np.array_equal(g, OB.motion_compensate(f, m, bs))


# ---- the codecs -------------------------------------------------------------------------------

N, GOP, BS, SR, Q = 5, 3, 16, 4, 32
CONFIGS = {"alone": ([], {}), "subpel4": (["--subpel", "4"], dict(subpel=4)), "bframes1": (["--bframes", "1"], dict(bframes=1)),
           "R": (["-R", "0.5"], dict(lam=0.5)), "me_levels1": (["--me_levels", "1"], dict(levels=1))}


@pytest.fixture(scope="module")
def seq():
    return R.subpel_sequence(64, 96, N, seed=4)


def _write_seq(d, frames):
    for i, f in enumerate(frames):
        Image.fromarray(f).save(os.path.join(d, f"in_{i:04d}.png"))
    return os.path.join(d, "in_%04d.png")


def _decoded(prefix):
    return [np.asarray(Image.open(f"{prefix}_{i:04d}.png").convert("RGB")) for i in range(N)]


@pytest.mark.parametrize("name", list(CONFIGS))
def test_ipp_encode_decode_matches_the_loop(tmp_path, seq, name):
    from vcf_amd.codec import parser as P
    from vcf_amd.codec.ipp import CoDec, _IPP, codec_class

    class Host(CoDec):
        def encode_decode_proxy(self, img, frame_type, seq_idx):     # an override: the frame-by-frame host loop
            return _IPP.encode_decode_proxy(self, img, frame_type, seq_idx)

    extra, kw = CONFIGS[name]
    pat = _write_seq(str(tmp_path), seq)
    flags = ["-N", str(N), "-G", str(GOP), "-M", str(BS), "-S", str(SR), "-q", str(Q), "--obmc"] + extra
    for cls, d in ((CoDec, "a"), (Host, "b")):
        os.makedirs(tmp_path / d)
        cls(P.parse(P.ipp_parser(), ["encode", "-i", pat, "-O", str(tmp_path / d / "v")] + flags)).encode()
    assert json.load(open(tmp_path / "a" / "v_meta.json"))["obmc"] is True
    # the resident path's files are the host loop's
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b")) and "v_P_1_enc.tif" in names
    match, mismatch, errors = filecmp.cmpfiles(tmp_path / "a", tmp_path / "b", names, shallow=False)
    assert not mismatch and not errors
    # the decoder reproduces the numpy loop
    dec = str(tmp_path / "dec" / "v")
    assert CoDec(P.parse(P.ipp_parser(), ["decode", "-i", str(tmp_path / "a" / "v"), "-O", dec, "-M", str(BS),
                                          "-q", str(Q)])).decode() == N
    want = T.loop(seq, GOP, BS, SR, Q, **kw)
    for i, got in enumerate(_decoded(dec)):
        assert np.array_equal(got, want[i]), f"frame {i}"
    if name == "alone":
        plain = T.loop(seq, GOP, BS, SR, Q, obmc=False)
        assert any(not np.array_equal(a, b) for a, b in zip(want, plain))
    # --st 2D-DWT round-trips
    p, cls = P.ipp_parser(space_transform="2D-DWT"), codec_class("2D-DWT")
    chain = ["--st", "2D-DWT", "-l", "3", "-w", "bior4.4", "-q", "16"]
    enc, dec = str(tmp_path / "wenc" / "v"), str(tmp_path / "wdec" / "v")
    cls(P.parse(p, ["encode", "-i", pat, "-O", enc] + [a for a in flags if a not in ("-q", str(Q))] + chain)).encode()
    assert cls(P.parse(p, ["decode", "-i", enc, "-O", dec, "-M", str(BS)] + chain)).decode() == N

    def rt(img):
        H, W = img.shape[:2]
        return O.dwt_decode_frame(O.dwt_encode_frame(img, "bior4.4", 3, 16), H, W, "bior4.4", 3, 16)
    want = T.loop(seq, GOP, BS, SR, 16, rt=rt, **kw)
    for i, got in enumerate(_decoded(dec)):
        assert np.array_equal(got, want[i]), f"2D-DWT frame {i}"


def test_device_ipp_files_equal_codec_files(tmp_path):
    """DeviceIPP(obmc=True): every gathered TIFF equals the file CoDec --obmc writes, and the fields agree."""
    from vcf_amd.codec import parser as P
    from vcf_amd.codec.ipp import CoDec
    from vcf_amd.codec.ipp_device import DeviceIPP
    from vcf_amd.device import DeviceBuffer
    n, gop, H, W = 5, 3, 64, 96
    frames = R.subpel_sequence(H, W, n, seed=6)
    pat = _write_seq(str(tmp_path), frames)
    enc = str(tmp_path / "enc" / "v")
    CoDec(P.parse(P.ipp_parser(), ["encode", "-i", pat, "-O", enc, "-N", str(n), "-G", str(gop), "-M", "16", "-S", "4",
                                   "--subpel", "4", "--obmc"])).encode()
    with pytest.raises(ValueError):
        DeviceIPP(None, 0, 1, n, H, W, 32, gop, 12, 4, False, obmc=True)
    job = DeviceIPP(None, 0, 1, n, H, W, 32, gop, 16, 4, False, subpel=4, obmc=True)
    sizes, got, mvs = job.run(DeviceBuffer.from_array(np.stack(frames)))
    files = []
    for g0 in range(0, n, gop):
        files.append(f"{enc}_I_{g0 // gop}_enc.tif")
        files += [f"{enc}_P_{(g0 // gop) * (gop - 1) + p - 1}_enc.tif" for p in range(1, min(gop, n - g0))]
    assert len(got) == n == len(files)
    for i, path in enumerate(files):
        want = open(path, "rb").read()
        assert bytes(got[i]) == want and sizes[i] == len(want), i
    with np.load(enc + "_mv.npz", allow_pickle=False) as z:
        assert np.array_equal(np.stack(mvs), z["mv_f32"])
    # the flag matters: without it the P files differ
    plain = DeviceIPP(None, 0, 1, n, H, W, 32, gop, 16, 4, False, subpel=4)
    _, got_plain, _ = plain.run(DeviceBuffer.from_array(np.stack(frames)))
    assert bytes(got_plain[0]) == bytes(got[0]) and bytes(got_plain[1]) != bytes(got[1])

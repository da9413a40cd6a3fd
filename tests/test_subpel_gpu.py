"""Sub-pel motion on the GPU (vcf_amd/csrc/vcf_ipp_subpel.hip) against the
numpy restatement of the rule (tests/subpel_ref.py): the refined motion
fields and the quarter-pel compensator bit for bit, pointer alignment and
written extents, and --subpel through the IPP codecs end to end."""
import ctypes
import filecmp
import os

import numpy as np
import pytest
from PIL import Image

import subpel_ref as R
from abi_buffers import Guarded
from oracle import oracle as O

pytestmark = pytest.mark.gpu

NULL = ctypes.c_void_p(0)
SHAPES = [(64, 96, 16, 4), (40, 56, 8, 3), (33, 35, 7, 0), (40, 64, 4, 3),
          (16, 16, 16, 8),     # a single block: every fractional candidate is invalid
          (61, 99, 12, 7),
          (10, 12, 16, 8)]     # an empty field


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


_pairs = {}


def _pair(H, W):
    """Two frames of the generator per frame size, made once."""
    if (H, W) not in _pairs:
        _pairs[H, W] = R.subpel_sequence(H, W, 2, seed=H + W)
    return _pairs[H, W]


@pytest.mark.parametrize("fast", [False, True], ids=["full", "tss"])
@pytest.mark.parametrize("H,W,bs,sr", SHAPES)
def test_fields_equal_the_rule(K, H, W, bs, sr, fast):
    a, b = _pair(H, W)
    whole = K.block_matching(a, b, bs, sr, fast)
    assert np.array_equal(K.block_matching(a, b, bs, sr, fast, subpel=1), whole)
    assert whole.shape == (H // bs, W // bs, 2)
    for n in (2, 4):
        got = K.block_matching(a, b, bs, sr, fast, subpel=n)
        assert np.array_equal(got, R.block_matching(a, b, bs, sr, fast, n)), n
    if (H, W) == (16, 16):
        assert np.array_equal(got, whole)


def test_flat_pair_keeps_the_centre(K):
    """All SADs equal: no neighbour is strictly smaller, the integer winner stays."""
    f = np.full((64, 64, 3), 77, np.uint8)
    for fast in (False, True):
        whole = K.block_matching(f, f, 16, 8, fast)
        for n in (2, 4):
            assert np.array_equal(K.block_matching(f, f, 16, 8, fast, subpel=n), whole)


def test_whole_pel_through_the_new_entry_equals_the_old(L):
    from vcf_amd.device import DeviceBuffer
    a, b = _pair(61, 99)
    for fast in (0, 1):
        out = []
        for name, extra in (("vcf_ipp_block_match", ()), ("vcf_ipp_block_match_subpel", (1,))):
            dr, dc = DeviceBuffer.from_array(a), DeviceBuffer.from_array(b)
            mv = np.full((5, 8, 2), np.nan, np.float32)
            dm, dg = DeviceBuffer.from_array(mv), DeviceBuffer(2 * 61 * 99)
            try:
                L.call(name, dr.ptr, dc.ptr, 61, 99, 12, 7, fast, *extra, dm.ptr, dg.ptr, None)
                out.append(dm.download(mv).copy())
            finally:
                for x in (dr, dc, dm, dg):
                    x.free()
        assert np.array_equal(out[0], out[1]) and not np.isnan(out[0]).any()


def test_bad_arguments_are_refused(L):
    from vcf_amd.device import DeviceBuffer
    d = DeviceBuffer(4 * 64 * 64 * 3)
    try:
        for bs, sr, n in ((16, 8, 3), (16, 8, 0), (16, 8, 8), (65, 8, 2), (16, 33, 2), (0, 8, 4)):
            with pytest.raises(L.VCFInvalidArgument) as e:
                L.call("vcf_ipp_block_match_subpel", d.ptr, d.ptr, 64, 64, bs, sr, 0, n, d.ptr, d.ptr, None)
            assert e.value.status == L.VCF_ERR_INVALID
    finally:
        d.free()
    f = np.zeros((32, 32, 3), np.uint8)
    from vcf_amd import ipp
    with pytest.raises(ValueError):
        ipp.block_matching(f, f, 16, 4, False, subpel=3)
    with pytest.raises(ValueError):
        ipp.motion_compensate(f, np.zeros((2, 2, 2), np.float32), 16, subpel=3)


def _quarter_field(rng, shape):
    return (rng.integers(-160, 161, shape) / 4.0).astype(np.float32)


def test_compensator_on_random_quarter_pel_fields(K):
    rng = np.random.Generator(np.random.PCG64(3))
    f = rng.integers(0, 256, (48, 80, 3), dtype=np.uint8)
    mv = _quarter_field(rng, (3, 5, 2))                    # multiples of 0.25 in [-40, 40], many invalid
    assert np.array_equal(K.motion_compensate(f, mv, 16, subpel=4), R.motion_compensate(f, mv, 16))
    mv = _quarter_field(rng, (3, 5, 2)) / 16               # small vectors: most valid, every (fx, fy)
    want = R.motion_compensate(f, mv, 16)
    assert not np.array_equal(want, R.motion_compensate(f, np.zeros_like(mv), 16))
    assert np.array_equal(K.motion_compensate(f, mv, 16, subpel=4), want)
    whole = rng.integers(-40, 41, (3, 5, 2)).astype(np.float32)
    old = K.motion_compensate(f, whole, 16)
    assert np.array_equal(K.motion_compensate(f, whole, 16, subpel=4), old)
    assert np.array_equal(old, O.ipp_motion_compensate(f, whole, 16))


@pytest.mark.parametrize("H,W,bs", [(33, 35, 7), (37, 50, 12), (16, 16, 16), (10, 12, 16), (21, 43, 4)])
def test_compensator_odd_shapes(K, H, W, bs):
    """Rows that are no multiple of 4 bytes, blocks that split a 4-byte group, a border outside
    the full blocks, an empty field; fields within +-2.75 pixels, so many vectors are valid."""
    rng = np.random.Generator(np.random.PCG64(H * W))
    f = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    mv = (rng.integers(-11, 12, (H // bs, W // bs, 2)) / 4.0).astype(np.float32)
    assert np.array_equal(K.motion_compensate(f, mv, bs, subpel=4), R.motion_compensate(f, mv, bs))


def _guarded_call(L, name, ins, in_off, outs, out_off, args, reject=False):
    """One call on Guarded buffers at the given byte offsets -> the outputs' bytes; guards checked."""
    from vcf_amd.device import synchronize
    gi = [Guarded(a.nbytes, o, a) for a, o in zip(ins, in_off)]
    go = [Guarded(n + 64, o) for n, o in zip(outs, out_off)]
    what = f"{name} in+{in_off} out+{out_off}"
    if reject:
        with pytest.raises(L.VCFInvalidArgument) as e:
            L.call(name, *args([g.ptr for g in gi], [g.ptr for g in go]))
        assert e.value.status == L.VCF_ERR_INVALID, what
        synchronize()
        for g in gi + go:
            g.check_untouched(what)
        return None
    L.call(name, *args([g.ptr for g in gi], [g.ptr for g in go]))
    synchronize()
    got = []
    for g, n in zip(go, outs):
        got.append(g.download()[:n].copy())
        g.check_outside([(0, n)], what)
        g.check(what)
    for g in gi:
        g.check_untouched(what)
    return got


OFFSETS = [(0, 0), (1, 0), (0, 1), (3, 5), (4, 8), (2, 2)]


@pytest.mark.parametrize("H,W,bs,sr", [(40, 64, 8, 3), (33, 35, 7, 2)])
def test_pointers_and_extents_of_the_search(L, H, W, bs, sr):
    a, b = _pair(H, W)
    gray = np.stack([O.ipp_gray(a), O.ipp_gray(b)]).reshape(-1)
    for fast in (0, 1):
        want = R.block_matching(a, b, bs, sr, bool(fast), 4)
        args = lambda i, o: (i[0], i[1], H, W, bs, sr, fast, 4, o[0], o[1], NULL)   # noqa: E731
        for oi, oo in OFFSETS:
            mv, g = _guarded_call(L, "vcf_ipp_block_match_subpel", [a, b], [oi, oi + 1], [want.nbytes, gray.size],
                                  [4 * oo, oo], args)
            assert np.array_equal(mv.view(np.float32).reshape(want.shape), want), (oi, oo)
            assert np.array_equal(g, gray)
        _guarded_call(L, "vcf_ipp_block_match_subpel", [a, b], [0, 0], [want.nbytes, gray.size], [1, 0], args,
                      reject=True)


@pytest.mark.parametrize("H,W,bs", [(48, 80, 16), (33, 35, 7)])
def test_pointers_and_extents_of_the_compensator(L, H, W, bs):
    rng = np.random.Generator(np.random.PCG64(H))
    f = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    mv = (rng.integers(-11, 12, (H // bs, W // bs, 2)) / 4.0).astype(np.float32)
    want = R.motion_compensate(f, mv, bs).reshape(-1)
    args = lambda i, o: (i[0], i[1], H, W, bs, o[0], NULL)   # noqa: E731
    for oi, oo in OFFSETS:
        got, = _guarded_call(L, "vcf_ipp_motion_compensate_qpel", [f, mv], [oi, 4 * oo], [want.size], [oo], args)
        assert np.array_equal(got, want), (oi, oo)
    _guarded_call(L, "vcf_ipp_motion_compensate_qpel", [f, mv], [0, 1], [want.size], [0], args, reject=True)


# ---- the codecs -------------------------------------------------------------------------------

def _write_seq(d, frames):
    for i, f in enumerate(frames):
        Image.fromarray(f).save(os.path.join(d, f"in_{i:04d}.png"))
    return os.path.join(d, "in_%04d.png")


def _loop(frames, gop, bs, sr, fast, Q, subpel, lam=0.0):
    """The reference's temporal_filter restated (as tests/test_ipp_gpu.py::_ipp_loop) with the
    sub-pel search and compensator of subpel_ref, over the oracle's 2D-DCT round trip."""
    def rt(img):
        H, W = img.shape[:2]
        return O.decode_frame(O.encode_frame(img, Q), H, W, Q)
    recon, mvs = [], []
    for g0 in range(0, len(frames), gop):
        ref = rt(frames[g0])
        recon.append(ref)
        for p in range(1, min(gop, len(frames) - g0)):
            cur = frames[g0 + p]
            mv = R.block_matching(ref, cur, bs, sr, fast, subpel)
            comp = R.motion_compensate(ref, mv, bs)
            if lam > 0:
                modes = O.ipp_rdo_modes(cur, comp, bs, Q, lam)
                ref = O.ipp_rdo_reconstruct(comp, rt(O.ipp_rdo_residual(cur, comp, modes, bs)), modes, bs)
            else:
                ref = O.ipp_reconstruct(comp, rt(O.ipp_residual(cur, comp)))
            recon.append(ref)
            mvs.append(mv)
    return recon, mvs


@pytest.fixture(scope="module")
def seq():
    return R.subpel_sequence(64, 96, 5, seed=4)


@pytest.mark.parametrize("subpel,lam", [(2, 0.0), (4, 0.0), (4, 0.5)], ids=["half", "quarter", "quarter-R"])
def test_ipp_dct_encode_decode_matches_the_loop(tmp_path, seq, subpel, lam):
    import json
    from vcf_amd.codec import parser as P
    from vcf_amd.codec.ipp import CoDec
    pat = _write_seq(str(tmp_path), seq)
    enc, dec = str(tmp_path / "enc" / "v"), str(tmp_path / "dec" / "v")
    flags = ["-N", "5", "-G", "3", "-M", "16", "-S", "4", "--subpel", str(subpel)] + (["-R", str(lam)] if lam else [])
    CoDec(P.parse(P.ipp_parser(), ["encode", "-i", pat, "-O", enc] + flags)).encode()
    assert json.load(open(enc + "_meta.json"))["subpel"] == subpel
    want, want_mv = _loop(seq, 3, 16, 4, False, 32, subpel, lam)
    with np.load(enc + "_mv.npz", allow_pickle=False) as z:
        assert np.array_equal(z["mv_f32"], np.stack(want_mv))
        assert (z["mv_f32"] != np.rint(z["mv_f32"])).any()
    assert CoDec(P.parse(P.ipp_parser(), ["decode", "-i", enc, "-O", dec, "-M", "16"])).decode() == 5
    for i in range(5):
        got = np.asarray(Image.open(f"{dec}_{i:04d}.png").convert("RGB"))
        assert np.array_equal(got, want[i]), f"frame {i}"


def test_host_loop_equals_resident_loop(tmp_path, seq):
    """_IPP._gop (what --st 2D-DWT and subclasses run) and CoDec._gop_resident write the same files."""
    from vcf_amd.codec import parser as P
    from vcf_amd.codec.ipp import CoDec, _IPP

    class Host(CoDec):
        def _gop(self, frames, g0, i_idx, p0):
            return _IPP._gop(self, frames, g0, i_idx, p0)

    pat = _write_seq(str(tmp_path), seq)
    flags = ["-N", "5", "-G", "3", "-M", "16", "-S", "4", "--subpel", "4"]
    for cls, name in ((CoDec, "a"), (Host, "b")):
        os.makedirs(tmp_path / name)
        cls(P.parse(P.ipp_parser(), ["encode", "-i", pat, "-O", str(tmp_path / name / "v")] + flags)).encode()
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b")) and "v_P_2_enc.tif" in names
    match, mismatch, errors = filecmp.cmpfiles(tmp_path / "a", tmp_path / "b", names, shallow=False)
    assert not mismatch and not errors


def test_no_flag_is_whole_pel_byte_for_byte(tmp_path, seq):
    from vcf_amd.codec import parser as P
    from vcf_amd.codec.ipp import CoDec
    pat = _write_seq(str(tmp_path), seq)
    for name, extra in (("a", []), ("b", ["--subpel", "1"])):
        os.makedirs(tmp_path / name)
        CoDec(P.parse(P.ipp_parser(), ["encode", "-i", pat, "-O", str(tmp_path / name / "v"), "-N", "5", "-G", "3",
                                       "-S", "4"] + extra)).encode()
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    match, mismatch, errors = filecmp.cmpfiles(tmp_path / "a", tmp_path / "b", names, shallow=False)
    assert not mismatch and not errors and "v_meta.json" in match and "v_mv.npz" in match


def test_ipp_over_2d_dwt_takes_the_flag(tmp_path, seq):
    from vcf_amd.codec import parser as P
    from vcf_amd.codec.ipp import codec_class
    pat = _write_seq(str(tmp_path), seq)
    enc, dec = str(tmp_path / "enc" / "v"), str(tmp_path / "dec" / "v")
    p, cls = P.ipp_parser(space_transform="2D-DWT"), codec_class("2D-DWT")
    chain = ["--st", "2D-DWT", "-l", "3", "-w", "bior4.4", "-q", "16"]
    cls(P.parse(p, ["encode", "-i", pat, "-O", enc, "-N", "5", "-G", "3", "-M", "16", "-S", "4", "--subpel", "4"]
                + chain)).encode()
    assert cls(P.parse(p, ["decode", "-i", enc, "-O", dec, "-M", "16"] + chain)).decode() == 5

    def rt(img):
        H, W = img.shape[:2]
        return O.dwt_decode_frame(O.dwt_encode_frame(img, "bior4.4", 3, 16), H, W, "bior4.4", 3, 16)
    want = []
    for g0 in range(0, 5, 3):
        ref = rt(seq[g0])
        want.append(ref)
        for q in range(1, min(3, 5 - g0)):
            comp = R.motion_compensate(ref, R.block_matching(ref, seq[g0 + q], 16, 4, False, 4), 16)
            ref = O.ipp_reconstruct(comp, rt(O.ipp_residual(seq[g0 + q], comp)))
            want.append(ref)
    for i in range(5):
        got = np.asarray(Image.open(f"{dec}_{i:04d}.png").convert("RGB"))
        assert np.array_equal(got, want[i]), f"frame {i}"


def test_device_ipp_files_equal_codec_files(tmp_path):
    """DeviceIPP(subpel=2): every gathered TIFF equals the file CoDec --subpel 2 writes, and the fields agree."""
    from vcf_amd.codec import parser as P
    from vcf_amd.codec.ipp import CoDec
    from vcf_amd.codec.ipp_device import DeviceIPP
    from vcf_amd.device import DeviceBuffer
    n, gop, H, W = 7, 3, 72, 96
    frames = R.subpel_sequence(H, W, n, seed=6)
    pat = _write_seq(str(tmp_path), frames)
    enc = str(tmp_path / "enc" / "v")
    CoDec(P.parse(P.ipp_parser(), ["encode", "-i", pat, "-O", enc, "-N", str(n), "-G", str(gop), "-M", "16", "-S", "8",
                                   "--subpel", "2"])).encode()
    job = DeviceIPP(None, 0, 1, n, H, W, 32, gop, 16, 8, False, subpel=2)
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
        assert np.array_equal(z["mv_f32"], np.stack(_loop(frames, gop, 16, 8, False, 32, 2)[1]))

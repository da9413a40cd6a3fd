"""B-frames on the GPU (vcf_amd/csrc/vcf_ipp_bipred.hip) against the numpy
restatement of the rule (tests/bipred_ref.py): both kernels bit for bit,
pointer alignment and written extents, the Python wrappers, and --bframes
through the IPP codecs end to end."""
import ctypes
import filecmp
import json
import os

import numpy as np
import pytest
from PIL import Image

import bipred_ref as B
import subpel_ref as R
from abi_buffers import Guarded
from oracle import oracle as O

pytestmark = pytest.mark.gpu

NULL = ctypes.c_void_p(0)
SHAPES = [(64, 96, 16),      # the plain case
          (33, 35, 7),       # rows that are no multiple of 4 bytes, a border outside the blocks
          (40, 64, 4),       # small blocks
          (61, 99, 12),      # rows that start off a 4-byte boundary (297-byte pitch): the byte path
          (64, 64, 64),      # the largest block
          (16, 16, 16),      # a single block
          (10, 12, 16),      # an empty field
          # the paths of the kernels' own mapping that the shapes above do not reach
          (21, 256, 7),      # word path, 21-byte block rows: words that straddle two blocks; 2 strips, their edge at byte 504
          (20, 200, 5),      # word path, 2 strips with their edge at byte 495: a word shared by two workgroups, stored by bytes
          (20, 257, 10),     # byte path with 3 strips
          (80, 120, 40)]     # the instantiation that holds 8 rows (5 here), one block per strip, 3 strips
OFFSETS = [(0, 0), (1, 0), (0, 1), (3, 5), (4, 8), (2, 2)]
GUARDED_SHAPES = [(40, 64, 8), (33, 35, 7), (21, 256, 7), (20, 200, 5), (20, 257, 10), (80, 120, 40)]


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


def _random(H, W, seed=0):
    rng = np.random.Generator(np.random.PCG64(1000 * H + W + seed))
    return [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(4)]


def _built(H, W, bs):
    """cur, cf, cb, rec in which every mode wins somewhere and exact ties occur: block columns cycle
    through cf exact (0), cb exact (1), cur between the two (2), cf == cb (a three-way tie -> 0) and
    cb as far from cur as cf on the other side (0 and 1 tie, the average exact -> 2)."""
    rng = np.random.Generator(np.random.PCG64(H * W + bs))
    cur = rng.integers(40, 216, (H, W, 3), dtype=np.uint8)
    cf, cb = cur.copy(), cur.copy()
    noise = rng.integers(1, 30, (H, W, 3), dtype=np.uint8)
    kind = ((np.arange(W) // bs)[None, :] + (np.arange(H) // bs)[:, None]) % 5
    k = kind[..., None]
    cf = np.where(k == 1, cur + noise, cf)
    cb = np.where(k == 0, cur - noise, cb)
    cf = np.where(k == 2, cur - noise, cf)
    cb = np.where(k == 2, cur + noise, cb)
    cf = np.where(k == 3, cur + 9, cf)
    cb = np.where(k == 3, cur + 9, cb)
    cf = np.where(k == 4, cur - 2 * (noise // 2), cf)
    cb = np.where(k == 4, cur + 2 * (noise // 2), cb)
    rec = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    return [a.astype(np.uint8) for a in (cur, cf, cb, rec)]


def _flat(H, W):
    f = np.full((H, W, 3), 77, np.uint8)
    return [f, f.copy(), f.copy(), np.full((H, W, 3), 128, np.uint8)]


@pytest.mark.parametrize("H,W,bs", SHAPES)
def test_both_kernels_equal_the_rule(K, H, W, bs):
    seen = set()
    for name, (cur, cf, cb, rec) in (("random", _random(H, W)), ("built", _built(H, W, bs)), ("flat", _flat(H, W)),
                                     ("cf == cb", [_random(H, W, 1)[i] for i in (0, 1, 1, 3)])):
        want_m, want_r = B.bipred_residual(cur, cf, cb, bs)
        got_m, got_r = K.bipred_residual(cur, cf, cb, bs)
        assert got_m.shape == (H // bs, W // bs) and got_m.dtype == np.uint8
        assert np.array_equal(got_m, want_m), name
        assert np.array_equal(got_r, want_r), name
        if name in ("flat", "cf == cb"):
            assert not want_m.any()           # exact ties go to mode 0
        if name == "built":
            seen |= set(want_m.reshape(-1).tolist())
        for modes in (want_m, (want_m + 1) % 3):
            assert np.array_equal(K.bipred_reconstruct(cf, cb, modes, rec, bs), B.bipred_reconstruct(cf, cb, modes, rec, bs)), name
    if (H // bs) * (W // bs) >= 5:
        assert seen == {0, 1, 2}
    if (H, W) == (10, 12):
        assert got_m.size == 0 and np.array_equal(got_r, np.clip(cur.astype(int) + 128, 0, 255))


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


@pytest.mark.parametrize("H,W,bs", GUARDED_SHAPES)
def test_pointers_and_extents(L, H, W, bs):
    """Every input at the first offset of a pair and every output at the second: (0, 0) and (4, 8) take
    the word kernels where the row pitch allows, the others the byte kernels; then once with every
    pointer at another offset."""
    cur, cf, cb, rec = _built(H, W, bs)
    want_m, want_r = B.bipred_residual(cur, cf, cb, bs)
    modes = (want_m + 1) % 3
    want_o = B.bipred_reconstruct(cf, cb, modes, rec, bs)
    enc = lambda i, o, b=bs, h=H: (i[0], i[1], i[2], h, W, b, o[0], o[1], NULL)            # noqa: E731
    dec = lambda i, o, b=bs, h=H: (i[0], i[1], i[2], i[3], h, W, b, o[0], NULL)            # noqa: E731
    cases = [([oi] * 4, [oo, oo]) for oi, oo in OFFSETS] + [([0, 1, 2, 3], [5, 2])]
    for oi, oo in cases:
        m, r = _guarded_call(L, "vcf_ipp_bipred_residual", [cur, cf, cb], oi[:3], [want_m.size, want_r.size], oo, enc)
        assert np.array_equal(m.reshape(want_m.shape), want_m) and np.array_equal(r, want_r.reshape(-1)), (oi, oo)
        o, = _guarded_call(L, "vcf_ipp_bipred_reconstruct", [cf, cb, modes, rec], oi, [want_o.size], oo[1:], dec)
        assert np.array_equal(o, want_o.reshape(-1)), (oi, oo)
    for b, h in ((0, H), (65, H), (-1, H), (bs, 65536)):
        _guarded_call(L, "vcf_ipp_bipred_residual", [cur, cf, cb], [0, 0, 0], [want_m.size, want_r.size], [0, 0],
                      lambda i, o: enc(i, o, b, h), reject=True)
        _guarded_call(L, "vcf_ipp_bipred_reconstruct", [cf, cb, modes, rec], [0, 0, 0, 0], [want_o.size], [0],
                      lambda i, o: dec(i, o, b, h), reject=True)


def test_a_mode_byte_above_two_behaves_as_zero_in_the_kernel(L):
    H, W, bs = 40, 64, 8
    cur, cf, cb, rec = _built(H, W, bs)
    modes = np.full((H // bs, W // bs), 200, np.uint8)
    modes[::2] = 3
    want = B.bipred_reconstruct(cf, cb, np.zeros_like(modes), rec, bs)
    o, = _guarded_call(L, "vcf_ipp_bipred_reconstruct", [cf, cb, modes, rec], [0, 0, 0, 0], [want.size], [0],
                       lambda i, o: (i[0], i[1], i[2], i[3], H, W, bs, o[0], NULL))
    assert np.array_equal(o, want.reshape(-1))


def test_wrappers_raise_before_any_device_work(K):
    f = np.zeros((32, 32, 3), np.uint8)
    m = np.zeros((2, 2), np.uint8)
    with pytest.raises(ValueError, match="mode 3"):
        K.bipred_reconstruct(f, f, np.array([[0, 1], [2, 3]], np.uint8), f, 16)
    for bad in (lambda: K.bipred_reconstruct(f, f, m[:1], f, 16), lambda: K.bipred_reconstruct(f, f, m.astype(np.int64), f, 16),
                lambda: K.bipred_reconstruct(f, f[:16], m, f, 16), lambda: K.bipred_residual(f, f, f[:, :16], 16),
                lambda: K.bipred_residual(f, f.astype(np.float32), f, 16), lambda: K.bipred_residual(f, f, f, 65)):
        with pytest.raises(ValueError):
            bad()
    assert K.bipred_reconstruct(f, f, m, f, 16).shape == f.shape


# ---- the codecs -------------------------------------------------------------------------------

def _write_seq(d, frames):
    for i, f in enumerate(frames):
        Image.fromarray(f).save(os.path.join(d, f"in_{i:04d}.png"))
    return os.path.join(d, "in_%04d.png")


@pytest.fixture(scope="module")
def seq():
    return R.subpel_sequence(64, 96, 7, seed=B.SEQ_SEED)


FLAGS = ["-N", "7", "-G", "5", "-M", "16", "-S", "4"]


@pytest.mark.parametrize("subpel", [1, 4])
@pytest.mark.parametrize("N", [1, 2])
def test_ipp_dct_encode_decode_matches_the_loop(tmp_path, seq, N, subpel):
    from vcf_amd.codec import parser as P
    from vcf_amd.codec.ipp import CoDec
    pat = _write_seq(str(tmp_path), seq)
    enc, dec = str(tmp_path / "enc" / "v"), str(tmp_path / "dec" / "v")
    CoDec(P.parse(P.ipp_parser(), ["encode", "-i", pat, "-O", enc, "--bframes", str(N), "--subpel", str(subpel)]
                  + FLAGS)).encode()
    want, want_mv, want_bmv, want_bmodes, want_types = B.loop(seq, 5, N, 16, 4, False, 32, subpel)
    meta = json.load(open(enc + "_meta.json"))
    assert meta["bframes"] == N and meta["frame_types"] == want_types and want_types.endswith("IP")
    assert meta["frame_types"][:5] == B.gop_types(5, N) and len(meta["B_info"]) == 2
    assert meta.get("subpel", 1) == subpel
    for n in range(2):
        assert os.path.exists(f"{enc}_B_{n}_enc.tif") and os.path.exists(f"{enc}_B_{n}_enc_shape.bin")
    assert not os.path.exists(f"{enc}_B_2_enc.tif") and meta["total_bits"] > sum(b["bits"] for b in meta["B_info"]) > 0
    with np.load(enc + "_mv.npz", allow_pickle=False) as z:
        assert np.array_equal(z["mv_f32"], np.stack(want_mv))
        assert np.array_equal(z["bmv_f32"], want_bmv)
        assert np.array_equal(z["bmodes_u8"], want_bmodes)
        assert set(z["bmodes_u8"].reshape(-1).tolist()) == {0, 1, 2}
    assert CoDec(P.parse(P.ipp_parser(), ["decode", "-i", enc, "-O", dec, "-M", "16"])).decode() == 7
    for i in range(7):
        got = np.asarray(Image.open(f"{dec}_{i:04d}.png").convert("RGB"))
        assert np.array_equal(got, want[i]), f"frame {i} ({want_types[i]})"


def _same_directories(a, b, must_have):
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b)) and must_have in names
    match, mismatch, errors = filecmp.cmpfiles(a, b, names, shallow=False)
    assert not mismatch and not errors
    return match


def test_host_loop_equals_resident_loop(tmp_path, seq):
    """_IPP._gop (what --st 2D-DWT and subclasses run) and CoDec._gop_resident write the same files."""
    from vcf_amd.codec import parser as P
    from vcf_amd.codec.ipp import CoDec, _IPP

    class Host(CoDec):
        def _gop(self, frames, g0, i_idx, p0):
            return _IPP._gop(self, frames, g0, i_idx, p0)

    pat = _write_seq(str(tmp_path), seq)
    for cls, name in ((CoDec, "a"), (Host, "b")):
        os.makedirs(tmp_path / name)
        cls(P.parse(P.ipp_parser(), ["encode", "-i", pat, "-O", str(tmp_path / name / "v"), "--bframes", "2", "--subpel",
                                     "4"] + FLAGS)).encode()
    match = _same_directories(tmp_path / "a", tmp_path / "b", "v_B_1_enc.tif")
    assert "v_mv.npz" in match and "v_meta.json" in match and "v_P_2_enc.tif" in match


def test_bframes_zero_is_no_flag_byte_for_byte(tmp_path, seq):
    from vcf_amd.codec import parser as P
    from vcf_amd.codec.ipp import CoDec
    pat = _write_seq(str(tmp_path), seq)
    for name, extra in (("a", []), ("b", ["--bframes", "0"])):
        os.makedirs(tmp_path / name)
        CoDec(P.parse(P.ipp_parser(), ["encode", "-i", pat, "-O", str(tmp_path / name / "v")] + FLAGS + extra)).encode()
    match = _same_directories(tmp_path / "a", tmp_path / "b", "v_P_4_enc.tif")
    assert "v_meta.json" in match and "v_mv.npz" in match
    assert not [n for n in os.listdir(tmp_path / "a") if "_B_" in n]
    assert not {"bframes", "frame_types", "B_info"} & set(json.load(open(tmp_path / "a" / "v_meta.json")))
    # a stream without the flag decodes as before: the plain IPP loop
    dec = str(tmp_path / "dec" / "v")
    assert CoDec(P.parse(P.ipp_parser(), ["decode", "-i", str(tmp_path / "a" / "v"), "-O", dec, "-M", "16"])).decode() == 7
    want = B.loop(seq, 5, 0, 16, 4, False, 32, 1)[0]
    for i in range(7):
        assert np.array_equal(np.asarray(Image.open(f"{dec}_{i:04d}.png").convert("RGB")), want[i]), f"frame {i}"


def test_ipp_over_2d_dwt_round_trips(tmp_path, seq):
    from vcf_amd.codec import parser as P
    from vcf_amd.codec.ipp import codec_class
    pat = _write_seq(str(tmp_path), seq)
    enc, dec = str(tmp_path / "enc" / "v"), str(tmp_path / "dec" / "v")
    p, cls = P.ipp_parser(space_transform="2D-DWT"), codec_class("2D-DWT")
    chain = ["--st", "2D-DWT", "-l", "3", "-w", "bior4.4", "-q", "16"]
    cls(P.parse(p, ["encode", "-i", pat, "-O", enc, "--bframes", "1"] + FLAGS + chain)).encode()
    assert cls(P.parse(p, ["decode", "-i", enc, "-O", dec, "-M", "16"] + chain)).decode() == 7

    def rt(img):
        H, W = img.shape[:2]
        return O.dwt_decode_frame(O.dwt_encode_frame(img, "bior4.4", 3, 16), H, W, "bior4.4", 3, 16)
    want, _, want_bmv, want_bmodes, types = B.loop(seq, 5, 1, 16, 4, False, 16, 1, rt=rt)
    assert json.load(open(enc + "_meta.json"))["frame_types"] == types == "IBPBPIP"
    with np.load(enc + "_mv.npz", allow_pickle=False) as z:
        assert np.array_equal(z["bmv_f32"], want_bmv) and np.array_equal(z["bmodes_u8"], want_bmodes)
    for i in range(7):
        got = np.asarray(Image.open(f"{dec}_{i:04d}.png").convert("RGB"))
        assert np.array_equal(got, want[i]), f"frame {i}"

"""Hierarchical motion search on the GPU (vcf_amd/csrc/vcf_ipp_hier.hip) against
the numpy restatement of the rule (tests/hier_ref.py): the fields bit for bit
over every level count, block path and plane parity, the level-0 identity with
the plain entries, pointer alignment and written extents, a caller's stream,
and --me_levels through the IPP codecs end to end."""
import ctypes
import filecmp
import json
import os
import types

import numpy as np
import pytest
from PIL import Image

import bipred_ref as BR
import hier_ref as R
import subpel_ref as S
from abi_buffers import Guarded
from oracle import oracle as O

pytestmark = pytest.mark.gpu

NULL = ctypes.c_void_p(0)
#          H    W   bs  sr  levels
SHAPES = [(16, 16, 16, 3, (1, 2, 3)),      # one block: the centre is the only valid candidate everywhere
          (32, 48, 16, 3, (1, 2, 3)),
          (37, 53, 8, 3, (1, 2)),          # odd planes at every level
          (48, 60, 12, 2, (1, 2)),         # b_l = 6 and 3: the byte paths, under a word level
          (128, 192, 64, 2, (3,)),
          (40, 24, 8, 4, (1, 2)),
          (10, 100, 16, 3, (1, 2, 3))]     # an empty field


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


def _pair(H, W, shift=(3, -2)):
    """Two frames of the generator per frame size and shift, made once."""
    if (H, W, shift) not in _pairs:
        _pairs[H, W, shift] = R.fast_sequence(2, H, W, shift, seed=H + W)
    return _pairs[H, W, shift]


@pytest.mark.parametrize("H,W,bs,sr,levels", SHAPES)
def test_fields_equal_the_rule(K, H, W, bs, sr, levels):
    a, b = _pair(H, W)
    for lv in levels:
        for n in (1, 4):
            got = K.block_matching(a, b, bs, sr, levels=lv, subpel=n)
            want = R.block_matching(a, b, bs, sr, lv, n)
            assert got.shape == want.shape == (H // bs, W // bs, 2)
            assert np.array_equal(got, want), (lv, n)


@pytest.mark.parametrize("sr", [1, 8, 32])
def test_search_ranges(K, sr):
    a, b = _pair(64, 96, (7, 5))
    for lv, n in ((2, 1), (1, 4)):
        assert np.array_equal(K.block_matching(a, b, 16, sr, levels=lv, subpel=n), R.block_matching(a, b, 16, sr, lv, n))


def test_flat_pair_tied_pair_and_fast_pair(K):
    f = np.full((64, 64, 3), 77, np.uint8)
    got = K.block_matching(f, f, 16, 2, levels=2)
    assert np.array_equal(got, R.block_matching(f, f, 16, 2, 2))
    assert np.array_equal(got, 4 * K.block_matching(f[:16, :16], f[:16, :16], 4, 2))   # the centre at every level
    # constant rows: every dx ties at every level of the pyramid, so scan order and centre decide
    rng = np.random.Generator(np.random.PCG64(8))
    rows = rng.integers(0, 256, (80, 1, 1), dtype=np.uint8)
    a = np.ascontiguousarray(np.broadcast_to(rows, (80, 64, 3))[8:72])
    b = np.ascontiguousarray(np.broadcast_to(rows, (80, 64, 3))[3:67])    # a's rows 5 further down
    for lv in (1, 2, 3):
        want = R.block_matching(a, b, 16, 2, lv)
        assert np.array_equal(K.block_matching(a, b, 16, 2, levels=lv), want), lv
        assert len({tuple(v) for v in want.reshape(-1, 2)}) > 1
    a, b = _pair(96, 128, (19, -13))
    got = K.block_matching(a, b, 16, 8, levels=2)
    assert np.array_equal(got, R.block_matching(a, b, 16, 8, 2))
    assert (got == (19, -13)).all(axis=2).sum() >= 27                     # tests/test_hier.py: 90 % of 30 blocks


def test_level_zero_through_the_new_entry_equals_the_old(L):
    from vcf_amd.device import DeviceBuffer
    a, b = _pair(61, 99)
    for subpel in (1, 4):
        out = []
        for name in ("old", "new"):
            dr, dc = DeviceBuffer.from_array(a), DeviceBuffer.from_array(b)
            mv = np.full((5, 8, 2), np.nan, np.float32)
            dm, dg = DeviceBuffer.from_array(mv), DeviceBuffer(2 * 61 * 99)
            try:
                if name == "new":
                    L.call("vcf_ipp_block_match_hier", dr.ptr, dc.ptr, 61, 99, 12, 7, 0, subpel, dm.ptr, dg.ptr,
                           2 * 61 * 99, None)
                elif subpel == 1:
                    L.call("vcf_ipp_block_match", dr.ptr, dc.ptr, 61, 99, 12, 7, 0, dm.ptr, dg.ptr, None)
                else:
                    L.call("vcf_ipp_block_match_subpel", dr.ptr, dc.ptr, 61, 99, 12, 7, 0, subpel, dm.ptr, dg.ptr, None)
                out.append(dm.download(mv).copy())
            finally:
                for x in (dr, dc, dm, dg):
                    x.free()
        assert np.array_equal(out[0], out[1]) and not np.isnan(out[0]).any()


def _guarded_call(L, ins, in_off, outs, out_off, args, reject=False):
    """One call on Guarded buffers at the given byte offsets -> the outputs' bytes; guards checked."""
    from vcf_amd.device import synchronize
    name = "vcf_ipp_block_match_hier"
    gi = [Guarded(a.nbytes, o, a) for a, o in zip(ins, in_off)]
    go = [Guarded(n + 64, o) for n, o in zip(outs, out_off)]
    what = f"{name} in+{in_off} out+{out_off}"
    try:
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
    finally:
        for g in gi + go:
            g.buf.free()


@pytest.mark.parametrize("H,W,bs,sr,lv", [(40, 64, 8, 3, 2), (37, 53, 8, 2, 1)])
def test_pointers_and_extents(L, K, H, W, bs, sr, lv):
    a, b = _pair(H, W)
    want, ws = R.block_matching(a, b, bs, sr, lv, 4), R.workspace(a, b, lv)
    assert ws.size == K.hier_workspace_bytes(H, W, lv)
    args = lambda i, o: (i[0], i[1], H, W, bs, sr, lv, 4, o[0], o[1], ws.size, NULL)   # noqa: E731
    for oi, oo in ((0, 0), (1, 0), (0, 1), (3, 3), (1, 3), (3, 1)):
        mv, g = _guarded_call(L, [a, b], [oi, (oi + 2) % 4], [want.nbytes, ws.size], [4 * oo, oo], args)
        assert np.array_equal(mv.view(np.float32).reshape(want.shape), want), (oi, oo)
        assert np.array_equal(g, ws), (oi, oo)
    _guarded_call(L, [a, b], [0, 0], [want.nbytes, ws.size], [1, 0], args, reject=True)       # mv_dev off by one
    short = lambda i, o: (i[0], i[1], H, W, bs, sr, lv, 4, o[0], o[1], ws.size - 1, NULL)     # noqa: E731
    _guarded_call(L, [a, b], [0, 0], [want.nbytes, ws.size], [0, 0], short, reject=True)


def test_bad_arguments_are_refused(L):
    from vcf_amd.device import DeviceBuffer
    d = DeviceBuffer(4 * 64 * 64 * 3)
    big = d.nbytes
    try:
        for bs, sr, lv, n in ((16, 8, 4, 1), (16, 8, -1, 1), (12, 8, 3, 1), (4, 8, 2, 1), (2, 8, 1, 1), (65, 8, 0, 1),
                              (0, 8, 0, 1), (16, 33, 1, 1), (16, -1, 2, 1), (16, 8, 1, 3), (16, 8, 2, 0)):
            with pytest.raises(L.VCFInvalidArgument) as e:
                L.call("vcf_ipp_block_match_hier", d.ptr, d.ptr, 64, 64, bs, sr, lv, n, d.ptr, d.ptr, big, None)
            assert e.value.status == L.VCF_ERR_INVALID
        for H, W in ((0, 64), (64, -3)):
            with pytest.raises(L.VCFInvalidArgument):
                L.call("vcf_ipp_block_match_hier", d.ptr, d.ptr, H, W, 16, 8, 1, 1, d.ptr, d.ptr, big, None)
        for k in range(4):
            p = [d.ptr] * 4
            p[k] = NULL
            with pytest.raises(L.VCFInvalidArgument):
                L.call("vcf_ipp_block_match_hier", p[0], p[1], 64, 64, 16, 8, 1, 1, p[2], p[3], big, None)
    finally:
        d.free()


def test_on_the_callers_stream_behind_a_memset(L):
    """The frames reach the inputs on the caller's stream behind a long memset: an entry that ran
    ahead of that stream would search the zeros the inputs held before."""
    from vcf_amd.device import DeviceBuffer, Stream, synchronize
    H, W, bs, sr, lv = 64, 96, 16, 4, 2
    a, b = _pair(H, W, (7, 5))
    want = R.block_matching(a, b, bs, sr, lv, 4)
    assert want.any()
    st, big = Stream(), DeviceBuffer(256 << 20)
    src = [DeviceBuffer.from_array(x) for x in (a, b)]
    din = [DeviceBuffer(a.nbytes) for _ in range(2)]
    nws = R.workspace(a, b, lv).size
    dm, snap, dg = DeviceBuffer(want.nbytes), DeviceBuffer(want.nbytes), DeviceBuffer(nws)
    try:
        for x in din:
            x.fill(0)
        dm.fill(0xEE)
        synchronize()
        for _ in range(4):
            big.fill(1, st)
        for x, y in zip(din, src):
            L.call("vcf_memcpy_dtod", x.ptr, y.ptr, a.nbytes, st.handle)
        L.call("vcf_ipp_block_match_hier", din[0].ptr, din[1].ptr, H, W, bs, sr, lv, 4, dm.ptr, dg.ptr, nws, st.handle)
        L.call("vcf_memcpy_dtod", snap.ptr, dm.ptr, want.nbytes, st.handle)
        L.call("vcf_memset", dm.ptr, 0xEE, want.nbytes, st.handle)
        st.synchronize()
        assert np.array_equal(snap.download(np.empty_like(want)), want)
    finally:
        for x in src + din + [dm, snap, dg, big]:
            x.free()
        st.close()


# ---- the codecs -------------------------------------------------------------------------------

N, GOP, BS, SR, LV = 6, 3, 16, 4, 2
FLAGS = ["-N", str(N), "-G", str(GOP), "-M", str(BS), "-S", str(SR)]


@pytest.fixture(scope="module")
def seq():
    return R.fast_sequence(N, 64, 96, (9, -6), seed=4)


def _write_seq(d, frames):
    for i, f in enumerate(frames):
        Image.fromarray(f).save(os.path.join(d, f"in_{i:04d}.png"))
    return os.path.join(d, "in_%04d.png")


def _search(levels):
    return lambda r, c, bs, sr, fast, subpel=1: R.block_matching(r, c, bs, sr, levels, subpel)


def _loop(frames, levels, subpel=1, lam=0.0, rt=None, Q=32):
    """The reference's temporal_filter restated (tests/test_subpel_gpu.py::_loop) over hier_ref's search."""
    rt = rt or BR.dct_round_trip(Q)
    recon, mvs = [], []
    for g0 in range(0, len(frames), GOP):
        ref = rt(frames[g0])
        recon.append(ref)
        for p in range(1, min(GOP, len(frames) - g0)):
            cur = frames[g0 + p]
            mv = R.block_matching(ref, cur, BS, SR, levels, subpel)
            comp = S.motion_compensate(ref, mv, BS)
            if lam > 0:
                modes = O.ipp_rdo_modes(cur, comp, BS, Q, lam)
                ref = O.ipp_rdo_reconstruct(comp, rt(O.ipp_rdo_residual(cur, comp, modes, BS)), modes, BS)
            else:
                ref = O.ipp_reconstruct(comp, rt(O.ipp_residual(cur, comp)))
            recon.append(ref)
            mvs.append(mv)
    return recon, mvs


def _same_files(a, b):
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b))
    match, mismatch, errors = filecmp.cmpfiles(a, b, names, shallow=False)
    assert not mismatch and not errors, (mismatch, errors)
    return names


def _decoded(dec, n):
    return [np.asarray(Image.open(f"{dec}_{i:04d}.png").convert("RGB")) for i in range(n)]


@pytest.mark.parametrize("extra", [[], ["--subpel", "4"], ["-R", "0.5"], ["--bframes", "2"],
                                   ["--bframes", "2", "--subpel", "4"]],
                         ids=["plain", "subpel4", "rdo", "bframes2", "bframes2-subpel4"])
def test_ipp_dct_host_loop_resident_loop_restated_loop_and_decoder(tmp_path, seq, monkeypatch, extra):
    from vcf_amd.codec import parser as P
    from vcf_amd.codec.ipp import CoDec, _IPP

    class Host(CoDec):
        def _gop(self, frames, g0, i_idx, p0):
            return _IPP._gop(self, frames, g0, i_idx, p0)

    pat = _write_seq(str(tmp_path), seq)
    for cls, name in ((CoDec, "a"), (Host, "b")):
        os.makedirs(tmp_path / name)
        cls(P.parse(P.ipp_parser(), ["encode", "-i", pat, "-O", str(tmp_path / name / "v"), "--me_levels", str(LV)]
                    + FLAGS + extra)).encode()
    assert "v_P_1_enc.tif" in _same_files(tmp_path / "a", tmp_path / "b")
    enc, dec = str(tmp_path / "a" / "v"), str(tmp_path / "dec" / "v")
    subpel = 4 if "--subpel" in extra else 1
    meta = json.load(open(enc + "_meta.json"))
    assert "me_levels" not in meta and not any("level" in k for k in meta)
    with np.load(enc + "_mv.npz", allow_pickle=False) as z:
        if "--bframes" in extra:
            monkeypatch.setattr(BR, "R", types.SimpleNamespace(block_matching=_search(LV),
                                                               motion_compensate=S.motion_compensate))
            want, want_mv, want_bmv, want_bmodes, _ = BR.loop(seq, GOP, 2, BS, SR, False, 32, subpel)
            assert np.array_equal(z["bmv_f32"], want_bmv) and np.array_equal(z["bmodes_u8"], want_bmodes)
        else:
            want, want_mv = _loop(seq, LV, subpel, 0.5 if "-R" in extra else 0.0)
        assert np.array_equal(z["mv_f32"], np.stack(want_mv))
        assert np.abs(z["mv_f32"]).max() > SR                # beyond the plain window
    assert CoDec(P.parse(P.ipp_parser(), ["decode", "-i", enc, "-O", dec, "-M", str(BS)])).decode() == N
    for i, got in enumerate(_decoded(dec, N)):
        assert np.array_equal(got, want[i]), f"frame {i}"


def test_level_zero_is_no_flag_byte_for_byte(tmp_path, seq):
    from vcf_amd.codec import parser as P
    from vcf_amd.codec.ipp import CoDec
    pat = _write_seq(str(tmp_path), seq)
    for name, extra in (("a", []), ("b", ["--me_levels", "0"])):
        os.makedirs(tmp_path / name)
        CoDec(P.parse(P.ipp_parser(), ["encode", "-i", pat, "-O", str(tmp_path / name / "v"), "--subpel", "2"] + FLAGS
                      + extra)).encode()
    names = _same_files(tmp_path / "a", tmp_path / "b")
    assert "v_meta.json" in names and "v_mv.npz" in names


def test_ipp_over_2d_dwt_takes_the_flag(tmp_path, seq):
    from vcf_amd.codec import parser as P
    from vcf_amd.codec.ipp import codec_class
    pat = _write_seq(str(tmp_path), seq)
    enc, dec = str(tmp_path / "enc" / "v"), str(tmp_path / "dec" / "v")
    p, cls = P.ipp_parser(space_transform="2D-DWT"), codec_class("2D-DWT")
    chain = ["--st", "2D-DWT", "-l", "3", "-w", "bior4.4", "-q", "16"]
    cls(P.parse(p, ["encode", "-i", pat, "-O", enc, "--me_levels", str(LV)] + FLAGS + chain)).encode()
    assert cls(P.parse(p, ["decode", "-i", enc, "-O", dec, "-M", str(BS)] + chain)).decode() == N

    def rt(img):
        H, W = img.shape[:2]
        return O.dwt_decode_frame(O.dwt_encode_frame(img, "bior4.4", 3, 16), H, W, "bior4.4", 3, 16)
    want, want_mv = _loop(seq, LV, rt=rt)
    with np.load(enc + "_mv.npz", allow_pickle=False) as z:
        assert np.array_equal(z["mv_f32"], np.stack(want_mv))
    for i, got in enumerate(_decoded(dec, N)):
        assert np.array_equal(got, want[i]), f"frame {i}"


def test_device_ipp_files_equal_codec_files(tmp_path):
    """DeviceIPP(levels=2): every gathered TIFF equals the file CoDec --me_levels 2 writes, and the fields agree."""
    from vcf_amd.codec import parser as P
    from vcf_amd.codec.ipp import CoDec
    from vcf_amd.codec.ipp_device import DeviceIPP
    from vcf_amd.device import DeviceBuffer
    n, gop, H, W = 7, 3, 72, 96
    frames = R.fast_sequence(n, H, W, (9, -6), seed=6)
    pat = _write_seq(str(tmp_path), frames)
    enc = str(tmp_path / "enc" / "v")
    CoDec(P.parse(P.ipp_parser(), ["encode", "-i", pat, "-O", enc, "-N", str(n), "-G", str(gop), "-M", "16", "-S", "4",
                                   "--me_levels", "2", "--subpel", "2"])).encode()
    job = DeviceIPP(None, 0, 1, n, H, W, 32, gop, 16, 4, False, subpel=2, levels=2)
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
        assert np.abs(z["mv_f32"]).max() > 4

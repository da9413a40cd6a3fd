"""Overlapped block motion compensation (--obmc) on the CPU: the properties of
the numpy restatement of the rule (tests/obmc_ref.py), what it does to the
prediction error on the sub-pel test sequence, the parser flag, the refusals,
and the host loop of the IPP codec over numpy stand-ins for the tools: the
meta.json key, the decoder's reconstructions and its refusal.  The GPU kernel
is held to obmc_ref in tests/test_obmc_gpu.py, which also codes against loop()."""
import json
import types

import numpy as np
import pytest

import bipred_ref as B
import hier_ref as HR
import obmc_ref as OB
import subpel_ref as R
from oracle import oracle as O


def _frame(H, W, seed):
    return np.random.Generator(np.random.PCG64(seed)).integers(0, 256, (H, W, 3), dtype=np.uint8)


# ---- the rule ---------------------------------------------------------------------------------

@pytest.mark.parametrize("bs", OB.BLOCK_SIZES)
def test_uniform_valid_field_is_the_plain_compensator(bs):
    H, W = 3 * bs + 3, 4 * bs + 3
    f = _frame(H, W, bs)
    # valid for every block: the frame has 3 more rows and columns than the full blocks
    for v in ((0.0, 0.0), (0.75, 1.25), (2.0, 3.0), (2.75, 2.5)):
        mv = np.tile(np.float32(v), (3, 4, 1))
        assert (OB.quarter(mv, bs, H, W) == np.rint(4 * mv)).all()
        want = R.motion_compensate(f, mv, bs)
        assert np.array_equal(OB.motion_compensate(f, mv, bs), want), v
        assert v == (0.0, 0.0) or not np.array_equal(want, R.motion_compensate(f, 0 * mv, bs))


@pytest.mark.parametrize("bs", OB.BLOCK_SIZES)
def test_single_block_frame_is_the_plain_compensator(bs):
    f = _frame(bs + 3, bs + 2, 100 + bs)
    for v in ((0.5, 0.75), (1.0, 2.25), (5.0, 0.0), (np.nan, 0.0)):     # valid, valid, invalid, invalid
        mv = np.float32(v).reshape(1, 1, 2)
        assert np.array_equal(OB.motion_compensate(f, mv, bs), R.motion_compensate(f, np.nan_to_num(mv, nan=99.0), bs)), v


def test_shared_vectors_give_the_plain_sample_and_the_rest_differs():
    bs, n = 8, 8
    f = _frame(n * bs, n * bs, 7)
    rng = np.random.Generator(np.random.PCG64(8))
    mv = (rng.integers(-8, 9, (n, n, 2)) / 4.0).astype(np.float32)
    mv[[0, -1]] = mv[:, [0, -1]] = 0                         # the border blocks stay valid
    mv[2:6, 2:6] = (1.25, -0.75)
    got, plain = OB.motion_compensate(f, mv, bs), R.motion_compensate(f, mv, bs)
    lo, hi = 2 * bs + bs // 2, 6 * bs - bs // 2              # the pixels whose four contributors lie in blocks 2 .. 5
    assert np.array_equal(got[lo:hi, lo:hi], plain[lo:hi, lo:hi])
    diff = (got != plain).any(axis=2)
    diff[lo:hi, lo:hi] = False
    assert diff.mean() > 0.25
    # one pixel by hand: (y, x) = (20, 19) of block (2, 2), v = 4 (lower half: neighbour row 3), u = 3 (left half: column 1)
    y, x = 20, 19
    q = OB.quarter(mv, bs, n * bs, n * bs)
    wy, wx = 3 * bs - 2 * 4 - 1, bs + 2 * 3 + 1
    acc = 0
    for row, w_r in ((2, wy), (3, 2 * bs - wy)):
        for col, w_c in ((2, wx), (1, 2 * bs - wx)):
            qx, qy = q[row, col]
            acc = acc + w_r * w_c * OB.sample(f, np.int64(qx), np.int64(qy), np.int64(y), np.int64(x))
    assert np.array_equal(got[y, x], (acc + 2 * bs * bs) >> 8)


def test_border_outside_the_full_blocks_is_zero_and_an_empty_field_gives_zeros():
    f = _frame(21, 43, 3) | 1
    mv = (np.random.Generator(np.random.PCG64(4)).integers(-6, 7, (5, 10, 2)) / 4.0).astype(np.float32)
    out = OB.motion_compensate(f, mv, 4)
    assert not out[20:].any() and not out[:, 40:].any() and out[:20, :40].all()
    assert not OB.motion_compensate(_frame(10, 12, 5), np.zeros((0, 0, 2), np.float32), 16).any()
    assert not OB.motion_compensate(_frame(40, 12, 5), np.zeros((2, 0, 2), np.float32), 16).any()
    with pytest.raises(ValueError):
        OB.motion_compensate(f, mv, 12)


def test_quarter_resolves_nan_infinity_and_huge_entries():
    mv = np.zeros((2, 3, 2), np.float32)
    mv[0, 0], mv[0, 1], mv[0, 2], mv[1, 0], mv[1, 1] = (np.nan, 0), (np.inf, 0), (0, -np.inf), (1e30, 1e30), (0.625, -0.125)
    mv[1, 2] = (0.375, 0.875)
    q = OB.quarter(mv, 16, 40, 56)
    assert q[0].tolist() == [[0, 0]] * 3 and q[1, 0].tolist() == [0, 0]
    assert q[1, 1].tolist() == [2, 0]          # 2.5 -> 2 (half to even), -0.5 -> -0
    assert q[1, 2].tolist() == [2, 4]          # 1.5 -> 2, 3.5 -> 4


@pytest.mark.parametrize("subpel", [1, 4], ids=["whole", "quarter"])
def test_prediction_error_on_the_test_sequence(subpel):
    """-M 16 -S 4 on subpel_sequence(96, 128, 3, seed=0): the overlapped prediction's summed squared
    error is below the plain one's (measured: x 0.80 at both precisions)."""
    seq = R.subpel_sequence(96, 128, 3, seed=0)
    plain = over = 0
    for t in (1, 2):
        mv = R.block_matching(seq[t - 1], seq[t], 16, 4, False, subpel)
        cur = seq[t].astype(np.int64)
        plain += int(((cur - R.motion_compensate(seq[t - 1], mv, 16)) ** 2).sum())
        over += int(((cur - OB.motion_compensate(seq[t - 1], mv, 16)) ** 2).sum())
    print(f"subpel {subpel}: plain SSE {plain}, OBMC SSE {over}, ratio {over / plain:.3f}")
    assert over < plain


# ---- the flag ---------------------------------------------------------------------------------

def test_parser_flag():
    from vcf_amd.codec import parser as P
    assert P.parse(P.ipp_parser(), ["encode"]).obmc is False
    assert P.parse(P.ipp_parser(), ["encode", "--obmc"]).obmc is True
    assert not hasattr(P.parse(P.ipp_parser(), ["decode"]), "obmc")


def test_refusals_and_combinations(tmp_path):
    import vcf_amd.codec.ipp as M
    from vcf_amd.codec import parser as P
    base = ["encode", "-i", "x.npy", "-O", str(tmp_path / "v"), "--obmc"]
    with pytest.raises(ValueError, match="-M"):
        M.CoDec(P.parse(P.ipp_parser(), base + ["-M", "12"]))
    M.CoDec(P.parse(P.ipp_parser(), base[:-1] + ["-M", "12"]))          # without the flag -M 12 stays legal
    for extra in (["-R", "0.5"], ["--bframes", "2"], ["--me_levels", "1"], ["--subpel", "4"]):
        assert M.CoDec(P.parse(P.ipp_parser(), base + extra)).obmc is True
    for bs in (4, 8, 32, 64):
        M.CoDec(P.parse(P.ipp_parser(), base + ["-M", str(bs)]))


def test_wrapper_rejects_a_block_size_before_any_device_work():
    from vcf_amd import ipp as K
    f = np.zeros((48, 48, 3), np.uint8)
    for bs in (12, 2, 128, 0):
        with pytest.raises(ValueError):
            K.motion_compensate(f, np.zeros((48 // max(bs, 1), 48 // max(bs, 1), 2), np.float32), bs, obmc=True)
    assert K.mc_entry(1, True) == K.mc_entry(4, True) == "vcf_ipp_motion_compensate_obmc"
    assert K.mc_entry(1) == "vcf_ipp_motion_compensate" and K.mc_entry(2) == "vcf_ipp_motion_compensate_qpel"


def test_argument_errors_come_before_any_device_work():
    """The made-up addresses are never touched, so this runs without a GPU."""
    import ctypes
    from vcf_amd import _lib as L
    A = ctypes.c_void_p(4096)
    fn = L.lib().vcf_ipp_motion_compensate_obmc
    for bs in (0, 2, 12, 128, -16):
        assert fn(A, A, 64, 64, bs, A, None) == L.VCF_ERR_INVALID
    for H, W in ((0, 64), (64, 0), (-1, 64)):
        assert fn(A, A, H, W, 16, A, None) == L.VCF_ERR_INVALID
    for args in ((None, A, A), (A, None, A), (A, A, None), (A, ctypes.c_void_p(4098), A)):
        assert fn(args[0], args[1], 64, 64, 16, args[2], None) == L.VCF_ERR_INVALID
    assert fn(A, A, 65536, 64, 16, A, None) == L.VCF_ERR_UNSUPPORTED


# ---- the coding loop --------------------------------------------------------------------------

def loop(frames, gop, bs, sr, Q, subpel=1, bframes=0, lam=0.0, levels=0, obmc=True, rt=None):
    """The IPP coding loop in numpy over a spatial round trip rt (default: the oracle's 2D-DCT at
    Q) with the overlapped compensator of obmc_ref -> the decoded frames in display order."""
    rt = rt or B.dct_round_trip(Q)

    def search(ref, cur):
        return HR.block_matching(ref, cur, bs, sr, levels, subpel) if levels else \
            R.block_matching(ref, cur, bs, sr, False, subpel)

    def mc(ref, mv):
        return OB.motion_compensate(ref, mv, bs) if obmc else R.motion_compensate(ref, mv, bs)

    recon = {}
    for g0 in range(0, len(frames), gop):
        t = B.gop_types(min(gop, len(frames) - g0), bframes)
        recon[g0] = rt(frames[g0])
        anchors = [i for i, c in enumerate(t) if c != "B"]
        for a, c in zip(anchors, anchors[1:]):
            ra, cur = recon[g0 + a], frames[g0 + c]
            comp = mc(ra, search(ra, cur))
            if lam > 0:
                modes = O.ipp_rdo_modes(cur, comp, bs, Q, lam)
                rc = O.ipp_rdo_reconstruct(comp, rt(O.ipp_rdo_residual(cur, comp, modes, bs)), modes, bs)
            else:
                rc = O.ipp_reconstruct(comp, rt(O.ipp_residual(cur, comp)))
            recon[g0 + c] = rc
            for d in range(a + 1, c):
                cur = frames[g0 + d]
                cf, cb = mc(ra, search(ra, cur)), mc(rc, search(rc, cur))
                modes, res = B.bipred_residual(cur, cf, cb, bs)
                recon[g0 + d] = B.bipred_reconstruct(cf, cb, modes, rt(res), bs)
    return [recon[i] for i in sorted(recon)]


def _tools():
    """The IPP tools in numpy, with the keywords the codec passes only when their flag is set."""
    return types.SimpleNamespace(
        block_matching=lambda r, c, bs, sr, fast, subpel=1, levels=0:
            HR.block_matching(r, c, bs, sr, levels, subpel) if levels else R.block_matching(r, c, bs, sr, fast, subpel),
        motion_compensate=lambda f, mv, bs, subpel=1, obmc=False:
            OB.motion_compensate(f, mv, bs) if obmc else R.motion_compensate(f, mv, bs),
        residual=O.ipp_residual, reconstruct=O.ipp_reconstruct,
        rdo_modes=O.ipp_rdo_modes, rdo_residual=O.ipp_rdo_residual, rdo_reconstruct=O.ipp_rdo_reconstruct,
        bipred_residual=B.bipred_residual, bipred_reconstruct=B.bipred_reconstruct)


def _stand_in(M):
    """CoDec over the oracle's 2D-DCT round trip at Q = 32, the way tests/test_bframes.py builds its
    stand-in; the decoder's frame is kept beside the (unwritten) code-stream so that decode() runs too."""
    class StandIn(M.CoDec):
        encoder_recon = None

        def encode_decode_proxy(self, img, frame_type, seq_idx):
            H, W = img.shape[:2]
            rec = O.decode_frame(O.encode_frame(img, 32), H, W, 32)
            np.save(f"{self.prefix}_{frame_type}_{seq_idx}_enc.npy", rec)
            return rec, 100000 * "IPB".index(frame_type) + 1000 * seq_idx + int(rec.sum() % 7)

        def _decode_frame(self, base):
            return np.load(base + ".npy")

        def _gop(self, frames, g0, i_idx, p0):
            r = super()._gop(frames, g0, i_idx, p0)
            self.encoder_recon = (self.encoder_recon or []) + list(r[3])
            return r
    return StandIn


SEQ = dict(H=32, W=48, n=5, gop=3, seed=9)


def _encode(monkeypatch, tmp_path, name, extra, M_bs="16"):
    import vcf_amd.codec.ipp as M
    from vcf_amd.codec import parser as P
    monkeypatch.setattr(M, "K", _tools())
    src = tmp_path / "frames.npy"
    if not src.exists():
        np.save(src, np.stack(R.subpel_sequence(SEQ["H"], SEQ["W"], SEQ["n"], seed=SEQ["seed"])))
    prefix = str(tmp_path / name / "v")
    enc = _stand_in(M)(P.parse(P.ipp_parser(), ["encode", "-i", str(src), "-O", prefix, "-N", str(SEQ["n"]), "-G",
                                               str(SEQ["gop"]), "-S", "2", "-M", M_bs] + extra))
    enc.encode()
    return json.load(open(prefix + "_meta.json")), prefix, enc


def _decode(tmp_path, prefix, M_bs="16"):
    import vcf_amd.codec.ipp as M
    from vcf_amd.codec import parser as P
    dec = _stand_in(M)(P.parse(P.ipp_parser(), ["decode", "-i", prefix, "-O", str(tmp_path / "dec" / "v"), "-M", M_bs]))
    dec.decode()
    return dec.recon


def test_meta_key_only_with_the_flag(monkeypatch, tmp_path):
    plain, _, _ = _encode(monkeypatch, tmp_path, "a", [])
    with_flag, _, _ = _encode(monkeypatch, tmp_path, "b", ["--obmc"])
    assert "obmc" not in plain and with_flag["obmc"] is True
    assert set(with_flag) == set(plain) | {"obmc"}


@pytest.mark.parametrize("extra", [[], ["--subpel", "4"], ["--bframes", "1"], ["-R", "0.5"], ["--me_levels", "1"]],
                         ids=["alone", "subpel4", "bframes1", "R", "me_levels1"])
def test_decoder_reproduces_the_encoder(monkeypatch, tmp_path, extra):
    meta, prefix, enc = _encode(monkeypatch, tmp_path, "e", ["--obmc"] + extra)
    assert meta["obmc"] is True
    got = _decode(tmp_path, prefix)
    # the encoder reconstructs what it predicts from: every frame but the B-frames
    kept = [i for i, t in enumerate(meta.get("frame_types", "IPPIP")) if t != "B"]
    assert len(got) == SEQ["n"] and len(enc.encoder_recon) == len(kept)
    kw = dict(subpel=4 if "--subpel" in extra else 1, bframes=1 if "--bframes" in extra else 0,
              lam=0.5 if "-R" in extra else 0.0, levels=1 if "--me_levels" in extra else 0)
    frames = R.subpel_sequence(SEQ["H"], SEQ["W"], SEQ["n"], seed=SEQ["seed"])
    want = loop(frames, SEQ["gop"], 16, 2, 32, **kw)
    for k, i in enumerate(kept):
        assert np.array_equal(got[i], enc.encoder_recon[k]), i
    for i in range(SEQ["n"]):
        assert np.array_equal(got[i], want[i]), i
    if not extra:   # the flag changes the frames: the same stream coded without it differs
        assert any(not np.array_equal(a, b) for a, b in zip(want, loop(frames, SEQ["gop"], 16, 2, 32, obmc=False)))


def test_decoder_refuses_obmc_under_another_block_size(monkeypatch, tmp_path):
    _, prefix, _ = _encode(monkeypatch, tmp_path, "e", ["--obmc"])
    with pytest.raises(ValueError, match="obmc"):
        _decode(tmp_path, prefix, "12")

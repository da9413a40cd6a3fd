"""Sub-pel motion (--subpel) on the CPU: the numpy restatement of the rule
(tests/subpel_ref.py) against the oracle where the two must agree, what the
refinement is worth on frames with true quarter-pel motion, the parser flag
and the metadata key.  The GPU kernels are held to subpel_ref in
tests/test_subpel_gpu.py."""
import json
import types

import numpy as np
import pytest

import subpel_ref as R
from oracle import oracle as O

PAIRS = [(64, 96, 16, 4), (40, 56, 8, 3)]


@pytest.fixture(scope="module")
def pairs():
    """Per (H, W, bs, sr): two frames of the generator and their fields at N = 1, 2, 4."""
    out = {}
    for H, W, bs, sr in PAIRS:
        a, b = R.subpel_sequence(H, W, 2, seed=H + W)
        out[H, W, bs, sr] = (a, b, {n: R.block_matching(a, b, bs, sr, False, n) for n in (1, 2, 4)})
    return out


@pytest.mark.parametrize("fast", [False, True], ids=["full", "tss"])
def test_whole_pel_reference_is_the_oracle(fast):
    a, b = R.subpel_sequence(48, 64, 2, seed=1)
    assert np.array_equal(R.block_matching(a, b, 16, 5, fast, 1), O.ipp_block_matching(a, b, 16, 5, fast))


def test_integer_fields_compensate_like_the_oracle():
    rng = np.random.Generator(np.random.PCG64(3))
    f = rng.integers(0, 256, (48, 80, 3), dtype=np.uint8)
    mv = rng.integers(-40, 41, (3, 5, 2)).astype(np.float32)     # many out of bounds
    assert np.array_equal(R.motion_compensate(f, mv, 16), O.ipp_motion_compensate(f, mv, 16))
    f = rng.integers(0, 256, (33, 35, 3), dtype=np.uint8)        # a zero border outside the full blocks
    mv = rng.integers(-3, 4, (4, 5, 2)).astype(np.float32)
    assert np.array_equal(R.motion_compensate(f, mv, 7), O.ipp_motion_compensate(f, mv, 7))


def test_prediction_rule_by_hand():
    r = np.array([[10, 20, 40], [50, 90, 170], [0, 0, 0]], np.uint8)
    assert R.predict(r, 0, 0, 2).tolist() == [[10, 20], [50, 90]]
    assert R.predict(r, 2, 0, 2).tolist() == [[15, 30], [70, 130]]               # half pel in x
    assert R.predict(r, 1, 3, 1).tolist() == [[(3 * 1 * 10 + 1 * 1 * 20 + 3 * 3 * 50 + 1 * 3 * 90 + 8) >> 4]]
    assert R.valid(4, 4, 2, 3, 3) and not R.valid(5, 4, 2, 3, 3) and not R.valid(-1, 0, 2, 3, 3)
    assert R.split(-1) == (-1, 3)


@pytest.mark.parametrize("case", PAIRS)
def test_refinement_never_raises_a_block_sad(pairs, case):
    H, W, bs, sr = case
    a, b, mv = pairs[case]
    s1, s2, s4 = (R.field_sad(a, b, mv[n], bs) for n in (1, 2, 4))
    assert (s2 <= s1).all() and (s4 <= s2).all()
    assert s4.sum() < s2.sum() < s1.sum()


@pytest.mark.parametrize("case", PAIRS)
def test_most_blocks_end_fractional(pairs, case):
    """True quarter-pel motion: at least 90 % of the blocks leave the integer grid."""
    _, _, mv = pairs[case]
    for n in (2, 4):
        q = np.rint(4 * mv[n]).astype(int)
        assert np.array_equal(q / 4.0, mv[n]) and (q % (4 // n) == 0).all()
        frac = ((q % 4) != 0).any(axis=2)
        assert frac.mean() >= 0.9, (n, frac.mean())
    fr = {tuple(v) for v in (np.rint(4 * mv[4]).astype(int) % 4).reshape(-1, 2)}
    assert len(fr) >= 5, fr


def test_parser_flag():
    from vcf_amd.codec import parser as P
    assert P.parse(P.ipp_parser(), ["encode"]).subpel == 1
    for n in (1, 2, 4):
        assert P.parse(P.ipp_parser(), ["encode", "--subpel", str(n)]).subpel == n
    with pytest.raises(SystemExit):
        P.parse(P.ipp_parser(), ["encode", "--subpel", "3"])
    assert not hasattr(P.parse(P.ipp_parser(), ["decode"]), "subpel")


def test_argument_errors_come_before_any_device_work():
    """Host-side checks: the made-up addresses are never touched, so this runs without a GPU."""
    import ctypes
    from vcf_amd import _lib as L
    A, M = ctypes.c_void_p(4096), ctypes.c_void_p(4097)
    lib = L.lib()
    assert lib.vcf_ipp_block_match_subpel(A, A, 64, 64, 16, 8, 0, 2, M, A, None) == L.VCF_ERR_INVALID
    assert b"aligned" in lib.vcf_last_error()
    assert lib.vcf_ipp_motion_compensate_qpel(A, M, 64, 64, 16, A, None) == L.VCF_ERR_INVALID
    assert b"aligned" in lib.vcf_last_error()
    for bs, sr, n in ((16, 8, 3), (16, 8, 0), (65, 8, 2), (16, 33, 4)):
        assert lib.vcf_ipp_block_match_subpel(A, A, 64, 64, bs, sr, 0, n, A, A, None) == L.VCF_ERR_INVALID


def _encode(monkeypatch, tmp_path, name, extra):
    """The host GOP loop over the numpy tools and the oracle's DCT round trip (no GPU)."""
    import vcf_amd.codec.ipp as M
    from vcf_amd.codec import parser as P
    monkeypatch.setattr(M, "K", types.SimpleNamespace(
        block_matching=lambda r, c, bs, sr, fast, subpel=1: R.block_matching(r, c, bs, sr, fast, subpel),
        motion_compensate=lambda f, mv, bs, subpel=1: R.motion_compensate(f, mv, bs),
        residual=O.ipp_residual, reconstruct=O.ipp_reconstruct))

    class StandIn(M.CoDec):
        def encode_decode_proxy(self, img, frame_type, seq_idx):
            H, W = img.shape[:2]
            return O.decode_frame(O.encode_frame(img, 32), H, W, 32), 8 * int(img.sum() % 997)

    np.save(tmp_path / "frames.npy", np.stack(R.subpel_sequence(32, 48, 3, seed=9)))
    prefix = str(tmp_path / name / "v")
    StandIn(P.parse(P.ipp_parser(), ["encode", "-i", str(tmp_path / "frames.npy"), "-O", prefix, "-N", "3", "-G", "3",
                                     "-S", "2"] + extra)).encode()
    with np.load(prefix + "_mv.npz", allow_pickle=False) as z:
        return json.load(open(prefix + "_meta.json")), z["mv_f32"]


def test_meta_names_the_precision_only_above_whole_pel(monkeypatch, tmp_path):
    plain, mv1 = _encode(monkeypatch, tmp_path, "a", [])
    one, mv1b = _encode(monkeypatch, tmp_path, "b", ["--subpel", "1"])
    assert "subpel" not in plain and "subpel" not in one
    assert plain == {**one, "total_bits": plain["total_bits"]} and np.array_equal(mv1, mv1b)
    assert np.array_equal(mv1, np.rint(mv1))
    four, mv4 = _encode(monkeypatch, tmp_path, "c", ["--subpel", "4"])
    assert four["subpel"] == 4 and set(four) == set(plain) | {"subpel"}
    assert (mv4 != np.rint(mv4)).any()

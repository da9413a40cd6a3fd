"""Hierarchical motion search (--me_levels) on the CPU: the numpy restatement of
the rule (tests/hier_ref.py) by hand and against the oracle where the two must
agree, what the pyramid recovers on fast motion, the parser flag, the refusals,
and that the flag adds nothing to the files or to the calls at level 0.  The
GPU kernels are held to hier_ref in tests/test_hier_gpu.py."""
import json
import types

import numpy as np
import pytest

import hier_ref as R
from oracle import oracle as O


def test_pyramid_by_hand():
    g = np.array([[0, 1, 10, 11, 255, 255, 9],
                  [2, 3, 12, 14, 255, 254, 9],
                  [7, 7, 0, 0, 100, 101, 9],
                  [7, 8, 0, 1, 102, 103, 9],
                  [5, 5, 5, 5, 5, 5, 5]], np.uint8)
    want = [[(0 + 1 + 2 + 3 + 2) >> 2, (10 + 11 + 12 + 14 + 2) >> 2, (255 + 255 + 255 + 254 + 2) >> 2],
            [(7 + 7 + 7 + 8 + 2) >> 2, (0 + 0 + 0 + 1 + 2) >> 2, (100 + 101 + 102 + 103 + 2) >> 2]]
    assert want == [[2, 12, 255], [7, 0, 102]]          # 1.5 -> 2, 11.75 -> 12, 7.25 -> 7, 0.25 -> 0, 101.5 -> 102
    h = R.halve(g)
    assert h.dtype == np.uint8 and h.tolist() == want   # the odd row and the odd column are dropped
    p = R.pyramid(g, 2)
    assert [a.shape for a in p] == [(5, 7), (2, 3), (1, 1)] and p[2].tolist() == [[(2 + 12 + 7 + 0 + 2) >> 2]]


@pytest.fixture(scope="module")
def pairs():
    return [R.fast_sequence(2, 48, 64, s, seed=i) for i, s in enumerate([(3, -2), (-5, 4), (1.5, 0.25)])]


def test_level_zero_is_the_oracle(pairs):
    flat = np.full((48, 64, 3), 91, np.uint8)
    for a, b in [(flat, flat)] + pairs:
        for bs, sr in ((16, 8), (12, 3)):
            assert np.array_equal(R.block_matching(a, b, bs, sr, 0), O.ipp_block_matching(a, b, bs, sr, False))


def test_both_statements_of_the_top_level_agree(pairs):
    a, b = pairs[0]
    pr, pc = R.pyramid(O.ipp_gray(a), 2), R.pyramid(O.ipp_gray(b), 2)
    for l, b_l, sr in ((2, 4, 3), (1, 6, 2), (2, 3, 2)):
        assert np.array_equal(R.plane_search(pr[l], pc[l], b_l, sr), R.plane_search_oracle(pr[l], pc[l], b_l, sr))


def _argmin_by_hand(rg, cg, b, cands):
    """argmin of (SAD, position in cands) over the candidates inside the plane, block (0, 0)."""
    H, W = rg.shape
    keys = [(int(np.abs(rg[dy:dy + b, dx:dx + b].astype(int) - cg[:b, :b].astype(int)).sum()), n, (dx, dy))
            for n, (dx, dy) in enumerate(cands) if dy >= 0 and dx >= 0 and dy + b <= H and dx + b <= W]
    return min(keys)[2]


def test_one_block_frame_against_a_hand_run_chain():
    a, b = R.fast_sequence(2, 23, 27, (6, 5), seed=11)      # one 16 x 16 block, vectors up to (11, 7)
    rg, cg = O.ipp_gray(a), O.ipp_gray(b)
    pr, pc = R.pyramid(rg, 2), R.pyramid(cg, 2)
    assert [p.shape for p in pr] == [(23, 27), (11, 13), (5, 6)]
    v = _argmin_by_hand(pr[2], pc[2], 4, [(dx, dy) for dy in range(-2, 3) for dx in range(-2, 3)])
    chain = [v]
    for l in (1, 0):
        cx, cy = 2 * v[0], 2 * v[1]
        ring = [(cx + ddx, cy + ddy) for ddy in (-1, 0, 1) for ddx in (-1, 0, 1) if (ddx, ddy) != (0, 0)]
        v = _argmin_by_hand(pr[l], pc[l], 16 >> l, [(cx, cy)] + ring)
        chain.append(v)
    got = R.chain(rg, cg, 16, 2, 2, top=R.plane_search)
    assert [tuple(g[0, 0]) for g in got] == chain
    assert chain[-1] == (6, 5)
    assert np.array_equal(R.block_matching(a, b, 16, 2, 2), np.array([[chain[-1]]], np.float32))


def test_invalid_neighbours_are_skipped_and_the_centre_wins_ties():
    rng = np.random.Generator(np.random.PCG64(2))
    rg = rng.integers(0, 256, (9, 9)).astype(np.uint8)
    zero = np.zeros((1, 1, 2), np.int64)
    # the block equals the reference one pixel down and right: neighbour 8 wins; up and left do not exist
    assert R.refine(rg, rg[1:, 1:].copy(), 8, zero).tolist() == [[[1, 1]]]
    # the exact match would be one pixel up and left of the corner: every candidate there is skipped
    cg = np.zeros((9, 9), np.uint8)
    cg[1:, 1:] = rg[:8, :8]
    got = R.refine(rg, cg, 8, zero)[0, 0]
    assert got.min() >= 0 and got.max() <= 1
    # all nine SADs equal: the centre (index 0) stays, also where the top level chose a corner
    flat = np.full((16, 16), 40, np.uint8)
    v = np.array([[[1, 2], [-2, 0]], [[0, -2], [-2, -2]]], np.int64)
    assert np.array_equal(R.refine(flat, flat, 4, v), 2 * v)
    f = np.full((64, 64, 3), 77, np.uint8)
    assert np.array_equal(R.block_matching(f, f, 16, 2, 2), 4 * O.ipp_block_matching(f[:16, :16], f[:16, :16], 4, 2))


def test_pyramid_recovers_a_vector_outside_the_window():
    """96 x 128, bs 16, S 8, true shift (19, -13), the generator's default texture (sinusoids of
    23 .. 97 pixels, noise blurred twice by a box of 9, sigma 2): at L = 2 at least 90 % of the
    blocks whose true match lies inside the frame get exactly (19, -13); at L = 0 none can."""
    H, W, bs = 96, 128, 16
    a, b = R.fast_sequence(2, H, W, (19, -13), seed=5)
    blocks = [(by, bx) for by in range(H // bs) for bx in range(W // bs)
              if R.inside(by * bs - 13, bx * bs + 19, bs, H, W)]
    assert len(blocks) == 30
    hits = {}
    for L in (0, 2):
        mv = R.block_matching(a, b, bs, 8, L)
        hits[L] = sum(tuple(mv[by, bx]) == (19.0, -13.0) for by, bx in blocks)
        assert np.abs(mv).max() <= 8 * 2 ** L + 2 ** L - 1
    print("blocks", len(blocks), "exact at L=0", hits[0], "at L=2", hits[2])
    assert hits[2] >= 0.9 * len(blocks)
    assert hits[0] == 0


def test_parser_flag():
    from vcf_amd.codec import parser as P
    assert P.parse(P.ipp_parser(), ["encode"]).me_levels == 0
    for n in range(4):
        assert P.parse(P.ipp_parser(), ["encode", "--me_levels", str(n)]).me_levels == n
    for bad in ("4", "-1"):
        with pytest.raises(SystemExit):
            P.parse(P.ipp_parser(), ["encode", "--me_levels", bad])
    assert not hasattr(P.parse(P.ipp_parser(), ["decode"]), "me_levels")   # the encoder's choice alone


def test_refusals():
    from vcf_amd import ipp
    from vcf_amd.codec import parser as P
    from vcf_amd.codec.ipp import CoDec
    for flags in (["-M", "12", "--me_levels", "3"], ["-M", "4", "--me_levels", "2"], ["--fast", "--me_levels", "1"]):
        with pytest.raises(ValueError):
            CoDec(P.parse(P.ipp_parser(), ["encode", "-O", "/tmp/never_written"] + flags))
    CoDec(P.parse(P.ipp_parser(), ["encode", "-O", "/tmp/never_written", "-M", "12", "--me_levels", "2"]))
    CoDec(P.parse(P.ipp_parser(), ["encode", "-O", "/tmp/never_written", "--fast"]))
    f = np.zeros((32, 32, 3), np.uint8)
    for kw in (dict(bs=12, levels=3), dict(bs=4, levels=2), dict(bs=16, fast=True, levels=1), dict(bs=16, levels=4),
               dict(bs=16, levels=-1), dict(bs=16, levels=1, variant=1)):
        with pytest.raises(ValueError):
            ipp.block_matching(f, f, sr=4, **kw)


def test_argument_errors_come_before_any_device_work():
    """Host-side checks: the made-up addresses are never touched, so this runs without a GPU."""
    import ctypes
    from vcf_amd import _lib as L
    A, M = ctypes.c_void_p(4096), ctypes.c_void_p(4097)
    lib, n = L.lib(), ctypes.c_int64(-1)
    assert lib.vcf_ipp_hier_workspace_bytes(37, 53, 2, ctypes.byref(n)) == L.VCF_OK
    assert n.value == 2 * (37 * 53 + 18 * 26 + 9 * 13)
    assert lib.vcf_ipp_hier_workspace_bytes(37, 53, 0, ctypes.byref(n)) == L.VCF_OK and n.value == 2 * 37 * 53
    for H, W, lv in ((37, 53, 4), (37, 53, -1), (0, 53, 1), (37, -1, 1)):
        assert lib.vcf_ipp_hier_workspace_bytes(H, W, lv, ctypes.byref(n)) == L.VCF_ERR_INVALID
    assert lib.vcf_ipp_hier_workspace_bytes(37, 53, 1, None) == L.VCF_ERR_INVALID
    big = 1 << 30
    assert lib.vcf_ipp_block_match_hier(A, A, 64, 64, 16, 8, 2, 1, M, A, big, None) == L.VCF_ERR_INVALID
    assert b"aligned" in lib.vcf_last_error()
    for bs, sr, lv, sp in ((16, 8, 4, 1), (16, 8, -1, 1), (12, 8, 3, 1), (4, 8, 2, 1), (65, 8, 0, 1), (0, 8, 0, 1),
                           (16, 33, 1, 1), (16, -1, 1, 1), (16, 8, 1, 3), (16, 8, 0, 0)):
        assert lib.vcf_ipp_block_match_hier(A, A, 64, 64, bs, sr, lv, sp, A, A, big, None) == L.VCF_ERR_INVALID
    need = 2 * (64 * 64 + 32 * 32 + 16 * 16)
    assert lib.vcf_ipp_block_match_hier(A, A, 64, 64, 16, 8, 2, 1, A, A, need - 1, None) == L.VCF_ERR_INVALID
    assert b"workspace" in lib.vcf_last_error()
    for k in range(4):
        args = [A, A, A, A]
        args[k] = None
        assert lib.vcf_ipp_block_match_hier(args[0], args[1], 64, 64, 16, 8, 2, 1, args[2], args[3], big,
                                            None) == L.VCF_ERR_INVALID
    # an empty field is legal and touches nothing
    assert lib.vcf_ipp_block_match_hier(A, A, 10, 100, 16, 8, 2, 4, A, A, big, None) == L.VCF_OK


def _encode(monkeypatch, tmp_path, name, extra, host=False):
    """The host GOP loops over the numpy tools and the oracle's DCT round trip (no GPU) -> (meta.json,
    the motion file's arrays, the keywords of every search)."""
    import bipred_ref as BR
    import subpel_ref as S
    import vcf_amd.codec.ipp as M
    from vcf_amd.codec import parser as P
    calls = []

    def search(r, c, bs, sr, fast, **kw):
        calls.append(dict(kw))
        return R.block_matching(r, c, bs, sr, kw.get("levels", 0), kw.get("subpel", 1))

    monkeypatch.setattr(M, "K", types.SimpleNamespace(
        block_matching=search, motion_compensate=lambda f, mv, bs, subpel=1: S.motion_compensate(f, mv, bs),
        residual=O.ipp_residual, reconstruct=O.ipp_reconstruct, bipred_residual=BR.bipred_residual))

    class StandIn(M.CoDec):
        def encode_decode_proxy(self, img, frame_type, seq_idx):
            H, W = img.shape[:2]
            return O.decode_frame(O.encode_frame(img, 32), H, W, 32), 8 * int(img.sum() % 997)

    np.save(tmp_path / "frames.npy", np.stack(R.fast_sequence(4, 32, 48, (5, -3), seed=9)))
    prefix = str(tmp_path / name / "v")
    StandIn(P.parse(P.ipp_parser(), ["encode", "-i", str(tmp_path / "frames.npy"), "-O", prefix, "-N", "4", "-G", "4",
                                     "-S", "1"] + extra)).encode()
    with np.load(prefix + "_mv.npz", allow_pickle=True) as z:
        return json.load(open(prefix + "_meta.json")), {k: z[k] for k in z.files}, calls


@pytest.mark.parametrize("extra", [[], ["--bframes", "1"], ["--subpel", "4"]], ids=["ipp", "bframes", "subpel"])
def test_the_flag_adds_no_key_no_array_and_no_keyword_at_level_zero(monkeypatch, tmp_path, extra):
    plain, arrays, calls = _encode(monkeypatch, tmp_path, "a", extra)
    assert calls and all("levels" not in c for c in calls)
    zero, arrays0, calls0 = _encode(monkeypatch, tmp_path, "b", extra + ["--me_levels", "0"])
    assert calls0 == calls and zero == plain
    assert set(arrays0) == set(arrays) and all(np.array_equal(arrays0[k], arrays[k]) for k in ("mv_f32",))
    two, arrays2, calls2 = _encode(monkeypatch, tmp_path, "c", extra + ["--me_levels", "2"])
    assert len(calls2) == len(calls) and all(c.get("levels") == 2 for c in calls2)
    assert [{k: v for k, v in c.items() if k != "levels"} for c in calls2] == calls
    assert set(two) == set(plain) and set(arrays2) == set(arrays)
    assert all(arrays2[k].shape == arrays[k].shape and arrays2[k].dtype == arrays[k].dtype for k in arrays)
    # -S 1 cannot follow 5 pixels a frame; two levels reach +-7
    assert np.abs(arrays["mv_f32"]).max() <= 1.75 and np.abs(arrays2["mv_f32"]).max() >= 4

"""CPU check of the tile geometry, plan and index maps that the 2D-KLT and 2D-LBT kernels share
(vcf_block_tile.h, host build with g++): over every block size and a set of frames, walking every
tile of the plan as the kernels' loops do, the scatter map fills the coefficient frame exactly
once, the gather map reads back what the scatter map wrote, the crop map fills the pixel frame
exactly once, and the plan is the one the launches have always used."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

HARNESS_SRC = os.path.join(ROOT, "tests", "cpu", "block_tile_harness.cpp")
BS = range(2, 17)
FRAMES = [(5, 7), (16, 16), (37, 45), (61, 77), (150, 210)]
SWEEP = (150, 210)
LDS = (48 * 1024, 80 * 1024, 156 * 1024)
PLAN = ("Hp", "Wp", "top", "left", "nbx", "nby", "N", "TB", "cls", "tiles", "chunks", "tbm", "lds")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    so = str(tmp_path_factory.mktemp("bt") / "block_tile_harness.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", os.path.join(ROOT, "vcf_amd", "csrc"),
                    HARNESS_SRC, "-o", so], check=True)
    L = ctypes.CDLL(so)
    pi32, pi64 = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)
    L.bt_plan.argtypes = [ctypes.c_int] * 5 + [pi32]
    L.bt_plan.restype = None
    L.bt_walk_scatter.argtypes = [ctypes.c_int] * 4 + [pi32, pi32]
    L.bt_walk_gather.argtypes = [ctypes.c_int] * 4 + [pi32, pi64]
    L.bt_walk_crop.argtypes = [ctypes.c_int] * 3 + [pi32, pi32, pi64]
    return L


def _p(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64 if a.dtype == np.int64 else ctypes.c_int32))


def plan(L, H, W, B, decode=False, elem=2):
    out = np.zeros(13, np.int32)
    L.bt_plan(H, W, B, int(decode), elem, _p(out))
    return dict(zip(PLAN, (int(x) for x in out)))


def scatter_expected(p, B, sub):
    """id = (b D + k) 3 + c at every byte of the padded coefficient frame, from the layouts' definitions."""
    D = B * B
    py, px, c = np.meshgrid(np.arange(p["Hp"]), np.arange(p["Wp"]), np.arange(3), indexing="ij")
    if sub:    # subband (ky, kx), nby x nbx coefficients, one per block
        ky, by, kx, bx = py // p["nby"], py % p["nby"], px // p["nbx"], px % p["nbx"]
    else:      # block (by, bx), B x B coefficients
        by, ky, bx, kx = py // B, py % B, px // B, px % B
    return ((by * p["nbx"] + bx) * D + ky * B + kx) * 3 + c


@pytest.mark.parametrize("B", BS)
def test_scatter_gather_and_crop_cover_their_frames_exactly_once(harness, B):
    D = B * B
    for H, W in FRAMES:
        p = plan(harness, H, W, B)
        assert (p["Hp"], p["Wp"]) == (-(-H // B) * B, -(-W // B) * B)
        assert (p["top"], p["left"]) == ((p["Hp"] - H) // 2, (p["Wp"] - W) // 2)
        assert p["N"] == p["nbx"] * p["nby"] == p["Hp"] * p["Wp"] // D
        assert p["tiles"] == -(-p["N"] // p["TB"])
        n = p["Hp"] * p["Wp"] * 3
        for sub in (0, 1):
            writes, ident = np.zeros(n, np.int32), np.full(n, -1, np.int32)
            assert harness.bt_walk_scatter(H, W, B, sub, _p(writes), _p(ident)) == 0
            assert (writes == 1).all(), (H, W, sub)
            assert np.array_equal(ident.reshape(p["Hp"], p["Wp"], 3), scatter_expected(p, B, sub)), (H, W, sub)
            reads, at = np.zeros(n, np.int32), np.full(n, -1, np.int64)
            assert harness.bt_walk_gather(H, W, B, sub, _p(reads), _p(at)) == 0
            assert (reads == 1).all(), (H, W, sub)
            assert np.array_equal(ident[at], np.arange(n)), (H, W, sub)      # (b, k, c) reads the byte written for it
        writes, ident = np.zeros(H * W * 3, np.int32), np.full(H * W * 3, -1, np.int32)
        outside = ctypes.c_int64(-1)
        assert harness.bt_walk_crop(H, W, B, _p(writes), _p(ident), ctypes.byref(outside)) == 0
        assert (writes == 1).all(), (H, W)
        assert outside.value == n - H * W * 3                                 # and nothing else
        y, x, c = np.meshgrid(np.arange(H), np.arange(W), np.arange(3), indexing="ij")
        py, px = y + p["top"], x + p["left"]
        want = (((py // B) * p["nbx"] + px // B) * D + (py % B) * B + px % B) * 3 + c
        assert np.array_equal(ident.reshape(H, W, 3), want), (H, W)


@pytest.mark.parametrize("B", BS)
def test_lds_bytes_fit_the_smallest_class(harness, B):
    D = B * B
    for H, W in FRAMES:
        for decode, elem in ((False, 2), (True, 2)) + (((False, 4), (True, 4)) if B <= 8 else ()):
            p = plan(harness, H, W, B, decode, elem)
            stage = (p["TB"] * (D | 1) * (2 if decode else elem) + 15) // 16 * 16
            assert p["lds"] == (3 if decode else 1) * stage + p["TB"] * (3 * D + 4)
            assert 0 <= p["cls"] <= 2 and p["lds"] <= LDS[p["cls"]]
            assert p["cls"] == 0 or p["lds"] > LDS[p["cls"] - 1]


def test_one_tile_rule_serves_both_codecs(harness):
    """8192 values per tile (16384 above D = 128) in whole waves, 64 to 1024 blocks: for every D <= 64,
    all the LBT kernels reach, that is the 8192 / D rule they had."""
    for B in BS:
        D = B * B
        TB = plan(harness, *SWEEP, B)["TB"]
        assert TB == min(1024, max(64, (16384 if D > 128 else 8192) // D // 64 * 64))
        if D <= 64:
            assert TB == min(1024, max(64, 8192 // D // 64 * 64))


def _staged(N, chunks, tbm, chunk=2048):
    return sum(-(-min(chunk, N - c * chunk) // tbm) for c in range(chunks))


def test_lbt_plans_are_the_recorded_ones(harness):
    """The sweep frame at B = 2..8: what vcf_lbt_tile_plan answers, and the table recorded when the
    query was added (B: blocks, TB, encode class, decode class, tiles, last tile, chunks, staged tiles).
    The one test of this module that loads the built library (a host-only call, no GPU)."""
    import vcf_amd.lbt as G
    table = {2: (7875, 1024, 0, 0, 8, 707, 4, 4), 3: (3500, 896, 1, 1, 4, 812, 2, 4), 4: (2014, 512, 1, 1, 4, 478, 1, 2),
             5: (1260, 320, 1, 1, 4, 300, 1, 3), 6: (875, 192, 1, 1, 5, 107, 1, 3), 7: (660, 128, 0, 1, 6, 20, 1, 3),
             8: (513, 128, 1, 1, 5, 1, 1, 3)}
    for B in range(2, 9):
        enc, dec = plan(harness, *SWEEP, B, False, 4), plan(harness, *SWEEP, B, True, 4)
        for p, decode in ((enc, False), (dec, True)):
            assert (p["TB"], p["cls"], p["tiles"], p["chunks"], p["tbm"]) == tuple(G.tile_plan(*SWEEP, B, decode))
        N, TB = enc["N"], enc["TB"]
        assert (N, TB, enc["cls"], dec["cls"], enc["tiles"], N - (enc["tiles"] - 1) * TB, enc["chunks"],
                _staged(N, enc["chunks"], enc["tbm"])) == table[B]


def test_klt_sweep_tile_counts(harness):
    """tests/klt_sweep_cases.py: 8, 4, 4, 6, 5, 4, 3 workgroups per frame, the last one partial."""
    for B, tiles in zip((2, 3, 5, 7, 11, 13, 16), (8, 4, 4, 6, 5, 4, 3)):
        for decode in (False, True):
            p = plan(harness, *SWEEP, B, decode, 2)
            assert p["tiles"] == tiles and p["N"] % p["TB"] != 0

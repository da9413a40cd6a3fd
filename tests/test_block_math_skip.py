"""CPU check of the encode's provable-zero row test (vcf_dct_block.h, host build
with g++ -ffp-contract=off): whenever the test says "skip", the real row pass
(dct2_8f + cvt_trunc_i32) gives 16/16 zero indices (64/64 for a channel whose
three pairs pass), and the bound is tight enough to pass for rows 2..7 of the
benchmark's frames."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from vcf_amd.synthetic import synth_frame

HARNESS_SRC = os.path.join(ROOT, "tests", "cpu", "skip_harness.cpp")
QS = [1, 32, 64, 1 << 20]   # the row pass's scale is 1/Q; channels share the column pass's units


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    so = str(tmp_path_factory.mktemp("hs") / "skip_harness.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
                    "-I", os.path.join(ROOT, "vcf_amd", "csrc"), HARNESS_SRC, "-o", so], check=True)
    L = ctypes.CDLL(so)
    pf, pu8, pi32 = (ctypes.POINTER(t) for t in (ctypes.c_float, ctypes.c_uint8, ctypes.c_int32))
    L.hs_row_pairs.argtypes = [ctypes.c_int, pf, pf, ctypes.c_int, pu8, pi32]
    L.hs_colpass.argtypes = [ctypes.c_int, pu8, pf]
    L.hs_block_verdicts.argtypes = [ctypes.c_int, pu8, ctypes.c_int, pu8]
    return L


def _ptr(a, t):
    return a.ctypes.data_as(ctypes.POINTER(t))


def run_pairs(L, ua, ub, Q):
    ua = np.ascontiguousarray(ua, np.float32)
    ub = np.ascontiguousarray(ub, np.float32)
    n = len(ua)
    skip = np.empty(n, np.uint8)
    idx = np.empty((n, 16), np.int32)
    L.hs_row_pairs(n, _ptr(ua, ctypes.c_float), _ptr(ub, ctypes.c_float), Q, _ptr(skip, ctypes.c_uint8),
                   _ptr(idx, ctypes.c_int32))
    return skip.astype(bool), idx


def scale_to(u, Q, t):
    """Rows u scaled so that the exact L1 bound 0.5 * sum|u| / Q equals t."""
    s = np.abs(u).sum(-1, keepdims=True)
    return u * (t[:, None] * Q / (0.5 * s))


def check(skip, idx, what):
    bad = skip & (idx != 0).any(1)
    assert not bad.any(), (what, int(bad.sum()), idx[bad][:4])


@pytest.mark.parametrize("Q", QS)
def test_random_rows_around_the_threshold(harness, Q):
    rng = np.random.Generator(np.random.PCG64(Q))
    n = 120_000
    shapes = [rng.normal(0, 1, (n // 3, 8)),                                  # dense
              rng.normal(0, 1, (n // 3, 8)) * (rng.random((n // 3, 8)) < 0.3),   # sparse
              rng.normal(0, 1, (n // 3, 8)) * np.exp2(-np.arange(8.0))]       # decaying, like smooth content
    ua = np.concatenate(shapes)
    ua[np.abs(ua).sum(1) == 0, 0] = 1.0
    ua = scale_to(ua, Q, rng.uniform(0.5, 1.5, n))
    ub = rng.permutation(ua) * rng.choice([0.0, 0.25, 1.0], (n, 1))           # the larger row decides
    skip, idx = run_pairs(harness, ua, ub, Q)
    check(skip, idx, "random")
    # the draw straddles the threshold, and the bound is not vacuous: rows it refuses do reach index +-1
    assert 0.2 < skip.mean() < 0.8
    assert (idx[~skip] != 0).any()


def basis():
    n = np.arange(8)
    return np.array([[np.sqrt((1 if k == 0 else 2) / 8) * np.cos(np.pi * (2 * m + 1) * k / 16) for m in n] for k in n])


@pytest.mark.parametrize("Q", QS)
def test_worst_case_rows(harness, Q):
    """Single spikes (the L2 form's worst case), alternating signs and the sign
    pattern of every basis row (the L1 form's: q[j] = a * sum|R[j]|), stepped
    finely through the threshold and to the floats next to it."""
    pats = [np.eye(8)[x] * s for x in range(8) for s in (1.0, -1.0)]
    pats += [(-1.0) ** np.arange(8), -((-1.0) ** np.arange(8))]
    pats += [np.sign(r) for r in basis()] + [-np.sign(r) for r in basis()]
    pats = np.array(pats)
    t = np.concatenate([np.linspace(0.9, 1.1, 2001), 1 / (1 + 2.0 ** -10) + np.arange(-40, 41) * 2.0 ** -24])
    ua = np.concatenate([scale_to(np.repeat(p[None], len(t), 0), Q, t) for p in pats])
    for ub in (np.zeros_like(ua), ua[::-1].copy(), -ua):
        skip, idx = run_pairs(harness, ua, ub, Q)
        check(skip, idx, "worst case")
        assert skip.any() and (~skip).any()
    # a spike at the largest basis entry reaches index 1 just above the threshold: the bound's 2 % is what is left
    spike = scale_to(np.eye(8)[:1], Q, np.array([1.03 / (2 * 0.4903926)]))
    skip, idx = run_pairs(harness, spike, np.zeros_like(spike), Q)
    assert not skip[0] and np.abs(idx[0]).max() == 1


def test_zero_and_negative_zero_rows(harness):
    z = np.zeros((2, 8), np.float32)
    z[1] = -0.0
    skip, idx = run_pairs(harness, z, z[::-1].copy(), 32)
    assert skip.all() and not idx.any()


def blocks_of(frame):
    H, W, _ = frame.shape
    return np.ascontiguousarray(frame.reshape(H // 8, 8, W // 8, 24).transpose(0, 2, 1, 3)).reshape(-1, 192)


def test_tight_enough_for_the_benchmark_frames(harness):
    """Seeds 0..3 are rank 0's frames of the headline.  A 64-block group (a wave)
    skips a channel's row pair only if all 64 blocks pass: rows 2..7 must pass in
    at least 99 % of the (group, channel) pairs at the benchmark's Q = 32, and a
    passed row pair really is all zeros through the host column and row pass."""
    Q = 32
    for seed in range(4):
        blk = blocks_of(synth_frame(2160, 3840, seed))
        n = len(blk)
        v = np.empty((n, 3, 8, 8), np.float32)
        harness.hs_colpass(n, _ptr(blk, ctypes.c_uint8), _ptr(v, ctypes.c_float))
        ok = np.empty((n, 3, 3), np.uint8)
        harness.hs_block_verdicts(n, _ptr(blk, ctypes.c_uint8), Q, _ptr(ok, ctypes.c_uint8))
        groups = ok.reshape(n // 64, 64, 3, 3).all(1)          # [group, channel, pair]
        frac = groups.all(2).mean()
        print(f"seed {seed}: rows 2..7 pass in {frac:.4%} of (group, channel) pairs; per pair {groups.mean((0, 1))}")
        assert frac >= 0.99, (seed, frac)
        for p in (1, 2, 3):
            skip, idx = run_pairs(harness, v[:, :, 2 * p].reshape(-1, 8), v[:, :, 2 * p + 1].reshape(-1, 8), Q)
            assert np.array_equal(skip, ok[:, :, p - 1].reshape(-1).astype(bool))
            check(skip, idx, ("frame", seed, p))

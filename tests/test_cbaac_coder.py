"""CPU check of the A8 coder step that every tiled CBAAC kernel shares (vcf_amd/csrc/vcf_cbaac_coder.h, host
build with g++): a whole-segment encoder and decoder made of the header's functions write the serial coder's
bytes (vcf_cbaac_encode, order 0) and read them back, on streams that reach every branch of the step, and
floordiv / floordiv_big equal integer division over the operands their comments and callers allow."""
import ctypes
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from vcf_amd import cbaac as C

HARNESS_SRC = os.path.join(ROOT, "tests", "cpu", "cbaac_coder_harness.cpp")
RANGES = (1, 2, 2**31 - 1, 2**31, 2**32 - 1, 2**32)
TOTALS = (1, 2, 255, 256, 257, 8448, 16383, 16384, 16385, 2**19)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    so = str(tmp_path_factory.mktemp("cc") / "cbaac_coder_harness.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-I",
                    os.path.join(ROOT, "vcf_amd", "csrc"), HARNESS_SRC, "-o", so], check=True)
    L = ctypes.CDLL(so)
    pu8, pi64, pf64 = (ctypes.POINTER(t) for t in (ctypes.c_uint8, ctypes.c_int64, ctypes.c_double))
    L.cc_encode.argtypes = [pu8, ctypes.c_int64, pu8, ctypes.c_int64, pi64]
    L.cc_encode.restype = ctypes.c_int64
    L.cc_decode.argtypes = [pu8, ctypes.c_int64, ctypes.c_int64, pu8]
    L.cc_decode.restype = None
    for f in (L.cc_floordiv, L.cc_floordiv_big):
        f.argtypes = [pf64, pf64, pf64, ctypes.c_int64]
        f.restype = None
    return L


def _p(a, t=ctypes.c_uint8):
    return a.ctypes.data_as(ctypes.POINTER(t))


def _streams():
    rng = np.random.default_rng(20261)
    for n in (0, 1, 2, 255, 256, 257, 4096):
        yield f"random{n}", rng.integers(0, 256, n, dtype=np.uint8)
    yield "zeros", np.zeros(40000, np.uint8)            # crosses the 16384 halving twice; long common prefixes
    yield "straddle", np.tile(np.array([127, 128], np.uint8), 10000)   # intervals either side of the midpoint
    yield "pending_flushed", _pending_stream(leave=False)    # the flush writes the long run
    yield "pending_emitted", _pending_stream(leave=True)     # a renormalisation writes it


def _pending_stream(leave, n=48):
    """The issue's alternating stream reaches the underflow branch but no more than 12 pending bits (22 over
    the other symbol pairs tried, at any length): more needs a code point within 2^-32 of a midpoint, which
    length does not buy.  So this stream is built: every symbol is the one whose interval holds the midpoint
    of the coder's interval (about 8 underflow steps each, never a common bit), so the flush writes a run of
    hundreds of bits; with `leave`, a last symbol 0 leaves the midpoint and the run is written by that
    step's renormalisation instead.  The coder here is the textbook loop on Python integers, used only to
    choose the symbols."""
    c, low, high, out = list(range(257)), 0, 2**32 - 1, []
    for i in range(n + leave):
        r, tot = high - low + 1, c[256]
        ends = [(low + r * c[s] // tot, low + r * c[s + 1] // tot - 1) for s in range(256)]
        s = 0 if i == n else next(s for s, (a, b) in enumerate(ends) if a <= 2**31 - 1 <= b)
        out.append(s)
        low, high = ends[s]
        while True:
            if high < 2**31 or low >= 2**31:
                low, high = (low << 1) & 0xFFFFFFFF, ((high << 1) & 0xFFFFFFFF) | 1
            elif low >= 2**30 and high < 3 * 2**30:
                low, high = (low << 1) & 0x7FFFFFFF, ((high << 1) & 0xFFFFFFFF) | 0x80000001
            else:
                break
        stale = c[256]
        f = [c[t + 1] - c[t] + (t == s) for t in range(256)]
        if stale >= 16384:
            f = [(x >> 1) + 1 for x in f]
        c = [sum(f[:t]) for t in range(257)]
    return np.array(out, np.uint8)


def test_bytes_equal_the_serial_coder_and_round_trip(harness):
    seen = np.zeros(5, np.int64)
    for name, sym in _streams():
        want = C.encode_symbols(sym, 0)
        out, stats = np.zeros(len(want) + 64, np.uint8), np.zeros(5, np.int64)
        nb = harness.cc_encode(_p(sym), sym.size, _p(out), out.size, _p(stats, ctypes.c_int64))
        assert nb == len(want) and out[:nb].tobytes() == want, name
        assert stats[0] == sym.size
        back = np.full(sym.size, 255, np.uint8)
        harness.cc_decode(_p(out), nb, sym.size, _p(back))
        assert np.array_equal(back, sym), name
        seen[:3] += stats[:3]
        seen[3:] = np.maximum(seen[3:], stats[3:])
    steps, common, underflow, emitted, flushed = (int(x) for x in seen)
    # the inputs reach the step's branches: no common bit (d == 0), underflow (p > 0), and more pending bits
    # than a word holds in one run, written by the flush and written by a renormalisation
    assert common < steps and common > 0
    assert underflow > 0
    assert flushed > 32
    assert emitted > 32


def _check(f, a, t):
    """f(a, t, 1.0 / t) == a // t for Python integers a, t (exact in a double)."""
    fa, ft = np.array([float(x) for x in a]), np.array([float(x) for x in t])
    assert all(int(x) == y for x, y in zip(fa, a)) and all(int(x) == y for x, y in zip(ft, t))
    q = np.empty(len(a), np.float64)
    f(_p(fa, ctypes.c_double), _p(ft, ctypes.c_double), _p(q, ctypes.c_double), len(a))
    bad = [(x, y, int(z)) for x, y, z in zip(a, t, q) if int(z) != x // y or z != np.floor(z)]
    assert not bad, bad[:5]


def test_floordiv_is_the_integer_quotient(harness):
    """a = range * c over t: the interval ends floor(range * cum / total) of every kernel."""
    cases = [(r * c, t) for r, t in itertools.product(RANGES, TOTALS) for c in (0, 1, t - 1, t)]
    rng = np.random.default_rng(20262)
    for _ in range(4000):
        t = int(rng.integers(1, 2**19 + 1)) if rng.random() < 0.5 else int(rng.integers(1, 16386))
        r = int(rng.integers(1, 2**32 + 1))
        r = min(r, (2**47 - 1) // t)                     # a < 2^47, the bound of floordiv's comment
        cases.append((r * int(rng.integers(0, t + 1)), t))
    _check(harness.cc_floordiv, *zip(*cases))


def test_floordiv_big_is_the_integer_quotient(harness):
    """a = (T + 1) * total - 1 over range, T < range: the scaled value of the lane decoder's search."""
    cases = [((T + 1) * tot - 1, r) for r, tot in itertools.product(RANGES, TOTALS)
             for T in sorted({0, 1 % r, (r - 2) % r, r - 1})]
    rng = np.random.default_rng(20263)
    for _ in range(4000):
        r = int(rng.integers(1, 2**32 + 1))
        tot = int(rng.integers(1, 16386))
        cases.append(((int(rng.integers(0, r)) + 1) * tot - 1, r))
    _check(harness.cc_floordiv_big, *zip(*cases))

"""The cases both 2D-DWT sweep test files run (tests/test_dwt_sweep.py on the
host, tests/test_dwt_sweep_gpu.py on the GPU), and their expected values,
computed once per process by the CPU oracle (oracle.oracle.dwt_encode_frame /
dwt_decode_frame, whose 1-D arithmetic tests/test_oracle_dwt.py pins to pywt
bit for bit for all 106 wavelets).  Nothing expected comes from the library.

vcf_dwt.hip compiles its fused forward, fused inverse and strip kernels once
per filter length F = 2 .. 18, picks among them (and the separable, band and
line kernels) by F, by the taps and by each level's plane size; what a call
launches is asked of the library itself (vcf_dwt_plan) by tests/test_dwt_sweep.py.
The groups, and the kernels each is there to reach:

ALL   every wavelet of the table through the shipped path on two tiny frames.
      70 x 90, L = 3: planes 35 x 45, 18 x 23, 9 x 12 -- a fused first level
      and two separable ones for F <= 18, the separable kernels alone above;
      the decode is fused for F <= 18 and takes pywt's short-input branch for
      longer filters (F/2 > 9).  37 x 53, L = 2, Q = 1: odd sizes at every level.
FAST  every wavelet with F <= 18 on 420 x 400 (LL1 = 210 x 200 = 42000 samples,
      above the 40000 under which later levels go separable).  L = 3, Q = 32:
      level 2 on the strip kernel's power-of-two quantizer for F <= 10, on the
      fused middle level (neither first nor last) for F = 12 .. 18.  L = 2,
      Q = 7: level 2 on the fused last level.  Decoded by the shipped path and
      by the A/B library's fused (1) and separable (2) decodes.
AB    one wavelet per fast length that no other GPU test runs, through the A/B
      library's fused (1), strip (6) and hybrid (20) encodes, where every level
      takes that kernel whatever its size.
TEN   the six 10-tap wavelets whose taps are not compiled in, on frames where
      db5 and bior4.4 (the controls) take the level-1+2 band kernel, the line
      inverse and the inverse levels 2+1 kernel: the generic F = 10 kernels
      with run-time taps, and the comparisons that must turn these wavelets away.
LONG  filters of 42 .. 102 taps on 128 x 120 (the separable kernels): L = 1
      has 64 x 60 subbands, short for none; L = 2 has 32 x 30, shorter than
      F/2 for dmey (62), db38 (76) and coif17 (102).
RAW   index pyramids no encoder writes, decoded (see RAW below).
BATCH five frames in one call against five calls, F = 4, 6, 14 and coif17.

Encode cases hold two frames per call, so the frame stride counts: a smooth one
(gradient plus low-amplitude noise: most detail indices 128) and a uniformly
random one (dense indices).
"""
import functools

import numpy as np

from decoder_inputs import index_plane
from oracle import oracle as O

# the 106 names of vcf_wavelets.h (tests/test_dwt_sweep.py compares), by filter length for F <= 18
FAST_BY_LEN = {
    2: ("bior1.1", "db1", "haar", "rbio1.1"),
    4: ("bior3.1", "db2", "rbio3.1", "sym2"),
    6: ("bior1.3", "bior2.2", "coif1", "db3", "rbio1.3", "rbio2.2", "sym3"),
    8: ("bior3.3", "db4", "rbio3.3", "sym4"),
    10: ("bior1.5", "bior2.4", "bior4.4", "db5", "rbio1.5", "rbio2.4", "rbio4.4", "sym5"),
    12: ("bior3.5", "bior5.5", "coif2", "db6", "rbio3.5", "rbio5.5", "sym6"),
    14: ("bior2.6", "db7", "rbio2.6", "sym7"),
    16: ("bior3.7", "db8", "rbio3.7", "sym8"),
    18: ("bior2.8", "bior6.8", "coif3", "db9", "rbio2.8", "rbio6.8", "sym9"),
}
FAST_NAMES = tuple(n for F in sorted(FAST_BY_LEN) for n in FAST_BY_LEN[F])
SLOW_NAMES = (("bior3.9", "rbio3.9", "dmey") + tuple(f"db{i}" for i in range(10, 39))
              + tuple(f"sym{i}" for i in range(10, 21)) + tuple(f"coif{i}" for i in range(4, 18)))
ALL_NAMES = FAST_NAMES + SLOW_NAMES
CT_NAMES = ("bior4.4", "db5")      # the 10-tap wavelets with compile-time taps
GENERIC_TEN = tuple(n for n in FAST_BY_LEN[10] if n not in CT_NAMES)


def flen(name):
    """The filter length, from the oracle's table."""
    return O.lib().vcfo_wavelet_len(O.wavelet_index(name))


def _case(group, wavelet, H, W, L, Q, **more):
    return dict(name=f"{group}-{wavelet}-{H}x{W}-l{L}-q{Q}", group=group, wavelet=wavelet, H=H, W=W, L=L, Q=Q, **more)


ALL_SHAPES = ((70, 90, 3, 7), (37, 53, 2, 1))
ALL = [_case("all", w, *s) for s in ALL_SHAPES for w in ALL_NAMES]

FAST_FRAME = (420, 400)
FAST_MIDDLE = (3, 32)      # (L, Q): level 2 neither first nor last
FAST_LAST = (2, 7)         # level 2 the last
FAST = [_case("fast", w, *FAST_FRAME, L, Q) for L, Q in (FAST_MIDDLE, FAST_LAST) for w in FAST_NAMES]
FAST_DECODE_VARIANTS = (0, 1, 2)

AB_NAMES = ("db2", "bior3.1", "db3", "bior2.2", "sym5", "rbio2.4", "db7", "bior2.6")
AB_SHAPES = ((141, 301, 4, 3), (96, 128, 3, 32))     # of test_dwt_gpu.test_dwt_vs_oracle
AB_VARIANTS = (1, 6, 20)
AB = [_case("ab", w, *s, variant=v) for s in AB_SHAPES for w in AB_NAMES for v in AB_VARIANTS]
for _c in AB:
    _c["name"] += f"-v{_c['variant']}"

# Q = 300 on the last shape: the controls' line and band21 kernels take their int16 dequantizer (Q > 256)
TEN_SHAPES = ((64, 512, 2, 32), (64, 512, 3, 7), (68, 516, 2, 300))
TEN = [_case("ten", w, *s) for s in TEN_SHAPES for w in GENERIC_TEN + CT_NAMES]

LONG_NAMES = ("db21", "coif7", "dmey", "db38", "coif17")
LONG = [_case("long", w, 128, 120, L, 5) for L in (1, 2) for w in LONG_NAMES]

BATCH_NAMES = ("bior3.1", "rbio2.2", "sym7", "coif17")      # F = 4, 6, 14, 102
BATCH_FRAMES = 5
BATCH = [_case("batch", w, 70, 90, 3, 7) for w in BATCH_NAMES]

# ---- RAW: decoded index pyramids no encoder writes, 70 x 90, L = 2 (planes 35 x 45 and 18 x 23: the fused
# inverse for F <= 18, the separable one for coif5, its short-input branch for db20 and dmey).
# Q = 1: LL uniform over what a 0 .. 255 frame can produce, per channel: 128 + [0, 255 * 2^L] for Y and
# 128 + [-127 * 2^L, 127 * 2^L] for Co and Cg (Y = R/4 + G/2 + B/4 is never negative, the chroma is centred;
# Y's range on all three channels decodes to 56 % clipped pixels under flat details, so no detail range
# could meet the cap).  The details are uniform over 128 +- spread: 127, the whole byte, or 80 where the
# whole byte exceeds the cap (bior3.1 0.5407, rbio2.2 0.5078).  The wavelet of each F is one whose reconstruction filters do not amplify
# uniform indices past the cap by themselves (rbio3.x and bior5.5 do).
# Q = 300: the sparse pattern of the KLT and LBT sweeps -- a wrapping detail (|k - 128| >= 110, Q * k past
# int16) clips every pixel its filters reach, so the details are 128 but for a share `density` of the
# positions within 3 steps of it and a share `rare` drawn from the whole byte, both smaller for the longer
# filters; LL as at Q = 1 with the ranges divided by 300.
# Comments: the share of the oracle's decoded pixels at 0 or 255 (at most RAW_CAP: a clipped pixel hides
# its arithmetic; tests/test_dwt_sweep.py recomputes it) and, at Q = 300, the indices that wrap in int16.
RAW_FRAME = (70, 90)
RAW_L = 2
RAW_CAP = 0.5


def _raw(wavelet, Q, seed, spread=127, rare=0.0, density=0.006):
    return dict(name=f"raw-{wavelet}-q{Q}", group="raw", wavelet=wavelet, H=RAW_FRAME[0], W=RAW_FRAME[1], L=RAW_L,
                Q=Q, seed=seed, spread=spread, rare=rare, density=density)


RAW = [
    _raw("haar", 1, 1),                                       # saturated 0.4477
    _raw("bior3.1", 1, 2, spread=80),                         # saturated 0.3648
    _raw("rbio2.2", 1, 3, spread=80),                         # saturated 0.4405
    _raw("sym4", 1, 4),                                       # saturated 0.4451
    _raw("rbio4.4", 1, 5),                                    # saturated 0.4461
    _raw("bior3.5", 1, 6),                                    # saturated 0.4634
    _raw("bior2.6", 1, 7),                                    # saturated 0.4086
    _raw("bior3.7", 1, 8),                                    # saturated 0.4543
    _raw("bior6.8", 1, 9),                                    # saturated 0.4383
    _raw("coif5", 1, 10),                                     # saturated 0.4502
    _raw("db20", 1, 11),                                      # saturated 0.4431
    _raw("dmey", 1, 12),                                      # saturated 0.4546
    _raw("haar", 300, 21, rare=0.004),                        # saturated 0.4315, 11 indices wrap
    _raw("bior3.1", 300, 22, rare=0.004),                     # saturated 0.3586, 17 indices wrap
    _raw("rbio2.2", 300, 23, rare=0.002),                     # saturated 0.4829, 5 indices wrap
    _raw("sym4", 300, 43, rare=0.002),                        # saturated 0.4221, 7 indices wrap
    _raw("rbio4.4", 300, 25, rare=0.002),                     # saturated 0.4575, 6 indices wrap
    _raw("bior3.5", 300, 43, rare=0.002),                     # saturated 0.3452, 7 indices wrap
    _raw("bior2.6", 300, 27, rare=0.002),                     # saturated 0.4043, 5 indices wrap
    _raw("bior3.7", 300, 28, rare=0.002),                     # saturated 0.3875, 10 indices wrap
    _raw("bior6.8", 300, 29, rare=0.002),                     # saturated 0.4484, 3 indices wrap
    _raw("coif5", 300, 30, rare=0.002),                       # saturated 0.4832, 6 indices wrap
    _raw("db20", 300, 47, rare=0.0007, density=0.001),        # saturated 0.4739, 4 indices wrap
    _raw("dmey", 300, 47, rare=0.0007),                       # saturated 0.4412, 4 indices wrap
]

_BY_NAME = {c["name"]: c for c in ALL + FAST + AB + TEN + LONG + BATCH + RAW}
assert len(_BY_NAME) == len(ALL + FAST + AB + TEN + LONG + BATCH + RAW)


def ids(cases):
    return [c["name"] for c in cases]


def by_name(name):
    return _BY_NAME[name]


def _ro(a):
    a.setflags(write=False)
    return a


def _frozen(d):
    for v in d.values():
        v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def frames(H, W, n=2):
    """n frames of H x W x 3 u8: even ones smooth (a gradient of its own per channel and frame plus
    noise of standard deviation 2), odd ones uniformly random."""
    rng = np.random.Generator(np.random.PCG64(H * 1009 + W * 7 + n))
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.empty((n, H, W, 3), np.uint8)
    for f in range(n):
        if f & 1:
            out[f] = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        else:
            g = np.stack([40 + 30 * c + (150 - 40 * c) * (x / W) + (50 + 10 * f) * (y / H) for c in range(3)], -1)
            out[f] = np.clip(np.rint(g + rng.normal(0, 2, g.shape)), 0, 255).astype(np.uint8)
    return _ro(out)


@functools.lru_cache(maxsize=None)
def expected(wavelet, H, W, L, Q, n=2):
    """Per frame of frames(H, W, n): (the oracle's subbands, the oracle's decode of them)."""
    out = []
    for f in frames(H, W, n):
        sb = _frozen(O.dwt_encode_frame(f, wavelet, L, Q))
        out.append((sb, _ro(O.dwt_decode_frame(sb, H, W, wavelet, L, Q))))
    return tuple(out)


def expected_of(case, n=2):
    return expected(case["wavelet"], case["H"], case["W"], case["L"], case["Q"], n)


def frames_of(case, n=2):
    return frames(case["H"], case["W"], n)


@functools.lru_cache(maxsize=None)
def raw_subbands(name):
    """{LL_L: u16, LH/HL/HH_r: u8} of a RAW case."""
    c = by_name(name)
    rng = np.random.Generator(np.random.PCG64(c["seed"]))
    shapes = O.dwt_shapes(c["H"], c["W"], c["L"])
    h, w = shapes[-1]
    top, half = (255 << c["L"]) // c["Q"], (127 << c["L"]) // c["Q"]
    ll = np.stack([rng.integers(0, top + 1, (h, w)), rng.integers(-half, half + 1, (h, w)),
                   rng.integers(-half, half + 1, (h, w))], -1)
    sb = {f"LL_{c['L']}": (128 + ll).astype(np.uint16)}      # (a negative index wraps in u16, as the encoder's does)
    for r in range(c["L"], 0, -1):
        shape = shapes[r - 1] + (3,)
        for s in ("LH", "HL", "HH"):
            if c["Q"] == 1 and c["spread"] == 127:
                k = index_plane("uniform", shape, np.uint8, rng)
            elif c["Q"] == 1:
                k = rng.integers(128 - c["spread"], 128 + c["spread"] + 1, shape).astype(np.uint8)
            else:
                k = np.where(rng.random(shape) < c["density"], rng.integers(125, 132, shape), 128)
                k = np.where(rng.random(shape) < c["rare"], rng.integers(0, 256, shape), k).astype(np.uint8)
            sb[f"{s}_{r}"] = k
    return _frozen(sb)


@functools.lru_cache(maxsize=None)
def raw_decoded(name):
    c = by_name(name)
    return _ro(O.dwt_decode_frame(raw_subbands(name), c["H"], c["W"], c["wavelet"], c["L"], c["Q"]))


def raw_saturation(name):
    """The share of the oracle's decoded pixels at 0 or 255."""
    d = raw_decoded(name)
    return float(np.mean((d == 0) | (d == 255)))


def raw_wraps(name):
    """The detail indices whose Q * k leaves int16."""
    c = by_name(name)
    return int(sum(np.count_nonzero(np.abs(v.astype(np.int64) - 128) * c["Q"] > 32767)
                   for k, v in raw_subbands(name).items() if not k.startswith("LL")))

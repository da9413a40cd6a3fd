"""The cases both MDCT sweep test files run (tests/test_mdct.py on the host,
tests/test_mdct_sweep_gpu.py on the GPU), and their references, computed once
per process by the float64 restatement (tests/mdct_restated.py).

The kernels of vcf_mdct_dz.hip pick their tile and one of three LDS classes
from the shape and the block size, so the sweep walks the block sizes on one
small frame, 150 x 210: every 3 <= B <= 64 gets at least 3 tiles each way
there.  ENCODE cases are encoded, and the restatement's indices decoded; RAW
cases are index frames no encoder writes, decoded only.  What every case
launches (vcf_mdct_tile_plan) is printed and checked by
test_mdct.py::test_sweep_reaches_every_lds_class.
"""
import functools

import numpy as np

import mdct_restated as M

X, P = M.NO_SUBBANDS, M.PERCEPTUAL
FRAME = (150, 210)


def _flag_name(flags):
    return ("_p" if flags & P else "") + ("_x" if flags & X else "")


def _enc(B, flags, Q, shape=FRAME):
    name = f"b{B}{_flag_name(flags)}_q{Q}" + ("" if shape == FRAME else f"_{shape[0]}x{shape[1]}")
    return dict(name=name, B=B, flags=flags, Q=Q, shape=shape)


# flags alternate 0 / -x down the list, Q cycles through 1, 5, 7, 32
_SWEEP_B = (3, 5, 7, 9, 11, 13, 17, 20, 24, 31, 33, 40, 48, 63, 64)
ENCODE = [_enc(B, (0, X)[i % 2], (1, 5, 7, 32)[i % 4]) for i, B in enumerate(_SWEEP_B)] + [
    _enc(8, P, 32),             # -p: float D on decode, 4 x 4 decode tiles of 7 x 5 segments
    _enc(8, P | X, 5),
    _enc(8, X, 4),
    # no 150 x 210 frame decodes in LDS class 0; these two (found with vcf_mdct_tile_plan) do, in
    # 2 x 2 tiles of 5 x 6 segments and, with -p, 1 x 2 tiles of 3 x 7 segments, the last ones partial
    _enc(7, 0, 32, (71, 59)),
    _enc(8, P, 7, (97, 21)),
    # nor does the -p decoder reach class 2 at 150 x 210; here it does: 2 x 2 tiles of 13 x 7 segments
    _enc(8, P, 5, (101, 203)),
]


def _raw(kind, B, flags, Q, seed, lo=0, hi=255, per_block=0.0, bound=600, shape=FRAME):
    return dict(name=f"{kind}_b{B}{_flag_name(flags)}_q{Q}", kind=kind, B=B, flags=flags, Q=Q, seed=seed, lo=lo, hi=hi,
                per_block=per_block, bound=bound, shape=shape)


# "dense": every index uniform over lo..hi, Q = 1.  "wrap": 128 everywhere but for about per_block
# positions per block and channel, which hold 128 + d with |Q d| > 32767 and |int16(Q d)| <= bound
# (Q = 700: d = +-93, +-94 -> -+436, +-264; Q = 1000: d = +-65, +-66 -> -+536, +-464; Q = 32767: every
# even d -> -d), so a dequantizer that does not wrap saturates where the restatement does not.
# Comments: share of the restatement's pixels at 0 or 255 (at most 0.5: a clipped pixel hides its
# arithmetic); for the wrap cases also the number of wrapping coefficients (at least 100).
# With -p the weights (down to 10 / 121) divide the wrapped value, so that case takes a smaller bound.
RAW = [
    _raw("dense", 5, 0, 1, 11),             # saturated 0.2908
    _raw("dense", 24, X, 1, 12),            # saturated 0.0581
    _raw("dense", 33, 0, 1, 13),            # saturated 0.0365
    _raw("dense", 64, X, 1, 14),            # saturated 0.0367
    _raw("dense", 8, P, 1, 15, 96, 160),    # saturated 0.2027; the whole range of k saturates 0.75 at B = 8
    _raw("wrap", 7, 0, 32767, 21, per_block=6),     # saturated 0.0041, 13699 wrapping
    _raw("wrap", 20, X, 1000, 22, per_block=12),    # saturated 0.1332, 4669 wrapping
    _raw("wrap", 48, 0, 700, 23, per_block=40),     # saturated 0.0016, 5092 wrapping
    _raw("wrap", 8, P, 32767, 24, per_block=6, bound=16),    # saturated 0.0000, 11018 wrapping
]

ENCODE_IDS = [c["name"] for c in ENCODE]
RAW_IDS = [c["name"] for c in RAW]
WHOLE_TILES = ("b40_x_q32",)    # the one case with tiles of several blocks and no partial last tile
BATCH = ((33, False), (24, True))    # three frames in one launch: B whose encode / decode is class 2


def by_name(name):
    return [c for c in ENCODE + RAW if c["name"] == name][0]


def wrap_steps(Q, bound):
    """The d = k - 128 of a wrap case: Q d leaves int16 and comes back within `bound` of zero."""
    d = np.arange(-128, 128)
    y = Q * d
    return d[(np.abs(y) > 32767) & (np.abs(y.astype(np.int16).astype(np.int64)) <= bound)]


def extents(case, decode):
    """(ext_x, ext_y): what the launch tiles -- the blocks of the padded frame on encode, the
    segments that meet the crop on decode."""
    H, W = case["shape"]
    B = case["B"]
    Hp, Wp, top, left = M.padded_shape(H, W, B)
    if not decode:
        return Wp // B, Hp // B
    return (left + W - 1) // B - left // B + 1, (top + H - 1) // B - top // B + 1


@functools.lru_cache(maxsize=None)
def frame(H, W, B):
    f = M.synth_frame(H, W, 100 + B)
    f.setflags(write=False)
    return f


def _frozen(d, keys):
    out = {k: d[k] for k in keys}
    for v in out.values():
        v.setflags(write=False)
    return out


def encode(case, order="fwd"):
    return M.encode(frame(*case["shape"], case["B"]), case["B"], case["Q"], case["flags"], order)


def decode(case, k, order="fwd"):
    return M.decode(k, *case["shape"], case["B"], case["Q"], case["flags"], order)


@functools.lru_cache(maxsize=None)
def encoded(name):
    """The restatement's indices and their float64 precursors ("fwd" order), shared and read-only."""
    return _frozen(encode(by_name(name)), ("k", "pre"))


@functools.lru_cache(maxsize=None)
def raw_k(name):
    """The index frame of a RAW case."""
    c = by_name(name)
    H, W = c["shape"]
    B = c["B"]
    Hp, Wp = M.padded_shape(H, W, B)[:2]
    rng = np.random.Generator(np.random.PCG64(c["seed"]))
    if c["kind"] == "dense":
        k = rng.integers(c["lo"], c["hi"] + 1, (Hp, Wp, 3), dtype=np.uint8)
    else:
        d = wrap_steps(c["Q"], c["bound"])
        assert len(d) >= 2
        hit = rng.random((Hp, Wp, 3)) < c["per_block"] / (B * B)
        k = np.where(hit, 128 + rng.choice(d, (Hp, Wp, 3)), 128).astype(np.uint8)
    k.setflags(write=False)
    return k


def indices(name):
    """What the decoder of a case is given: the restatement's own indices, or the raw frame."""
    return raw_k(name) if "kind" in by_name(name) else encoded(name)["k"]


@functools.lru_cache(maxsize=None)
def decoded(name):
    """The restatement's decode of indices(name) ("fwd" order), shared and read-only."""
    return _frozen(decode(by_name(name), indices(name)), ("rgb", "pre"))

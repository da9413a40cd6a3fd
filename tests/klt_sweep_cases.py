"""The cases both KLT sweep test files run (tests/test_klt.py on the host,
tests/test_klt_sweep_gpu.py on the GPU), and their references, computed once
per process by the float64 restatement (tests/klt_restated.py).

There is no tile-plan query for this codec: vcf_klt_dz.hip takes its tile from
the block size alone (TB = 8192 / D blocks, 16384 / D above D = 128, in whole
waves, 64 to 1024), never from the frame, and its LDS class follows from TB
and D.  Walking B therefore walks every tile and class; on the 150 x 210 frame
of the sweep B = 2, 3, 5, 7, 11, 13, 16 give 8, 4, 4, 6, 5, 4, 3 workgroups per
frame, the last one partial every time.

The weights are a seeded random orthonormal matrix per channel, not a trained
basis: the kernels are handed their weights either way, and no eigenvalue is
degenerate.  ENCODE cases are encoded, and the restatement's indices decoded
with the float32 weights; RAW cases are index frames no encoder writes.
"""
import functools

import numpy as np

import klt_restated as K

X = K.NO_SUBBANDS
FRAME = (150, 210)
SWEEP_B = (2, 3, 5, 7, 11, 13, 16)


def _enc(B, flags, Q):
    return dict(name=f"b{B}{'_x' if flags else ''}_q{Q}", B=B, flags=flags, Q=Q)


ENCODE = [_enc(B, flags, Q) for B in SWEEP_B for flags in (0, X) for Q in (1, 32, 300)]


def _raw(B, flags, Q, seed, lo=0, hi=255, density=1.0, rare=0.0):
    return dict(name=f"raw_b{B}{'_x' if flags else ''}_q{Q}", kind="raw", B=B, flags=flags, Q=Q, seed=seed, lo=lo, hi=hi,
                density=density, rare=rare)


def _raw300(B, flags, seed):
    """At Q = 300 one index step moves a block's pixels by 300 / B and a wrapping index (|k - 128| >=
    110) clips its whole block, so a dense frame would be all 0 and 255: k is 128 but for a share of
    positions within 3 steps of it (the pixels' standard deviation comes to about 80) and, in about
    one block in 5, one index drawn from the whole range."""
    return _raw(B, flags, 300, seed, 125, 131, 0.006, 0.2 / (3 * B * B))


# Q = 1: every index uniform over 0..255.  Comments: share of the restatement's pixels at 0 or 255
# (at most 0.5: a clipped pixel hides its arithmetic).
RAW = [
    _raw(2, 0, 1, 31),      # saturated 0.2952
    _raw(3, X, 1, 32),      # saturated 0.2953
    _raw(5, 0, 1, 33),      # saturated 0.2907
    _raw(7, X, 1, 34),      # saturated 0.2887
    _raw(11, 0, 1, 35),     # saturated 0.2865
    _raw(13, X, 1, 36),     # saturated 0.2900
    _raw(16, 0, 1, 37),     # saturated 0.2878
    _raw300(2, X, 41),      # saturated 0.1863, 233 indices wrap in int16
    _raw300(3, 0, 42),      # saturated 0.2038, 94
    _raw300(5, X, 43),      # saturated 0.2226, 33
    _raw300(7, 0, 44),      # saturated 0.2402, 22
    _raw300(11, X, 45),     # saturated 0.2154, 5
    _raw300(13, 0, 46),     # saturated 0.1850, 3
    _raw300(16, X, 47),     # saturated 0.2316, 5
]

ENCODE_IDS = [c["name"] for c in ENCODE]
RAW_IDS = [c["name"] for c in RAW]


def by_name(name):
    return [c for c in ENCODE + RAW if c["name"] == name][0]


@functools.lru_cache(maxsize=None)
def frame(B):
    f = K.synth_frame(*FRAME, 200 + B)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def weights(B):
    """float64 (3, D, D): per channel the orthonormal factor of a seeded normal matrix."""
    rng = np.random.Generator(np.random.PCG64(300 + B))
    w = np.stack([np.linalg.qr(rng.normal(size=(B * B, B * B)))[0] for _ in range(3)])
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def weights32(B):
    w = weights(B).astype(np.float32)
    w.setflags(write=False)
    return w


def _frozen(d, keys):
    out = {k: d[k] for k in keys}
    for v in out.values():
        v.setflags(write=False)
    return out


def encode(case, order="fwd"):
    return K.encode(frame(case["B"]), weights(case["B"]), case["B"], case["Q"], case["flags"], order)


def decode(case, k, order="fwd"):
    return K.decode(k, *FRAME, weights32(case["B"]), case["B"], case["Q"], case["flags"], order)


@functools.lru_cache(maxsize=None)
def encoded(name):
    """The restatement's indices, before and after the wrap to u8, and the float64 coefficients."""
    return _frozen(encode(by_name(name)), ("k", "k32", "pre"))


@functools.lru_cache(maxsize=None)
def raw_k(name):
    c = by_name(name)
    shape = K.padded_shape(*FRAME, c["B"])[:2] + (3,)
    rng = np.random.Generator(np.random.PCG64(c["seed"]))
    k = rng.integers(c["lo"], c["hi"] + 1, shape)
    k = np.where(rng.random(shape) < c["density"], k, 128)
    k = np.where(rng.random(shape) < c["rare"], rng.integers(0, 256, shape), k).astype(np.uint8)
    k.setflags(write=False)
    return k


def indices(name):
    return raw_k(name) if "kind" in by_name(name) else encoded(name)["k"]


@functools.lru_cache(maxsize=None)
def decoded(name):
    return _frozen(decode(by_name(name), indices(name)), ("rgb", "pre"))

"""The cases both 2D-LBT sweep test files run (tests/test_lbt.py on the host,
tests/test_lbt_sweep_gpu.py on the GPU), and their references, computed once
per process by the row-wise restatement (tests/lbt_restated.py).

vcf_lbt.hip takes its encode / decode tile and LDS class from the block size
alone, and the moments kernel's chunks and staged tiles from the block size and
the number of blocks; what a frame launches is asked of the library itself
(vcf_lbt_tile_plan) by tests/test_lbt.py.  On the 150 x 210 frame of the sweep
B = 2 .. 8 give 8, 4, 4, 4, 5, 6, 5 encode and decode workgroups per frame, the
last one partial and no whole number of waves every time.

The encoder is a seeded random orthonormal matrix and the decoder its
transpose, not a trained pair: the kernels are handed their weights either way,
and orthonormal rows give indices that use the whole range (the 0.02-std
initial weights would give 128 everywhere).  ENCODE cases are encoded, and the
restatement's indices decoded; RAW cases are index frames no encoder writes.
"""
import functools

import numpy as np

import lbt_restated as R

X = R.NO_SUBBANDS
P = R.PERCEPTUAL
FRAME = (150, 210)
CHUNK_FRAME = (362, 366)     # B = 8: 46 x 46 = 2116 blocks, two moment chunks, 68 blocks in the second
SWEEP_B = (2, 3, 4, 5, 6, 7, 8)
TRAIN_B = (2, 5, 6, 7)       # the block sizes no fixture trains
RAW_MEAN = 3.25


def _suffix(flags):
    return ("_p" if flags & P else "") + ("_x" if flags & X else "")


def _enc(B, flags, Q):
    return dict(name=f"b{B}{_suffix(flags)}_q{Q}", B=B, flags=flags, Q=Q)


ENCODE = [_enc(B, flags, Q) for B in SWEEP_B for flags in (0, X) for Q in (1, 8, 32)]
# -p: B = 8 has the reference's own tables, B = 5 the resized ones (vcf_dct_perceptual_tables)
ENCODE += [_enc(B, flags, 8) for B in (8, 5) for flags in (P, P | X)]


def _raw(B, flags, Q, seed, lo=0, hi=255, density=1.0, rare=0.0):
    return dict(name=f"raw_b{B}{_suffix(flags)}_q{Q}", kind="raw", B=B, flags=flags, Q=Q, seed=seed, lo=lo, hi=hi,
                density=density, rare=rare)


def _raw300(B, flags, seed):
    """The KLT sweep's sparse pattern: at Q = 300 a wrapping index (|k - 128| >= 110) clips its whole
    block, so k is 128 but for 0.6 % of the positions within 3 steps of it and, in about one block in
    5, one index drawn from the whole range."""
    return _raw(B, flags, 300, seed, 125, 131, 0.006, 0.2 / (3 * B * B))


# Q = 1: every index uniform over 0..255.  Comments: share of the restatement's pixels at 0 or 255 (at
# most 0.5: a clipped pixel hides its arithmetic), the pixel-boundary share (at most 0.01) and, at
# Q = 300, the indices that wrap in int16.
RAW = [
    _raw(2, 0, 1, 32),       # saturated 0.2991, boundary 0.0002
    _raw(3, X, 1, 33),       # saturated 0.2925, boundary 0.0006
    _raw(4, 0, 1, 34),       # saturated 0.2910, boundary 0.0009
    _raw(5, X, 1, 35),       # saturated 0.2886, boundary 0.0019
    _raw(6, 0, 1, 36),       # saturated 0.2904, boundary 0.0033
    _raw(7, X, 1, 37),       # saturated 0.2904, boundary 0.0046
    _raw(8, 0, 1, 38),       # saturated 0.2896, boundary 0.0072
    _raw300(2, X, 42),       # saturated 0.1910, 217 indices wrap
    _raw300(3, 0, 43),       # saturated 0.2031, 94
    _raw300(4, X, 44),       # saturated 0.2041, 49
    _raw300(5, 0, 45),       # saturated 0.2138, 30
    _raw300(6, X, 46),       # saturated 0.2213, 22
    _raw300(7, 0, 47),       # saturated 0.2455, 22
    _raw300(8, X, 48),       # saturated 0.2217, 15
    _raw300(8, P, 49),       # -p, the float64 division of a wrapped int16: saturated 0.3355, 14, boundary 0.0005
]

ENCODE_IDS = [c["name"] for c in ENCODE]
RAW_IDS = [c["name"] for c in RAW]


def by_name(name):
    return [c for c in ENCODE + RAW if c["name"] == name][0]


def _ro(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def frame(B):
    return _ro(R.synth_frame(*FRAME, 400 + B))


@functools.lru_cache(maxsize=None)
def chunk_frame():
    return _ro(R.synth_frame(*CHUNK_FRAME, 9))


@functools.lru_cache(maxsize=None)
def orthonormal(D, seed):
    """float32 (D, D): the orthonormal factor of a seeded normal matrix."""
    rng = np.random.Generator(np.random.PCG64(seed))
    return _ro(np.linalg.qr(rng.normal(size=(D, D)))[0].astype(np.float32))


def we(B):
    return orthonormal(B * B, 500 + B)


@functools.lru_cache(maxsize=None)
def wd(B):
    return _ro(np.ascontiguousarray(we(B).T))


@functools.lru_cache(maxsize=None)
def mean(B):
    return R.mean_of(frame(B), B)


def mean_of(case):
    return np.float32(RAW_MEAN) if "kind" in case else mean(case["B"])


@functools.lru_cache(maxsize=None)
def tables(B):
    """-p's uint8 tables for block size B as the library resizes them (host only; tests/test_abi.py
    pins them to the oracle), None at B = 8 where the restatement has the reference's own."""
    if B == 8:
        return None
    import vcf_amd._lib as L
    y, c = np.empty((B, B), np.uint8), np.empty((B, B), np.uint8)
    assert L.lib().vcf_dct_perceptual_tables(B, y.ctypes.data, c.ctypes.data) == 0
    return _ro(y), _ro(c)


def _tables_of(case):
    return tables(case["B"]) if case["flags"] & P else None


def _frozen(d):
    for v in d.values():
        v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def encoded(name):
    """dict(k, pre, mag) of lbt_restated.encode."""
    c = by_name(name)
    return _frozen(R.encode(frame(c["B"]), we(c["B"]), mean(c["B"]), c["B"], c["Q"], c["flags"], _tables_of(c)))


@functools.lru_cache(maxsize=None)
def raw_k(name):
    c = by_name(name)
    shape = R.padded_shape(*FRAME, c["B"])[:2] + (3,)
    rng = np.random.Generator(np.random.PCG64(c["seed"]))
    k = rng.integers(c["lo"], c["hi"] + 1, shape)
    k = np.where(rng.random(shape) < c["density"], k, 128)
    k = np.where(rng.random(shape) < c["rare"], rng.integers(0, 256, shape), k).astype(np.uint8)
    return _ro(k)


def indices(name):
    return raw_k(name) if "kind" in by_name(name) else encoded(name)["k"]


@functools.lru_cache(maxsize=None)
def decoded(name):
    """dict(rgb, pre, mag) of lbt_restated.decode of indices(name)."""
    c = by_name(name)
    return _frozen(R.decode(indices(name), *FRAME, wd(c["B"]), mean_of(c), c["B"], c["Q"], c["flags"], _tables_of(c)))


# ---- short training at the block sizes no fixture has ----------------------
def _distance(a, b):
    return float(max(np.max(np.abs(a[0] - b[0])), np.max(np.abs(a[1] - b[1]))))


def proxy_distance(Xc, we0, wd0, epochs):
    """(float64 restatement's (We, Wd), d_proxy): d_proxy is how far the restatement run in float32
    ends from the one run in float64, the stand-in for a fixture's d_ref."""
    w64 = R.train(Xc, we0, wd0, epochs)
    return w64, _distance(R.train(Xc, we0, wd0, epochs, dtype=np.float32), w64)


@functools.lru_cache(maxsize=None)
def proxy_ratios():
    """name -> d_ref / d_proxy over the 20-epoch fixtures (d_ref: torch's float32 run against the
    float64 restatement, recorded in the manifest)."""
    from test_lbt import SHORT, load
    out = {}
    for case in SHORT:
        z = load(case)
        Xc = R.centred(z["rgb"], case["B"], float(z["mean_ref"])).astype(np.float64)
        out[case["name"]] = case["d_ref"] / proxy_distance(Xc, z["we0"], z["wd0"], case["epochs"])[1]
    return out


def proxy_scale():
    """c: the largest d_ref / d_proxy over the fixtures.  4 x c x d_proxy carries the fixtures'
    4 x d_ref criterion over to a frame that has no torch run."""
    return max(proxy_ratios().values())


@functools.lru_cache(maxsize=None)
def train_frame(B):
    return _ro(R.synth_frame(37, 45, 600 + B))


@functools.lru_cache(maxsize=None)
def trained(B, epochs=20):
    """dict(we, wd (float64 restatement), d_proxy, mean, X) for train_frame(B) from the product's
    initial weights."""
    import vcf_amd.lbt as G
    f = train_frame(B)
    m = R.mean_of(f, B)
    Xc = R.centred(f, B, m).astype(np.float64)
    (w_e, w_d), d = proxy_distance(Xc, *G.initial_weights(B), epochs)
    return dict(we=_ro(w_e), wd=_ro(w_d), d_proxy=d, mean=m, X=_ro(Xc))

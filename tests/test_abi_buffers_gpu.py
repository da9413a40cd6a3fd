"""Pointer alignment and output extents of the transform entry points.

The contract (include/vcf_amd.h, "Alignment and extents"): byte-typed frame
pointers need no alignment; typed pointers need their element's; a call writes
only its documented output extent.  Every row below calls one entry point
through vcf_amd._lib.call with raw pointers into tests/abi_buffers.Guarded
buffers, at the (input, output) offset pairs PAIRS -- in bytes for byte-typed
pointers, in whole elements for typed ones -- and asserts, per pair, equality
with the oracle (or the fixture) that entry point's own test uses, never with
the aligned run, and intact guards on every buffer, inputs included.  Each
typed pointer is also moved one byte off its alignment: VCF_ERR_INVALID, with
every output payload and guard as it was filled.

Which kernel path a shape reaches is said at its row; the dispatch that keeps
a vector path from a pointer that does not allow it is host code
(vcf_dct_dz.hip make_geom / rgb_needs_bytes, vcf_ipp.hip ipp_tss16_kernel's
`words`), so no case here runs a vector access at a misaligned address.
"""
import ctypes
import functools

import numpy as np
import pytest

from abi_buffers import Guarded
from oracle import oracle as O
from oracle import plugins as P
from vcf_amd import _lib
from vcf_amd.device import set_device, synchronize

pytestmark = pytest.mark.gpu

PAIRS = [(0, 0), (1, 0), (0, 1), (3, 5), (4, 8), (8, 4), (2, 2)]
NULL = ctypes.c_void_p(0)


@pytest.fixture(scope="module")
def L():
    set_device(0)
    return _lib


SLACK = 64   # payload bytes past every output's extent, which must keep their fill


class In:
    """An input; elem = the alignment its pointer needs (its item size unless the entry asks for more)."""

    def __init__(self, arr, elem=None):
        self.arr = np.ascontiguousarray(arr)
        self.elem = elem or self.arr.dtype.itemsize


class Out:
    """An output extent of want.nbytes whose bytes must equal `want`, or satisfy cmp(what, got,
    want) where the entry point's own test is not exact; want = a byte count: scratch, guards only."""

    def __init__(self, want, cmp=None, elem=None, zeroed=False):
        self.zeroed = zeroed   # the caller zeroes it (a bad-index flag)
        self.scratch = isinstance(want, int)
        self.want = np.zeros(want, np.uint8) if self.scratch else np.ascontiguousarray(want)
        self.cmp = cmp
        self.elem = elem or self.want.dtype.itemsize


def _run(L, name, ins, outs, args, in_off, out_off, reject=False):
    gi = [Guarded(i.arr.nbytes, in_off[n], i.arr) for n, i in enumerate(ins)]
    go = [Guarded(o.want.nbytes + SLACK, out_off[n]) for n, o in enumerate(outs)]
    for g, o in zip(go, outs):
        if o.zeroed:
            g.upload(np.zeros_like(o.want))
    a = args([g.ptr for g in gi], [g.ptr for g in go])
    what = f"{name} in+{in_off} out+{out_off}"
    if reject:
        with pytest.raises(L.VCFInvalidArgument) as e:
            L.call(name, *a)
        assert e.value.status == L.VCF_ERR_INVALID, what
        synchronize()
        for g in gi + go:
            g.check_untouched(what)
        return
    L.call(name, *a)
    synchronize()
    for g, o in zip(go, outs):
        got = g.download()[:o.want.nbytes]
        if o.cmp is not None:
            o.cmp(what, got.view(o.want.dtype).reshape(o.want.shape), o.want)
        elif not o.scratch:
            bad = np.flatnonzero(got != o.want.view(np.uint8).reshape(-1))
            assert bad.size == 0, f"{what}: {bad.size} output byte(s) differ from the reference, first at {int(bad[0])}"
        g.check_outside([(0, o.want.nbytes)], what)
        g.check(what)
    for g in gi:
        g.check_untouched(what)


def _sweep(L, name, ins, outs, args):
    """The accepted offset pairs, then each typed pointer one byte off its alignment."""
    for oi, oo in PAIRS:
        _run(L, name, ins, outs, args, [oi * i.elem for i in ins], [oo * o.elem for o in outs])
    for n, i in enumerate(ins):
        if i.elem > 1:
            _run(L, name, ins, outs, args, [1 if m == n else 0 for m in range(len(ins))], [0] * len(outs), reject=True)
    for n, o in enumerate(outs):
        if o.elem > 1:
            _run(L, name, ins, outs, args, [0] * len(ins), [1 if m == n else 0 for m in range(len(outs))], reject=True)


def _frames(H, W, seed):
    """Two frames: uniform noise (every index byte busy), and a smooth ramp (the encode's
    zero row pairs and the decode's DC-only waves)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    y, x = np.mgrid[0:H, 0:W]
    ramp = np.stack([(x + y) // 4 + 60, 200 - y // 3, (x // 5) + 90], -1).clip(0, 255).astype(np.uint8)
    return np.stack([rng.integers(0, 256, (H, W, 3), dtype=np.uint8), ramp])


# ---- fused 8x8 DCT (vcf_dct_dz.hip): kTile = 256 blocks per encode workgroup, TB = 32 blocks per
# decode workgroup; the 16-byte copies need nbx % 16 == 0 and k_dev % 16 == 0, the 8-byte RGB words
# H, W % 8 == 0 and rgb_dev % 8 == 0 -- so among PAIRS only offsets 0 and (for RGB) 8 keep a vector path.
DCT8_SHAPES = [
    (8, 8),      # one block: byte copy both ways (nbx = 1)
    (13, 29),    # padded: PAD instantiations, byte copy
    (16, 128),   # nbx = 16, 32 blocks: a partial tile on the 16-byte path of move_runs_tab; decode: partial TB tile, bytes
    (32, 512),   # 256 blocks: one full tile, move_runs_full; decode: two full TB tiles per block row, 16-byte staging
    (40, 512),   # 320 blocks: a full tile (move_runs_full) plus a partial one (move_runs_tab, 16-byte)
    (8, 256),    # decode: nbx = 32, exactly one whole TB tile
    (8, 384),    # decode: nbx = 48, a whole TB tile plus one of 16 blocks (byte staging)
]


@functools.lru_cache(maxsize=None)
def _dct8_ref(H, W, Q, flags):
    fr = _frames(H, W, H * 1000 + W)
    k = np.stack([O.encode_frame(f, Q, flags) for f in fr])
    y = np.stack([O.decode_frame(kk, H, W, Q, flags) for kk in k])
    return fr, k, y


@pytest.mark.parametrize("H,W", DCT8_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("flags", [0, 1, 2], ids=["sub", "x", "p"])
@pytest.mark.parametrize("Q", [32, 7])
def test_dct8_encode_and_decode(L, H, W, flags, Q):
    fr, k, y = _dct8_ref(H, W, Q, flags)
    _sweep(L, "vcf_dct_dz_encode", [In(fr)], [Out(k)], lambda i, o: (i[0], 2, H, W, 8, Q, flags, o[0], NULL))
    _sweep(L, "vcf_dct_dz_decode", [In(k)], [Out(y)], lambda i, o: (i[0], 2, H, W, 8, Q, flags, o[0], NULL))


# ---- generic-B DCT (vcf_dct_any.hip): byte loads and stores of the u8 frames throughout; B = 4 has a
# compiled plan, B = 7 a run-time one; 13 x 29 pads for both, 28 x 28 for neither.
@pytest.mark.parametrize("H,W", [(13, 29), (28, 28)], ids=lambda v: str(v))
@pytest.mark.parametrize("B", [4, 7])
def test_dct_any_k32_raw(L, B, H, W):
    fr = _frames(H, W, B * 100 + H)
    for flags in (0, 1):
        k = np.stack([O.encode_frame_b(f, B, 7, flags) for f in fr])
        y = np.stack([O.decode_frame_b(kk, H, W, B, 7, flags) for kk in k])
        _sweep(L, "vcf_dct_dz_encode_any", [In(fr)], [Out(k)], lambda i, o: (i[0], 2, H, W, B, 7, flags, o[0], NULL))
        _sweep(L, "vcf_dct_dz_decode_any", [In(k)], [Out(y)], lambda i, o: (i[0], 2, H, W, B, 7, flags, o[0], NULL))
    k32 = np.stack([O.encode_frame_b(f, B, 7, 0, k32=True) for f in fr])
    assert k32.dtype == np.int32
    y32 = np.stack([O.decode_frame_b(kk, H, W, B, 7, 0) for kk in k32])
    _sweep(L, "vcf_dct_dz_encode_k32", [In(fr)], [Out(k32)], lambda i, o: (i[0], 2, H, W, B, 7, 0, o[0], NULL))
    _sweep(L, "vcf_dct_dz_decode_k32", [In(k32)], [Out(y32)], lambda i, o: (i[0], 2, H, W, B, 7, 0, o[0], NULL))
    c = np.stack([O.dct_raw_encode_b(f, B, 0) for f in fr])
    assert c.dtype == np.float32
    c16 = np.clip(np.trunc(c / 3), -32768, 32767).astype(np.int16)   # what another quantizer hands back
    yr = np.stack([O.dct_raw_decode_b(cc, H, W, B, 0) for cc in c16])
    _sweep(L, "vcf_dct_raw_encode", [In(fr)], [Out(c)], lambda i, o: (i[0], 2, H, W, B, 0, o[0], NULL))
    _sweep(L, "vcf_dct_raw_decode", [In(c16)], [Out(yr)], lambda i, o: (i[0], 2, H, W, B, 0, o[0], NULL))


# ---- lapped 2D-MDCT (vcf_mdct_dz.hip): byte loads and stores; the reference frames' fixtures, B = 8:
# 37 x 45 (padded, subbands) and 40 x 48 -x.
@pytest.mark.parametrize("case", ["smooth_37x45", "rand_40x48_x"])
def test_mdct(L, case):
    from test_mdct import CASES, load, params
    c = [c for c in CASES if c["name"] == case][0]
    z = load(c)
    B, Q, fl = params(c)
    assert B == 8
    H, W = z["rgb"].shape[:2]
    rgb, k, y = (np.stack([z[n], z[n]]) for n in ("rgb", "k", "decoded"))
    _sweep(L, "vcf_mdct_dz_encode", [In(rgb)], [Out(k)], lambda i, o: (i[0], 2, H, W, B, Q, fl, o[0], NULL))
    _sweep(L, "vcf_mdct_dz_decode", [In(k)], [Out(y)], lambda i, o: (i[0], 2, H, W, B, Q, fl, o[0], NULL))


# ---- IPP (vcf_ipp.hip).  bs 16 / sr 8 on 64 x 64: the full search on words (LDS words built from
# bytes) and, fast, ipp_tss16_kernel, whose block (1, 1) is the one with its window inside the frame:
# whole words from the luma plane when the gray workspace is 4-byte aligned, bytes when it is not.
# bs 7 / sr 3 on 33 x 35: the byte kernels, pixels outside the full-block area.
def _moving(H, W, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    base = rng.integers(0, 256, (H + 8, W + 8, 3)).astype(np.float64)
    for _ in range(2):   # smooth enough for the search to have a gradient
        base = (base + np.roll(base, 1, 0) + np.roll(base, 1, 1) + np.roll(base, (1, 1), (0, 1))) / 4
    ref = base[4:4 + H, 4:4 + W]
    cur = base[2:2 + H, 5:5 + W] + rng.integers(-3, 4, (H, W, 3))
    return ref.clip(0, 255).astype(np.uint8), cur.clip(0, 255).astype(np.uint8)


@pytest.mark.parametrize("H,W,bs,sr", [(64, 64, 16, 8), (33, 35, 7, 3)])
def test_ipp(L, H, W, bs, sr):
    ref, cur = _moving(H, W, H + bs)
    gray = np.stack([O.ipp_gray(ref), O.ipp_gray(cur)])
    for fast in (0, 1):
        mv = O.ipp_block_matching(ref, cur, bs, sr, bool(fast))
        assert np.any(mv != 0)
        _sweep(L, "vcf_ipp_block_match", [In(ref), In(cur)], [Out(mv), Out(gray)],
               lambda i, o: (i[0], i[1], H, W, bs, sr, fast, o[0], o[1], NULL))
    comp = O.ipp_motion_compensate(ref, mv, bs)
    _sweep(L, "vcf_ipp_motion_compensate", [In(ref), In(mv)], [Out(comp)],
           lambda i, o: (i[0], i[1], H, W, bs, o[0], NULL))
    n = H * W * 3
    res = O.ipp_residual(cur, comp)
    _sweep(L, "vcf_ipp_residual", [In(cur), In(comp)], [Out(res)], lambda i, o: (i[0], i[1], n, o[0], NULL))
    _sweep(L, "vcf_ipp_reconstruct", [In(comp), In(res)], [Out(O.ipp_reconstruct(comp, res))],
           lambda i, o: (i[0], i[1], n, o[0], NULL))


# ---- IPP block RDO (vcf_ipp_rdo.hip), bs 8 on 21 x 26: byte loads of the frames, one wave per full
# block, pixels outside the full blocks; the float64 costs are the typed pointer.
def test_ipp_rdo(L):
    H, W, bs, Q, lam = 21, 26, 8, 32, 0.5
    cur, comp = _moving(H, W, 77)
    m, c = O.ipp_rdo_modes(cur, comp, bs, Q, lam, with_costs=True)
    m, c = np.ascontiguousarray(m, np.uint8), np.ascontiguousarray(c, np.float64)
    _sweep(L, "vcf_ipp_rdo_modes", [In(cur), In(comp)], [Out(m), Out(c)],
           lambda i, o: (i[0], i[1], H, W, bs, Q, ctypes.c_double(lam), o[0], o[1], NULL))
    m[0, 1] ^= 1   # both modes present whatever the decision was
    res = O.ipp_rdo_residual(cur, comp, m, bs)
    _sweep(L, "vcf_ipp_rdo_residual", [In(cur), In(comp), In(m)], [Out(res)],
           lambda i, o: (i[0], i[1], i[2], H, W, bs, o[0], NULL))
    _sweep(L, "vcf_ipp_rdo_reconstruct", [In(comp), In(res), In(m)], [Out(O.ipp_rdo_reconstruct(comp, res, m, bs))],
           lambda i, o: (i[0], i[1], i[2], H, W, bs, o[0], NULL))


# ---- pixel codecs (vcf_plugins.hip), 67 x 131 x 3: the kernels take 4 pixels (12 bytes) or 16 bytes
# per lane on words where the address allows (offsets 0, 4, 8 here) and bytes elsewhere and in the
# tail (26331 bytes = 16 * 1645 + 11).
def test_pixel_codecs(L):
    rng = np.random.Generator(np.random.PCG64(5))
    rgb = rng.integers(0, 256, (67, 131, 3), dtype=np.uint8)
    npx, n = 67 * 131, 67 * 131 * 3
    ycc = P.ycrcb_from_rgb(rgb)
    _sweep(L, "vcf_ycrcb_from_rgb", [In(rgb)], [Out(ycc)], lambda i, o: (i[0], npx, o[0], NULL))
    _sweep(L, "vcf_ycrcb_to_rgb", [In(ycc)], [Out(P.ycrcb_to_rgb(ycc))], lambda i, o: (i[0], npx, o[0], NULL))
    k16 = np.ascontiguousarray(P.ycrcb_dz_encode(rgb, 5), np.uint16)
    _sweep(L, "vcf_ycrcb_dz_encode", [In(rgb)], [Out(k16)], lambda i, o: (i[0], npx, 5, o[0], NULL))
    _sweep(L, "vcf_ycrcb_dz_decode", [In(k16)], [Out(P.ycrcb_dz_decode(k16, 5))], lambda i, o: (i[0], npx, 5, o[0], NULL))
    k8 = P.dz_u8_encode(rgb, 5)
    _sweep(L, "vcf_dz_u8_encode", [In(rgb)], [Out(k8)], lambda i, o: (i[0], n, 5, o[0], NULL))
    _sweep(L, "vcf_dz_u8_decode", [In(k8)], [Out(P.dz_u8_decode(k8, 5))], lambda i, o: (i[0], n, 5, o[0], NULL))


# ---- 2D-DWT (vcf_dwt.hip and its level kernels), bior4.4, l = 2.  rgb_dev, packed_dev and
# workspace_dev must be 16-byte aligned (include/vcf_amd.h), so every pointer here moves in steps of
# 16 bytes and is rejected one byte off.  24 x 32: subband widths 16 and 8, hw * 3 % 4 == 0, the
# dword copy-out eligible; 26 x 30: widths 15 and 8, byte copy-out.  Two frames: 24 x 32 packs to an
# even frame size, 26 x 30 to 2595 bytes, so its frame 1 starts at an odd address and its packed LL
# band takes the byte form of load_u16_le / buffer_store_u16_le.
def _within_one(unpack):
    def cmp(what, got, want):
        for f in range(want.shape[0]):
            for name, (g, w) in unpack(got[f], want[f]).items():
                d = g.astype(np.int64) - w.astype(np.int64)
                if name is not None and not name.startswith("LL"):
                    d = (d + 128) % 256 - 128   # u8 indices wrap
                assert np.abs(d).max(initial=0) <= 1, f"{what} {name}: off by {np.abs(d).max()}"
    return cmp


@pytest.mark.parametrize("H,W", [(24, 32), (26, 30)], ids=lambda v: str(v))
def test_dwt(L, H, W):
    import vcf_amd.dwt as DW
    wv, lv, Q = "bior4.4", 2, 32
    _, pb, wb = DW.layout(H, W, lv)
    fr = _frames(H, W, H * 7 + W)
    sub = [O.dwt_encode_frame(f, wv, lv, Q) for f in fr]
    packed = np.stack([DW.pack(x, H, W, lv) for x in sub])
    assert packed.shape == (2, pb) and (pb % 2 == 1) == ((H, W) == (26, 30))
    y = np.stack([O.dwt_decode_frame(x, H, W, wv, lv, Q) for x in sub])
    wi = DW.wavelet_index(wv)
    enc = lambda i, o: (i[0], 2, H, W, wi, lv, Q, o[0], o[1], NULL)
    _sweep(L, "vcf_dwt_dz_encode", [In(fr, 16)], [Out(packed, elem=16), Out(2 * wb, elem=16)], enc)
    _sweep(L, "vcf_dwt_dz_decode", [In(packed, 16)], [Out(y, elem=16), Out(2 * wb, elem=16)], enc)
    # the lifting form: within one index / one byte of the exact form (tests/test_dwt_lift_gpu.py)
    idx = _within_one(lambda g, w: {n: (DW.unpack(g, H, W, lv)[n], v) for n, v in DW.unpack(w, H, W, lv).items()})
    pix = _within_one(lambda g, w: {None: (g, w)})
    _sweep(L, "vcf_dwt_dz_encode_lift", [In(fr, 16)], [Out(packed, idx, 16), Out(2 * wb, elem=16)], enc)
    _sweep(L, "vcf_dwt_dz_decode_lift", [In(packed, 16)], [Out(y, pix, 16), Out(2 * wb, elem=16)], enc)


# ---- 2D-KLT (vcf_klt_dz.hip, staging of vcf_block_tile.h), B = 4 on 13 x 29 (padded, 32 blocks: one
# partial tile): byte loads and stores of the frames; the int64 moments and the float64 / float32
# weights are the typed pointers.  Moments exact; indices and pixels by test_klt_gpu._compare.
def test_klt(L):
    import klt_restated as K
    import klt_sweep_cases as S
    from test_klt_gpu import _compare
    H, W, B, Q = 13, 29, 4, 32
    D = B * B
    fr = np.stack([K.synth_frame(H, W, 5), K.synth_frame(H, W, 6)])
    m = [K.moments(f, B) for f in fr]
    s1, s2 = np.stack([a for a, _ in m]), np.stack([b for _, b in m])
    assert s1.shape == (2, 3, D) and s1.dtype == np.int64
    _sweep(L, "vcf_klt_moments", [In(fr)], [Out(s1), Out(s2)], lambda i, o: (i[0], 2, H, W, B, o[0], o[1], NULL))
    w64, w32 = np.stack([S.weights(B)] * 2), np.stack([S.weights32(B)] * 2)
    for flags in (0, K.NO_SUBBANDS):
        e = [K.encode(f, w64[0], B, Q, flags) for f in fr]
        k = np.stack([x["k"] for x in e])
        im = np.stack([K.index_margin(x["pre"], Q) for x in e])
        _sweep(L, "vcf_klt_dz_encode", [In(fr), In(w64)], [Out(k, lambda what, g, w: _compare(what, g, w, im))],
               lambda i, o: (i[0], 2, H, W, B, Q, flags, i[1], o[0], NULL))
        d = [K.decode(kk, H, W, w32[0], B, Q, flags) for kk in k]
        pm = np.stack([K.pixel_margin(x["pre"]) for x in d])
        _sweep(L, "vcf_klt_dz_decode", [In(k), In(w32)],
               [Out(np.stack([x["rgb"] for x in d]), lambda what, g, w: _compare(what, g, w, pm))],
               lambda i, o: (i[0], 2, H, W, B, Q, flags, i[1], o[0], NULL))


# ---- 2D-LBT (vcf_lbt.hip, staging of vcf_block_tile.h), B = 8 on 13 x 29 (padded to 16 x 32, 8 blocks:
# one partial tile, one moments chunk): byte loads and stores of the frames; the float64 moments and the
# float32 matrices and means are the typed pointers.  Moments exact (every partial sum is a multiple of
# 1/16 below 2^53); indices and pixels by test_lbt_gpu's criteria: equal to the restatement off the
# boundary set, one step on it.
def test_lbt(L):
    import lbt_restated as R
    import lbt_sweep_cases as S
    from test_lbt_gpu import _check_indices, _check_pixels
    H, W, B, Q = 13, 29, 8, 32
    D = B * B
    fr = np.stack([R.synth_frame(H, W, 7), R.synth_frame(H, W, 8)])
    X = [R.blocks(f, B).astype(np.float64) for f in fr]
    s1, s2 = np.stack([x.sum(0) for x in X]), np.stack([x.T @ x for x in X])
    assert s1.shape == (2, D) and s2.shape == (2, D, D) and s1.dtype == np.float64
    _sweep(L, "vcf_lbt_moments", [In(fr)], [Out(s1), Out(s2)], lambda i, o: (i[0], 2, H, W, B, o[0], o[1], NULL))
    we = np.stack([S.we(B), np.ascontiguousarray(S.we(B)[::-1])]).astype(np.float32)
    wd = np.ascontiguousarray(we.transpose(0, 2, 1))
    mean = np.array([R.mean_of(f, B) for f in fr], np.float32)
    for flags in (0, R.NO_SUBBANDS):
        e = [R.encode(fr[f], we[f], mean[f], B, Q, flags) for f in range(2)]
        k = np.stack([x["k"] for x in e])

        def idx(what, g, w, e=e):
            for f in range(2):
                _check_indices(g[f], e[f], D)
        _sweep(L, "vcf_lbt_dz_encode", [In(fr), In(we), In(mean)], [Out(k, idx)],
               lambda i, o: (i[0], 2, H, W, B, Q, flags, i[1], i[2], o[0], NULL))
        d = [R.decode(k[f], H, W, wd[f], mean[f], B, Q, flags) for f in range(2)]

        def pix(what, g, w, d=d):
            for f in range(2):
                _check_pixels(g[f], d[f], D, d[f]["rgb"])
        _sweep(L, "vcf_lbt_dz_decode", [In(k), In(wd), In(mean)], [Out(np.stack([x["rgb"] for x in d]), pix)],
               lambda i, o: (i[0], 2, H, W, B, Q, flags, i[1], i[2], o[0], NULL))


# ---- VQ (vcf_vq.hip): byte loads of the image, the centroids through LDS; D = 12 (2 x 2 x 3) and
# D = 3 (1 x 1 x 3), K = 5.  Labels, distances, sums, counts and the decoded image exact
# (tests/vq_restated.py restates the arithmetic bit for bit).
@pytest.mark.parametrize("BS", [2, 1])
def test_vq(L, BS):
    import vq_restated as R
    H, W, C, K = 10, 14, 3, 5
    rng = np.random.Generator(np.random.PCG64(40 + BS))
    img = rng.integers(0, 256, (H, W, C), dtype=np.uint8)
    X = R.blocks(img, BS)
    cent = np.ascontiguousarray(X[:K].astype(np.float64) + rng.normal(size=(K, X.shape[1])))
    labels, best, _ = R.assign(X, cent)
    _sweep(L, "vcf_vq_assign", [In(img), In(cent)], [Out(labels), Out(best)],
           lambda i, o: (i[0], H, W, C, BS, i[1], K, o[0], o[1], NULL))
    sums, counts = R.accumulate(X, labels, K)
    _sweep(L, "vcf_vq_accumulate", [In(img), In(labels)], [Out(sums), Out(counts)],
           lambda i, o: (i[0], H, W, C, BS, i[1], K, o[0], o[1], NULL))
    lab2 = labels.reshape(H // BS, W // BS)
    _sweep(L, "vcf_vq_decode", [In(lab2), In(cent)], [Out(R.decode(lab2, cent, BS, C)), Out(np.zeros(1, np.int32), zeroed=True)],
           lambda i, o: (i[0], H // BS, W // BS, C, BS, i[1], K, o[0], o[1], NULL))


# ---- the rest of the pixel codecs and quantizers on 67 x 131 x 3 (vcf_plugins.hip, vcf_quant.hip):
# one element per lane through pointers of the element type.
def test_ycocg_lloydmax_deadzone(L):
    rng = np.random.Generator(np.random.PCG64(6))
    rgb = rng.integers(0, 256, (67, 131, 3), dtype=np.uint8)
    npx, n = 67 * 131, 67 * 131 * 3
    k16 = np.ascontiguousarray(P.ycocg_dz_encode(rgb, 5), np.uint16)
    _sweep(L, "vcf_ycocg_dz_encode", [In(rgb)], [Out(k16)], lambda i, o: (i[0], npx, 5, o[0], NULL))
    _sweep(L, "vcf_ycocg_dz_decode", [In(k16)], [Out(P.ycocg_dz_decode(k16, 5))], lambda i, o: (i[0], npx, 5, o[0], NULL))
    y16 = np.ascontiguousarray(P.ycocg_i16(rgb), np.int16)
    _sweep(L, "vcf_ycocg_i16_from_rgb", [In(rgb)], [Out(y16)], lambda i, o: (i[0], npx, 0, o[0], NULL))
    _sweep(L, "vcf_ycocg_i16_to_rgb", [In(y16)], [Out(P.ycocg_i16_to_rgb(y16))], lambda i, o: (i[0], npx, 0, o[0], NULL))
    # LloydMax on the u8 image, range 0..255, Q = 16: counts channel-major int64, indices u8, levels u8
    counts = np.stack([P.histogram(rgb[..., c], 0, 255) for c in range(3)]).astype(np.int64)
    _sweep(L, "vcf_lm_histogram", [In(rgb)], [Out(counts)],
           lambda i, o: (i[0], _lib.VCF_DTYPE_U8, npx, 3, 0, 255, o[0], NULL))
    k, cents = P.lm_quantize(rgb, 16, 0, 255)
    cd = np.ascontiguousarray(np.stack(cents), np.float64)
    N = cd.shape[1]
    _sweep(L, "vcf_lm_encode", [In(rgb), In(cd)], [Out(k)],
           lambda i, o: (i[0], _lib.VCF_DTYPE_U8, npx, 3, i[1], N, o[0], _lib.VCF_DTYPE_U8, NULL))
    _sweep(L, "vcf_lm_decode", [In(k), In(cd)], [Out(P.lm_dequantize(k, cents)), Out(np.zeros(1, np.int32), zeroed=True)],
           lambda i, o: (i[0], _lib.VCF_DTYPE_U8, npx, 3, i[1], N, o[0], _lib.VCF_DTYPE_U8, o[1], NULL))
    # the deadzone quantizer plug-in: int16 coefficients -> int32 indices -> int16 values (numpy's wrap)
    x = rng.integers(-3000, 3000, n).astype(np.int16)
    k32 = (x / 7).astype(np.int32)
    _sweep(L, "vcf_deadzone_quantize", [In(x)], [Out(k32)], lambda i, o: (i[0], _lib.VCF_DTYPE_I16, n, 7, o[0], NULL))
    ki = k32.astype(np.int16)
    _sweep(L, "vcf_deadzone_dequantize", [In(ki)], [Out((np.int16(7) * ki).astype(np.int16))],
           lambda i, o: (i[0], _lib.VCF_DTYPE_I16, n, 7, o[0], NULL))

"""The four GPU decoders on input that none of the project's encoders produces
(tests/decoder_inputs.py; its host-side checks are tests/test_decoder_inputs.py).

- Inflate (csrc/vcf_inflate.hip): status 0 exactly where zlib accepts the
  strip at its declared length, the bytes zlib gives, each hand-built class
  its own status, and no byte written outside a strip's span -- accepted or
  rejected -- by the product kernel and by the window-check build, which also
  counts no ring read outside the valid span on any accepted strip.
- Tiled CBAAC (csrc/vcf_cbaac_gpu.hip): the wave and the lane decoder equal
  the host decoders, segment by segment, on valid, truncated, bit-flipped,
  random and constant payloads.
- DCT decode (csrc/vcf_dct_dz.hip, vcf_dct_any.hip) and DWT decode
  (csrc/vcf_dwt*.hip) on arbitrary index values, where the reference's int16
  arithmetic wraps: equal to the oracle, every product variant.
"""
import functools

import numpy as np
import pytest

import decoder_inputs as DI
from oracle import oracle as O
from test_decoder_inputs import host_decode, host_encode

pytestmark = pytest.mark.gpu

# ---- inflate ----------------------------------------------------------------------------

_LAUNCH = 2000    # strips per launch
_GAP = 64         # bytes kept between two strips' output spans
_FILL = 0xA5


@functools.lru_cache(maxsize=None)
def _inflated(wincheck):
    """The whole corpus through vcf_inflate_strips (or the window-check build),
    called as StripInflater.inflate_into calls it, in launches of at most
    _LAUNCH strips.  Every launch's outputs share one buffer pre-filled with
    0xA5, strip starts at offsets = 1, 2, 3 (mod 16) with at least _GAP bytes
    between spans.  -> (status per strip, output bytes per strip, names of the
    strips with a changed byte in the gap before or after them, violations)."""
    from vcf_amd import _lib as L
    from vcf_amd.device import DeviceBuffer
    corpus = DI.inflate_corpus()
    status, outs, dirty, viols = [], [], [], []
    for s0 in range(0, len(corpus), _LAUNCH):
        part = corpus[s0:s0 + _LAUNCH]
        n = len(part)
        comp = np.frombuffer(b"".join(e[1] for e in part), np.uint8)
        comp_len = np.array([len(e[1]) for e in part], np.int32)
        comp_off = (np.cumsum(comp_len, dtype=np.int64) - comp_len).astype(np.int64)
        out_len = np.array([e[2] for e in part], np.int32)
        out_off = np.empty(n, np.int64)
        pos = 0
        for i in range(n):
            pos = (pos + _GAP + 15) // 16 * 16 + 1 + i % 3
            out_off[i] = pos
            pos += int(out_len[i])
        total = pos + _GAP
        assert (comp_off + comp_len <= comp.size).all() and (out_off + out_len + _GAP <= total).all()
        bufs = [DeviceBuffer.from_array(a) for a in (comp, comp_off, comp_len, out_off, out_len)]
        dc, dco, dcl, doo, dol = bufs
        dout = DeviceBuffer.from_array(np.full(total, _FILL, np.uint8))
        dst = DeviceBuffer.from_array(np.full(n, 12345, np.int32))
        bufs += [dout, dst]
        if wincheck:
            dv = DeviceBuffer.from_array(np.full(n, 0xFFFFFFFF, np.uint32))
            bufs.append(dv)
            L.call_ab("vcf_inflate_strips_wincheck", dc.ptr, dco.ptr, dcl.ptr, n, dout.ptr, doo.ptr, dol.ptr, dst.ptr,
                      dv.ptr, None)
            viols.append(dv.download(np.empty(n, np.uint32)))
        else:
            L.call("vcf_inflate_strips", dc.ptr, dco.ptr, dcl.ptr, n, dout.ptr, doo.ptr, dol.ptr, dst.ptr, None)
        status.append(dst.download(np.empty(n, np.int32)))
        host = dout.download(np.empty(total, np.uint8))
        for b in bufs:
            b.free()
        span = np.zeros(total, bool)
        for o, ln in zip(out_off, out_len):
            span[o:o + ln] = True
        bad = np.nonzero(~span & (host != _FILL))[0]
        for p in bad[:50]:                      # name the strips on either side of a changed gap byte
            i = int(np.searchsorted(out_off, p, side="right")) - 1
            dirty.append((part[max(i, 0)][0], int(p - out_off[max(i, 0)])))
        outs += [host[o:o + ln].tobytes() for o, ln in zip(out_off, out_len)]
    return np.concatenate(status), outs, dirty, (np.concatenate(viols) if wincheck else None)


@pytest.mark.parametrize("wincheck", [False, True], ids=["product", "wincheck"])
def test_inflate_accepts_exactly_what_zlib_accepts(wincheck):
    corpus = DI.inflate_corpus()
    status, outs, _, _ = _inflated(wincheck)
    wrong = [(e[0], int(s)) for e, s in zip(corpus, status) if (s == 0) != (e[3] is not None)]
    assert not wrong, (len(wrong), wrong[:20])
    differ = [e[0] for e, s, o in zip(corpus, status, outs) if e[3] is not None and o != e[3]]
    assert not differ, (len(differ), differ[:20])


@pytest.mark.parametrize("wincheck", [False, True], ids=["product", "wincheck"])
def test_inflate_writes_only_inside_each_strip(wincheck):
    """Every byte between two strips' spans still holds the fill, around
    accepted and rejected strips alike."""
    dirty = _inflated(wincheck)[2]
    assert not dirty, dirty[:20]


@pytest.mark.parametrize("wincheck", [False, True], ids=["product", "wincheck"])
def test_inflate_status_of_hand_built_streams(wincheck):
    names = [e[0] for e in DI.inflate_corpus()]
    status = _inflated(wincheck)[0]
    got = {n: int(status[names.index(n)]) for n in DI.hand_status()}
    assert got == DI.hand_status()


def test_inflate_window_check_counts_no_violation():
    corpus = DI.inflate_corpus()
    status, _, _, viol = _inflated(True)
    assert np.array_equal(status, _inflated(False)[0])
    bad = [e[0] for e, s, v in zip(corpus, status, viol) if s == 0 and v != 0]
    assert not bad, (len(bad), bad[:20])


# ---- tiled CBAAC ------------------------------------------------------------------------

@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("seg_len", [256, 4096])
def test_cbaac_decoders_equal_host_on_any_bytes(order, seg_len):
    from vcf_amd import tcbaac as T
    entries = DI.cbaac_payloads(host_encode, order, seg_len)
    want = [host_decode(e) for e in entries]
    for variant in (1, 2) if order == 0 else (1,):     # one wave / one lane (order 0) per segment
        coder = T.TiledCoder(order, seg_len, kernel=variant)
        for e, w in zip(entries, want):
            kind, _, _, n, prior, seg_bytes, payload, _ = e
            got = coder.decode(payload, seg_bytes, n, prior)
            rows = 0 if prior is None else prior.shape[0] if prior.ndim == 2 else 1
            assert np.array_equal(got, w), (variant, kind, n, rows, np.nonzero(got != w)[0][:5])


@pytest.mark.parametrize("variant", [1, 2])
def test_cbaac_batched_decode_on_any_bytes(variant):
    """vcf_cbaac_tiled_decode_classes over six frames of different payload
    kinds, outputs at an unaligned stride: every frame as decoded alone."""
    from vcf_amd import _lib as L
    from vcf_amd.device import DeviceBuffer
    n, seg, kinds = 10001, 256, ("valid", "half", "bitflip", "random", "zeros", "ones")
    entries = [e for e in DI.cbaac_payloads(host_encode, 0, seg)
               if e[3] == n and e[4] is not None and e[4].ndim == 2 and e[0] in kinds]
    assert [e[0] for e in entries] == list(kinds)
    F, ns, stride = len(entries), (n + seg - 1) // seg, n + 3
    offs, base = [], 0
    for e in entries:
        offs.append(np.concatenate([[0], np.cumsum(e[5])]) + base)
        base += len(e[6])
    offs = np.concatenate(offs).astype(np.int64)
    assert offs.size == F * (ns + 1) and base == offs[-1]
    priors = np.stack([e[4] for e in entries]).astype(np.uint16)
    src, doffs, dpr = (DeviceBuffer.from_array(np.frombuffer(b"".join(e[6] for e in entries), np.uint8)),
                       DeviceBuffer.from_array(offs), DeviceBuffer.from_array(priors))
    out = DeviceBuffer.from_array(np.full(F * stride, _FILL, np.uint8))
    L.call_ab("vcf_cbaac_tiled_decode_classes_variant", variant, src.ptr, doffs.ptr, F, n, 0, dpr.ptr, priors.shape[1],
              seg, out.ptr, stride, None)
    got = out.download(np.empty(F * stride, np.uint8)).reshape(F, stride)
    for f, e in enumerate(entries):
        assert np.array_equal(got[f, :n], host_decode(e)), e[0]
    assert (got[:, n:] == _FILL).all()          # the bytes between two frames' outputs


# ---- DCT decode ---------------------------------------------------------------------------

_DCT_Q = (1, 7, 32, 64, 255, 256, 30001, 32767)


@pytest.mark.parametrize("shape", [(8, 8), (13, 29), (72, 136), (24, 4104)])
def test_dct_decode_variants_on_any_indices(shape):
    """Variants 0 (dequantization table), 1 (lane per block) and 2 (32-bit
    multiply) on every index class, the six classes as one batch per call."""
    import vcf_amd.dct as D
    H, W = shape
    Hp, Wp = D.padded_shape(H, W)
    for flags in range(4):
        for Q in _DCT_Q:
            k = DI.dct_index_frames(Hp, Wp, H * W + 8 * Q + flags)
            want = np.stack([O.decode_frame(f, H, W, Q, flags) for f in k])
            for v in (0, 1, 2):
                got = D.decode(k, H, W, Q, flags, variant=v)
                bad = [c for c, g, w in zip(DI.PLANE_CLASSES, got, want) if not np.array_equal(g, w)]
                assert not bad, (flags, Q, v, bad)


def test_dct_decode_mixed_batch_equals_single_frames():
    import vcf_amd.dct as D
    H, W, Q = 72, 136, 255
    k = DI.dct_index_frames(H, W, 77)[[0, 2, 1, 4, 3]]      # uniform, zeros, edges, smooth, max
    for v in (0, 1, 2):
        got = D.decode(k, H, W, Q, 0, variant=v)
        for f in range(5):
            assert np.array_equal(got[f], D.decode(k[f], H, W, Q, 0, variant=v)), (v, f)
            assert np.array_equal(got[f], O.decode_frame(k[f], H, W, Q, 0)), (v, f)


@pytest.mark.parametrize("B", [4, 7, 16])
def test_dct_decode_any_block_size_on_any_indices(B):
    import vcf_amd.dct as D
    H, W = 53, 91
    Hp, Wp = D.padded_shape(H, W, B)
    for flags in (0, 1):
        for Q in (1, 64, 30001):
            k = DI.dct_index_frames(Hp, Wp, B * 1000 + Q + flags)
            got = D.decode(k, H, W, Q, flags, block_size=B)
            for c, g, f in zip(DI.PLANE_CLASSES, got, k):
                assert np.array_equal(g, O.decode_frame_b(f, H, W, B, Q, flags)), (flags, Q, c)


# ---- DWT decode ---------------------------------------------------------------------------

def _unfused(DW, *a):
    """DW.decode with the inverse levels 2 + 1 as two line-kernel launches."""
    return DW.decode(*a, schedule={"band21": 0})


@pytest.mark.parametrize("wavelet", ["bior4.4", "db5"])
@pytest.mark.parametrize("H,W,levels", [(40, 40, 2), (44, 60, 3), (90, 140, 3), (96, 136, 2), (200, 480, 4),
                                        (20, 1030, 2)])
def test_dwt_decode_paths_on_any_indices(wavelet, H, W, levels):
    """Arbitrary LL (u16) and detail (u8) values in place of the encoder's
    (every class on all bands, and sets whose LL and details differ):
    the default path, the two-launch path, the tiled kernels (17) and the
    separable kernels (2) equal the oracle."""
    import vcf_amd.dwt as DW
    shapes = O.dwt_shapes(H, W, levels)
    for Q in (1, 32, 300):
        sets = DI.dwt_subband_sets(shapes, levels, H * W + Q)
        want = np.stack([O.dwt_decode_frame(s, H, W, wavelet, levels, Q) for s in sets])
        paths = (("default", DW.decode(sets, H, W, wavelet, levels, Q)),
                 ("unfused", _unfused(DW, sets, H, W, wavelet, levels, Q)),
                 ("tiled", DW.decode(sets, H, W, wavelet, levels, Q, variant=17)),
                 ("separable", DW.decode(sets, H, W, wavelet, levels, Q, variant=2)))
        for name, got in paths:
            assert len(got) == len(want) == len(DI.DWT_SET_NAMES)
            bad = [c for c, g, w in zip(DI.DWT_SET_NAMES, got, want) if not np.array_equal(g, w)]
            assert not bad, (Q, name, bad)


@pytest.mark.parametrize("H,W,levels", [(23, 2, 2), (67, 45, 2)])
def test_dwt_decode_20_taps_on_any_indices(H, W, levels):
    import vcf_amd.dwt as DW
    shapes = O.dwt_shapes(H, W, levels)
    for Q in (1, 32, 300):
        sets = DI.dwt_subband_sets(shapes, levels, H * W + Q)
        for v in (0, 2):                                    # the automatic choice and the separable kernels
            got = DW.decode(sets, H, W, "db10", levels, Q, variant=v)
            assert len(got) == len(sets) == len(DI.DWT_SET_NAMES)
            for c, g, s in zip(DI.DWT_SET_NAMES, got, sets):
                assert np.array_equal(g, O.dwt_decode_frame(s, H, W, "db10", levels, Q)), (Q, v, c)

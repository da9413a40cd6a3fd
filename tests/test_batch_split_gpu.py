"""Every batched kernel across its launch split, and the any-B decode across its workspace chunks.

The launchers put frames (or strips) on a grid dimension and loop in launches of 65535, shifting
their pointers by the first frame of each launch; any_decode (vcf_dct_any.hip) loops over chunks of
frames whose workspace stays within 1 GiB.  The batches of tests/batch_split_cases.py reach the
second iteration of each loop: N = 65562 frames that repeat a pool of 251 distinct ones (with their
own weights, means and offset tables), compared frame by frame, whole arrays, with the reference's
output for the pool entry; tests/test_batch_split.py proves on the host that a frame mix-up cannot
go unseen.  The tolerance-based codecs use the comparators and margins of their own test files.
The entries that refuse a larger batch instead of splitting it (tiled CBAAC: 65535 frames, the DWT:
65535 planes) run the largest batch they take, built from the same pool.
"""
import time

import numpy as np
import pytest

import batch_split_cases as S

pytestmark = pytest.mark.gpu

N = S.N


def _up(a):
    from vcf_amd.device import DeviceBuffer
    return DeviceBuffer.from_array(np.ascontiguousarray(a))


def _down(buf, shape, dtype=np.uint8):
    out = buf.download(np.empty(shape, dtype))
    buf.free()
    return out


def _free(*bufs):
    for b in bufs:
        b.free()


# ---- 8 x 8 DCT ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.DCT_IDS)
def test_dct8_encode_and_decode(name):
    import vcf_amd.dct as D
    c = [c for c in S.DCT if c["name"] == name][0]
    ref = S.dct(name)
    H, W, Q, fl = c["H"], c["W"], c["Q"], c["flags"]
    k = D.encode(S.batch(ref["rgb"]), Q, fl)
    want_k = S.batch(ref["k"])
    assert k.shape == want_k.shape and np.array_equal(k, want_k)
    want = S.batch(ref["decoded"])
    for variant in S.DCT_DECODE_VARIANTS:
        got = D.decode(want_k, H, W, Q, fl, variant=variant)
        assert got.shape == want.shape and np.array_equal(got, want), f"decode variant {variant}"


# ---- 2D-MDCT -------------------------------------------------------------------------------
def test_mdct_encode_and_decode():
    import mdct_restated as M
    import vcf_amd.mdct as G
    from test_mdct_gpu import _compare      # the comparator test_mdct_sweep_gpu.py imports too
    c, ref = S.MDCT, S.mdct()
    B, H, W, Q, fl = c["B"], c["H"], c["W"], c["Q"], c["flags"]
    assert G.padded_shape(H, W, B)[:2] == ref["k"].shape[1:3]
    # the pool in one launch against the float64 restatement ...
    k_pool = G.encode(ref["rgb"], Q, fl, B)
    _compare("pool indices", k_pool, ref["k"], M.index_margin(ref["k_pre"], Q))
    rgb_pool = G.decode(ref["k"], H, W, Q, fl, B)
    _compare("pool pixels", rgb_pool, ref["decoded"], M.pixel_margin(ref["decoded_pre"]))
    # ... and the batch bit for bit equal to it: no result depends on the batch position
    assert np.array_equal(G.encode(S.batch(ref["rgb"]), Q, fl, B), S.batch(k_pool))
    assert np.array_equal(G.decode(S.batch(ref["k"]), H, W, Q, fl, B), S.batch(rgb_pool))


# ---- 2D-KLT --------------------------------------------------------------------------------
def test_klt_moments():
    import vcf_amd.klt as G
    B, H, W = (S.BLOCK[x] for x in "BHW")
    ref = S.klt()
    S1, S2 = G.moments(S.batch(ref["rgb"]), B)
    assert S1.dtype == np.int64 and S2.dtype == np.int64
    assert np.array_equal(S1, S.batch(ref["S1"])) and np.array_equal(S2, S.batch(ref["S2"]))


@pytest.mark.parametrize("flags", [0, 1])
def test_klt_encode_and_decode_with_weights_per_frame(flags):
    import vcf_amd.klt as G
    from test_klt_gpu import _compare       # the comparator test_klt_sweep_gpu.py imports too
    B, H, W, Q = (S.BLOCK[x] for x in "BHWQ")
    ref = S.klt(flags)
    D = B * B
    Hp, Wp = G.padded_shape(H, W, B)[:2]
    rgb, w64, k, w32 = (_up(S.batch(ref[x])) for x in ("rgb", "w64", "k", "w32"))
    got_k = _down(G.encode_device(rgb, N, H, W, w64, Q, flags, block_size=B), (N, Hp, Wp, 3))
    got = _down(G.decode_device(k, N, H, W, w32, Q, flags, block_size=B), (N, H, W, 3))
    _free(rgb, w64, k, w32)
    assert (N, 3, D, D) == S.batch(ref["w64"]).shape
    _compare("indices", got_k, S.batch(ref["k"]), S.batch(ref["k_margin"]))
    _compare("pixels", got, S.batch(ref["decoded"]), S.batch(ref["decoded_margin"]))


# ---- 2D-LBT --------------------------------------------------------------------------------
def test_lbt_moments():
    import vcf_amd.lbt as G
    ref = S.lbt()
    S1, S2 = G.moments(S.batch(ref["rgb"]), S.BLOCK["B"])
    assert np.array_equal(S1, S.batch(ref["S1"])) and np.array_equal(S2, S.batch(ref["S2"]))


def test_lbt_training_lands_on_its_own_frame():
    """LBT_EPOCHS epochs from initial matrices of the frame's own: the rule of
    test_lbt_sweep_gpu.test_short_training_at_untested_block_sizes, every frame against the restatement's
    run for its pool entry."""
    import lbt_restated as R
    import lbt_sweep_cases as LS
    import vcf_amd.lbt as G
    B = S.BLOCK["B"]
    ref, want = S.lbt(), S.lbt_training()
    t = G.train(S.batch(ref["rgb"]), B, S.LBT_EPOCHS, init=(S.batch(want["we0"]), S.batch(want["wd0"])))
    c = LS.proxy_scale()
    e = S.entry_of()
    dE = np.max(np.abs(t["we"] - want["we"][e]), axis=(1, 2))
    dD = np.max(np.abs(t["wd"] - want["wd"][e]), axis=(1, 2))
    ratio = np.maximum(dE, dD) / (c * want["d_proxy"][e])
    print(f"|W - restated| / (c x d_proxy): largest {ratio.max():.3f} (first launch {ratio[:S.SPLIT].max():.3f}, "
          f"second {ratio[S.SPLIT:].max():.3f}), c {c:.3f}")
    assert np.all(np.abs(t["mean"].astype(np.float64) - want["mean"][e].astype(np.float64)) <= 2.0 ** -17)
    assert np.all(ratio <= 4)
    # the kernel's own float32 report of (loss, MSE, mean log variance) at its final weights
    loss = np.empty((S.P, 3))
    first = {int(p): int(np.argmax(e == p)) for p in range(S.P)}
    for p, f in first.items():
        X = R.centred(ref["rgb"][p], B, float(t["mean"][f])).astype(np.float64)
        loss[p] = R.loss_terms(X, t["we"][f].astype(np.float64), t["wd"][f].astype(np.float64))
    # equal entries train equally, bit for bit: a table shifted by the wrong stride fails here exactly
    rep = np.array([first[int(p)] for p in e])
    for what in ("we", "wd", "mean", "loss"):
        assert np.array_equal(t[what], t[what][rep]), what
    assert np.allclose(t["loss"], loss[e], rtol=1e-3, atol=1e-6)


@pytest.mark.parametrize("flags", [0, 1])
def test_lbt_encode_and_decode_with_weights_and_means_per_frame(flags):
    import vcf_amd.lbt as G
    from test_lbt_gpu import _check_indices, _check_pixels      # as test_lbt_sweep_gpu.py imports them
    B, H, W, Q = (S.BLOCK[x] for x in "BHWQ")
    ref = S.lbt(flags)
    Hp, Wp = G.padded_shape(H, W, B)[:2]
    rgb, we, wd, mean, k = (_up(S.batch(ref[x])) for x in ("rgb", "we", "wd", "mean", "k"))
    got_k = _down(G.encode_device(rgb, N, H, W, we, mean, Q, flags, block_size=B), (N, Hp, Wp, 3))
    got = _down(G.decode_device(k, N, H, W, wd, mean, Q, flags, block_size=B), (N, H, W, 3))
    _free(rgb, we, wd, mean, k)
    _check_indices(got_k, dict(k=S.batch(ref["k"]), pre=S.batch(ref["k_pre"]), mag=S.batch(ref["k_mag"])), B * B)
    want = S.batch(ref["decoded"])
    _check_pixels(got, dict(pre=S.batch(ref["decoded_pre"]), mag=S.batch(ref["decoded_mag"])), B * B, want)


# ---- distortion and SSIM -------------------------------------------------------------------
def test_distortion_records():
    import vcf_amd.distortion as G
    ref = S.distortion()
    d = G.measure(S.batch(ref["a"]), S.batch(ref["b"]))
    assert d.sse.shape == (N, 3)
    for what in ("sse", "sad", "max_abs"):
        assert np.array_equal(getattr(d, what).astype(np.int64), S.batch(ref[what])), what


def test_ssim_records():
    import vcf_amd.distortion as G
    ref = S.ssim()
    s = G.ssim(S.batch(ref["a"]), S.batch(ref["b"]))
    assert s.windows == ref["windows"] == 1
    assert np.array_equal(s.sum_k, S.batch(ref["sum_k"]))
    assert np.array_equal(s.min_k, S.batch(ref["min_k"]))


# ---- inflate -----------------------------------------------------------------------------
def test_inflate_strips():
    from vcf_amd.device import DeviceBuffer, Stream
    from vcf_amd.zlib_gpu import StripInflater
    comp, coff, clen, ooff, olen, want = S.inflate_batch()
    out = DeviceBuffer(want.size)
    out.fill(0xA5)
    inf = StripInflater()
    inf.inflate_into(comp, coff, clen, out, ooff, olen, Stream())       # raises unless every status is 0
    got = _down(out, want.shape)
    inf.close()
    assert np.array_equal(got, want)


# ---- 2D-DWT: the largest batch ---------------------------------------------------------------
@pytest.mark.parametrize("wavelet", S.DWT_WAVELETS)
def test_dwt_largest_batch(wavelet):
    """21845 frames: plane = blockIdx.z reaches 65534.  Encode and decode equal the oracle's, bit for
    bit; the decode is given the oracle's subbands."""
    import vcf_amd.dwt as DW
    from vcf_amd.device import DeviceBuffer
    H, W, L, Q = (S.DWT[x] for x in "HWLQ")
    n = S.DWT_N
    ref = S.dwt(wavelet)
    shapes, pb, wb = DW.layout(H, W, L)
    Ho, Wo = 2 * shapes[0][0], 2 * shapes[0][1]
    assert ref["packed"].shape == (S.P, pb) and ref["decoded"].shape == (S.P, Ho, Wo, 3)
    wi = DW.wavelet_index(wavelet)
    rgb, packed_in = _up(S.batch(ref["rgb"], n)), _up(S.batch(ref["packed"], n))
    packed, out, ws = DeviceBuffer(n * pb), DeviceBuffer(n * Ho * Wo * 3), DeviceBuffer(n * wb)
    DW.encode_device(rgb, n, H, W, wi, L, Q, packed, ws)
    got_packed = _down(packed, (n, pb))
    DW.decode_device(packed_in, n, H, W, wi, L, Q, out, ws)
    got = _down(out, (n, Ho, Wo, 3))
    _free(rgb, packed_in, ws)
    assert np.array_equal(got_packed, S.batch(ref["packed"], n))
    assert np.array_equal(got, S.batch(ref["decoded"], n))


# ---- tiled CBAAC: the batch limit and the largest batch --------------------------------------------
def _cbaac_calls(kind, nf, b, stride):
    """The (entry, arguments) of the prior, encode and decode stage of a kind, over nf frames."""
    if kind == "tiled2d":
        (H, W, C), (th, tw), K = (S.CBAAC2D[x] for x in ("shape", "tile", "nclass"))
        n = H * W * C
        return (("vcf_cbaac_tiled2d_prior_frames", (b["sym"].ptr, nf, H, W, C, n, th, tw, K, b["prior"].ptr, b["hist"].ptr, None)),
                ("vcf_cbaac_tiled2d_encode_frames", (b["sym"].ptr, nf, H, W, C, n, b["prior"].ptr, K, th, tw, b["out"].ptr,
                                                     b["cap"], b["sizes"].ptr, b["ws"].ptr, None)),
                ("vcf_cbaac_tiled2d_decode_frames", (b["src"].ptr, b["offs"].ptr, nf, H, W, C, b["prior"].ptr, K, th, tw,
                                                     b["dec"].ptr, stride, None)))
    n, seg = S.CBAAC["n"], S.CBAAC["seg_len"]
    if kind == "classes":
        K = S.CBAAC["nclass"]
        return (("vcf_cbaac_tiled_prior_classes", (b["sym"].ptr, nf, n, n, seg, K, b["prior"].ptr, b["hist"].ptr, None)),
                ("vcf_cbaac_tiled_encode_classes", (b["sym"].ptr, nf, n, n, 0, b["prior"].ptr, K, seg, b["out"].ptr, b["cap"],
                                                    b["sizes"].ptr, b["ws"].ptr, None)),
                ("vcf_cbaac_tiled_decode_classes", (b["src"].ptr, b["offs"].ptr, nf, n, 0, b["prior"].ptr, K, seg, b["dec"].ptr,
                                                    stride, None)))
    return (("vcf_cbaac_tiled_prior_frames", (b["sym"].ptr, nf, n, n, b["prior"].ptr, b["hist"].ptr, None)),
            ("vcf_cbaac_tiled_encode_frames", (b["sym"].ptr, nf, n, n, 0, b["prior"].ptr, seg, b["out"].ptr, b["cap"],
                                               b["sizes"].ptr, b["ws"].ptr, None)),
            ("vcf_cbaac_tiled_decode_frames", (b["src"].ptr, b["offs"].ptr, nf, n, 0, b["prior"].ptr, seg, b["dec"].ptr, stride,
                                               None)))


# one wave per segment (1) and one lane per segment (2, what the library picks at this many segments);
# the tiles of the two-dimensional context have one kernel
@pytest.mark.parametrize("kind,variant", [("frames", 1), ("frames", 2), ("classes", 1), ("classes", 2), ("tiled2d", 0)])
def test_cbaac_batch_limit_and_largest_batch(kind, variant):
    """65536 frames are VCF_ERR_INVALID at every stage; 65535, where frame 65534 addresses the last
    row of every per-frame table, give every frame the host serial coder's prior rows, byte counts
    and bytes, and the decoder gives every frame's symbols back from the host coder's streams."""
    from vcf_amd import _lib as L
    from vcf_amd.device import DeviceBuffer
    F, over = S.CBAAC_N, S.CBAAC_N + 1
    ref = S.cbaac(kind)
    n = int(np.prod(ref["sym"].shape[1:]))
    parts, cap = ref["sizes"].shape[1], ref["payload"].shape[1]
    rows = ref["prior"].size // (S.P * 256)
    lib = L.lib()
    if kind == "tiled2d":
        ws = int(lib.vcf_cbaac_tiled2d_workspace(over, *S.CBAAC2D["shape"], *S.CBAAC2D["tile"]))
    else:
        ws = int(lib.vcf_cbaac_tiled_frames_workspace(over, n, S.CBAAC["seg_len"]))
    stride = n + 3                                          # decoded frames at every alignment, gaps between them
    flat, offs = S.cbaac_streams(kind, over)
    # every buffer holds 65536 frames: the calls that must be refused could reach nothing outside
    b = dict(cap=cap, sym=_up(S.batch(ref["sym"], over)), src=_up(flat), offs=_up(offs), ws=DeviceBuffer(ws),
             prior=DeviceBuffer(512 * rows * over), hist=DeviceBuffer(1024 * rows * over), out=DeviceBuffer(cap * over),
             sizes=DeviceBuffer(8 * (parts + 1) * over), dec=DeviceBuffer(stride * over))
    b["dec"].fill(0xA5)
    b["out"].fill(0)

    def run(entry, args):                                   # a variant: the coders' twins (a prior has one kernel)
        if variant and "_prior_" not in entry:
            return L.call_ab(entry + "_variant", variant, *args)
        return L.call(entry, *args)
    try:
        for stage in _cbaac_calls(kind, over, b, stride):
            with pytest.raises(L.VCFInvalidArgument, match="n_frames 65536"):
                run(*stage)
        prior_stage, encode_stage, decode_stage = _cbaac_calls(kind, F, b, stride)
        run(*prior_stage)
        prior = b["prior"].download(np.empty((F,) + ref["prior"].shape[1:], np.uint16))
        assert np.array_equal(prior, S.batch(ref["prior"], F))
        del prior                                           # the device's rows are the host's: the next stages read them
        run(*encode_stage)
        sizes = b["sizes"].download(np.empty((F, parts + 1), np.int64))
        out = b["out"].download(np.empty((F, cap), np.uint8))
        run(*decode_stage)
        dec = b["dec"].download(np.empty((F, stride), np.uint8))
    finally:
        _free(*(v for v in b.values() if isinstance(v, DeviceBuffer)))
    want_sizes = S.batch(ref["sizes"], F)
    assert np.array_equal(sizes[:, :parts], want_sizes) and np.array_equal(sizes[:, parts], want_sizes.sum(axis=1))
    used = np.arange(cap) < sizes[:, parts:]
    assert np.array_equal(out[used], S.batch(ref["payload"], F)[used])
    for f in S.CBAAC_PROBES:                                # these frames coded on the host by themselves
        host = S.cbaac_probe(kind, f)
        assert list(sizes[f, :parts]) == [len(h) for h in host] and out[f, :sizes[f, parts]].tobytes() == b"".join(host), f
    assert np.array_equal(dec[:, :n], S.batch(ref["sym"], F).reshape(F, n))
    assert np.all(dec[:, n:] == 0xA5)                       # nothing written between the frames


# ---- any-B decode: the workspace chunks ----------------------------------------------------------
@pytest.mark.parametrize("name", S.ANY_IDS)
def test_any_b_decode_over_workspace_chunks(name):
    import vcf_amd.dct as D
    c = [c for c in S.ANY if c["name"] == name][0]
    n, H, W = c["n"], c["H"], c["W"]
    assert D.padded_shape(H, W, S.ANY_B) == (H, W)
    chunk = S.chunk_frames(n, H, W, S.ANY_B, c["mode"])
    assert chunk == c["chunk"] and -(-n // chunk) > 1, "the shape no longer takes several chunks"
    k, want = S.any_frames(name)
    t0 = time.perf_counter()
    decode = D.decode_k32 if c["mode"] == "k32" else D.decode
    got = decode(k, H, W, S.ANY_Q, D.VCF_DCT_NO_SUBBANDS, block_size=S.ANY_B)
    print(f"{name}: {n} frames of {H} x {W}, {-(-n // chunk)} chunks of {chunk}, decode and copies "
          f"{time.perf_counter() - t0:.2f} s")
    assert got.shape == want.shape and got.dtype == np.uint8
    for f in range(n):
        assert np.array_equal(got[f], want[f]), f"frame {f}"

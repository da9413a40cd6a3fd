"""vcf_dct_dz_encode_rdoq on the GPU against the numpy restatement of its rule (tests/rdoq_ref.py):
bit-equality over shapes, steps, layouts, weights and tables, the lambda = 0 identity with the plain
kernel, the rule's consequences, the rejected calls, the launch split, the caller's stream and the
codec round trip.  Every reference is the oracle's float32 coefficients through the rule in float64."""
import os

import numpy as np
import pytest
from PIL import Image

import rdoq_ref as RR
from abi_buffers import Guarded
from oracle import ref_numpy as RN
from vcf_amd import _lib as L
from vcf_amd import dct as D
from vcf_amd import rdoq as R
from vcf_amd.codec import parser as P
from vcf_amd.device import DeviceBuffer, HostBuffer, Stream

pytestmark = pytest.mark.gpu

NOSUB = D.VCF_DCT_NO_SUBBANDS
MUS = (0.0, 0.05, 0.3, 10.0)


def _tile():
    return L.lib().vcf_dct_rdoq_tile()


def _noise(shape, seed):
    return np.random.Generator(np.random.PCG64(seed)).integers(0, 256, shape, dtype=np.uint8)


def _random_table(n, seed):
    return np.random.Generator(np.random.PCG64(seed)).random((n, 64, 3, 256)) * 16.0      # [0, 16)


def _own_table(frames, Q):
    """cost_table of every frame's own plain histogram on the (8, 8) grid."""
    return R.cost_table(np.stack([RR.counts_of(RN.encode_frame(f, Q)) for f in frames]))


def _gpu(frames, Q, lam, bits, flags=0):
    """frames n x H x W x 3, bits cost_frames x 64 x 3 x 256 -> n x Hp x Wp x 3."""
    n, H, W, _ = frames.shape
    Hp, Wp = D.padded_shape(H, W)
    src, tab = DeviceBuffer.from_array(frames), DeviceBuffer.from_array(np.ascontiguousarray(bits, np.float64))
    try:
        out = R.encode_device(src, n, H, W, Q, lam, tab, len(bits), flags)
        res = out.download(np.empty((n, Hp, Wp, 3), np.uint8))
        out.free()
        return res
    finally:
        src.free()
        tab.free()


def _check_frame(rgb, got, Q, lam, bits, sub, plain):
    """One frame of one launch: the restatement's bytes; never up; zeros stay; not dearer than plain."""
    assert np.array_equal(got, RR.encode_frame(rgb, Q, lam, bits, sub))
    k, k0 = got.astype(np.int32) - 128, plain.astype(np.int32) - 128
    assert np.all(np.abs(k) <= np.abs(k0)) and np.all(k[k0 == 0] == 0)
    j, j0 = RR.total_cost(rgb, got, Q, lam, bits, sub), RR.total_cost(rgb, plain, Q, lam, bits, sub)
    print(f"Q {Q} lambda {lam:g}: sum J {j:.6g} <= {j0:.6g}, {np.count_nonzero(k != k0)} of "
          f"{np.count_nonzero(k0)} non-zero indices lowered")
    assert j <= j0


def _shapes():
    # padding on both axes; aligned; two full tiles and a partial one (16-byte copy-out: 32 blocks a row)
    return [(61, 77), (64, 96), (8 * (2 * _tile() // 32 + 1), 256)]


@pytest.mark.parametrize("sub", [True, False], ids=["subbands", "x"])
@pytest.mark.parametrize("Q", [3, 5, 32, 64])
@pytest.mark.parametrize("shape", [0, 1, 2], ids=["61x77", "64x96", "tiles"])
def test_bit_equal_with_the_restatement(shape, Q, sub):
    H, W = _shapes()[shape]
    if shape == 2:
        nblocks = (H // 8) * (W // 8)
        assert nblocks > 2 * _tile() and nblocks % _tile() != 0
    rgb = _noise((H, W, 3), 100 + shape)
    # mid-grey noise of small amplitude in the lower half: zero and small indices at every Q
    rgb[H // 2:] = 118 + rgb[H // 2:] // 12
    flags = 0 if sub else NOSUB
    plain_gpu = D.encode(rgb, Q, flags)
    assert np.array_equal(plain_gpu, RN.encode_frame(rgb, Q, sub))
    tables = (_random_table(1, 7 * Q + shape), _own_table(rgb[None], Q))
    for bits in tables:
        for mu in MUS:
            lam = mu * Q * Q
            got = _gpu(rgb[None], Q, lam, bits, flags)[0]
            if mu == 0.0:
                assert np.array_equal(got, plain_gpu)                     # byte for byte the plain kernel
            _check_frame(rgb, got, Q, lam, bits[0], sub, plain_gpu)


@pytest.mark.parametrize("Q", [5, 32])
def test_a_batch_with_a_table_per_frame_and_with_one_table(Q):
    frames = _noise((3, 64, 96, 3), 11)
    frames[1] = 120 + frames[1] // 16
    bits = _random_table(3, 12)
    bits[1] *= 0.25
    plain = D.encode(frames, Q)
    for mu in MUS:
        lam = mu * Q * Q
        got = _gpu(frames, Q, lam, bits)
        one = _gpu(frames, Q, lam, bits[2:3])
        for f in range(3):
            _check_frame(frames[f], got[f], Q, lam, bits[f], True, plain[f])
            _check_frame(frames[f], one[f], Q, lam, bits[2], True, plain[f])
            if mu == 0.0:
                assert np.array_equal(got[f], plain[f]) and np.array_equal(one[f], plain[f])


def test_every_pointer_offset():
    """rgb_dev and k_dev at every offset 0..15 from a 16-byte boundary: 16 blocks a row, so the aligned
    call takes the 16-byte copy-out and the 8-byte loads, the others the byte paths."""
    H, W, Q, lam = 64, 128, 32, 0.3 * 32 * 32
    rgb = _noise((2, H, W, 3), 21)
    rgb[1] = 100 + rgb[1] // 8
    bits = _random_table(2, 22)
    want = np.stack([RR.encode_frame(rgb[f], Q, lam, bits[f]) for f in range(2)])
    tab = DeviceBuffer.from_array(bits)
    for off in range(16):
        src, out = Guarded(rgb.nbytes, off, rgb), Guarded(want.nbytes, off)
        L.call("vcf_dct_dz_encode_rdoq", src.ptr, 2, H, W, 8, Q, 0, tab.ptr, 2, bits.size, lam, out.ptr, None)
        assert np.array_equal(out.download().reshape(want.shape), want), off
        out.check(f"offset {off}")
    tab.free()


def test_never_up_and_the_zero_skip_on_a_smooth_frame():
    from vcf_amd.synthetic import synth_frame
    H, W, Q = 256, 512, 32
    rgb = synth_frame(H, W, 3)
    plain = D.encode(rgb, Q)
    assert np.mean(plain == 128) > 0.9                       # most row pairs are proven zero
    bits = _own_table(rgb[None], Q)
    for mu in (0.2, 10.0):
        got = _gpu(rgb[None], Q, mu * Q * Q, bits)[0]
        _check_frame(rgb, got, Q, mu * Q * Q, bits[0], True, plain)
    assert np.array_equal(_gpu(rgb[None], Q, 0.0, bits)[0], plain)


def test_wrapped_indices_are_the_plain_kernel_s():
    rgb = np.zeros((64, 96, 3), np.uint8)
    rgb[:, ::2] = 255
    rgb[8:24, :48] = 255
    rgb[32:40] = _noise((8, 96, 3), 31)
    bits = _random_table(1, 32)
    for sub in (True, False):
        flags = 0 if sub else NOSUB
        plain = D.encode(rgb, 1, flags)
        k0 = (RR._layout(RR.coefficients(rgb) / 1, sub)).astype(np.int32)
        wrapped = (k0 < -128) | (k0 > 127)
        assert wrapped.sum() > 50
        got = _gpu(rgb[None], 1, 10.0, bits, flags)[0]
        assert np.array_equal(got[wrapped], plain[wrapped])
        assert np.array_equal(got, RR.encode_frame(rgb, 1, 10.0, bits[0], sub))


# ---- rejected calls ------------------------------------------------------------------
def test_rejected_calls_write_nothing_and_the_table_is_read_only():
    H, W, Q, n = 24, 40, 32, 2
    rgb = _noise((n, H, W, 3), 41)
    bits = _random_table(n, 42)
    src = Guarded(rgb.nbytes, 0, rgb)
    tab = Guarded(bits.nbytes, 0, bits)
    out = Guarded(n * H * W * 3 + 512)                       # more than the n * Hp * Wp * 3 bytes written
    lib = L.lib()
    cap = bits.size

    def call(**kw):
        a = dict(rgb=src.ptr, n=n, H=H, W=W, B=8, Q=Q, flags=0, cost=tab.ptr, cf=n, cap=cap, lam=1.0, k=out.ptr)
        a.update(kw)
        return lib.vcf_dct_dz_encode_rdoq(a["rgb"], a["n"], a["H"], a["W"], a["B"], a["Q"], a["flags"], a["cost"],
                                          a["cf"], a["cap"], a["lam"], a["k"], None)

    INV, UNS = L.VCF_ERR_INVALID, L.VCF_ERR_UNSUPPORTED
    rejected = [
        (dict(rgb=None), INV), (dict(k=None), INV), (dict(cost=None), INV),
        (dict(n=0), INV), (dict(n=-1), INV),
        (dict(cf=0), INV), (dict(cf=3), INV), (dict(n=3, cf=2), INV),
        (dict(cap=cap - 1), INV), (dict(cf=1, cap=64 * 3 * 256 - 1), INV),
        (dict(cost=tab.buf.address(tab.start + 4)), INV),
        (dict(lam=-1.0), INV), (dict(lam=float("nan")), INV), (dict(lam=float("inf")), INV),
        (dict(Q=0), INV), (dict(Q=-3), INV),
        (dict(B=16), UNS), (dict(B=4), UNS), (dict(flags=D.VCF_DCT_PERCEPTUAL), UNS),
    ]
    for kw, status in rejected:
        assert call(**kw) == status, kw
        assert lib.vcf_last_error()
        out.check_untouched(str(kw))
        tab.check_untouched(str(kw))
    # an accepted call writes n * Hp * Wp * 3 bytes and nothing else, and leaves the table alone
    assert call() == 0
    out.check_outside([(0, n * H * W * 3)], "accepted call")
    out.check("accepted call")
    tab.check_untouched("accepted call")
    got = out.download(count=n * H * W * 3).reshape(n, H, W, 3)
    for f in range(n):
        assert np.array_equal(got[f], RR.encode_frame(rgb[f], Q, 1.0, bits[f]))
    assert call(cf=1, cap=64 * 3 * 256) == 0                 # one table needs one table's capacity


# ---- the launch split ----------------------------------------------------------------
def test_a_batch_over_the_launch_split():
    n, Q, lam = 65537, 5, 0.3 * 25
    base = _noise((251, 8, 8, 3), 51)
    frames = np.ascontiguousarray(base[np.arange(n) % 251])
    for f, seed in ((0, 52), (65534, 53), (65535, 54), (65536, 55)):
        frames[f] = _noise((8, 8, 3), seed)
    bits = _random_table(1, 56)
    got = _gpu(frames, Q, lam, bits)
    for f in (0, 65534, 65535, 65536):
        assert np.array_equal(got[f], RR.encode_frame(frames[f], Q, lam, bits[0])), f
    assert np.array_equal(got[252:502], got[1:251])          # the same frames, the same bytes


# ---- the caller's stream -------------------------------------------------------------
def test_on_a_caller_stream_between_an_upload_and_a_download():
    H, W, Q, n = 256, 512, 32, 8
    lam = 0.2 * Q * Q
    real, decoy = _noise((n, H, W, 3), 61), _noise((n, H, W, 3), 62)
    bits = _random_table(n, 63)
    want = _gpu(real, Q, lam, bits)
    assert not np.array_equal(want, _gpu(decoy, Q, lam, bits))
    st = Stream()
    hin, hout = HostBuffer(real.nbytes), HostBuffer(want.nbytes)
    hin.array[:] = real.reshape(-1)
    hout.array[:] = 0
    src, tab, out = DeviceBuffer.from_array(decoy), DeviceBuffer.from_array(bits), DeviceBuffer(want.nbytes)
    out.fill(0)
    L.call("vcf_device_sync")
    src.upload(hin.array, st)
    R.encode_device(src, n, H, W, Q, lam, tab, n, out=out, stream=st)
    out.download(hout.array, st)
    st.synchronize()
    assert np.array_equal(hout.array.reshape(want.shape), want)
    for b in (src, tab, out, hin, hout):
        b.free()
    st.close()


# ---- the pipeline and the codec ------------------------------------------------------
def _pipeline_ref(rgb, Q, mu, iterations=1, sub=True):
    lam = mu * Q * Q
    idx = RN.encode_frame(rgb, Q)
    for it in range(iterations):
        bits = R.cost_table(RR.counts_of(idx))
        last = it == iterations - 1
        idx = RR.encode_frame(rgb, Q, lam, bits, sub if last else True)
    return idx


@pytest.mark.parametrize("flags", [0, NOSUB], ids=["subbands", "x"])
def test_the_two_pass_pipeline_and_its_iterations(flags):
    """Q = 8, mu = 1: on both frames every one of the first three passes moves indices (the restatement is
    asked first), so a pipeline that ignored `iterations`, rebuilt the table from the plain indices again or
    mixed up its scratch and output buffers under -x gives other bytes."""
    Q, mu = 8, 1.0
    frames = _noise((2, 61, 77, 3), 71)
    frames[1] = 110 + frames[1] // 10
    sub = flags == 0
    want = [[RN.encode_frame(f, Q, sub) for f in frames]]
    want += [[_pipeline_ref(f, Q, mu, it, sub) for f in frames] for it in (1, 2, 3)]
    for it in (1, 2, 3):
        moved = [int(np.count_nonzero(a != b)) for a, b in zip(want[it - 1], want[it])]
        print(f"pass {it}: {moved} indices move")
        assert min(moved) > 0
    for it in (1, 2, 3):
        got = R.encode(frames, Q, R.lambda_of(mu, Q), flags, iterations=it)
        for f in range(2):
            assert np.array_equal(got[f], want[it][f]), (it, f)
    with pytest.raises(ValueError):
        R.encode(frames, 16, 1.0, iterations=5)
    with pytest.raises(ValueError):
        R.encode(frames, 16, 1.0, iterations=0)


def _png(path, rgb):
    Image.fromarray(rgb).save(path)
    return str(path)


@pytest.mark.parametrize("entropy", ["TIFF", "TCBAAC2D"])
def test_codec_round_trip(tmp_path, entropy):
    from vcf_amd.codec.dct2d import CoDec
    Q, mu = 32, 0.5          # every frame's indices move (asserted below against the plain encode)
    enc_args = lambda: P.parse(P.dct_parser(entropy=entropy, rdoq=True),                         # noqa: E731
                               ["encode", "--rdoq", str(mu), "-c", entropy, "-q", str(Q)])
    dec_args = lambda: P.parse(P.dct_parser(entropy=entropy), ["decode", "-c", entropy, "-q", str(Q)])   # noqa: E731
    shapes = [(72, 104), (61, 77), (72, 104)]
    frames = [_noise((h, w, 3), 80 + i) // (1 + i) for i, (h, w) in enumerate(shapes)]
    pairs = [(_png(tmp_path / f"original_{i:04d}.png", f), str(tmp_path / f"encoded_{i:04d}"))
             for i, f in enumerate(frames)]
    codec = CoDec(enc_args())
    ext = codec.file_extension
    sizes = codec.encode_fns(pairs, batch=3)
    for i, ((src, out), n) in enumerate(zip(pairs, sizes)):
        single = str(tmp_path / f"single_{i}")
        assert CoDec(enc_args()).encode_fn(src, single) == n == os.path.getsize(out + ext)
        assert open(single + ext, "rb").read() == open(out + ext, "rb").read()
        assert open(single + "_shape.bin", "rb").read() == open(out + "_shape.bin", "rb").read()
        assert sorted(os.path.basename(p) for p in os.listdir(tmp_path) if p.startswith(f"single_{i}")) == \
            sorted([f"single_{i}{ext}", f"single_{i}_shape.bin"])                       # no side file
        # a codec built without the flag decodes it, to the image of the restatement's indices
        dec = str(tmp_path / f"decoded_{i}.png")
        CoDec(dec_args()).decode_fn(out, dec)
        h, w = shapes[i]
        ref = _pipeline_ref(frames[i], Q, mu)
        assert np.count_nonzero(ref != RN.encode_frame(frames[i], Q)) > 50
        want = D.decode(ref, h, w, Q)
        assert np.array_equal(np.asarray(Image.open(dec).convert("RGB")), want)


def test_rd_curve_with_rdoq():
    """mu = 0 gives the plain curve; mu = 0.5 the RMSE of the restatement's indices decoded (both are
    sqrt(integer SSE / samples) in float64, so they agree to rounding), which is not the plain curve's."""
    from vcf_amd.codec.rde import rd_curve
    Qs, mu = [16, 32], 0.5
    frames = _noise((2, 64, 96, 3), 91) // 2
    plain = rd_curve(frames, Qs)
    zero = rd_curve(frames, Qs, rdoq=0.0)
    some = rd_curve(frames, Qs, rdoq=mu)
    for Q, a, b, c in zip(Qs, plain, zero, some):
        assert np.array_equal(a["bytes"], b["bytes"]) and np.array_equal(a["rmse"], b["rmse"])
        for f in range(2):
            ref = _pipeline_ref(frames[f], Q, mu)
            assert np.count_nonzero(ref != RN.encode_frame(frames[f], Q)) > 0
            y = D.decode(ref, 64, 96, Q).astype(np.float64)
            want = np.sqrt(np.mean((frames[f].astype(np.float64) - y) ** 2))
            assert np.isclose(c["rmse"][f], want, rtol=1e-12, atol=0), (Q, f, c["rmse"][f], want)
            assert c["rmse"][f] != a["rmse"][f]

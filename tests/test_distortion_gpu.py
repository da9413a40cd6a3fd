"""vcf_distortion_u8 on the GPU (vcf_distortion.hip through vcf_amd.distortion): the records must
equal, exactly, the int64 restatement written here, at every tail case of the kernel's 48-byte
spans and 16-byte loads, for every channel count, for batches, on another stream and twice into
the same records."""
import ctypes
import functools

import numpy as np
import pytest

from vcf_amd import distortion as DS
from vcf_amd._lib import call
from vcf_amd.device import DeviceBuffer, Stream

pytestmark = pytest.mark.gpu

SPAN = 48                 # bytes a lane takes per step (vcf_distortion.hip kSpan)
TILE = 256 * 2 * SPAN     # a workgroup's share per step: kThreads * kUnroll spans = 24 576 bytes


def restated(a, b):
    """(sse, sad, max_abs) per frame and channel of N x H x W x C u8 frames, in int64."""
    d = np.abs(a.astype(np.int64) - b.astype(np.int64))
    n, _, _, C = d.shape
    d = d.reshape(n, -1, C)
    mx = d.max(axis=1) if d.shape[1] else np.zeros((n, C), np.int64)
    return (d * d).sum(axis=1), d.sum(axis=1), mx


def check(m, a, b):
    sse, sad, mx = restated(a, b)
    assert m.sse.dtype == np.uint64 and m.sad.dtype == np.uint64 and m.max_abs.dtype == np.uint32
    assert np.array_equal(m.sse.astype(np.int64), sse)
    assert np.array_equal(m.sad.astype(np.int64), sad)
    assert np.array_equal(m.max_abs.astype(np.int64), mx)


def pair(shape, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.integers(0, 256, shape, dtype=np.uint8), rng.integers(0, 256, shape, dtype=np.uint8)


def hw(samples, C):
    """H x W with H * W * C == samples: the sizes below are chosen to be multiples of C."""
    assert samples % C == 0
    px = samples // C
    for h in (64, 33, 31, 16, 12, 11, 8, 5, 4, 3, 2):
        if px % h == 0 and px // h >= h:
            return h, px // h
    return 1, px


# H * W * C of one frame, multiples of 12 (so of every C) unless marked: 48 = one span; 96 +- a 16-byte load;
# 16 k + 5-like sizes are covered per C below; one span short of, exactly, and one span over a workgroup's share
SIZES = [12, 36, 48, 60, 96, 144, 16 * 12 * 3 + 12, TILE - SPAN, TILE, TILE + SPAN, 2 * TILE + 5 * SPAN + 24]


@pytest.mark.parametrize("C", [1, 2, 3, 4])
@pytest.mark.parametrize("n", [1, 5])
def test_sizes_by_channels(C, n):
    for i, samples in enumerate(SIZES):
        H, W = hw(samples, C)
        a, b = pair((n, H, W, C), 1000 * C + 10 * i + n)
        check(DS.measure(a, b), a, b)


@pytest.mark.parametrize("C,H,W", [(1, 1, 1), (1, 1, 47), (1, 1, 48), (1, 7, 7), (1, 1, 16 * 9 + 5), (1, 3, 16 * 7 + 5),
                                   (2, 1, 1), (3, 1, 1), (4, 1, 1), (3, 1, 16), (3, 1, 17), (3, 5, 23), (2, 7, 53 // 2),
                                   (3, 61, 77), (4, 61, 77), (1, 61, 77), (2, 61, 77)])
@pytest.mark.parametrize("n", [1, 5])
def test_odd_sizes(C, H, W, n):
    """H*W*C = 1, 47, 48, 49, 16k + 5, frames that are no multiple of 16 bytes (so frames 1.. of a batch start off
    a 16-byte boundary and the channel classes rotate), and several workgroups a frame (61 x 77 x 3)."""
    a, b = pair((n, H, W, C), 7 * H + W + 100 * C + n)
    check(DS.measure(a, b), a, b)


def test_identical_frames():
    a, _ = pair((3, 40, 56, 3), 5)
    m = DS.measure(a, a)
    assert not m.sse.any() and not m.sad.any() and not m.max_abs.any()
    assert np.isinf(DS.psnr(a, a)).all() and np.isinf(DS.psnr(a[0], a[0]))
    assert DS.rmse(a[0], a[0]) == 0.0 and DS.mse(a[0], a[0]) == 0.0


def test_one_byte_at_the_very_end():
    a, _ = pair((5, 37, 53, 3), 6)
    b = a.copy()
    b[-1, -1, -1, -1] ^= 0x5A
    d = int(abs(int(a[-1, -1, -1, -1]) - int(b[-1, -1, -1, -1])))
    m = DS.measure(a, b)
    check(m, a, b)
    assert m.sse.sum() == d * d and m.sse[4, 2] == d * d and m.sad[4, 2] == d and m.max_abs[4, 2] == d


def test_host_values():
    a, b = pair((2, 30, 44, 3), 8)
    sse, _, _ = restated(a, b)
    want = sse.sum(axis=1).astype(np.float64) / (30 * 44 * 3)
    assert np.array_equal(DS.mse(a, b), want)
    assert np.array_equal(DS.rmse(a, b), np.sqrt(want))
    assert np.array_equal(DS.psnr(a, b), 10.0 * np.log10(255.0 ** 2 / want))
    assert DS.rmse(a[1], b[1]) == float(np.sqrt(want[1])) and isinstance(DS.rmse(a[1], b[1]), float)
    g = DS.measure(a[0, :, :, 0], b[0, :, :, 0])          # H x W: one grey frame
    assert g.sse.shape == (1, 1) and int(g.sse[0, 0]) == int(sse[0, 0])


@functools.lru_cache(maxsize=None)
def big():
    """One 4K RGB pair, all 0 against all 255, measured once: sums past 2^32 per channel."""
    H, W = 2160, 3840
    a, b = DeviceBuffer(H * W * 3), DeviceBuffer(H * W * 3)
    a.fill(0)
    b.fill(255)
    out = DS.sse_device(a, b, 1, H, W, 3)
    m = DS.records(out, 1, 3, H * W)
    for buf in (a, b, out):
        buf.free()
    return m


def test_sums_past_32_bits():
    m = big()
    px = 2160 * 3840
    assert px * 65025 > 2 ** 32
    assert m.sse.tolist() == [[px * 65025] * 3] and m.sad.tolist() == [[px * 255] * 3] and m.max_abs.tolist() == [[255] * 3]
    assert m.rmse()[0] == 255.0 and m.psnr()[0] == 0.0


def test_stream_repeat_and_offsets():
    """A non-default stream; twice into the same records (the call zeroes them: no doubling); and frame sets whose
    addresses differ by no multiple of 16 (the kernel's bytewise reads of b)."""
    n, H, W, C = 3, 29, 31, 3
    a, b = pair((n, H, W, C), 9)
    F = n * H * W * C
    st = Stream()
    da, db = DeviceBuffer(F + 16), DeviceBuffer(F + 16)
    out = DeviceBuffer(n * C * DS.RECORD.itemsize)
    out.fill(0xFF, st)
    try:
        da.upload(a, st)
        db.upload(b, st)
        DS.sse_device(da, db, n, H, W, C, out, st)
        first = DS.records(out, n, C, H * W, st)
        check(first, a, b)
        DS.sse_device(da, db, n, H, W, C, out, st)
        second = DS.records(out, n, C, H * W, st)
        assert np.array_equal(first.sse, second.sse) and np.array_equal(first.sad, second.sad)
        assert np.array_equal(first.max_abs, second.max_abs)
        rec = np.zeros((n, C), DS.RECORD)
        out.download(rec, st)
        st.synchronize()
        assert not rec["pad"].any()
        for oa, ob in ((3, 3), (0, 5), (7, 2)):
            da.upload(a, st, offset=oa)
            db.upload(b, st, offset=ob)
            call("vcf_distortion_u8", da.address(oa), db.address(ob), n, H, W, C, out.ptr, st.handle)
            check(DS.records(out, n, C, H * W, st), a, b)
    finally:
        st.synchronize()
        for buf in (da, db, out):
            buf.free()
        st.close()


def test_default_out_and_small_buffers():
    a, b = pair((1, 8, 8, 3), 10)
    da, db = DeviceBuffer.from_array(a), DeviceBuffer.from_array(b)
    out = DS.sse_device(da, db, 1, 8, 8, 3)
    check(DS.records(out, 1, 3, 64), a, b)
    with pytest.raises(ValueError):
        DS.sse_device(da, db, 2, 8, 8, 3)                 # the inputs hold one frame
    with pytest.raises(ValueError):
        DS.sse_device(da, db, 1, 8, 8, 3, out=DeviceBuffer(8))
    assert ctypes.sizeof(ctypes.c_uint64) * 3 == DS.RECORD.itemsize

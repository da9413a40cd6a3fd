"""The fixtures of the caller-stream tests (tests/stream_cases.py), without a GPU.

tests/test_streams_gpu.py tells a call that read the right input at the right
time from one that read the decoy, or a stale buffer, by the output alone.  That
works only if the oracle's outputs for `real` and `decoy` differ in most of
their elements; it is a property of the fixtures and is checked here, with the
shapes and element types the header states for every entry's output."""
import numpy as np
import pytest

import stream_cases as C


def _row(name):
    return C.by_name(name)


def _elements(row, which):
    """The output for `which` as one flat list of typed pieces, each with its mask of defined elements."""
    blob, mask = row.expected(which)
    out = []
    for (off, dtype, shape), p in zip(row.spec(), row.pieces(which)):
        n = p.nbytes
        m = np.ones(p.size, bool) if mask is None else mask[off:off + n].reshape(p.size, -1).all(axis=1)
        out.append((blob[off:off + n].view(dtype).reshape(-1), m))
    return out


def test_the_table_is_the_one_the_gpu_tests_name():
    assert tuple(r.name for r in C.rows()) == C.NAMES
    assert tuple(r.name for r in C.extra_rows()) == C.EXTRA_NAMES
    assert set(C.FIRST_CALL) <= set(C.NAMES + C.EXTRA_NAMES)
    assert {r.group for r in C.rows()} == {"scratch", "library", "memset"}


@pytest.mark.parametrize("name", C.NAMES + C.EXTRA_NAMES)
def test_real_and_decoy_outputs_differ_in_most_elements(name):
    row = _row(name)
    assert row.real.shape == row.decoy.shape and row.real.dtype == row.decoy.dtype
    assert np.mean(row.real != row.decoy) > 0.5          # (index frames sit near 128 and 255 - 128 = 127: not all differ)
    differ = total = 0
    for (a, ma), (b, mb) in zip(_elements(row, "real"), _elements(row, "decoy")):
        m = ma | mb
        differ += int(np.count_nonzero((a != b) & m))
        total += int(np.count_nonzero(m))
    print(f"{name}: {differ} of {total} output elements differ ({differ / total:.3f})")
    assert 2 * differ > total


# what include/vcf_amd.h states for every entry's output: the element type and the shape
HEADER = {
    "dct16_decode_small": [(np.uint8, (1, 40, 56, 3))],                 # n_frames * H * W * 3 bytes at rgb_dev
    "dct16_decode_large": [(np.uint8, (3, 200, 300, 3))],
    "dct7_encode": [(np.uint8, (1, 21, 35, 3))],                        # Hp x Wp x 3, H, W rounded up to B
    "dct7_decode": [(np.uint8, (1, 20, 30, 3))],
    "dct7_decode_k32": [(np.uint8, (2, 15, 18, 3))],
    "dct13_raw_decode_p": [(np.uint8, (1, 27, 40, 3))],
    "dct191_encode": [(np.uint8, (1, 382, 191, 3))],
    "dwt_encode_pipe": [(np.uint8, (2, 6 * 128 * 128 + 9 * (128 * 128 + 256 * 256 + 512 * 512)))],   # u16 LL, u8 details
    "dwt_decode_pipe": [(np.uint8, (2, 1024, 1024, 3))],
    "zlib_strips": [(np.uint8, (4, None)), (np.int32, (4,))],           # slots of slot_bytes; sizes_dev
    "inflate_strips": [(np.uint8, (4, 4096)), (np.int32, (4,))],        # out_len bytes per strip; status_dev
    "index_hist_u8": [(np.uint32, (2, 4, 3, 256))],                     # n_frames x rows * cols x 3 x 256
    "ssim_u8": [(np.int64, (2, 3, 3))],                                 # n_frames x C records of 3 x 8 bytes
    "vq_accumulate": [(np.int64, (5, 12)), (np.int64, (5,))],           # K x D sums, K counts
    "lm_histogram": [(np.int64, (3, 256))],                             # channels x (max - min + 1)
    "mdct_dz_encode": [(np.uint8, (1, 36, 42, 3))],                     # Hp = ceil((H + 2B) / B) * B
    "klt_dz_encode": [(np.uint8, (1, 16, 20, 3))],
    "dwt_encode_small": [(np.uint8, (2, 6 * 6 * 8 + 9 * (6 * 8 + 12 * 16)))],
    "dct16_encode_small": [(np.uint8, (1, 48, 64, 3))],
    "dct17_decode_warm": [(np.uint8, (1, 68, 85, 3))],
}


@pytest.mark.parametrize("name", C.NAMES + C.EXTRA_NAMES)
def test_expected_outputs_have_the_header_s_shapes_and_types(name):
    row = _row(name)
    spec = row.spec()
    assert len(spec) == len(HEADER[name])
    for (off, dtype, shape), (hd, hs) in zip(spec, HEADER[name]):
        assert dtype == np.dtype(hd) and off % 16 == 0
        assert len(shape) == len(hs) and all(b is None or a == b for a, b in zip(shape, hs)), (shape, hs)
    blob, mask = row.expected()
    assert blob.dtype == np.uint8 and blob.size == row.out_bytes
    assert mask is None or (mask.shape == blob.shape and mask.any())


def test_zlib_slots_and_workspace():
    from vcf_amd import zlib_gpu as Z
    row = _row("zlib_strips")
    (_, _, (n, slot)), _ = row.spec()
    assert n == C.ZSTRIPS and slot == Z.bound(C.ZSTRIP) and slot % 4 == 0
    assert row.ws_bytes() == Z.workspace(C.ZSTRIPS) > 0
    sizes = row.pieces()[1]
    assert np.all((0 < sizes) & (sizes <= slot))


def test_zlib_strips_are_of_both_parse_kinds():
    """Two strips for the lazy parse on the caller's stream, two for the side stream's kernels."""
    from deflate_cases import lazy_rule
    for which in ("real", "decoy"):
        a = getattr(_row("zlib_strips"), which)
        kinds = [lazy_rule(a[i * C.ZSTRIP:(i + 1) * C.ZSTRIP].tobytes())[2] for i in range(C.ZSTRIPS)]
        assert sorted(kinds) == [False, False, True, True], (which, kinds)


def test_inflate_input_is_the_deflate_row_s_output():
    z, i = _row("zlib_strips"), _row("inflate_strips")
    out, sizes = z.pieces()
    slot = out.shape[1]
    for s in range(C.ZSTRIPS):
        assert np.array_equal(i.real[s * slot:s * slot + sizes[s]], out[s, :sizes[s]])
    assert np.array_equal(i.pieces()[0].reshape(-1), z.real)
    assert np.array_equal(i.pieces("decoy")[0].reshape(-1), z.decoy)


def test_dwt_rows_take_the_pipeline():
    """enc_pipe = 1 / dec_pipe = 1 pipeline a call only with a fast filter and pipeline_default's batch
    (vcf_dwt.hip:1957, :2041); the small frame of the first-call test must not."""
    assert C.dwt_pipeline_runs(**C.DWT)
    assert not C.dwt_pipeline_runs(n=2, H=24, W=32, wavelet="bior4.4", levels=2)
    assert not C.dwt_pipeline_runs(**{**C.DWT, "n": 1})
    assert not C.dwt_pipeline_runs(**{**C.DWT, "H": 1023})
    assert _row("dwt_encode_pipe").ws_bytes() == _row("dwt_decode_pipe").ws_bytes() > 0


@pytest.mark.parametrize("name", ["mdct_dz_encode", "klt_dz_encode"])
def test_restated_rows_are_pinned_bit_for_bit(name):
    """The MDCT and KLT references are float64 restatements, equal to the kernels but for coefficients
    within 1e-9 of a quantizer threshold (tests/test_mdct_gpu.py): the real input has none."""
    margin = _row(name).exact_margin()
    print(f"{name}: least distance from a threshold {margin:.3e}")
    assert margin > 1e-6


def test_scratch_rows_grow_in_the_order_the_growth_test_needs():
    """The bytes each step of test_scratch_grows_under_queued_work asks for (stream_cases.scratch_bytes,
    restated from vcf_dct_any.hip), in the order its comments rely on: the decode scratch small < large;
    the run-time scratch B = 7 encode < B = 7 decode < B = 191 encode, the last even by its lower bound."""
    S = C.scratch_bytes
    small, large = S(40, 56, 16, decode=True)[0], S(200, 300, 16, n=3, decode=True)[0]
    assert S(40, 56, 16, decode=True)[1] == 0 and (small, large) == (48 * 64 * 6, 3 * 208 * 304 * 6) and small < large
    assert small == _row("dct16_decode_small").real.size * 2 and large == _row("dct16_decode_large").real.size * 2
    enc7, dec7, enc191 = S(20, 30, 7)[1], S(20, 30, 7, decode=True)[1], S(193, 191, 191, bluestein=True)[1]
    assert enc7 == 45 * (49 + 14 * 256) * 4 and dec7 == 2 * enc7
    assert 0 < enc7 < dec7 < enc191
    assert S(20, 30, 7, decode=True)[0] <= small            # B = 7's decode scratch: wait only after the warm call


def test_first_call_rows_never_grow_a_scratch_buffer():
    """test_first_call_of_a_process_on_a_caller_stream: the twiddle row takes no scratch at all, and the
    warm row asks for more of both buffers than any first-call row after it."""
    S = C.scratch_bytes
    assert S(40, 56, 16) == (0, 0)
    assert C.FIRST_CALL[0] == "dct16_encode_small" and C.FIRST_CALL_WARM in C.EXTRA_NAMES
    warm = S(68, 85, 17, decode=True)
    for need in (S(20, 30, 7), S(27, 40, 13, decode=True)):
        assert need[0] <= warm[0] and need[1] < warm[1], (need, warm)

"""The 2D-DWT kernels over every wavelet of the table and every compiled filter
length, against the CPU oracle, bit for bit (cases and what each group is there
to reach: tests/dwt_sweep_cases.py; that the library's dispatch sends them
there: tests/test_dwt_sweep.py, from vcf_dwt_plan).

An encode case encodes two frames in one call and compares every subband of
both with the oracle's; then the oracle's subbands (not the GPU's, so that a
decode bug cannot hide behind an encode bug) are decoded and compared with the
oracle's decode.  Every comparison is np.array_equal.

Measured on an MI355X: the 420 cases of this file pass in 15.7 s, the slowest
(a 420 x 400 case with its oracle) in 0.25 s.
"""
import numpy as np
import pytest

import dwt_sweep_cases as S

pytestmark = pytest.mark.gpu


def _check_encode(case, variant=0, n=2):
    import vcf_amd.dwt as DW
    want = S.expected_of(case, n)
    got = DW.encode(S.frames_of(case, n), case["wavelet"], case["L"], case["Q"], variant=variant)
    assert len(got) == n
    for f in range(n):
        assert sorted(got[f]) == sorted(want[f][0])
        for name, arr in want[f][0].items():
            assert got[f][name].dtype == arr.dtype and np.array_equal(got[f][name], arr), (case["name"], variant, f, name)
    return got


def _check_decode(case, variant=0, n=2):
    import vcf_amd.dwt as DW
    want = S.expected_of(case, n)
    out = DW.decode([dict(sb) for sb, _ in want], case["H"], case["W"], case["wavelet"], case["L"], case["Q"],
                    variant=variant)
    for f in range(n):
        assert out[f].shape == want[f][1].shape
        assert np.array_equal(out[f], want[f][1]), (case["name"], variant, f)


@pytest.mark.parametrize("name", S.ids(S.ALL))
def test_every_wavelet_shipped_path(name):
    c = S.by_name(name)
    _check_encode(c)
    _check_decode(c)


@pytest.mark.parametrize("name", S.ids(S.FAST))
def test_fast_lengths_strip_and_fused_levels(name):
    c = S.by_name(name)
    _check_encode(c)
    for v in S.FAST_DECODE_VARIANTS:
        _check_decode(c, v)


@pytest.mark.parametrize("name", S.ids(S.AB))
def test_uncovered_lengths_forced_kernels(name):
    """test_dwt_gpu.test_dwt_vs_oracle's shapes and refusals, for lengths it does not run."""
    import vcf_amd.dwt as DW
    from oracle import oracle as O
    c = S.by_name(name)
    _check_encode(c, c["variant"])
    dec_variant = {6: 1, 20: 0}.get(c["variant"], c["variant"])
    if min(O.dwt_shapes(c["H"], c["W"], c["L"])[-1]) < S.flen(c["wavelet"]) // 2:
        # pywt's short-input branch: an explicit request for the fused tiles is refused
        if dec_variant == 1:
            with pytest.raises(NotImplementedError):
                DW.decode(dict(S.expected_of(c)[0][0]), c["H"], c["W"], c["wavelet"], c["L"], c["Q"], variant=1)
        dec_variant = 0
    _check_decode(c, dec_variant)


@pytest.mark.parametrize("name", S.ids(S.TEN))
def test_ten_taps_generic_and_compiled(name):
    c = S.by_name(name)
    _check_encode(c)
    _check_decode(c)


@pytest.mark.parametrize("name", S.ids(S.LONG))
def test_long_filters(name):
    c = S.by_name(name)
    _check_encode(c)
    _check_decode(c)


@pytest.mark.parametrize("name", S.ids(S.RAW))
def test_raw_pyramids_decode(name):
    import vcf_amd.dwt as DW
    c = S.by_name(name)
    out = DW.decode(dict(S.raw_subbands(name)), c["H"], c["W"], c["wavelet"], c["L"], c["Q"])
    assert np.array_equal(out, S.raw_decoded(name))


@pytest.mark.parametrize("name", S.ids(S.BATCH))
def test_batch_of_five_equals_single_calls(name):
    """Five frames in one call give what five calls give, and what the oracle gives, both ways."""
    import vcf_amd.dwt as DW
    c = S.by_name(name)
    n = S.BATCH_FRAMES
    frames = S.frames_of(c, n)
    args = (c["wavelet"], c["L"], c["Q"])
    batch = _check_encode(c, n=n)
    dec = DW.decode(batch, c["H"], c["W"], *args)
    for f in range(n):
        one = DW.encode(frames[f], *args)[0]
        for sub in batch[f]:
            assert np.array_equal(batch[f][sub], one[sub]), (f, sub)
        assert np.array_equal(dec[f], DW.decode(one, c["H"], c["W"], *args)), f
    _check_decode(c, n=n)

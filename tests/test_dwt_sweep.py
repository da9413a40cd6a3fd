"""The 2D-DWT sweep (tests/dwt_sweep_cases.py) reaches the kernels it is there
for -- asked of the library's own dispatch (vcf_dwt_plan, the function the
launches consult; host only) and of the oracle's wavelet table -- and its RAW
inputs show their arithmetic.  tests/test_dwt_sweep_gpu.py runs the cases."""
import ctypes
import os
import re

import pytest

import dwt_sweep_cases as S
from conftest import ROOT
from oracle import oracle as O


def _plan(case_or_wavelet, H=None, W=None, L=None):
    import vcf_amd.dwt as DW
    if isinstance(case_or_wavelet, dict):
        c = case_or_wavelet
        return DW.plan(c["H"], c["W"], c["wavelet"], c["L"], 2)
    return DW.plan(H, W, case_or_wavelet, L, 2)


def _kinds(levels):
    return [k for k, _ in levels]


def test_all_names_are_the_wavelet_table():
    """ALL runs every entry of vcf_wavelets.h's table, the library and the oracle know each under the
    same index, and FAST is exactly the wavelets of at most 18 taps, keyed by their length."""
    import vcf_amd.dwt as DW
    src = open(os.path.join(ROOT, "vcf_amd", "csrc", "vcf_wavelets.h")).read()
    table = re.search(r"kWavelets\[\]\s*=\s*\{(.*?)\n\};", src, flags=re.S).group(1)
    names = re.findall(r"\{\s*\"([^\"]+)\"", table)
    assert len(names) == 106 and len(set(names)) == 106
    assert sorted(S.ALL_NAMES) == sorted(names) and len(S.ALL_NAMES) == 106
    for shape in S.ALL_SHAPES:
        assert sorted(c["wavelet"] for c in S.ALL if (c["H"], c["W"], c["L"], c["Q"]) == shape) == sorted(names)
    for n in names:
        assert DW.wavelet_index(n) == O.wavelet_index(n) == names.index(n), n
    for n in names:
        F = S.flen(n)
        assert (n in S.FAST_NAMES) == (F <= 18), n
        if F <= 18:
            assert n in S.FAST_BY_LEN[F], n
    assert sorted(S.FAST_BY_LEN) == list(range(2, 19, 2))
    assert sorted({S.flen(n) for n in names}) == list(range(2, 77, 2)) + [78, 84, 90, 96, 102]
    assert {c["wavelet"] for c in S.FAST if c["L"] == 3} == {c["wavelet"] for c in S.FAST if c["L"] == 2} == set(S.FAST_NAMES)


def test_all_group_plans():
    """The tiny frames of ALL: F <= 18 on a fused first level, separable later levels and the fused
    inverse; longer filters on the separable kernels, and on the short-input decode at the 9 x 12
    level of the 70 x 90 frame (F/2 > 9 for every F >= 20)."""
    for c in S.ALL:
        enc, dec = _plan(c)
        F = S.flen(c["wavelet"])
        if F <= 18 and c["wavelet"] not in S.CT_NAMES:
            assert _kinds(enc) == ["fused"] + ["separable"] * (c["L"] - 1), c["name"]
            assert _kinds(dec) == ["fused"] * c["L"], c["name"]
        elif F > 18:
            assert set(_kinds(enc)) == {"separable"}, c["name"]
            assert set(_kinds(dec)) <= {"separable", "separable_short"}, c["name"]
            if (c["H"], c["W"]) == (70, 90):
                assert _kinds(dec)[2] == "separable_short", c["name"]


def test_fast_group_reaches_every_compiled_length():
    """Across FAST, at every F = 2 .. 18: a fused first level, a fused level that is not the first, a
    fused last level and the fused inverse; at F <= 10 a strip level, at F >= 12 a fused level that is
    neither first nor last; and no wavelet but db5 and bior4.4 on compile-time taps."""
    seen = {F: set() for F in S.FAST_BY_LEN}
    for c in S.FAST:
        enc, dec = _plan(c)
        F, L = S.flen(c["wavelet"]), c["L"]
        for l, (kind, ct) in enumerate(enc, 1):
            assert bool(ct) == (c["wavelet"] in S.CT_NAMES and kind != "separable"), c["name"]
            if kind == "fused":
                seen[F] |= {"first"} if l == 1 else {"non-first"}
                seen[F] |= {"last"} if l == L else set()
                seen[F] |= {"middle"} if 1 < l < L else set()
            if kind == "strip":
                assert 1 < l < L and c["Q"] & (c["Q"] - 1) == 0
                seen[F].add("strip")
        if c["wavelet"] in S.CT_NAMES:
            assert set(_kinds(dec)) <= {"line", "band21"} and all(ct for _, ct in dec), c["name"]
        else:
            assert _kinds(dec) == ["fused"] * L and not any(ct for _, ct in dec), c["name"]
            seen[F].add("inverse")
        # what the group exists for: level 2 reads a plane above the separable threshold
        assert _kinds(enc)[1] != "separable", c["name"]
    for F, got in seen.items():
        assert {"first", "non-first", "last", "inverse"} <= got, (F, got)
        assert ("strip" in got) == (F <= 10), (F, got)
        assert ("middle" in got) == (F >= 12), (F, got)


def test_ten_group_generic_and_control():
    """The six generic 10-tap wavelets are turned away from the band, line and band21 kernels and from
    the compile-time taps on every TEN frame; db5 and bior4.4 take all of them there."""
    for w in S.GENERIC_TEN + S.CT_NAMES:
        assert S.flen(w) == 10
    assert len(S.GENERIC_TEN) == 6
    seen = {w: set() for w in S.CT_NAMES}
    for c in S.TEN:
        enc, dec = _plan(c)
        if c["wavelet"] in S.GENERIC_TEN:
            assert set(_kinds(enc)) <= {"fused", "separable"} and _kinds(enc)[0] == "fused", c["name"]
            assert _kinds(dec) == ["fused"] * c["L"], c["name"]
            assert not any(ct for _, ct in enc + dec), c["name"]
        else:
            ct = 1 if c["wavelet"] == "bior4.4" else 2
            assert enc[:2] == [("band12", ct)] * 2 and dec[:2] == [("band21", ct)] * 2, c["name"]
            assert dec[2:] == [("line", ct)] * (c["L"] - 2), c["name"]
            seen[c["wavelet"]] |= set(_kinds(enc) + _kinds(dec))
    for w, got in seen.items():
        assert {"band12", "band21", "line"} <= got, (w, got)


def test_long_group_is_separable_and_short_where_claimed():
    for c in S.LONG:
        enc, dec = _plan(c)
        F = S.flen(c["wavelet"])
        assert F >= 42 and set(_kinds(enc)) == {"separable"}, c["name"]
        short = c["L"] == 2 and F >= 62
        assert _kinds(dec) == ["separable"] * (c["L"] - 1) + ["separable_short" if short else "separable"], c["name"]
    assert sorted(S.flen(w) for w in S.LONG_NAMES) == [42, 42, 62, 76, 102]


def test_ab_raw_and_batch_lengths():
    """AB: one wavelet per fast length no earlier GPU test runs, two each at 4, 6, 10 and 14; RAW: every
    F = 2 .. 18, then 30, 40 and 62 taps, at both Q; BATCH: F = 4, 6, 14 and 102."""
    assert sorted(S.flen(w) for w in S.AB_NAMES) == [4, 4, 6, 6, 10, 10, 14, 14]
    assert not set(S.AB_NAMES) & set(S.CT_NAMES)
    for Q in (1, 300):
        assert [S.flen(c["wavelet"]) for c in S.RAW if c["Q"] == Q] == list(range(2, 19, 2)) + [30, 40, 62]
    assert [S.flen(w) for w in S.BATCH_NAMES] == [4, 6, 14, 102]
    for c in S.RAW:
        enc, dec = _plan(c)
        F = S.flen(c["wavelet"])
        want = "fused" if F <= 18 else "separable"
        assert _kinds(dec) == [want, "separable_short" if F >= 40 else want], c["name"]


def test_c3_plan_is_the_shipped_one():
    """Config C3 (2160 x 3840, bior4.4, L = 5): levels 1 + 2 in the band kernel, 3 and 4 (540 x 960 and
    270 x 480 input planes) on strips, 5 (135 x 240 = 32400 samples) separable; the decode on line
    kernels down to the levels 2 + 1 band.  db5 the same on its own taps."""
    for w, ct in (("bior4.4", 1), ("db5", 2)):
        enc, dec = _plan(w, 2160, 3840, 5)
        assert enc == [("band12", ct), ("band12", ct), ("strip", ct), ("strip", ct), ("separable", 0)]
        assert dec == [("band21", ct), ("band21", ct), ("line", ct), ("line", ct), ("line", ct)]
    # a 10-tap wavelet without compiled taps on the same frame
    enc, dec = _plan("sym5", 2160, 3840, 5)
    assert enc == [("fused", 0), ("strip", 0), ("strip", 0), ("strip", 0), ("separable", 0)]
    assert dec == [("fused", 0)] * 5


def test_plan_errors():
    import vcf_amd._lib as L
    v = [(ctypes.c_int32 * 5)(*[-7] * 5) for _ in range(4)]
    f = L.lib().vcf_dwt_plan
    assert f(0, 90, 0, 3, 1, *v) == L.VCF_ERR_INVALID
    assert f(70, 90, 106, 3, 1, *v) == L.VCF_ERR_INVALID
    assert f(70, 90, -1, 3, 1, *v) == L.VCF_ERR_INVALID
    assert f(70, 90, 0, 0, 1, *v) == L.VCF_ERR_INVALID
    assert f(70, 90, 0, 31, 1, *v) == L.VCF_ERR_INVALID
    assert f(70, 90, 0, 3, -1, *v) == L.VCF_ERR_INVALID
    assert f(70, 90, 0, 3, 21846, *v) == L.VCF_ERR_INVALID
    assert f(70, 90, 0, 3, 1, None, v[1], v[2], v[3]) == L.VCF_ERR_INVALID
    assert all(x == -7 for a in v for x in a)      # nothing written on an error
    assert f(70, 90, 0, 3, 0, *v) == 0 and f(70, 90, 0, 3, 21845, *v) == 0
    assert all(x != -7 for a in v for x in a[:3]) and all(x == -7 for a in v for x in a[3:])


@pytest.mark.parametrize("name", S.ids(S.RAW))
def test_raw_inputs_show_their_arithmetic(name):
    """At most half of the oracle's decoded pixels sit at 0 or 255; at Q = 300 a few detail indices
    (and only a few) wrap in int16, at Q = 1 the details use their whole range."""
    import numpy as np
    c = S.by_name(name)
    assert S.raw_saturation(name) <= S.RAW_CAP
    sb = S.raw_subbands(name)
    det = np.concatenate([v.ravel() for k, v in sb.items() if not k.startswith("LL")])
    if c["Q"] == 300:
        assert 3 <= S.raw_wraps(name) <= 20
    else:
        assert (det.min(), det.max()) == ((0, 255) if c["spread"] == 127 else (128 - c["spread"], 128 + c["spread"]))
        ll = sb[f"LL_{c['L']}"].astype(np.int16).astype(int) - 128
        assert ll[..., 0].min() >= 0 and ll[..., 0].max() > 900 and ll[..., 1:].min() < -400 and ll[..., 1:].max() > 400

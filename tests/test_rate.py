"""The host side of the rate control: the entropy of counts, the two byte models, the bisection
rule against a Python restatement of it, and the new command-line flags."""
import math

import numpy as np
import pytest

from vcf_amd import rate as R
from vcf_amd.codec import parser as P
from vcf_amd.codec import ratecontrol as RC


# ---- entropy_bits / estimate_bytes -------------------------------------------------------------
def test_entropy_of_hand_made_counts():
    c = np.zeros((4, 256), np.uint32)
    c[0, 77] = 1000                    # a single symbol
    c[1, :] = 5                        # uniform over the 256 symbols: 8 bits each
    c[3, 3], c[3, 200] = 6, 2          # 6 * log2(8 / 6) + 2 * log2(8 / 2)
    bits = R.entropy_bits(c)
    assert bits.dtype == np.float64 and bits.shape == (4,)
    assert bits[0] == 0.0
    assert bits[1] == 8.0 * 5 * 256
    assert bits[2] == 0.0              # empty: no NaN
    assert bits[3] == 6 * math.log2(8 / 6) + 2 * 2.0
    assert np.isfinite(bits).all()


def test_entropy_is_reproducible_and_checks_its_input():
    rng = np.random.Generator(np.random.PCG64(5))
    c = rng.integers(0, 1 << 20, (3, 2, 3, 256), dtype=np.uint32)
    a, b = R.entropy_bits(c), R.entropy_bits(c.copy())
    assert a.shape == (3, 2, 3) and np.array_equal(a, b)
    # the stated order: ascending symbol, one add at a time
    one = c[1, 0, 2].astype(np.float64)
    N = 0.0
    for v in range(256):
        N += one[v]
    want = 0.0
    for v in range(256):
        if one[v] > 0:
            want += one[v] * np.log2(N / one[v])
    assert a[1, 0, 2] == want
    with pytest.raises(ValueError):
        R.entropy_bits(np.zeros((3, 255), np.uint32))
    with pytest.raises(TypeError):
        R.entropy_bits(np.zeros((3, 256), np.float32))


def test_estimate_models():
    c = np.zeros((2, 2, 3, 256), np.uint32)
    c[0, 0, 0, :] = 4                  # 1024 symbols x 8 bits = 1024 bytes
    c[0, 1, 0, 9] = 1024               # the other region: one symbol, 0 bits on its own
    c[0, 0, 1, 7] = 9
    sub = R.estimate_bytes(c, "subband")
    assert sub.dtype == np.int64
    assert sub.tolist() == [1024 + 3 * R.MODEL_BYTES, 0]      # frame 1 is empty: 0 bytes, no model
    # order0 merges the regions: channel 0 is then 2048 symbols, half of them one value
    merged = np.zeros(256)
    merged[:] = 4
    merged[9] += 1024
    bits = sum(m * math.log2(2048 / m) for m in merged)
    assert R.estimate_bytes(c, "order0").tolist() == [math.ceil(bits / 8), 0]
    with pytest.raises(ValueError):
        R.estimate_bytes(c, "order1")
    with pytest.raises(ValueError):
        R.estimate_bytes(c[0], "subband")
    assert "model" in R.estimate_bytes.__doc__ and "not a claim" in R.estimate_bytes.__doc__


# ---- the bisection -----------------------------------------------------------------------------
def restated(rate, budget, q_min, q_max):
    """The rule of the issue for one frame, in plain Python: -> (q, met, probes)."""
    probes = 1
    if rate(q_max) > budget:
        return q_max, False, probes
    if q_min == q_max:
        return q_max, True, probes
    probes += 1
    if rate(q_min) <= budget:
        return q_min, True, probes
    lo, hi = q_min, q_max
    while hi > lo + 1:
        mid = (lo + hi) // 2
        probes += 1
        if rate(mid) <= budget:
            hi = mid
        else:
            lo = mid
    return hi, True, probes


def monotone(q):
    return 90000 // q + 40


def bumpy(q):
    """Falls with q on the whole, with bumps of up to 30 % that break monotony."""
    return 90000 // q + 40 + (q * 7919 % 13) * (27000 // q) // 12


@pytest.mark.parametrize("rate", [monotone, bumpy], ids=["monotone", "non_monotone"])
@pytest.mark.parametrize("q_min,q_max", [(1, 2048), (1, 1), (3, 4), (5, 100), (17, 1000)])
def test_bisection_is_the_stated_rule(rate, q_min, q_max):
    if rate is bumpy:
        assert any(bumpy(q + 1) > bumpy(q) for q in range(1, 2048))
    budgets = np.array([10, 41, 84, 85, 200, 1000, 4321, 20000, 89999, 90040, 10 ** 7], np.int64)
    calls = []

    def rate_fn(q, active):
        calls.append((q.copy(), active.copy()))
        return np.array([rate(int(x)) for x in q], np.int64)

    q, met, got, steps = RC.bisect_q(rate_fn, budgets, q_min, q_max)
    bound = math.ceil(math.log2(q_max - q_min + 1)) + 2
    assert RC.probe_bound(q_min, q_max) == bound
    assert steps == len(calls) <= bound
    per_frame = np.sum([a for _, a in calls], axis=0)
    for i, b in enumerate(budgets):
        wq, wmet, wprobes = restated(rate, int(b), q_min, q_max)
        assert (int(q[i]), bool(met[i])) == (wq, wmet), (i, b)
        assert per_frame[i] == wprobes <= bound
        assert got[i] == rate(int(q[i]))
        if met[i]:
            assert rate(int(q[i])) <= b                     # the budget is met
        else:
            assert q[i] == q_max and rate(q_max) > b        # nothing within the range does
    if rate is monotone:                                     # then the rule's outcome is the smallest q that fits
        for i, b in enumerate(budgets):
            fits = [x for x in range(q_min, q_max + 1) if rate(x) <= b]
            assert (int(q[i]) == fits[0]) if fits else not met[i]


def test_bisection_arguments():
    with pytest.raises(ValueError):
        RC.bisect_q(lambda q, a: q, [1], 0, 8)
    with pytest.raises(ValueError):
        RC.bisect_q(lambda q, a: q, [1], 9, 8)
    q, met, got, steps = RC.bisect_q(lambda q, a: q, np.zeros(0, np.int64))
    assert len(q) == 0 and steps == 0


def test_budgets_and_runs():
    assert RC.budgets_of(3, 64, 96, target_bpp=1.0).tolist() == [768] * 3
    assert RC.budgets_of(2, 64, 96, target_bytes=[5, 9]).tolist() == [5, 9]
    assert RC.budgets_of(2, 10, 10, target_bpp=0.33).tolist() == [4, 4]     # floor(4.125)
    for kw in ({}, dict(target_bytes=1, target_bpp=1.0), dict(target_bytes=-1)):
        with pytest.raises(ValueError):
            RC.budgets_of(1, 8, 8, **kw)
    q = np.array([4, 4, 9, 9, 9, 4, 4])
    act = np.array([1, 1, 1, 0, 1, 1, 1], bool)
    assert RC._runs(q, act) == [(0, 2, 4), (2, 1, 9), (4, 1, 9), (5, 2, 4)]


# ---- the command line ---------------------------------------------------------------------------
NEW_ENCODE = dict(target_bpp=None, target_bytes=None, rate="estimate", q_min=1, q_max=2048)
NEW_DECODE = dict(q_from_files=False)


def _ns(p, argv):
    d = vars(P.parse(p, argv))
    d.pop("func")
    return d


def test_new_flags_parse():
    d = _ns(P.rate_control_parser(), ["encode", "--target_bpp", "0.75", "--rate", "coded", "-B", "16", "-x"])
    assert d["target_bpp"] == 0.75 and d["target_bytes"] is None and d["rate"] == "coded"
    assert d["block_size_DCT"] == 16 and d["disable_subbands"]
    d = _ns(P.rate_control_parser(), ["encode", "--target_bytes", "4000", "--q_min", "2", "--q_max", "99"])
    assert (d["target_bytes"], d["q_min"], d["q_max"], d["rate"]) == (4000, 2, 99, "estimate")
    assert _ns(P.rate_control_parser(), ["decode", "--q_from_files"])["q_from_files"] is True
    d = _ns(P.iii_parser(rate_control=True), ["encode", "--target_bpp", "2", "-N", "3"])
    assert d["target_bpp"] == 2.0 and d["number_of_frames"] == 3
    assert _ns(P.iii_parser(rate_control=True), ["decode", "--q_from_files"])["q_from_files"] is True
    with pytest.raises(BaseException):
        P.rate_control_parser().parse_args(["encode", "--rate", "guess"])


@pytest.mark.parametrize("transform", ["2D-DCT", "2D-DWT", "2D-MDCT", "2D-KLT", "2D-LBT"])
def test_existing_defaults_are_unchanged(transform):
    """The Namespace of every existing parser is what it was; with the new flags it is the same
    Namespace plus their defaults, which take the existing path (None / False)."""
    for sub, new in (("encode", NEW_ENCODE), ("decode", NEW_DECODE)):
        plain = _ns(P.iii_parser(transform=transform), [sub])
        assert not set(plain) & set(new)
        with_flags = _ns(P.iii_parser(transform=transform, rate_control=True), [sub])
        assert with_flags == {**plain, **new}
    assert list(_ns(P.iii_parser(), ["encode"]).items()) == [
        ("debug", False), ("subparser_name", "encode"), ("transform", "2D-DCT"), ("number_of_frames", 20),
        ("block_size_DCT", 8), ("color_transform", "YCoCg"), ("perceptual_quantization", False),
        ("Lambda", None), ("disable_subbands", False), ("quantizer", "deadzone"), ("QSS", 32),
        ("entropy_image_codec", "TIFF"), ("original", "/tmp/original.png"), ("encoded", "/tmp/encoded")]
    for sub, new in (("encode", NEW_ENCODE), ("decode", NEW_DECODE)):
        plain = _ns(P.dct_parser(), [sub])
        assert not set(plain) & set(new)
        assert _ns(P.rate_control_parser(), [sub]) == {**plain, **new}


def test_new_flags_are_refused_off_the_dct_path():
    for transform in ("2D-DWT", "2D-MDCT", "2D-KLT", "2D-LBT"):
        for sub, argv in (("encode", ["--target_bpp", "1"]), ("encode", ["--target_bytes", "900"]),
                          ("decode", ["--q_from_files"])):
            args = P.parse(P.iii_parser(transform=transform, rate_control=True), [sub, "-T", transform] + argv)
            with pytest.raises(NotImplementedError):
                RC.refuse_unless_dct(args, args.transform)
        RC.refuse_unless_dct(P.parse(P.iii_parser(transform=transform, rate_control=True), ["encode", "-T", transform]),
                             transform)
    RC.refuse_unless_dct(P.parse(P.iii_parser(rate_control=True), ["encode", "--target_bpp", "1"]), "2D-DCT")
    lm = P.parse(P.dct_parser(quantizer="LloydMax"), ["encode", "-a", "LloydMax"])
    from vcf_amd.codec.dct2d import CoDec
    with pytest.raises(NotImplementedError):
        RC._check_codec(CoDec(lm))
    with pytest.raises(NotImplementedError):
        RC._check_codec(object())

"""RDOQ without a GPU: the cost table, the numpy restatement of the rule (tests/rdoq_ref.py), the
--rdoq option and the codecs' refusals.  The kernel itself is tests/test_rdoq_gpu.py's."""
import numpy as np
import pytest

import rdoq_ref as RR
from oracle import ref_numpy as RN
from vcf_amd import rdoq as R
from vcf_amd.codec import parser as P


# ---- cost_table ---------------------------------------------------------------------
def test_cost_table_on_hand_made_counts():
    c = np.zeros((1, 64, 3, 256), np.uint32)
    c[0, 1, 0, 128] = 1000                       # a single symbol
    c[0, 2, :, :] = 7                            # uniform
    c[0, 3, 1, 128], c[0, 3, 1, 129], c[0, 3, 1, 127] = 90, 5, 5
    bits = R.cost_table(c)
    assert bits.shape == c.shape and bits.dtype == np.float64
    assert np.isfinite(bits).all() and (bits >= 0).all()
    assert np.array_equal(bits[0, 0], np.full((3, 256), 8.0))                 # empty: log2(256 / 1)
    assert bits[0, 1, 0, 128] == np.log2(1256.0 / 1001.0)
    assert np.all(bits[0, 1, 0, :128] == np.log2(1256.0)) and np.all(bits[0, 1, 0, 129:] == np.log2(1256.0))
    assert np.array_equal(bits[0, 2], np.full((3, 256), 8.0))                 # (7 * 256 + 256) / 8
    assert bits[0, 3, 1, 129] == bits[0, 3, 1, 127] == np.log2(356.0 / 6.0)   # equal counts, equal bits
    assert bits[0, 3, 1, 128] < bits[0, 3, 1, 129] < bits[0, 3, 1, 0]
    with pytest.raises(TypeError):
        R.cost_table(c.astype(np.float32))
    with pytest.raises(ValueError):
        R.cost_table(np.zeros((3, 255), np.uint32))


def test_lambda_scales_with_q_squared():
    assert R.lambda_of(0.2, 32) == 0.2 * 32 * 32 and R.lambda_of(0, 5) == 0.0
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            R.lambda_of(bad, 32)


# ---- the restatement ----------------------------------------------------------------
def _frame(H, W, seed):
    return np.random.Generator(np.random.PCG64(seed)).integers(0, 256, (H, W, 3), dtype=np.uint8)


@pytest.mark.parametrize("Q", [3, 32])
@pytest.mark.parametrize("subbands", [True, False])
def test_lambda_zero_is_the_oracle_s_encode(Q, subbands):
    rgb = _frame(29, 45, 1)
    bits = np.random.Generator(np.random.PCG64(2)).random((64, 3, 256)) * 16
    assert np.array_equal(RR.encode_frame(rgb, Q, 0.0, bits, subbands), RN.encode_frame(rgb, Q, subbands))


def _one(c, Q, lam, bits):
    """The rule on one coefficient at region 0, channel 0."""
    a = np.zeros((8, 8, 3), np.float32)
    a[0, 0, 0] = c
    return int(RR.decide(a, Q, lam, bits)[0, 0, 0])


def test_the_rule_on_hand_made_coefficients():
    Q = 10
    bits = np.zeros((64, 3, 256))
    bits[0, 0, 128 + 3], bits[0, 0, 128 + 2], bits[0, 0, 128] = 5.0, 4.0, 1.0
    # c = 34: k0 = 3 (d = 4), 2 (d = 14), 0 (d = 34)
    assert _one(34.0, Q, 0.0, bits) == 3
    assert _one(34.0, Q, 179.0, bits) == 3          # 16 + 5 l < 196 + 4 l  <=>  l < 180
    assert _one(34.0, Q, 181.0, bits) == 2
    assert _one(34.0, Q, 180.0, bits) == 2          # a tie goes to the smaller magnitude
    # 2 against 0: 196 + 4 l against 1156 + l: l = 320 ties, and 0 wins it
    assert _one(34.0, Q, 319.0, bits) == 2 and _one(34.0, Q, 320.0, bits) == 0
    # negative side mirrors (its own table entries)
    bits[0, 0, 128 - 3], bits[0, 0, 128 - 2] = 5.0, 4.0
    assert _one(-34.0, Q, 180.0, bits) == -2 and _one(-34.0, Q, 179.0, bits) == -3
    # k0 = 1: the only other candidate is 0, compared once
    bits[0, 0, 128 + 1] = 3.0
    assert _one(14.0, Q, 89.0, bits) == 1 and _one(14.0, Q, 90.0, bits) == 0    # 16 + 3 l against 196 + l
    # zero skips a level when the level between is dear
    bits[0, 0, 128 + 2] = 1000.0
    assert _one(34.0, Q, 300.0, bits) == 0          # 16 + 1500 > 1156 + 300
    assert _one(4.0, Q, 1e9, bits) == 0             # k0 = 0 stays


def test_indices_beyond_a_byte_are_untouched():
    bits = np.zeros((64, 3, 256))
    bits[:, :, 128] = 0.0
    bits[:, :, :128] = 50.0
    bits[:, :, 129:] = 50.0
    for c, k0 in ((1285.0, 128), (-1295.0, -129), (2000.0, 200)):
        assert _one(c, 10, 1e6, bits) == k0
    assert _one(1275.0, 10, 1e6, bits) == 0 and _one(-1285.0, 10, 1e6, bits) == 0    # 127 and -128 are candidates
    rgb = np.full((8, 8, 3), 255, np.uint8)         # Y = 127, DC = 1016: beyond a byte at Q = 1
    assert np.array_equal(RR.encode_frame(rgb, 1, 1e6, bits)[0, 0], RN.encode_frame(rgb, 1)[0, 0])


def test_never_up_and_never_dearer():
    rgb = _frame(40, 56, 3)
    bits = np.random.Generator(np.random.PCG64(4)).random((64, 3, 256)) * 16
    for Q, mu in ((5, 0.3), (32, 10.0)):
        lam = mu * Q * Q
        k0 = RN.encode_frame(rgb, Q).astype(np.int32) - 128
        k = RR.encode_frame(rgb, Q, lam, bits).astype(np.int32) - 128
        assert np.all(np.abs(k) <= np.abs(k0)) and np.all(k[k0 == 0] == 0) and np.any(k != k0)
        assert RR.total_cost(rgb, k + 128, Q, lam, bits) <= RR.total_cost(rgb, k0 + 128, Q, lam, bits)


def test_counts_of_is_the_histogram_s_layout():
    idx = RN.encode_frame(_frame(32, 48, 5), 8)
    c = RR.counts_of(idx)
    assert c.sum() == idx.size and np.all(c.sum(axis=2) == idx.size // (64 * 3))
    assert c[0, 1, idx[0, 0, 1]] >= 1


# ---- the option ---------------------------------------------------------------------
FACTORIES = [
    (lambda **kw: P.dct_parser(**kw), ["encode"]),
    (lambda **kw: P.iii_parser(**kw), ["encode"]),
    (lambda **kw: P.iii_parser(rate_control=True, **kw), ["encode"]),
    (lambda **kw: P.rd_curve_parser(**kw), []),
]


@pytest.mark.parametrize("make,argv", FACTORIES)
def test_the_flag_parses_through_each_factory(make, argv):
    a = P.parse(make(rdoq=True), argv + ["--rdoq", "0.2"])
    assert a.rdoq == 0.2
    assert P.parse(make(rdoq=True), argv).rdoq is None
    plain = vars(P.parse(make(), argv))
    assert "rdoq" not in plain                       # without the keyword: the Namespace as it was
    with_kw = vars(P.parse(make(rdoq=True), argv))
    assert {k: v for k, v in with_kw.items() if k != "rdoq"} == plain
    assert not hasattr(P.parse(make(), argv + ["--rdoq", "0.2"]), "rdoq")   # unknown there, as before


def test_decode_and_rate_control_have_no_flag():
    assert not hasattr(P.parse(P.dct_parser(rdoq=True), ["decode"]), "rdoq")
    assert not hasattr(P.parse(P.rate_control_parser(), ["encode"]), "rdoq")


# ---- refusals -----------------------------------------------------------------------
def _args(*argv):
    return P.parse(P.dct_parser(rdoq=True, quantizer=P.quantizer_of(list(argv))), ["encode", "--rdoq", "0.2", *argv])


@pytest.mark.parametrize("argv", [("-B", "16"), ("-p",), ("-L", "1.0"), ("-a", "LloydMax")])
def test_the_codec_refuses_what_rdoq_does_not_cover(argv):
    from vcf_amd.codec.dct2d import CoDec
    with pytest.raises(NotImplementedError, match="--rdoq"):
        CoDec(_args(*argv))


def test_a_negative_mu_is_an_error():
    from vcf_amd.codec.dct2d import CoDec
    with pytest.raises(ValueError):
        CoDec(P.parse(P.dct_parser(rdoq=True), ["encode", "--rdoq", "-1"]))


@pytest.mark.parametrize("transform", ["2D-DWT", "2D-MDCT", "2D-KLT", "2D-LBT"])
def test_iii_refuses_the_other_transforms(transform):
    from vcf_amd.codec.iii import CoDec
    a = P.parse(P.iii_parser(transform=transform, rdoq=True), ["encode", "-T", transform, "--rdoq", "0.2"])
    with pytest.raises(NotImplementedError, match="--rdoq"):
        CoDec(a)


def test_rd_curve_refuses_other_block_sizes_and_p():
    from vcf_amd.codec.rde import rd_curve
    from vcf_amd.dct import VCF_DCT_PERCEPTUAL
    f = np.zeros((16, 16, 3), np.uint8)
    with pytest.raises(NotImplementedError):
        rd_curve(f, [32], block_size=16, rdoq=0.2)
    with pytest.raises(NotImplementedError):
        rd_curve(f, [32], flags=VCF_DCT_PERCEPTUAL, rdoq=0.2)

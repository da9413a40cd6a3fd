"""The 2D-KLT kernels over block sizes, flags, Q and raw indices.

vcf_klt_dz.hip takes its tile and LDS class from the block size (see
tests/klt_sweep_cases.py), so the cases walk B = 2 .. 16, odd sizes included,
with and without -x, at Q = 1 (where the encoder's wrap to u8 takes a few
percent of the indices), 32 and 300, with seeded random orthonormal weights,
and add index frames no encoder writes.  tests/test_klt.py proves on the host
that no reference depends on the summation order.  The comparison is
test_klt_gpu._compare: equal to the float64 restatement, but for positions
within 1e-9 of a threshold where the GPU is one step away, at most 1 in 10^5."""
import pytest

import klt_restated as K
import klt_sweep_cases as S
from test_klt_gpu import _compare

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    import vcf_amd.klt as G
    return G


def _decode_equals_the_restatement(G, name):
    c = S.by_name(name)
    want = S.decoded(name)
    got = G.decode(S.indices(name), *S.FRAME, c["Q"], c["flags"], c["B"], S.weights32(c["B"]))
    _compare(f"{name} pixels", got, want["rgb"], K.pixel_margin(want["pre"]))


@pytest.mark.parametrize("name", S.ENCODE_IDS)
def test_encode_and_decode_against_the_restatement(G, name):
    c = S.by_name(name)
    want = S.encoded(name)
    k, _ = G.encode(S.frame(c["B"]), c["Q"], c["flags"], c["B"], weights=S.weights(c["B"]))
    _compare(f"{name} indices", k, want["k"], K.index_margin(want["pre"], c["Q"]))
    _decode_equals_the_restatement(G, name)


@pytest.mark.parametrize("name", S.RAW_IDS)
def test_raw_indices_against_the_restatement(G, name):
    _decode_equals_the_restatement(G, name)

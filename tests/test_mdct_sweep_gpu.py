"""The lapped 2D-MDCT kernels over block sizes, tiles and raw indices.

What vcf_mdct_dz.hip does depends on the block size: the tile, the LDS class
(three encode and six decode instantiations), the guards of the 8-wide
coefficient groups, the scale and the synthesis normalisation.  The cases of
tests/mdct_sweep_cases.py walk 3 <= B <= 64 on one small frame, with -x, -p and
several Q, and add index frames no encoder writes: dense ones, and ones whose
Q (k - 128) leaves int16.  tests/test_mdct.py proves on the host what each case
launches and that its reference does not depend on the summation order.  The
comparison is test_mdct_gpu._compare: equal to the float64 restatement, but for
positions within 1e-9 of a threshold where the GPU is one step away, at most 1
in 10^5."""
import numpy as np
import pytest

import mdct_restated as M
import mdct_sweep_cases as S
from test_mdct_gpu import _compare

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    import vcf_amd.mdct as G
    return G


def _decode_equals_the_restatement(G, name):
    c = S.by_name(name)
    H, W = c["shape"]
    want = S.decoded(name)
    print(f"{name} decode plan (TX, TY, class, tiles): {G.tile_plan(H, W, c['B'], c['flags'], True)}")
    _compare(f"{name} pixels", G.decode(S.indices(name), H, W, c["Q"], c["flags"], c["B"]), want["rgb"],
             M.pixel_margin(want["pre"]))


@pytest.mark.parametrize("name", S.ENCODE_IDS)
def test_encode_and_decode_against_the_restatement(G, name):
    c = S.by_name(name)
    H, W = c["shape"]
    want = S.encoded(name)
    print(f"{name} encode plan (TX, TY, class, tiles): {G.tile_plan(H, W, c['B'], c['flags'], False)}")
    _compare(f"{name} indices", G.encode(S.frame(H, W, c["B"]), c["Q"], c["flags"], c["B"]), want["k"],
             M.index_margin(want["pre"], c["Q"]))
    _decode_equals_the_restatement(G, name)


@pytest.mark.parametrize("name", S.RAW_IDS)
def test_raw_indices_against_the_restatement(G, name):
    _decode_equals_the_restatement(G, name)


def test_class_2_batch_equals_single_frames(G):
    """Three frames in one launch of the 156 KiB kernels: no result depends on the batch position."""
    H, W = S.FRAME
    frames = np.stack([M.synth_frame(H, W, s) for s in (1, 2, 3)])
    for B, decode in S.BATCH:
        assert G.tile_plan(H, W, B, 0, decode)[2] == 2
        k = G.encode(frames, 7, 0, B)
        y = G.decode(k, H, W, 7, 0, B)
        for i in range(3):
            ki = G.encode(frames[i], 7, 0, B)
            assert np.array_equal(k[i], ki)
            assert np.array_equal(y[i], G.decode(ki, H, W, 7, 0, B))
        assert not np.array_equal(k[0], k[1])

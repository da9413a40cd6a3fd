"""The 2D-LBT kernels over every block size, many tiles per frame and raw indices.

vcf_lbt.hip takes its tile and LDS class from the block size, so the cases (tests/lbt_sweep_cases.py)
walk B = 2 .. 8 on a 150 x 210 frame: 4 to 8 encode and decode workgroups per frame with a partial last
tile, both LDS classes, 2 to 4 staged tiles and up to 4 chunks in the moments kernel, with and without
-x, at Q = 1 (where the clamp takes a few percent of the indices), 8 and 32, -p at B = 8 and 5, with a
seeded orthonormal encoder and its transpose, and index frames no encoder writes (uniform at Q = 1;
at Q = 300 the int16 dequantizer wraps).  tests/test_lbt.py proves on the host, from
vcf_lbt_tile_plan, that the launches are those, and that every case shows its arithmetic.  The
comparison is test_lbt_gpu's: equal to the restatement off the boundary set, one step on it.

Measured on an MI355X (printed by the tests before they assert): 50 index frames and 65 pixel frames
compared, no position differing, on the boundary sets (at most 0.19 % of the indices, 0.72 % of the
pixels) or off them; every moment sum equal; 20 epochs at B = 2, 5, 6, 7 end 1.00, 1.25, 1.18 and 2.37 x
d_proxy from the restatement (bound 4 x c x d_proxy = 11.2 x d_proxy, c = 2.804 from fixture rand_9x9).
"""
import numpy as np
import pytest

import lbt_restated as R
import lbt_sweep_cases as S
from test_lbt_gpu import _check_indices, _check_pixels

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    import vcf_amd.lbt as G
    return G


def _decode_equals_the_restatement(G, name):
    c = S.by_name(name)
    want = S.decoded(name)
    got = G.decode(S.indices(name), *S.FRAME, c["Q"], c["flags"], c["B"], S.wd(c["B"]), S.mean_of(c))
    assert got.shape == S.FRAME + (3,) and got.dtype == np.uint8
    _check_pixels(got, want, c["B"] ** 2, want["rgb"])


@pytest.mark.parametrize("name", S.ENCODE_IDS)
def test_encode_and_decode_against_the_restatement(G, name):
    c = S.by_name(name)
    B = c["B"]
    want = S.encoded(name)
    k, w_back, m_back = G.encode(S.frame(B), c["Q"], c["flags"], B, weights=S.we(B), mean=S.mean(B))
    assert k.shape == want["k"].shape and k.dtype == np.uint8
    assert np.array_equal(w_back, S.we(B)) and m_back == S.mean(B)
    _check_indices(k, want, B * B)
    _decode_equals_the_restatement(G, name)


@pytest.mark.parametrize("name", S.RAW_IDS)
def test_raw_indices_against_the_restatement(G, name):
    _decode_equals_the_restatement(G, name)


def test_moments_are_exact_over_chunks(G):
    """Several staged tiles per workgroup and several workgroups per frame and channel: every sum is
    the float64 one, for a single frame and for two frames in one launch."""
    for f, Bs in ((S.frame, S.SWEEP_B), (lambda B: S.chunk_frame(), (8,))):
        for B in Bs:
            a = f(B)
            b = np.ascontiguousarray(a[::-1, ::-1])
            want = []
            for rgb in (a, b):
                X = R.blocks(rgb, B).astype(np.float64)
                want.append((X.sum(0), X.T @ X))
            S1, S2 = G.moments(a, B)
            assert np.array_equal(S1, want[0][0]) and np.array_equal(S2, want[0][1]), (a.shape, B)
            S1, S2 = G.moments(np.stack([a, b]), B)
            for i in range(2):
                assert np.array_equal(S1[i], want[i][0]) and np.array_equal(S2[i], want[i][1]), (a.shape, B, i)


@pytest.mark.parametrize("B", [7, 2])
def test_batch_of_multi_tile_frames(G, B):
    """Three 150 x 210 frames, each with its own matrices and mean, in one launch: blockIdx.y together
    with blockIdx.x > 0."""
    H, W = S.FRAME
    D, Q = B * B, 8
    frames = np.stack([S.frame(B), R.synth_frame(H, W, 700 + B), R.synth_frame(H, W, 710 + B)])
    wes = np.stack([S.we(B), S.orthonormal(D, 720 + B), S.we(B)[::-1]])
    wds = np.ascontiguousarray(wes.transpose(0, 2, 1))
    means = np.array([S.mean(B), 3.5, -20.25], np.float32)
    for fl in (0, R.NO_SUBBANDS):
        ks = G.encode(frames, Q, fl, B, weights=wes, mean=means)[0]
        for i in range(3):
            assert np.array_equal(ks[i], G.encode(frames[i], Q, fl, B, weights=wes[i], mean=means[i])[0]), (fl, i)
        _check_indices(ks[1], R.encode(frames[1], wes[1], means[1], B, Q, fl), D)
        out = G.decode(ks, H, W, Q, fl, B, wds, means)
        for i in range(3):
            assert np.array_equal(out[i], G.decode(ks[i], H, W, Q, fl, B, wds[i], means[i])), (fl, i)
        d = R.decode(ks[1], H, W, wds[1], means[1], B, Q, fl)
        _check_pixels(out[1], d, D, d["rgb"])
    assert not np.array_equal(ks[0], ks[2])


@pytest.mark.parametrize("B", S.TRAIN_B)
def test_short_training_at_untested_block_sizes(G, B):
    """20 epochs from the product's initial weights on a 37 x 45 frame: both matrices within
    4 x c x d_proxy of the float64 row-wise restatement's.  d_proxy is how far the restatement's own
    float32 run ends from it, and c the largest d_ref / d_proxy over the 20-epoch fixtures
    (lbt_sweep_cases.proxy_scale; tests/test_lbt.py), so this is the fixtures' 4 x d_ref criterion
    carried over to block sizes that have no torch run."""
    want = S.trained(B)
    c = S.proxy_scale()
    rgb = S.train_frame(B)
    t = G.train(rgb, B, 20, init=G.initial_weights(B))
    dE, dD = float(np.max(np.abs(t["we"] - want["we"]))), float(np.max(np.abs(t["wd"] - want["wd"])))
    print(f"B = {B}: |We - restated| {dE:.3e}, |Wd - restated| {dD:.3e}, d_proxy {want['d_proxy']:.3e}, c {c:.3f}, "
          f"ratio to d_proxy {max(dE, dD) / want['d_proxy']:.2f}, to c x d_proxy {max(dE, dD) / (c * want['d_proxy']):.2f}")
    assert abs(float(t["mean"]) - float(want["mean"])) <= 2.0 ** -17
    X = R.centred(rgb, B, float(t["mean"])).astype(np.float64)
    loss = R.loss_terms(X, t["we"].astype(np.float64), t["wd"].astype(np.float64))
    assert np.allclose(t["loss"], loss, rtol=1e-3, atol=1e-6)      # the kernel's own float32 report
    assert max(dE, dD) <= 4 * c * want["d_proxy"]

"""What makes tests/test_batch_split_gpu.py meaningful, proved on the host.

The GPU tests compare every frame of a batch of N > 65535 frames with the
reference's output for the pool entry the frame repeats.  That tells a frame
mix-up only if no two pool entries have the same expected output, if the batch
crosses the launchers' 65535-frame split, if the second launch does not start
on a multiple of the pool, and if the builder really places entry f % 251 at
frame f.  For the any-B decode the shapes must give more than one workspace
chunk by the launcher's own rule, and the frames must differ."""
import numpy as np
import pytest

import batch_split_cases as S
from oracle import oracle as O


def test_the_batch_crosses_the_split_off_the_pool_period():
    assert S.P == 251 and S.SPLIT == 65535
    assert S.N > S.SPLIT
    assert (S.N - S.SPLIT) % S.P != 0
    assert S.SPLIT % S.P == 24          # frame f of the second launch never repeats frame f - 65535
    assert S.N - S.SPLIT == 27          # a short, odd second launch
    assert S.PROBES == (0, 65534, 65535, 65536, S.N - 1)


def _expected_pools():
    out = {}
    for name in S.DCT_IDS:
        out[f"dct {name} indices"] = S.dct(name)["k"]
        out[f"dct {name} pixels"] = S.dct(name)["decoded"]
    out["mdct indices"], out["mdct pixels"] = S.mdct()["k"], S.mdct()["decoded"]
    for fl in (0, 1):
        k, b = S.klt(fl), S.lbt(fl)
        out[f"klt flags {fl} indices"], out[f"klt flags {fl} pixels"] = k["k"], k["decoded"]
        out[f"lbt flags {fl} indices"], out[f"lbt flags {fl} pixels"] = b["k"], b["decoded"]
    out["klt S1"], out["klt S2"], out["klt weights"] = S.klt()["S1"], S.klt()["S2"], S.klt()["w32"]
    out["lbt S1"], out["lbt S2"], out["lbt mean"] = S.lbt()["S1"], S.lbt()["S2"], S.lbt()["mean"]
    t = S.lbt_training()
    out["lbt trained we"], out["lbt trained wd"] = t["we"], t["wd"]
    d = S.distortion()
    out["distortion records"] = np.stack([d["sse"], d["sad"], d["max_abs"]], -1)
    out["distortion sse"] = d["sse"]
    s = S.ssim()
    out["ssim sum_k"], out["ssim min_k"] = s["sum_k"], s["min_k"]
    for w in S.DWT_WAVELETS:
        out[f"dwt {w} subbands"], out[f"dwt {w} pixels"] = S.dwt(w)["packed"], S.dwt(w)["decoded"]
    return out


@pytest.fixture(scope="module")
def pools():
    return _expected_pools()


def test_expected_outputs_are_pairwise_distinct(pools):
    for what, pool in pools.items():
        assert np.asarray(pool).shape[0] == S.P, what
        assert S.pairwise_distinct(pool), f"{what}: two pool entries have the same expected output"


def test_the_builder_places_entry_f_mod_251_at_frame_f(pools):
    e = S.entry_of()
    assert e.shape == (S.N,)
    for what in ("dct 5x7_q7 indices", "klt weights", "lbt mean", "distortion records"):
        pool = np.asarray(pools[what])
        big = S.batch(pool)
        assert big.shape == (S.N,) + pool.shape[1:] and big.dtype == pool.dtype
        for f in S.PROBES:
            assert np.array_equal(big[f], pool[f % S.P]), (what, f)
        # the second launch's frame f holds neither frame f - 65535's content nor frame (f % 65535)'s
        for f in range(S.SPLIT, S.N):
            assert not np.array_equal(big[f], big[f - S.SPLIT]), (what, f)


def test_the_dwt_batch_is_the_largest_the_entries_take():
    import vcf_amd.dwt as DW
    assert S.DWT_N == 21845 and 3 * S.DWT_N == S.SPLIT      # the last plane is 65534
    assert S.DWT_N % S.P != 0
    c = S.DWT
    for w in S.DWT_WAVELETS:
        assert DW.plan(c["H"], c["W"], w, c["L"], S.DWT_N) == DW.plan(c["H"], c["W"], w, c["L"], 1)
    assert [O.lib().vcfo_wavelet_len(O.wavelet_index(w)) for w in S.DWT_WAVELETS] == [2, 4]
    assert S.batch(S.dwt("haar")["packed"], S.DWT_N).shape == (S.DWT_N, DW.layout(c["H"], c["W"], c["L"])[1])


def test_the_lbt_training_moves_the_weights():
    t = S.lbt_training()
    assert np.all(np.max(np.abs(t["we"] - t["we0"]), axis=(1, 2)) > 1e-4)
    assert np.all(np.max(np.abs(t["wd"] - t["wd0"]), axis=(1, 2)) > 1e-4)
    assert np.all(t["d_proxy"] > 0)


def test_the_inflate_tables_differ_from_strip_to_strip():
    comp, coff, clen, ooff, olen, want = S.inflate_batch()
    assert len(clen) == S.N and comp.size == clen.sum() and want.size == olen.sum()
    assert olen.min() == 1 and olen.max() == 40
    z = S.inflate()
    assert len(set(z["raw"])) == S.P and len(set(z["streams"])) == S.P      # pairwise distinct
    for s in S.PROBES:
        assert comp[coff[s]:coff[s] + clen[s]].tobytes() == z["streams"][s % S.P]
        assert want[ooff[s]:ooff[s] + olen[s]].tobytes() == z["raw"][s % S.P]
    # no table of the second launch equals the first launch's at the same place
    for t in (coff, ooff):
        assert not np.any(t[S.SPLIT:] == t[:S.N - S.SPLIT])
    assert not np.array_equal(clen[S.SPLIT:], clen[:S.N - S.SPLIT])
    assert not np.array_equal(olen[S.SPLIT:], olen[:S.N - S.SPLIT])


@pytest.mark.parametrize("kind", S.CBAAC_KINDS)
def test_the_cbaac_batch_is_the_largest_the_entries_take(kind):
    from vcf_amd import tcbaac as T
    F = S.CBAAC_N
    assert F == 65535 and F % S.P == 24                     # frame 65534 holds entry 23, not the pool's last
    assert S.CBAAC_PROBES[0] == 0 and S.CBAAC_PROBES[-1] == F - 1 and len(S.CBAAC_PROBES) == 5
    assert list(S.CBAAC_PROBES) == sorted(set(S.CBAAC_PROBES))
    assert len({f % S.P for f in S.CBAAC_PROBES}) == 5      # five different pool entries
    ref = S.cbaac(kind)
    total = ref["sizes"].sum(axis=1)
    assert np.all(ref["sizes"] > 0) and total.max() <= ref["payload"].shape[1]
    for what in ("sym", "prior", "payload"):                # a frame mix-up shows at every stage
        assert ref[what].shape[0] == S.P and S.pairwise_distinct(ref[what]), (kind, what)
    if kind == "tiled2d":
        shape, (th, tw), K = (S.CBAAC2D[x] for x in ("shape", "tile", "nclass"))
        assert ref["sizes"].shape == (S.P, T.n_tiles2d(shape, th, tw)) and ref["sizes"].shape[1] == 8
        assert shape[0] % th and shape[1] % tw              # tiles cropped both ways
    else:
        n, seg = S.CBAAC["n"], S.CBAAC["seg_len"]
        K = S.CBAAC["nclass"] if kind == "classes" else 1
        assert ref["sizes"].shape == (S.P, T.n_segments(n, seg)) and ref["sizes"].shape[1] == 2 and n % seg
        if K > 1:                                           # each segment codes with a row of its own
            assert ref["prior"].shape == (S.P, K, 256) and np.all(np.any(ref["prior"][:, 0] != ref["prior"][:, 1], axis=1))
    # the streams the decoders are given: frame f's slices are pool entry f % 251's bytes, and the
    # host's own decoder turns them back into the frame
    flat, offs = S.cbaac_streams(kind, F)
    assert offs.shape == (F, ref["sizes"].shape[1] + 1) and offs[0, 0] == 0 and offs[-1, -1] == flat.size
    assert np.array_equal(offs[1:, 0], offs[:-1, -1])
    for f in S.CBAAC_PROBES:
        p = f % S.P
        parts = S.cbaac_probe(kind, f)
        assert [flat[a:b].tobytes() for a, b in zip(offs[f, :-1], offs[f, 1:])] == parts, (kind, f)
        data = b"".join(parts)
        if kind == "tiled2d":
            back = T.host_decode2d(data, ref["sizes"][p], shape, ref["prior"][p], th, tw, K)
        else:
            rows = ref["prior"][p].reshape(-1, 256)
            back = np.concatenate([T.host_decode_prior(s, min(seg, n - i * seg), rows[i * K // len(parts)])
                                   for i, s in enumerate(parts)])
        assert np.array_equal(back, ref["sym"][p]), (kind, f)


@pytest.mark.parametrize("name", S.ANY_IDS)
def test_any_b_shapes_take_more_than_one_chunk(name):
    c = [c for c in S.ANY if c["name"] == name][0]
    assert c["H"] % S.ANY_TILE == 0 and c["W"] % S.ANY_TILE == 0 and S.ANY_TILE % S.ANY_B == 0
    assert c["H"] * c["W"] * 3 < 1 << 31                    # the launcher's frame limit
    chunk = S.chunk_frames(c["n"], c["H"], c["W"], S.ANY_B, c["mode"])
    assert chunk == c["chunk"] and chunk < c["n"]
    assert c["n"] % chunk != 0 or chunk == 1                # a ragged last chunk where chunks hold two frames
    # the smallest such shape: one tile less in either direction fits a frame more into the chunk
    assert S.chunk_frames(c["n"], c["H"] - S.ANY_TILE, c["W"], S.ANY_B, c["mode"]) > chunk
    k, dec = S.any_tiles(name)
    assert S.pairwise_distinct(k) and S.pairwise_distinct(dec)
    assert np.mean((dec == 0) | (dec == 255)) <= 0.5        # a clipped pixel hides its arithmetic
    assert len(np.unique(dec)) > 32

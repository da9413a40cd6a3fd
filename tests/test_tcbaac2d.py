"""Container version 4 (`-c TCBAAC2D`: tiles with a two-dimensional context)
on the host: the serial host coder (vcf_cbaac2d_*) writes the bytes of the
numpy restatement of the format (tests/tcbaac2d_restated.py), round-trips,
the container parses back, versions 1-3 still read through the same
decompress(), corrupt headers decode to the reference's zeros, and the format
is smaller than version 3 on DCT indices.  The GPU coder is held to the host
coder's bytes in tests/test_tcbaac2d_gpu.py."""
import os
import struct

import numpy as np
import pytest

import tcbaac2d_restated as R
from conftest import GOLDEN
from tcbaac2d_cases import cases
from vcf_amd import tcbaac as T

CASES = cases()
ZEROS = np.zeros((10, 10), np.uint8)


def _host(img, tile, nclass):
    return T.HostTiledCBAACCodec(nclass=nclass, ctx2d=True, tile=tile).compress(img).getvalue()


@pytest.fixture(scope="module")
def restated():
    """name -> (tile bytes, prior rows, halvings) of the restatement, computed once."""
    return {name: R.encode_tiles(img, *tile, nclass) for name, (img, tile, nclass) in CASES.items()}


@pytest.mark.parametrize("name", list(CASES))
def test_host_bytes_equal_restatement(name, restated):
    img, (th, tw), nclass = CASES[name]
    tiles, rows, _ = restated[name]
    assert np.array_equal(T.prior2d_of(img, th, tw, nclass), rows)
    host = T.host_tiles2d(img, rows, th, tw, nclass)
    assert [len(h) for h in host] == [len(t) for t in tiles]
    assert host == tiles
    assert _host(img, (th, tw), nclass) == R.container(img.shape, th, tw, nclass, rows, tiles)


def test_uniform_case_reaches_every_context_value_and_the_halving_rule(restated):
    img, (th, tw), nclass = CASES["uniform"]
    assert restated["uniform"][2] >= 1                       # a model halved
    assert np.unique(img).size == 256
    used = set()
    for c, t, y0, x0, h, w in R.tiles(img.shape, th, tw):
        used |= set(np.unique(R.contexts(img[y0:y0 + h, x0:x0 + w, c])).tolist())
    assert used == set(range(16))


def test_all_128_uses_one_context():
    img, (th, tw), nclass = CASES["all_128"]
    rows = T.prior2d_of(img, th, tw, nclass).reshape(nclass, 16, 256)
    assert np.all(rows[:, 1:] == 1)                          # 15 empty rows per class
    used = sorted({t * nclass // 4 for t in range(4)})       # 2 x 2 tiles over 8 classes
    assert np.all(rows[used, 0, 128] == 1 + 8192) and rows.sum() == rows.size + 8192 * len(used)


@pytest.mark.parametrize("name", list(CASES))
def test_host_round_trip_and_container_fields(name):
    img, (th, tw), nclass = CASES[name]
    data = _host(img, (th, tw), nclass)
    for codec in (T.HostTiledCBAACCodec(), T.HostTiledCBAACCodec(nclass=nclass, ctx2d=True, tile=(th, tw))):
        got = codec.decompress(data)
        assert got.shape == img.shape and np.array_equal(got, img)
    shape, pth, ptw, pk, rows, tile_bytes, payload = T._parse2d(data)
    f = R.parse(data)
    assert shape == img.shape == f["shape"] and (pth, ptw, pk) == (th, tw, nclass) == (f["th"], f["tw"], f["nclass"])
    assert f["version"] == T.VERSION_2D == 4 and f["nctx"] == 16 and f["n_tiles"] == tile_bytes.size
    assert tile_bytes.size == T.n_tiles2d(img.shape, th, tw) == len(R.tiles(R.planes(img).shape, th, tw))
    assert list(tile_bytes) == f["sizes"] and payload == f["payload"] and np.array_equal(rows, f["rows"])
    assert T.pack2d(shape, pth, ptw, pk, rows, tile_bytes, payload) == data


def test_restatement_decodes_host_bytes():
    for name in ("cropped_3ch", "two_dims", "one_row"):
        img, tile, nclass = CASES[name]
        assert np.array_equal(R.decompress(_host(img, tile, nclass)), img), name


def test_versions_1_to_3_decode_through_the_same_reader():
    rng = np.random.Generator(np.random.PCG64(8))
    img = np.where(rng.random((40, 50, 3)) < 0.9, 128, rng.integers(0, 256, (40, 50, 3))).astype(np.uint8)
    reader = T.HostTiledCBAACCodec(ctx2d=True)
    assert T.HostTiledCBAACCodec.decompress is T.TiledCBAACCodec.decompress      # one reader, both codecs
    for order, prior, nclass in ((0, False, 1), (1, False, 1), (0, True, 1), (1, True, 1), (0, True, 5)):
        data = T.HostTiledCBAACCodec(order, 1024, prior, nclass).compress(img).getvalue()
        assert T.container_version(data) == (1 if not prior else 2 if nclass == 1 else 3)
        # the container of versions 1-3 as before: segments of the host coder behind pack()
        pr = T.prior_of(img, nclass, 1024) if prior else None
        segs = T.host_segments_prior(img, pr, 1024, order) if prior else T.host_segments(img, order, 1024)
        assert data == T.pack(img.shape, order, 1024, [len(s) for s in segs], b"".join(segs), pr)
        assert np.array_equal(reader.decompress(data), img)


def _fields_at(data):
    nd = struct.unpack_from("<I", data, 0)[0]
    return 4 + 4 * nd + 4      # the offset of `version`; th, tw, n_tiles, nclass, nctx follow


def _corrupt():
    img, tile, nclass = CASES["cropped_3ch"]
    good = _host(img, tile, nclass)
    p = _fields_at(good)
    f = R.parse(good)

    def patched(off, value):
        b = bytearray(good)
        struct.pack_into("<I", b, off, value)
        return bytes(b)

    idx = f["header_bytes"] - sum(len(R.varint(s)) for s in f["sizes"])      # where the tile index starts
    sizes = list(f["sizes"])
    bigger = good[:idx] + b"".join(R.varint(s + (i == len(sizes) - 1)) for i, s in enumerate(sizes)) + f["payload"]
    overlong = good[:idx] + b"\x80" * 6 + b"\x01" + good[idx + len(R.varint(sizes[0])):]
    return {
        "n_tiles_below_shape": patched(p + 12, f["n_tiles"] - 1),
        "n_tiles_above_shape": patched(p + 12, f["n_tiles"] + 1),
        "nctx_15": patched(p + 20, 15),
        "nctx_17": patched(p + 20, 17),
        "th_0": patched(p + 4, 0),
        "tw_0": patched(p + 8, 0),
        "nclass_0": patched(p + 16, 0),
        "varints_overrun": good[:f["header_bytes"] - 2],            # the data end inside the tile index
        "varint_overlong": overlong,
        "sizes_past_payload": bigger,
        "payload_cut": good[:-1],
        "version_5": patched(p, 5),
        "shape_4_dims": struct.pack("<I", 4) + struct.pack("<I", 1) + good[4:],
    }


@pytest.mark.parametrize("kind", list(_corrupt()))
def test_corrupt_version_4_headers_decode_to_reference_zeros(kind):
    bad = _corrupt()[kind]
    for codec in (T.HostTiledCBAACCodec(), T.TiledCBAACCodec()):     # rejected on the host: no device is touched
        assert np.array_equal(codec.decompress(bad), ZEROS), kind


def test_golden_fixture():
    """tests/golden/tcbaac2d.npz (make_golden_tcbaac2d.py): symbols and the host coder's containers."""
    d = np.load(os.path.join(GOLDEN, "tcbaac2d.npz"))
    names = [k[4:] for k in d.files if k.startswith("sym_")]
    assert set(names) >= {"cropped_3ch", "tiles_16x32", "all_128"}
    for name in names:
        img, tile, nclass = CASES[name]
        assert np.array_equal(d[f"sym_{name}"], img), name
        assert d[f"bytes_{name}"].tobytes() == _host(img, tile, nclass), name
        assert np.array_equal(T.HostTiledCBAACCodec().decompress(d[f"bytes_{name}"].tobytes()), img), name
    assert os.path.getsize(os.path.join(GOLDEN, "tcbaac2d.npz")) < 1 << 20


def test_codec_is_registered():
    from vcf_amd.codec import parser as P
    from vcf_amd.codec.dct2d import ENTROPY_CODECS
    c = ENTROPY_CODECS["TCBAAC2D"]()
    assert c.ctx2d and c.ORDER == 0 and c.file_extension == ".tadpt_arith"
    assert c.tile == T.TILE_2D == (64, 64) and c.nclass == T.PRIOR_CLASSES
    import argparse
    enc, dec = argparse.ArgumentParser(), argparse.ArgumentParser()
    P.add_filter(enc, dec)
    assert "TCBAAC2D" in enc.format_help() and "TCBAAC2D" in dec.format_help()      # the -c help names it


def test_version_4_is_smaller_than_version_3_on_dct_indices():
    """The rate condition: the DCT indices (numpy restatement of the encode,
    Q = 32) of a deterministic synthetic frame, whole files, headers and
    priors included, version 4 at its defaults against version 3 at CLASS_SEG."""
    from oracle import ref_numpy
    from vcf_amd.synthetic import synth_frame
    k = ref_numpy.encode_frame(synth_frame(256, 384, 3), 32)
    v3 = T.HostTiledCBAACCodec(0, T.CLASS_SEG, prior=True, nclass=T.PRIOR_CLASSES).compress(k).getvalue()
    v4 = T.HostTiledCBAACCodec(nclass=T.PRIOR_CLASSES, ctx2d=True).compress(k).getvalue()
    assert T.container_version(v3) == 3 and T.container_version(v4) == 4
    print(f"version 3: {len(v3)} bytes, version 4: {len(v4)} bytes")
    assert len(v4) < len(v3)
    assert np.array_equal(T.HostTiledCBAACCodec().decompress(v4), k)

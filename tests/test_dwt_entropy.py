"""-c under the 2D-DWT codec, the parts that need no GPU: the constructor over
the registry, the LL byte view through the host byte-symbol coders, the plane
descriptors of the batch path against dwt.layout / unpack, and the subband
files of the reference's own `2D-DWT.py encode -c z_lib -l 2 -w bior4.4` run
on a 34 x 50 image (tests/golden/dwt_zlib_ref_34x50.npz: the input, the
arrays inside its seven .npz files and the order it wrote them in)."""
import os

import numpy as np
import pytest

from vcf_amd import dwt as DW
from vcf_amd import tcbaac as T
from vcf_amd.codec import parser as P
from vcf_amd.codec.dwt2d import CoDec as DWTCoDec
from vcf_amd.codec.dwt2d import ll_bytes, ll_from_bytes
from vcf_amd.codec.entropy import ENTROPY_CODECS, make_entropy

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "dwt_zlib_ref_34x50.npz")


def _codec(sub, *flags):
    return DWTCoDec(P.parse(P.dwt_parser(), [sub, *flags]))


@pytest.mark.parametrize("c", sorted(ENTROPY_CODECS))
def test_constructs_for_every_registered_codec(c):
    args = P.parse(P.dwt_parser(), ["encode", "-c", c])
    codec = DWTCoDec(args)
    want = make_entropy(args)
    assert type(codec.entropy) is type(want)
    assert codec.file_extension == want.file_extension and codec.file_extension.startswith(".")
    assert codec.byte_symbols == (c not in ("TIFF", "z_lib"))


def test_unknown_codec_is_refused():
    args = P.parse(P.dwt_parser(), ["encode"])
    args.entropy_image_codec = "no_such_codec"
    with pytest.raises(NotImplementedError):
        DWTCoDec(args)


def _ll():
    rng = np.random.Generator(np.random.PCG64(11))
    ll = rng.integers(0, 1001, (5, 7, 3)).astype(np.uint16)
    ll[0, 0], ll[4, 6] = (1000, 256, 255), (0, 999, 513)
    return ll


def test_ll_byte_view_is_little_endian_and_checked():
    ll = _ll()
    b = ll_bytes(ll)
    assert b.shape == (5, 7, 6) and b.dtype == np.uint8
    assert np.array_equal(b[..., 0::2].astype(np.uint16) | (b[..., 1::2].astype(np.uint16) << 8), ll)
    assert np.array_equal(ll_from_bytes(b), ll) and ll_from_bytes(b).dtype == np.uint16
    for bad in (b.astype(np.uint16), b[..., :3], np.zeros((10, 10), np.uint8)):
        with pytest.raises(ValueError):
            ll_from_bytes(bad)


@pytest.mark.parametrize("c", ["CBAAC", "CBAHC", "TCBAAC2D"])
def test_ll_past_255_survives_the_host_byte_symbol_coders(c, tmp_path):
    """view(uint8) -> coder -> view(uint16), values up to 1000; TCBAAC2D through the host coder
    vcf_cbaac2d_* (HostTiledCBAACCodec writes the GPU codec's bytes)."""
    ll = _ll()
    codec = _codec("encode", "-c", c)
    if c == "TCBAAC2D":
        codec.entropy = T.HostTiledCBAACCodec(0, prior=True, nclass=codec.entropy.nclass, ctx2d=True,
                                              tile=codec.entropy.tile)
    fn = str(tmp_path / "enc")
    cs = codec._compress_subband(ll, "LL_5", fn)
    got = codec._decompress_subband(cs.getvalue(), "LL_5", fn)
    assert got.dtype == np.uint16 and np.array_equal(got, ll)
    if c == "CBAHC":                                   # the side file is named after the subband file
        assert os.path.exists(fn + "_LL_5_adaptive_huffman_tree.pkl.gz")
    detail = (ll & 255).astype(np.uint8)               # a detail subband goes through as it is
    back = codec._decompress_subband(codec._compress_subband(detail, "HH_1", fn).getvalue(), "HH_1", fn)
    assert back.dtype == np.uint8 and np.array_equal(back, detail)


def test_native_codecs_carry_uint16_ll_as_it_is(tmp_path):
    ll = _ll()
    for c in ("TIFF", "z_lib"):
        codec = _codec("encode", "-c", c)
        got = codec._decompress_subband(codec._compress_subband(ll, "LL_5", "x").getvalue(), "LL_5", "x")
        assert got.dtype == np.uint16 and np.array_equal(got, ll), c


@pytest.mark.parametrize("H,W,levels", [(34, 50, 3), (160, 136, 1), (1, 1, 1)])
def test_plane_descriptors_equal_layout_and_unpack(H, W, levels):
    shapes, pb, _ = DW.layout(H, W, levels)
    planes = DW.subband_planes(H, W, levels)
    assert [p[0] for p in planes] == DW.subband_names(levels)
    # unpack()'s views of a frame whose bytes are their own offsets (mod 251): every plane starts where its view does
    packed = (np.arange(pb) % 251).astype(np.uint8)
    views = DW.unpack(packed, H, W, levels)
    start = packed.__array_interface__["data"][0]
    for name, off, h, w, c in planes:
        v = views[name]
        assert v.__array_interface__["data"][0] - start == off, name
        assert (h, w) == v.shape[:2] and c == v.shape[2] * v.dtype.itemsize and h * w * c == v.nbytes, name
    assert planes[0][4] == 6 and all(p[4] == 3 for p in planes[1:])
    assert planes[0][2:4] == shapes[-1] and planes[-1][2:4] == shapes[0]
    assert planes[-1][1] + planes[-1][2] * planes[-1][3] * 3 == pb
    # two frames' descriptor table: offsets a frame apart, tile0 the running tile count, 64 x 64 tiles
    arrays = [(f * pb + off, h, w, c) for f in range(2) for _, off, h, w, c in planes]
    desc, nt = T.plane_descriptors(arrays)
    assert desc.dtype.itemsize == 24 and len(desc) == 2 * len(planes)
    tiles = [c * -(-h // 64) * -(-w // 64) for _, h, w, c in arrays]
    assert nt == sum(tiles)
    assert list(desc["tile0"]) == list(np.cumsum([0] + tiles[:-1]))
    assert [tuple(int(v) for v in d) for d in desc[["base", "H", "W", "C"]].tolist()] == arrays
    for (_, h, w, c), t in zip(arrays, tiles):
        assert t == T.n_tiles2d((h, w, c), 64, 64)
    assert int(desc["base"][len(planes)]) == pb


def test_plane_descriptors_expected_counts():
    """The numbers by hand: 160 x 136 at L = 1 has 80 x 68 subbands = 2 x 2 tiles per channel."""
    planes = DW.subband_planes(160, 136, 1)
    assert [(h, w, c) for _, _, h, w, c in planes] == [(80, 68, 6)] + [(80, 68, 3)] * 3
    assert [off for _, off, *_ in planes] == [0, 32640, 48960, 65280]
    desc, nt = T.plane_descriptors([(off, h, w, c) for _, off, h, w, c in planes])
    assert list(desc["tile0"]) == [0, 24, 36, 48] and nt == 60
    desc, nt = T.plane_descriptors([(off, h, w, c) for _, off, h, w, c in DW.subband_planes(1, 1, 1)])
    assert list(desc["tile0"]) == [0, 6, 9, 12] and nt == 15 and list(desc["base"]) == [0, 6, 9, 12]
    for bad in ([(0, 0, 4, 3)], [(-1, 4, 4, 3)]):
        with pytest.raises(ValueError):
            T.plane_descriptors(bad)


def test_plane_list_entry_points_check_the_descriptors_before_any_launch():
    """vcf_cbaac_tiled2d_*_planes validate the host copy of the descriptors first: a list that
    leaves the buffer, a wrong tile0 or tile count returns VCF_ERR_INVALID with nothing
    launched (no GPU here: the pointers are never followed)."""
    from vcf_amd import _lib as L
    planes = [(off, h, w, c) for _, off, h, w, c in DW.subband_planes(34, 50, 3)]
    _, pb, _ = DW.layout(34, 50, 3)
    fake = 0x1000

    def encode(desc, nt, nbytes, tile=(64, 64), nclass=8):
        L.call("vcf_cbaac_tiled2d_encode_planes", fake, nbytes, desc.ctypes.data, fake, len(desc), nt, fake, nclass,
               tile[0], tile[1], fake, 1 << 20, fake, fake, None)

    desc, nt = T.plane_descriptors(planes)
    with pytest.raises(L.VCFInvalidArgument):
        encode(desc, nt, pb - 1)                      # the last array ends one byte past the buffer
    with pytest.raises(L.VCFInvalidArgument):
        encode(desc, nt + 1, pb)
    bad = desc.copy()
    bad["tile0"][2] += 1
    with pytest.raises(L.VCFInvalidArgument):
        encode(bad, nt, pb)
    bad = desc.copy()
    bad["W"][1] = 0
    with pytest.raises(L.VCFInvalidArgument):
        encode(bad, nt, pb)
    bad = desc.copy()
    bad["base"][0] = -1
    with pytest.raises(L.VCFInvalidArgument):
        encode(bad, nt, pb)
    with pytest.raises((L.VCFInvalidArgument, L.VCFUnsupported)):
        encode(desc, nt, pb, tile=(64, 512))
    with pytest.raises(L.VCFInvalidArgument):
        L.call("vcf_cbaac_tiled2d_decode_planes", fake, fake, desc.ctypes.data, fake, len(desc), nt, fake, 8, 64, 64,
               fake, pb - 1, None)
    with pytest.raises(L.VCFInvalidArgument):
        L.call("vcf_cbaac_tiled2d_prior_planes", fake, pb - 1, desc.ctypes.data, fake, len(desc), nt, 64, 64, 8, fake,
               fake, None)


def test_reference_zlib_run_names_and_arrays(tmp_path):
    """The reference's subband arrays equal the CPU oracle's indices of the same image (what
    the GPU transform is held to), and our -c z_lib writes them under the reference's file names
    and reads back the reference's arrays."""
    from oracle import oracle as O
    with np.load(GOLDEN) as z:
        img, order = z["input"], [str(s) for s in z["file_order"]]
        ref = {n: z[n] for n in DW.subband_names(2)}
    assert order == [f"enc_{n}.npz" for n in DW.subband_names(2)]
    ours = O.dwt_encode_frame(img, "bior4.4", 2, 32)
    assert list(ours) == list(ref)
    for n in ref:
        assert ours[n].dtype == ref[n].dtype and np.array_equal(ours[n], ref[n]), n
    enc = _codec("encode", "-c", "z_lib", "-l", "2", "-w", "bior4.4")
    fn = str(tmp_path / "enc")
    size = enc.write_decom_fn(ref, fn)
    assert sorted(os.listdir(tmp_path)) == sorted(order)
    assert size == sum(os.path.getsize(tmp_path / f) for f in order)
    dec = _codec("decode", "-c", "z_lib", "-l", "2", "-w", "bior4.4")
    back = dec.read_decom_fn(fn)
    for n in ref:
        assert back[n].dtype == ref[n].dtype and np.array_equal(back[n], ref[n]), n
    assert dec._geometry(back) == (34, 50)


def test_geometry_refuses_what_does_not_fit_the_pyramid():
    dec = _codec("decode", "-l", "2")
    planes = DW.subband_planes(34, 50, 2)
    good = {n: ((h, w, 3), np.uint16 if c == 6 else np.uint8) for n, _, h, w, c in planes}
    assert dec._geometry_of(good) == (34, 50)
    for name, entry in (("HL_2", ((9, 12, 3), np.uint8)), ("LL_2", ((9, 13, 3), np.uint8)),
                        ("LL_2", ((8, 13, 3), np.uint16)), ("HH_1", ((10, 10), np.uint8)),
                        ("LH_1", ((17, 25, 6), np.uint8))):
        with pytest.raises(ValueError):
            dec._geometry_of({**good, name: entry})

"""The 2D-DWT codec's batch paths (encode_fns / decode_fns: the pyramid coded
in HBM) against its single-frame path, file for file and pixel for pixel, and
-c under the DWT for every registered codec.

Shapes: 34 x 50 at L = 3 (subbands down to 5 x 7: every tile partial, odd sizes
through the 'per' padding; -q 8 so that LL + 128 passes 255), 160 x 136 at L = 1
(80 x 68 subbands: 2 x 2 ragged tiles per channel), and a batch of three frames
of two shapes (grouping; several frames' descriptors in one launch)."""
import os
import shutil

import numpy as np
import pytest

import tcbaac2d_restated as R
from vcf_amd import dwt as DW
from vcf_amd import tcbaac as T
from vcf_amd.codec import parser as P
from vcf_amd.codec.dwt2d import CoDec, ll_bytes
from vcf_amd.codec.eic import read_image, write_image
from vcf_amd.codec.entropy import ENTROPY_CODECS

pytestmark = pytest.mark.gpu

CASES = {"34x50_L3_db5": ("db5", 3, [(34, 50)]),
         "34x50_L3_bior": ("bior4.4", 3, [(34, 50)]),
         "160x136_L1": ("bior4.4", 1, [(160, 136)]),
         "two_shapes_L3": ("bior4.4", 3, [(34, 50), (160, 136), (34, 50)])}


def _image(H, W, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    y, x = np.mgrid[0:H, 0:W]
    base = np.stack([(5 * x + 3 * y) % 256, (2 * y + x * x // 9) % 256, 255 - (x * y // 5) % 256], -1)
    return np.clip(base + rng.integers(-40, 41, (H, W, 3)), 0, 255).astype(np.uint8)


def _flags(c, wavelet, levels):
    return ["-c", c, "-w", wavelet, "-l", str(levels), "-q", "8"]


def _codec(sub, flags):
    return CoDec(P.parse(P.dwt_parser(), [sub] + flags))


def _stage(tmp_path, shapes):
    srcs = []
    for i, (H, W) in enumerate(shapes):
        srcs.append(str(tmp_path / f"in{i}.png"))
        write_image(srcs[-1], _image(H, W, 7 + i))
    return srcs


def _files(prefix, levels, ext):
    return {n: open(f"{prefix}_{n}{ext}", "rb").read() for n in DW.subband_names(levels)}


def _round_trip(tmp_path, c, name):
    """Both encoders' files and all four decodes of one case -> (srcs, batch files, single files)."""
    wavelet, levels, shapes = CASES[name]
    flags = _flags(c, wavelet, levels)
    srcs = _stage(tmp_path, shapes)
    enc = _codec("encode", flags)
    ext = enc.file_extension
    bat = [str(tmp_path / f"b{i}") for i in range(len(srcs))]
    one = [str(tmp_path / f"s{i}") for i in range(len(srcs))]
    sizes = enc.encode_fns(list(zip(srcs, bat)), batch=16)
    fb = [_files(p, levels, ext) for p in bat]
    fs = []
    for i, (s, o) in enumerate(zip(srcs, one)):
        assert _codec("encode", flags).encode_fn(s, o) == sizes[i], i
        fs.append(_files(o, levels, ext))
    for i in range(len(srcs)):
        for n in fb[i]:
            assert fb[i][n] == fs[i][n], (i, n)                   # the same files, whichever path wrote them
    dec = _codec("decode", flags)
    want = []
    for i, p in enumerate(one):
        dec.decode_fn(p, str(tmp_path / f"w{i}.png"))
        want.append(read_image(str(tmp_path / f"w{i}.png"))[0])
    for src_set, tag in ((bat, "db"), (one, "ds")):                # batched decode of either path's files
        outs = [str(tmp_path / f"{tag}{i}.png") for i in range(len(srcs))]
        _codec("decode", flags).decode_fns(list(zip(src_set, outs)), batch=16)
        for i, o in enumerate(outs):
            got = read_image(o)[0]
            assert got.shape == want[i].shape and np.array_equal(got, want[i]), (tag, i)
    return srcs, fb, fs


@pytest.mark.parametrize("name", list(CASES))
def test_tcbaac2d_batch_files_equal_the_single_array_path(tmp_path, name):
    wavelet, levels, shapes = CASES[name]
    srcs, fb, _ = _round_trip(tmp_path, "TCBAAC2D", name)
    single = T.TiledCBAACCodec(0, prior=True, nclass=T.PRIOR_CLASSES, ctx2d=True, tile=T.TILE_2D)
    ll_max = 0
    for i, src in enumerate(srcs):
        sb = DW.encode(read_image(src)[0], wavelet, levels, 8)[0]
        ll_max = max(ll_max, int(sb[f"LL_{levels}"].max()))
        for n, arr in sb.items():
            sym = ll_bytes(arr) if n.startswith("LL_") else arr
            assert fb[i][n] == single.compress(sym).getvalue(), (i, n)
            if sym.size <= 6000:                                    # the numpy restatement, where it is quick
                assert fb[i][n] == R.compress(sym), (i, n)
    if levels == 3:
        assert ll_max > 255                                        # the byte view carries a high byte that matters


@pytest.mark.parametrize("name", list(CASES))
def test_tiff_batch_files_equal_the_host_writer(tmp_path, name):
    from vcf_amd.codec.tiff import imread_bytes, imwrite_bytes
    _, levels, _ = CASES[name]
    _, fb, _ = _round_trip(tmp_path, "TIFF", name)
    for files in fb:                                               # and the host writer itself, not only encode_fn
        for n, data in files.items():
            assert data == imwrite_bytes(imread_bytes(data)), n
        assert imread_bytes(files[f"LL_{levels}"]).dtype == np.uint16


@pytest.fixture(scope="module")
def tiff_pixels(tmp_path_factory):
    d = tmp_path_factory.mktemp("tiff_ref")
    src = str(d / "in.png")
    write_image(src, _image(34, 50, 3))
    flags = _flags("TIFF", "bior4.4", 2)
    _codec("encode", flags).encode_fn(src, str(d / "e"))
    _codec("decode", flags).decode_fn(str(d / "e"), str(d / "o.png"))
    return src, read_image(str(d / "o.png"))[0]


@pytest.mark.parametrize("c", sorted(ENTROPY_CODECS))
def test_every_codec_round_trips_to_the_tiff_pixels(tmp_path, tiff_pixels, c):
    """The indices are the same under every -c, so the pixels must be; both paths."""
    src, want = tiff_pixels
    flags = _flags(c, "bior4.4", 2)
    enc = _codec("encode", flags)
    n = enc.encode_fn(src, str(tmp_path / "e"))
    names = [f"e_{s}{enc.file_extension}" for s in DW.subband_names(2)]
    assert n == sum(os.path.getsize(tmp_path / f) for f in names)
    _codec("decode", flags).decode_fn(str(tmp_path / "e"), str(tmp_path / "o.png"))
    assert np.array_equal(read_image(str(tmp_path / "o.png"))[0], want)
    assert _codec("encode", flags).encode_fns([(src, str(tmp_path / "b"))]) == [n]
    _codec("decode", flags).decode_fns([(str(tmp_path / "b"), str(tmp_path / "ob.png"))])
    assert np.array_equal(read_image(str(tmp_path / "ob.png"))[0], want)


def test_corrupt_tcbaac2d_subband_is_refused_before_any_launch(tmp_path):
    """A truncated file, and a whole stream of the wrong shape: ValueError from the host-side
    checks of both decode paths; the plane-list coder refuses the mismatch itself as well."""
    flags = _flags("TCBAAC2D", "bior4.4", 3)
    src = str(tmp_path / "in.png")
    write_image(src, _image(34, 50, 5))
    enc = _codec("encode", flags)
    enc.encode_fns([(src, str(tmp_path / "e"))])
    ext = enc.file_extension
    names = [f"e_{n}{ext}" for n in DW.subband_names(3)]

    def broken(tag, victim, data):
        for f in names:
            shutil.copy(tmp_path / f, tmp_path / f.replace("e_", tag + "_", 1))
        with open(tmp_path / f"{tag}_{victim}{ext}", "wb") as f:
            f.write(data)
        return str(tmp_path / tag)

    whole = open(tmp_path / f"e_HL_2{ext}", "rb").read()
    other = open(tmp_path / f"e_HL_1{ext}", "rb").read()         # a valid stream, 17 x 25 where 9 x 13 belongs
    ll = open(tmp_path / f"e_LL_3{ext}", "rb").read()
    for tag, victim, data in (("trunc", "HL_2", whole[:len(whole) // 2]), ("shape", "HL_2", other),
                              ("llview", "LL_3", other), ("detail6", "HH_3", ll)):
        bad = broken(tag, victim, data)
        with pytest.raises(ValueError):
            _codec("decode", flags).decode_fns([(bad, str(tmp_path / "o.png"))])
        with pytest.raises(ValueError):
            _codec("decode", flags).decode_fn(bad, str(tmp_path / "o.png"))
        assert not os.path.exists(tmp_path / "o.png")
    from vcf_amd.device import DeviceBuffer
    coder = T.PlaneBatch2D()
    buf = DeviceBuffer(9 * 13 * 3)
    with pytest.raises(ValueError):                                # the stream's shape is not the array's
        coder.decode([T._parse2d(other)], buf, [(0, 9, 13, 3)])
    with pytest.raises(ValueError):                                # the array does not fit the buffer
        coder.decode([T._parse2d(other)], buf, [(0, 17, 25, 3)])

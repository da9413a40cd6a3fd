"""Container version 4 on the GPU (vcf_cbaac_tiled2d_* in
vcf_amd/csrc/vcf_cbaac_gpu.hip): every tile's bytes equal the host serial
coder's (vcf_cbaac2d_encode, itself held to the numpy restatement in
tests/test_tcbaac2d.py), the GPU prior rows equal the host's, the GPU decoder
inverts them; batches equal frames coded singly; `-c TCBAAC2D` through the
2D-DCT codec and the HBM-resident III path."""
import numpy as np
import pytest

from tcbaac2d_cases import batch_frames, cases
from vcf_amd import tcbaac as T

pytestmark = pytest.mark.gpu

CASES = cases()


@pytest.mark.parametrize("name", list(CASES))
def test_tiles_equal_host_coder_and_round_trip(name):
    img, (th, tw), nclass = CASES[name]
    coder = T.Tiled2DCoder((th, tw), nclass)
    sizes, payload = coder.encode(img)
    rows = T.prior2d_of(img, th, tw, nclass)
    assert np.array_equal(coder.last_prior, rows)
    host = T.host_tiles2d(img, rows, th, tw, nclass)
    assert list(sizes) == [len(h) for h in host]
    ends = np.cumsum(sizes)
    for t, h in enumerate(host):                                  # tile for tile
        assert payload[int(ends[t] - sizes[t]):int(ends[t])] == h, t
    got = coder.decode(payload, sizes, img.shape, rows, nclass)
    assert got.shape == img.shape and np.array_equal(got, img)
    # the codec: the host codec's container, read back by a codec with other defaults
    data = T.TiledCBAACCodec(nclass=nclass, ctx2d=True, tile=(th, tw)).compress(img).getvalue()
    assert data == T.HostTiledCBAACCodec(nclass=nclass, ctx2d=True, tile=(th, tw)).compress(img).getvalue()
    assert np.array_equal(T.TiledCBAACCodec().decompress(data), img)


def test_batch_of_frames_equals_frames_coded_singly():
    """3 frames of 61 x 77 x 3 in one launch per stage, from an unaligned
    start, equal the frames coded one by one; the batched decode inverts them."""
    from vcf_amd import _lib as L
    from vcf_amd.device import DeviceBuffer
    frames = batch_frames()
    F, shape = frames.shape[0], frames.shape[1:]
    n = int(np.prod(shape))
    buf = DeviceBuffer.from_array(np.concatenate([np.zeros(1, np.uint8), frames.ravel()]))
    fb = T.FrameBatch2D(F, shape, T.TILE_2D, 4)
    fb.launch(buf, 1)
    heads, got = fb.headers(), fb.download()
    single = T.Tiled2DCoder(T.TILE_2D, 4)
    for f in range(F):
        s, p = single.encode(frames[f])
        assert list(got[f][0]) == list(s) and got[f][1] == p, f
        assert np.array_equal(got[f][2], single.last_prior), f
        want = T.HostTiledCBAACCodec(nclass=4, ctx2d=True).compress(frames[f]).getvalue()
        assert heads[f] + got[f][1] == fb.header(f) + got[f][1] == want, f
    nt = T.n_tiles2d(shape, *T.TILE_2D)
    payload = b"".join(e[1] for e in got)
    offs, base = [], 0
    for e in got:
        offs.append(np.concatenate([[0], np.cumsum(e[0])]) + base)
        base += len(e[1])
    offs = np.concatenate(offs).astype(np.int64)
    assert offs.size == F * (nt + 1)
    priors = np.stack([e[2] for e in got]).astype(np.uint16)
    src, doffs, dpr = (DeviceBuffer.from_array(np.frombuffer(payload, np.uint8)), DeviceBuffer.from_array(offs),
                       DeviceBuffer.from_array(priors))
    out = DeviceBuffer(F * n)
    L.call("vcf_cbaac_tiled2d_decode_frames", src.ptr, doffs.ptr, F, *shape, dpr.ptr, 4, *T.TILE_2D, out.ptr, n, None)
    dec = out.download(np.empty(F * n, np.uint8))
    assert np.array_equal(dec.reshape(frames.shape), frames)


def test_tile_limits_are_errors():
    from vcf_amd._lib import VCFUnsupported
    img = np.full((4, 600, 1), 128, np.uint8)
    with pytest.raises(VCFUnsupported):
        T.Tiled2DCoder((4, 512), 1).encode(img)                   # wider than the LDS rows
    with pytest.raises(ValueError):
        T.Tiled2DCoder(T.TILE_2D, 1).encode(np.zeros((2, 3, 4, 5), np.uint8))


def test_dct_codec_with_tcbaac2d_frame(tmp_path):
    """2D-DCT encode -c TCBAAC2D then decode reproduces the pixels -c TCBAACP
    reproduces; the file is a version-4 container of the frame's indices."""
    from PIL import Image

    from vcf_amd.codec import parser as P
    from vcf_amd.codec.dct2d import CoDec
    from vcf_amd.synthetic import synth_frame
    rgb = synth_frame(64, 96, 6)
    src = str(tmp_path / "f.png")
    Image.fromarray(rgb).save(src)
    outs = {}
    for ec in ("TCBAAC2D", "TCBAACP"):
        CoDec(P.parse(P.dct_parser(), ["encode", "-c", ec])).encode_fn(src, str(tmp_path / ec))
        CoDec(P.parse(P.dct_parser(), ["decode", "-c", ec])).decode_fn(str(tmp_path / ec), str(tmp_path / f"{ec}.png"))
        outs[ec] = np.asarray(Image.open(str(tmp_path / f"{ec}.png")))
    assert outs["TCBAAC2D"].shape == rgb.shape and np.array_equal(outs["TCBAAC2D"], outs["TCBAACP"])
    data = open(str(tmp_path / "TCBAAC2D.tadpt_arith"), "rb").read()
    assert T.container_version(data) == T.VERSION_2D
    k = T.TiledCBAACCodec().decompress(open(str(tmp_path / "TCBAACP.tadpt_arith"), "rb").read())
    assert data == T.HostTiledCBAACCodec(nclass=T.PRIOR_CLASSES, ctx2d=True).compress(k).getvalue()


def test_device_iii_with_tcbaac2d_equals_the_codec():
    """The HBM-resident III path with entropy="TCBAAC2D" on one rank: every
    gathered container equals TiledCBAACCodec.compress of the frame's indices."""
    from vcf_amd import dct
    from vcf_amd.codec.dct2d import ENTROPY_CODECS
    from vcf_amd.codec.iii_device import DeviceIII
    from vcf_amd.device import DeviceBuffer
    frames = batch_frames()                                       # 61 x 77: padded to 64 x 80, unaligned frames
    n, H, W = frames.shape[:3]
    job = DeviceIII(None, 0, 1, n, H, W, 32, entropy="TCBAAC2D")
    sizes, got = job.run(DeviceBuffer.from_array(frames))
    k = dct.encode(frames, Q=32)
    codec = ENTROPY_CODECS["TCBAAC2D"]()
    for i in range(n):
        want = codec.compress(k[i]).getvalue()
        assert bytes(got[i]) == want and sizes[i] == len(want), i
        assert np.array_equal(codec.decompress(bytes(got[i])), k[i]), i
    with pytest.raises(ValueError):
        DeviceIII(None, 0, 1, n, H, W, 32, entropy="CBAAC")

"""The batched encode_fns / decode_fns of the block codecs (2D-DCT, 2D-MDCT,
2D-KLT) against encode_fn / decode_fn on each frame alone.

Five frames, 37x45 and 24x40 interleaved, batch=2: a padded edge, at least two
blocks per side, two shape groups in one batch and a last partial batch.  Every
file the batch writes must equal the file the single-frame path writes: the
.tif (the GPU deflate of the batch is held to zlib's bytes by
tests/test_deflate_gpu.py), _shape.bin, the index arrays, KLT's weights, and
the decoded pixels.  (A batch .tif that zlib rejects with "incorrect data
check" is the deflate, which runs on a stream of its own, having read the
indices before the encode kernel on the null stream had written them.)  The DCT case has two shapes, so its pinned single-shape
PNG path declines and the general batch loop runs."""
import os

import numpy as np
import pytest
from PIL import Image

from vcf_amd.codec import parser as P
from vcf_amd.codec.tiff import imread_bytes

pytestmark = pytest.mark.gpu

SHAPES = [(37, 45), (24, 40), (37, 45), (24, 40), (37, 45)]
FLAGS = ["-B", "8", "-q", "16"]


def _dct():
    import mdct_restated
    from vcf_amd.codec.dct2d import CoDec
    return CoDec, P.dct_parser, mdct_restated.synth_frame


def _mdct():
    import mdct_restated
    from vcf_amd.codec.mdct2d import CoDec
    return CoDec, P.mdct_parser, mdct_restated.synth_frame


def _klt():
    import klt_restated
    from vcf_amd.codec.klt2d import CoDec
    return CoDec, P.klt_parser, klt_restated.synth_frame


def _read(fn):
    with open(fn, "rb") as f:
        return f.read()


@pytest.mark.parametrize("which", [_mdct, _klt, _dct], ids=["2D-MDCT", "2D-KLT", "2D-DCT"])
def test_batches_write_what_single_frames_write(tmp_path, which):
    CoDec, parser, synth_frame = which()
    args = lambda sub: P.parse(parser(), [sub] + FLAGS)   # noqa: E731
    pairs = []
    for i, (h, w) in enumerate(SHAPES):
        src = str(tmp_path / f"orig_{i:04d}.png")
        Image.fromarray(synth_frame(h, w, 10 + i)).save(src)
        pairs.append((src, str(tmp_path / f"enc_{i:04d}")))

    c = CoDec(args("encode"))
    if which is _dct:
        assert c._encode_fns_staged(pairs, 2, 4) is None     # two shapes: the general loop
    sizes = c.encode_fns(pairs, batch=2, io_threads=4)
    assert len(sizes) == len(pairs)
    single = CoDec(args("encode"))
    for i, ((src, out), n) in enumerate(zip(pairs, sizes)):
        one = str(tmp_path / f"one_{i:04d}")
        assert single.encode_fn(src, one) == os.path.getsize(one + ".tif")
        assert n == os.path.getsize(out + ".tif")
        assert _read(out + "_shape.bin") == _read(one + "_shape.bin")
        assert np.array_equal(imread_bytes(_read(out + ".tif")), imread_bytes(_read(one + ".tif")))
        if which is _klt:
            with np.load(out + "_weights.npz") as a, np.load(one + "_weights.npz") as b:
                assert list(a.keys()) == list(b.keys()) == ["weights"]
                assert a["weights"].dtype == b["weights"].dtype and np.array_equal(a["weights"], b["weights"])
        assert _read(out + ".tif") == _read(one + ".tif")

    dpairs = [(out, str(tmp_path / f"dec_{i:04d}.png")) for i, (_, out) in enumerate(pairs)]
    dsizes = CoDec(args("decode")).decode_fns(dpairs, batch=2)
    single = CoDec(args("decode"))
    for i, ((out, dec), n) in enumerate(zip(dpairs, dsizes)):
        one = str(tmp_path / f"one_dec_{i:04d}.png")
        single.decode_fn(out, one)
        assert n == os.path.getsize(dec)
        y = np.asarray(Image.open(dec))
        assert y.shape == SHAPES[i] + (3,)
        assert np.array_equal(y, np.asarray(Image.open(one)))

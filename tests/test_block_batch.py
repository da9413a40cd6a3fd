"""The batch pipeline of the block codecs (codec/blockcodec.py encode_fns /
decode_fns) on its own: a stub codec whose hooks record their calls stands in
for the GPU and the files.  No GPU and no library needed."""
import io
import threading

import numpy as np
import pytest

from vcf_amd.codec.blockcodec import BlockCoDec


class Stub(BlockCoDec):
    """Frames are named by the integer they are filled with; 'files' live in dicts."""

    def __init__(self, frames, as_bytes=()):
        self.lm = None
        self.frames = frames              # in_fn -> array
        self.as_bytes = set(as_bytes)     # frame values whose payload is a finished file
        self.lock = threading.Lock()
        self.group_calls, self.compressed, self.files, self.sides, self.shapes_set = [], [], {}, {}, []

    def encode_read_fn(self, fn):
        if isinstance(self.frames[fn], Exception):
            raise self.frames[fn]
        return self.frames[fn]

    def _check_frame(self, img):
        assert img.ndim == 3

    def _set_shape(self, shape):
        self.shapes_set.append(tuple(shape))

    def _encode_group(self, frames, shape):
        assert isinstance(frames, np.ndarray) and frames.shape[1:] == shape
        ids = [int(f[0, 0, 0]) for f in frames]
        self.group_calls.append((shape, ids))
        return [(b"file%d" % v if v in self.as_bytes else np.full(2, v, np.uint8), "extra%d" % v) for v in ids]

    def compress(self, k):
        with self.lock:
            self.compressed.append(int(k[0]))
        return io.BytesIO(b"z" * (10 + int(k[0])))

    def _write_side(self, out_fn, shape, extra):
        with self.lock:
            self.sides[out_fn] = (tuple(shape), extra)

    def encode_write_fn(self, cs, fn):
        cs.seek(0)
        data = cs.read()
        with self.lock:
            self.files[fn] = data
        return len(data)

    # decode side: the 'code-stream' of a frame is its id, the side file gives the shape
    def decode_read_fn(self, fn):
        return self.frames[fn][0]

    def _read_side(self, fn):
        return self.frames[fn][1], "w%d" % self.frames[fn][0]

    def decompress(self, cs):
        return cs * 100

    def _decode_group(self, items, shape, extras):
        self.group_calls.append((shape, list(items), list(extras)))
        return [np.full(shape, i // 100, np.uint8) for i in items]

    def decode_write_fn(self, y, fn):
        with self.lock:
            self.files[fn] = y
        return int(y[0, 0, 0]) + 1000


A, B = (4, 6, 3), (2, 8, 3)
# shapes by frame id: batches of 3 -> [A B A] [B B A] [A]
SHAPES = [A, B, A, B, B, A, A]


def _encode_stub(**kw):
    frames = {"in%d" % v: np.full(s, v, np.uint8) for v, s in enumerate(SHAPES)}
    return Stub(frames, **kw), [("in%d" % v, "out%d" % v) for v in range(len(SHAPES))]


def test_encode_sizes_groups_and_order():
    c, pairs = _encode_stub()
    sizes = c.encode_fns(pairs, batch=3, io_threads=4)
    assert sizes == [10 + v for v in range(7)]                      # input order, across batches and groups
    # once per shape group per batch, groups in first-seen order, frames of a group in order
    assert c.group_calls == [(A, [0, 2]), (B, [1]), (B, [3, 4]), (A, [5]), (A, [6])]
    assert c.shapes_set == [A, A, A]                                # each batch's last frame
    assert c.sides == {"out%d" % v: (s, "extra%d" % v) for v, s in enumerate(SHAPES)}
    assert c.files == {"out%d" % v: b"z" * (10 + v) for v in range(7)}


def test_bytes_payloads_bypass_compress():
    c, pairs = _encode_stub(as_bytes=(1, 5))
    sizes = c.encode_fns(pairs, batch=3, io_threads=2)
    assert sorted(c.compressed) == [0, 2, 3, 4, 6]
    assert c.files["out1"] == b"file1" and c.files["out5"] == b"file5"
    assert sizes[1] == 5 and sizes[5] == 5 and sizes[0] == 10


def test_empty_pairs():
    c, _ = _encode_stub()
    assert c.encode_fns([]) == [] and c.decode_fns(iter(())) == []
    assert c.group_calls == [] and c.files == {} and c.shapes_set == []


def test_a_failing_read_propagates():
    c, pairs = _encode_stub()
    c.frames["in4"] = OSError("in4 is gone")
    with pytest.raises(OSError, match="in4 is gone"):
        c.encode_fns(pairs, batch=3, io_threads=4)


def test_decode_sizes_groups_and_order():
    frames = {"enc%d" % v: (v, s) for v, s in enumerate(SHAPES)}
    c = Stub(frames)
    sizes = c.decode_fns([("enc%d" % v, "dec%d" % v) for v in range(7)], batch=3, io_threads=4)
    assert sizes == [1000 + v for v in range(7)]
    assert c.group_calls == [(A, [0, 200], ["w0", "w2"]), (B, [100], ["w1"]), (B, [300, 400], ["w3", "w4"]),
                             (A, [500], ["w5"]), (A, [600], ["w6"])]
    assert c.shapes_set == [A, A, A]
    assert all(c.files["dec%d" % v].shape == s and c.files["dec%d" % v][0, 0, 0] == v for v, s in enumerate(SHAPES))

"""Container version 4 of `.tadpt_arith` (tiled CBAAC with a two-dimensional
context) restated in plain numpy and Python from its specification: the tile
scan, the context rule, the prior rows and the container.  The adaptive model
is CBAAC.py:17-47's rule restated as tests/test_cbaac.py states it (256
frequencies, +1 per update, every frequency (f >> 1) + 1 when the stale total
has reached 16384); the arithmetic coder is the A8 stand-in the version 1-3
tests use (tests/golden/shims/arithmetic_coding)."""
import os
import struct
import sys

import numpy as np

from conftest import GOLDEN


def _a8():
    """The A8 stand-in coder's two classes."""
    shims = os.path.join(GOLDEN, "shims")
    if shims not in sys.path:
        sys.path.insert(0, shims)
    from arithmetic_coding.arithmetic_coding import Arithmetic_Decoding, Arithmetic_Encoding
    return Arithmetic_Encoding, Arithmetic_Decoding


NCTX = 16
MAX_FREQ = 16384
PRIOR_SCALE = 8192


class Model:
    """AdaptiveModel with given starting frequencies; counts its halvings."""

    def __init__(self, freq):
        self.freq = np.asarray(freq, np.int64).copy()
        self.total = int(self.freq.sum())
        self.halvings = 0

    def get_range(self, s):
        lo = int(self.freq[:s].sum())
        return lo, lo + int(self.freq[s]), self.total

    def get_symbol_from_scaled_value(self, v):
        cum = np.cumsum(self.freq)
        s = int(np.searchsorted(cum, v, side="right"))
        return s, int(cum[s] - self.freq[s]), int(cum[s])

    def update(self, s):
        stale = self.total
        self.freq[s] += 1
        if stale >= MAX_FREQ:
            self.freq = (self.freq >> 1) + 1
            self.halvings += 1
        self.total = int(self.freq.sum())


def planes(img):
    img = np.asarray(img, np.uint8)
    if img.ndim == 2:
        img = img[:, :, None]
    assert img.ndim == 3
    return img


def tiles(shape3, th, tw):
    """(channel, tile index in the channel, y0, x0, h, w) in container order:
    channel-major, then tile row, then tile column; edge tiles cropped."""
    H, W, C = shape3
    out = []
    for c in range(C):
        t = 0
        for y0 in range(0, H, th):
            for x0 in range(0, W, tw):
                out.append((c, t, y0, x0, min(th, H - y0), min(tw, W - x0)))
                t += 1
    return out


def contexts(tile):
    """ctx = 4 q(|left - 128|) + q(|up - 128|), q = min(., 3); absent neighbours count 0."""
    a = np.minimum(np.abs(tile.astype(np.int64) - 128), 3)
    wn = np.zeros_like(a)
    nn = np.zeros_like(a)
    wn[:, 1:] = a[:, :-1]
    nn[1:, :] = a[:-1, :]
    return 4 * wn + nn


def class_of(t_in_channel, n_t, nclass):
    return t_in_channel * nclass // n_t


def prior_rows(img, th, tw, nclass):
    """(nclass * 16, 256): row (class, ctx) = 1 + floor(hist * 8192 / n), ones when n = 0."""
    img = planes(img)
    tl = tiles(img.shape, th, tw)
    n_t = len(tl) // img.shape[2] if img.shape[2] else 0
    hist = np.zeros((nclass, NCTX, 256), np.int64)
    for c, t, y0, x0, h, w in tl:
        tile = img[y0:y0 + h, x0:x0 + w, c]
        np.add.at(hist[class_of(t, n_t, nclass)], (contexts(tile).ravel(), tile.ravel()), 1)
    n = hist.sum(axis=2, keepdims=True)
    rows = 1 + hist * PRIOR_SCALE // np.maximum(n, 1)
    return rows.reshape(nclass * NCTX, 256).astype(np.uint16)


def encode_tile(tile, rows16):
    """-> (the tile's bytes, halvings of its models)."""
    models = [Model(r) for r in rows16]
    enc, bits = _a8()[0](), []
    for s, k in zip(tile.ravel().tolist(), contexts(tile).ravel().tolist()):
        enc.encode_symbol(s, models[k], bits)
        models[k].update(s)
    enc.flush(bits)
    bits += [0] * (-len(bits) % 8)
    return np.packbits(np.array(bits, np.uint8)).tobytes(), sum(m.halvings for m in models)


def decode_tile(data, h, w, rows16):
    models = [Model(r) for r in rows16]
    dec = _a8()[1]()
    dec.start(np.unpackbits(np.frombuffer(data, np.uint8)))
    a = np.zeros((h, w), np.int64)      # min(|s - 128|, 3) of what is decoded so far
    out = np.zeros((h, w), np.uint8)
    for y in range(h):
        for x in range(w):
            k = 4 * (a[y, x - 1] if x else 0) + (a[y - 1, x] if y else 0)
            s = dec.decode_symbol(models[k])
            models[k].update(s)
            out[y, x] = s
            a[y, x] = min(abs(s - 128), 3)
    return out


def encode_tiles(img, th, tw, nclass, rows=None):
    """-> (list of tile bytes, prior rows, total halvings)."""
    img = planes(img)
    rows = prior_rows(img, th, tw, nclass) if rows is None else rows
    tl = tiles(img.shape, th, tw)
    n_t = len(tl) // img.shape[2] if img.shape[2] else 0
    out, halvings = [], 0
    for c, t, y0, x0, h, w in tl:
        k = class_of(t, n_t, nclass)
        data, hv = encode_tile(img[y0:y0 + h, x0:x0 + w, c], rows[k * NCTX:(k + 1) * NCTX])
        out.append(data)
        halvings += hv
    return out, rows, halvings


def varint(v):
    out = bytearray()
    while True:
        b = v & 0x7F
        v >>= 7
        out.append(b | (0x80 if v else 0))
        if not v:
            return bytes(out)


def sparse_rows(rows):
    out = b""
    for r in np.asarray(rows):
        sy = np.flatnonzero(r != 1)
        out += struct.pack("<H", sy.size) + sy.astype(np.uint8).tobytes() + r[sy].astype("<u2").tobytes()
    return out


def container(shape, th, tw, nclass, rows, tile_data):
    head = struct.pack(f"<I{len(shape)}I", len(shape), *shape) + b"VCFT"
    head += struct.pack("<IIIIII", 4, th, tw, len(tile_data), nclass, NCTX)
    return head + sparse_rows(rows) + b"".join(varint(len(t)) for t in tile_data) + b"".join(tile_data)


def compress(img, th=64, tw=64, nclass=8):
    img = np.asarray(img, np.uint8)
    data, rows, _ = encode_tiles(img, th, tw, nclass)
    return container(img.shape, th, tw, nclass, rows, data)


def parse(data):
    """-> dict of the container's fields (no validation beyond the layout)."""
    nd = struct.unpack_from("<I", data, 0)[0]
    shape = struct.unpack_from(f"<{nd}I", data, 4)
    p = 4 + 4 * nd
    assert data[p:p + 4] == b"VCFT"
    version, th, tw, nt, nclass, nctx = struct.unpack_from("<IIIIII", data, p + 4)
    p += 28
    rows = np.ones((nclass * nctx, 256), np.uint16)
    for r in range(nclass * nctx):
        m = struct.unpack_from("<H", data, p)[0]
        sy = np.frombuffer(data, np.uint8, m, p + 2)
        rows[r, sy] = np.frombuffer(data, "<u2", m, p + 2 + m)
        p += 2 + 3 * m
    sizes = []
    for _ in range(nt):
        v, sh = 0, 0
        while True:
            b = data[p]
            p += 1
            v |= (b & 0x7F) << sh
            sh += 7
            if b < 0x80:
                break
        sizes.append(v)
    return dict(shape=tuple(shape), version=version, th=th, tw=tw, n_tiles=nt, nclass=nclass, nctx=nctx, rows=rows,
                sizes=sizes, payload=data[p:], header_bytes=p)


def decompress(data):
    f = parse(data)
    shape = f["shape"]
    shape3 = shape if len(shape) == 3 else shape + (1,)
    out = np.zeros(shape3, np.uint8)
    tl = tiles(shape3, f["th"], f["tw"])
    n_t = len(tl) // shape3[2] if shape3[2] else 0
    p = 0
    for (c, t, y0, x0, h, w), nb in zip(tl, f["sizes"]):
        k = class_of(t, n_t, f["nclass"])
        out[y0:y0 + h, x0:x0 + w, c] = decode_tile(f["payload"][p:p + nb], h, w, f["rows"][k * NCTX:(k + 1) * NCTX])
        p += nb
    return out.reshape(shape)

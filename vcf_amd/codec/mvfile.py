"""The coded motion file of the IPP coder ({prefix}_mv.vmv, --mvc; not in the
reference): every field as median-predicted signed exp-Golomb codes
(vcf_mv_encode of include/vcf_amd.h, "Coded motion fields"), the mode maps as
one zlib stream.

Layout, little endian: the magic b"VMV1"; six u32 nby, nbx, subpel, n_P, n_B,
has_modes; per field a u32 byte length and the payload -- the n_P fields of the
P-frames first, then the B-frames' as forward, backward per B-frame; last a u32
length and one zlib level-6 stream of the mode bytes (the -R maps of the
P-frames when n_B = 0, the B-frames' maps otherwise; nby * nbx bytes per frame),
the length 0 when has_modes is 0.  Nothing follows.
"""
from __future__ import annotations

import struct
import zlib

import numpy as np

from .. import ipp as K

MAGIC = b"VMV1"
CODEC = "median-eg0"
_HEAD = struct.Struct("<4s6I")
_MAX_BLOCKS = 1 << 24   # per side: far beyond any frame


def _quarter_pels(field, step) -> np.ndarray:
    f = np.asarray(field, np.float32)
    q = np.rint(f.astype(np.float64) * 4)
    if not np.all(np.isfinite(q)) or np.any(q != f.astype(np.float64) * 4) or np.any(np.abs(q) > 1 << 15):
        raise ValueError("motion field: vectors must be multiples of a quarter pel within +-2^13 pixels")
    q = q.astype(np.int32)
    if np.any(q % step):
        raise ValueError(f"motion field: vectors off the 1/{4 // step}-pel grid")
    return q


def pack(mv, subpel: int = 1, bmv=None, modes=None) -> bytes:
    """mv: (n_P, nby, nbx, 2) float32; bmv: (n_B, 2, nby, nbx, 2) or None; modes: the u8 mode maps
    ((n_P, nby, nbx) of -R, or (n_B, nby, nbx) beside bmv) or None."""
    if subpel not in (1, 2, 4):
        raise ValueError(f"subpel {subpel!r}: 1, 2 or 4")
    step = 4 // subpel
    mv = np.asarray(mv, np.float32)
    if mv.ndim != 4 or mv.shape[3] != 2:
        raise ValueError("mv: expected (n_P, nby, nbx, 2)")
    n_p, nby, nbx = mv.shape[:3]
    fields = [mv[i] for i in range(n_p)]
    n_b = 0
    if bmv is not None:
        bmv = np.asarray(bmv, np.float32)
        if bmv.ndim != 5 or bmv.shape[1:] != (2, nby, nbx, 2):
            raise ValueError(f"bmv: expected (n_B, 2, {nby}, {nbx}, 2)")
        n_b = bmv.shape[0]
        fields += [bmv[i, d] for i in range(n_b) for d in range(2)]
    out = [_HEAD.pack(MAGIC, nby, nbx, subpel, n_p, n_b, int(modes is not None))]
    for f in fields:
        s = K.mv_encode(_quarter_pels(f, step), step)
        out += [struct.pack("<I", len(s)), s]
    z = b""
    if modes is not None:
        m = np.ascontiguousarray(modes, np.uint8)
        if m.shape != ((n_b if bmv is not None else n_p), nby, nbx):
            raise ValueError(f"modes: shape {m.shape}")
        z = zlib.compress(m.tobytes(), 6)
    out += [struct.pack("<I", len(z)), z]
    return b"".join(out)


def unpack(data: bytes) -> dict:
    """-> {"nby", "nbx", "subpel", "n_P", "n_B", "mv_f32", "bmv_f32" / None, "modes" / None}; ValueError for
    anything pack() does not write."""
    data = bytes(data)
    if len(data) < _HEAD.size:
        raise ValueError("motion file: shorter than its header")
    magic, nby, nbx, subpel, n_p, n_b, has_modes = _HEAD.unpack_from(data)
    if magic != MAGIC:
        raise ValueError(f"motion file: magic {magic!r} (expected {MAGIC!r})")
    if subpel not in (1, 2, 4) or has_modes > 1 or nby > _MAX_BLOCKS or nbx > _MAX_BLOCKS:
        raise ValueError(f"motion file: header nby {nby}, nbx {nbx}, subpel {subpel}, has_modes {has_modes}")
    pos = _HEAD.size

    def chunk():
        nonlocal pos
        if pos + 4 > len(data):
            raise ValueError("motion file: ends inside a length")
        n, = struct.unpack_from("<I", data, pos)
        if pos + 4 + n > len(data):
            raise ValueError("motion file: ends inside a payload")
        pos += 4 + n
        return data[pos - n:pos]

    if (n_p + 2 * n_b) * 4 > len(data) - pos:      # every field has a length word: bounds the loop
        raise ValueError(f"motion file: {n_p} + 2 * {n_b} fields in {len(data)} bytes")
    step = 4 // subpel

    def field():
        c = chunk()
        if nby * nbx * 2 > 8 * len(c):             # a block takes at least two bits: bounds the allocation
            raise ValueError(f"motion file: {nby} x {nbx} vectors in {len(c)} bytes")
        return K.mv_decode(c, nby, nbx, step).astype(np.float32) / np.float32(4)

    fields = [field() for _ in range(n_p + 2 * n_b)]
    mv = np.stack(fields[:n_p]).astype(np.float32) if n_p else np.zeros((0, nby, nbx, 2), np.float32)
    bmv = np.stack(fields[n_p:]).reshape(n_b, 2, nby, nbx, 2).astype(np.float32) if n_b else None
    z, modes = chunk(), None
    if has_modes:
        n = (n_b if n_b else n_p) * nby * nbx
        d = zlib.decompressobj()
        try:
            raw = d.decompress(z, n + 1)
        except zlib.error as e:
            raise ValueError(f"motion file: mode stream: {e}") from None
        if len(raw) != n or not d.eof or d.unused_data or d.unconsumed_tail:
            raise ValueError(f"motion file: the mode stream does not hold exactly {n} bytes")
        modes = np.frombuffer(raw, np.uint8).reshape(n_b if n_b else n_p, nby, nbx)
    elif z:
        raise ValueError("motion file: a mode stream without has_modes")
    if pos != len(data):
        raise ValueError(f"motion file: {len(data) - pos} bytes after the last stream")
    return {"nby": nby, "nbx": nbx, "subpel": subpel, "n_P": n_p, "n_B": n_b, "mv_f32": mv, "bmv_f32": bmv,
            "modes": modes}


def check_header(f: dict, nby: int, nbx: int, subpel: int, n_p: int, n_b: int) -> None:
    """The decoder's check of an unpacked file against meta.json and the frame size."""
    want = {"nby": nby, "nbx": nbx, "subpel": subpel, "n_P": n_p, "n_B": n_b}
    bad = {k: (f[k], v) for k, v in want.items() if f[k] != v}
    if bad:
        raise ValueError("motion file: header disagrees with meta.json / the frame size: " +
                         ", ".join(f"{k} {a} (expected {b})" for k, (a, b) in bad.items()))


def write(path: str, mv, subpel: int = 1, bmv=None, modes=None) -> int:
    data = pack(mv, subpel, bmv, modes)
    with open(path, "wb") as f:
        f.write(data)
    return len(data)


def read(path: str) -> dict:
    with open(path, "rb") as f:
        return unpack(f.read())

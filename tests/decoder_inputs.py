"""Inputs for the GPU decoders that none of the project's encoders produces
(tests/test_decoder_inputs.py checks them on the host, tests/
test_decoder_inputs_gpu.py feeds them to the kernels).  Deterministic: numpy's
PCG64 under fixed seeds.  Nothing here imports the package; the CBAAC payloads
take the host coder as an argument.

- inflate_corpus(): zlib streams of shapes zlib.compress(level, 15, 8) never
  writes (small windows, memLevel 1 / 9, every flush mode, 64 KiB stored
  blocks, trailing bytes), bit-flipped deflate bodies resealed with the adler32
  of what they now decode to (valid streams no compressor writes), plain
  bit flips and truncations, and hand-built fixed / dynamic blocks at the
  format's edges.
- cbaac_payloads(): segment byte strings for the tiled CBAAC decoders: valid,
  cut short, bit-flipped, random, all 0x00, all 0xFF.
- index_plane(): index values for the transforms' decoders.
"""
import functools
import zlib

import numpy as np

from deflate_corrupt import _Bits, _CLEN_ORDER, _canonical
from test_inflate_gpu import _data

MAX_STRIP = 65536
KINDS = ("sparse", "text", "image", "random")


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def zlib_verdict(stream, out_len):
    """What zlib makes of `stream` as a strip of out_len bytes: the bytes, or
    None when zlib rejects it (or does not reach the stream's end) or the
    output is not out_len bytes long.  Bytes after the adler32 are ignored,
    as zlib.decompress ignores them."""
    d = zlib.decompressobj()
    try:
        out = d.decompress(stream)
    except zlib.error:
        return None
    return out if d.eof and len(out) == out_len else None


# ---- encoder shapes ---------------------------------------------------------------------

def _encoder_shapes():
    out = []
    rng = _rng(101)
    flushes = (("sync", zlib.Z_SYNC_FLUSH), ("full", zlib.Z_FULL_FLUSH), ("partial", zlib.Z_PARTIAL_FLUSH),
               ("block", zlib.Z_BLOCK))
    for kind in KINDS:
        for n in (1, 1023, 20000, 65536):
            raw = _data(kind, n, rng)
            for wbits in range(9, 16):
                c = zlib.compressobj(6, zlib.DEFLATED, wbits, 8)
                out.append((f"enc:w{wbits}:{kind}:{n}", c.compress(raw) + c.flush(), n, raw))
            for mem in (1, 9):
                c = zlib.compressobj(6, zlib.DEFLATED, 15, mem)
                out.append((f"enc:mem{mem}:{kind}:{n}", c.compress(raw) + c.flush(), n, raw))
            for piece in (257, 4099):
                for fname, mode in flushes:
                    c = zlib.compressobj(6, zlib.DEFLATED, 15, 8)
                    s = b"".join(c.compress(raw[i:i + piece]) + c.flush(mode) for i in range(0, n, piece))
                    out.append((f"enc:{fname}{piece}:{kind}:{n}", s + c.flush(), n, raw))
            for t in (1, 2, 3):
                tail = bytes(rng.integers(0, 256, t, dtype=np.uint8))
                out.append((f"enc:trailing{t}:{kind}:{n}", zlib.compress(raw, 6) + tail, n, raw))
        for n in (65535, 65536, 65537):
            raw = _data(kind, n, rng)
            out.append((f"enc:stored:{kind}:{n}", zlib.compress(raw, 0), n, raw))
    return out


# ---- mutants ----------------------------------------------------------------------------

def _level(raw, level, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, 15, 8, strategy)
    return c.compress(raw) + c.flush()


def _resealed():
    """-> (entries, stats): one bit of a stream's deflate body flipped; where
    raw inflate still reaches the end of the data within 65 536 bytes, the
    adler32 of that output is appended and that length declared."""
    out = []
    stats = {"flips": 0, "resealed": 0, "differ": 0, "length_differs": 0}
    rng = _rng(202)
    for kind in ("sparse", "text"):
        raw = _data(kind, 20000, rng)
        for cname, stream in (("l1", _level(raw, 1)), ("l6", _level(raw, 6)), ("fixed", _level(raw, 6, zlib.Z_FIXED))):
            head, body = stream[:2], bytearray(stream[2:-4])
            for i, bit in enumerate(rng.integers(0, 8 * len(body), 400)):
                bit = int(bit)
                stats["flips"] += 1
                body[bit >> 3] ^= 1 << (bit & 7)
                d = zlib.decompressobj(-15)
                try:
                    got = d.decompress(bytes(body), MAX_STRIP + 1)
                    ok = d.eof and len(got) <= MAX_STRIP
                except zlib.error:
                    ok = False
                if ok:
                    # the deflate data may now end before the body does: what follows it would
                    # be read as the adler, so the body is cut at the end of the data
                    used = len(body) - len(d.unused_data)
                    s = head + bytes(body[:used]) + zlib.adler32(got).to_bytes(4, "big")
                    out.append((f"reseal:{kind}:{cname}:{i}:bit{bit}", s, len(got), got))
                    stats["resealed"] += 1
                    stats["differ"] += got != raw
                    stats["length_differs"] += len(got) != len(raw)
                body[bit >> 3] ^= 1 << (bit & 7)
    return out, stats


def _plain_mutants():
    out = []
    raw = _data("image", 3000, _rng(303))
    bases = (("l6", _level(raw, 6)), ("l1", _level(raw, 1)), ("fixed", _level(raw, 6, zlib.Z_FIXED)),
             ("l0", _level(raw, 0)), ("huff", _level(raw, 6, zlib.Z_HUFFMAN_ONLY)))
    for name, s in bases:
        for bit in range(8 * 96):
            m = bytearray(s)
            m[bit >> 3] ^= 1 << (bit & 7)
            out.append((f"flip:{name}:{bit}", bytes(m), 3000, None))
        for n in range(len(s)):
            out.append((f"trunc:{name}:{n}", s[:n], 3000, None))
        out.append((f"len-1:{name}", s, 2999, None))
        out.append((f"len+1:{name}", s, 3001, None))
    return [(n, s, ln, zlib_verdict(s, ln)) for n, s, ln, _ in out]


# ---- hand-built blocks --------------------------------------------------------------------

_LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195,
             227, 258)
_LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
_DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
              4097, 6145, 8193, 12289, 16385, 24577)
_DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)


def _fixed_sym(b, s):
    """A literal/length symbol 0..287 in the fixed code (RFC 1951 3.2.6)."""
    if s < 144:
        b.code(0x30 + s, 8)
    elif s < 256:
        b.code(0x190 + s - 144, 9)
    elif s < 280:
        b.code(s - 256, 7)
    else:
        b.code(0xC0 + s - 280, 8)


def _length(b, length, sym=_fixed_sym):
    i = 28 if length == 258 else max(j for j in range(28) if _LEN_BASE[j] <= length)
    sym(b, 257 + i)
    b.put(length - _LEN_BASE[i], _LEN_EXTRA[i])


def _fixed_match(b, length, dist):
    _length(b, length)
    i = max(j for j in range(30) if _DIST_BASE[j] <= dist)
    b.code(i, 5)
    b.put(dist - _DIST_BASE[i], _DIST_EXTRA[i])


def _start(cmf=0x78, flg=0x9C):
    b = _Bits()
    b.put(cmf, 8)
    b.put(flg, 8)
    return b


def _stored(b, data, final=0, nlen=None):
    b.put(final, 1)
    b.put(0, 2)
    if b.n:
        b.put(0, 8 - b.n)
    b.put(len(data), 16)
    b.put((len(data) ^ 0xFFFF) if nlen is None else nlen, 16)
    b.out += data          # byte aligned here


def _seal(b, raw):
    """(stream, out_len, want) of a valid stream: the adler32 after the byte-aligned end."""
    return b.bytes() + zlib.adler32(raw).to_bytes(4, "big"), len(raw), raw


def _prefix_then_match(p, length, dist):
    """p bytes in a stored block, then a fixed block with one match and the end-of-block code."""
    pre = bytes(_rng(p + dist).integers(0, 256, p, dtype=np.uint8))
    b = _start()
    if p:
        _stored(b, pre)
    b.put(1, 1)
    b.put(1, 2)
    _fixed_match(b, length, dist)
    _fixed_sym(b, 256)
    if dist > p:
        return b.bytes() + bytes(8), p + length, None
    raw = bytearray(pre)
    for _ in range(length):
        raw.append(raw[-dist])
    return _seal(b, bytes(raw))


def _dynamic_head(b, hlit, hdist, clen, final=1):
    b.put(final, 1)
    b.put(2, 2)
    b.put(hlit - 257, 5)
    b.put(hdist - 1, 5)
    b.put(19 - 4, 4)
    for s in _CLEN_ORDER:
        b.put(clen.get(s, 0), 3)
    return _canonical({s: n for s, n in clen.items() if n})


def _dynamic_trees(b, litlen, dist):
    """A final dynamic block's header and trees; lengths 0, 1 and 2 only
    (sent with code-length symbols 0, 1, 2 and 18, a complete 2-bit code).
    -> (literal/length codes, distance codes)."""
    cl = _dynamic_head(b, len(litlen), len(dist), {0: 2, 1: 2, 2: 2, 18: 2})
    seq = list(litlen) + list(dist)
    i = 0
    while i < len(seq):
        run = 1
        while i + run < len(seq) and seq[i + run] == seq[i]:
            run += 1
        if seq[i] == 0 and run >= 11:
            r = min(run, 138)
            b.code(*cl[18])
            b.put(r - 11, 7)
            i += r
        else:
            b.code(*cl[seq[i]])
            i += 1
    lit = _canonical({s: n for s, n in enumerate(litlen) if n})
    dst = _canonical({s: n for s, n in enumerate(dist) if n}) if any(dist) else {}
    return lit, dst


def _lens(n, ones):
    a = [0] * n
    for s, v in ones.items():
        a[s] = v
    return a


def _hand_built():
    """-> [(name, stream, out_len, want or None, the GPU inflate's status)]"""
    out = []

    def add(name, triple, status):
        out.append(("hand:" + name, triple[0], triple[1], triple[2], status))

    # a match's distance against the bytes written so far
    add("dist=p:1", _prefix_then_match(1, 3, 1), 0)
    add("dist=p:32768", _prefix_then_match(32768, 3, 32768), 0)
    add("dist=p+1:0", _prefix_then_match(0, 3, 1), -4)
    add("dist=p+1:1", _prefix_then_match(1, 3, 2), -4)
    add("dist=p+1:32767", _prefix_then_match(32767, 3, 32768), -4)   # p + 1 = 32 769 has no distance code
    add("far258:32768", _prefix_then_match(32768, 258, 32768), 0)
    add("far258:65278", _prefix_then_match(65278, 258, 32768), 0)     # ends at byte 65 536: the ring wraps
    b = _start()
    b.put(1, 1)
    b.put(1, 2)
    _fixed_sym(b, 0x5A)
    for _ in range(254):
        _fixed_match(b, 258, 1)
    _fixed_match(b, 3, 1)
    _fixed_sym(b, 256)
    add("run258", _seal(b, b"\x5A" * 65536), 0)
    # codes the fixed trees have and the format does not
    for d in (30, 31):
        b = _start()
        b.put(1, 1)
        b.put(1, 2)
        for _ in range(4):
            _fixed_sym(b, 65)
        _length(b, 3)
        b.code(d, 5)
        _fixed_sym(b, 256)
        add(f"distcode{d}", (b.bytes() + bytes(8), 7, None), -3)
    for s in (286, 287):
        b = _start()
        b.put(1, 1)
        b.put(1, 2)
        for _ in range(4):
            _fixed_sym(b, 65)
        _fixed_sym(b, s)
        b.code(0, 5)
        _fixed_sym(b, 256)
        add(f"lensym{s}", (b.bytes() + bytes(8), 7, None), -3)
    # block headers
    b = _start()
    _stored(b, b"abcdef", 1, nlen=(6 ^ 0xFFFF) ^ 0x0100)
    add("nlen", (b.bytes() + zlib.adler32(b"abcdef").to_bytes(4, "big"), 6, None), -2)
    b = _start()
    b.put(1, 1)
    b.put(3, 2)
    add("btype3", (b.bytes() + bytes(16), 6, None), -2)
    for name, hlit, hdist in (("hlit30", 287, 1), ("hdist31", 257, 32)):
        b = _start()
        _dynamic_head(b, hlit, hdist, {0: 2, 1: 2, 2: 2, 18: 2})
        add(name, (b.bytes() + bytes(64), 6, None), -2)
    b = _start()
    cl = _dynamic_head(b, 257, 1, {16: 1, 0: 1})
    b.code(*cl[16])
    b.put(0, 2)
    add("repeat_first", (b.bytes() + bytes(64), 6, None), -2)
    b = _start()
    cl = _dynamic_head(b, 257, 1, {18: 1, 0: 1})
    for _ in range(2):          # 2 x 138 zeros > 257 + 1 lengths
        b.code(*cl[18])
        b.put(127, 7)
    add("repeat_past_end", (b.bytes() + bytes(64), 6, None), -2)
    # distance trees with no code, and with a single code of length 1
    b = _start()
    lit, _ = _dynamic_trees(b, _lens(257, {97: 1, 98: 2, 256: 2}), [0])
    for s in (97, 98, 97, 97, 98, 256):
        b.code(*lit[s])
    add("no_distance_codes", _seal(b, b"abaab"), 0)
    for name, bit, status in (("one_distance_code", 0, 0), ("one_distance_code_twin", 1, -3)):
        b = _start()
        lit, _ = _dynamic_trees(b, _lens(258, {97: 1, 256: 2, 257: 2}), [1])
        for s in (97, 97, 97, 257):
            b.code(*lit[s])
        b.put(bit, 1)           # the distance tree's only code is "0" (distance 1); "1" is unused
        b.code(*lit[256])
        add(name, _seal(b, b"a" * 6) if status == 0 else (b.bytes() + bytes(8), 6, None), status)
    # zlib headers (RFC 1950), each with the one defect named
    body = zlib.compress(b"header", 6)[2:]

    def fcheck(cmf, flg):
        return flg + (31 - ((cmf << 8) | flg) % 31) % 31

    add("cm7", (bytes([0x77, fcheck(0x77, 0x80)]) + body, 6, None), -1)
    add("cinfo8", (bytes([0x88, fcheck(0x88, 0x80)]) + body, 6, None), -1)
    add("fdict", (bytes([0x78, fcheck(0x78, 0xA0)]) + body, 6, None), -1)
    add("fcheck", (bytes([0x78, 0x9D]) + body, 6, None), -1)
    add("cinfo0", (bytes([0x08, fcheck(0x08, 0x80)]) + body, 6, b"header"), 0)   # a 256-byte window is valid
    return out


# ---- the corpus ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _corpus():
    res, stats = _resealed()
    hand = _hand_built()
    entries = _encoder_shapes() + res + _plain_mutants() + [h[:4] for h in hand]
    return entries, stats, {h[0]: h[4] for h in hand}


def inflate_corpus():
    """[(name, stream, out_len, want bytes or None)]; want is None when zlib
    rejects the stream or its output is not out_len bytes."""
    return _corpus()[0]


def reseal_stats():
    """{"flips", "resealed", "differ" (from the base's bytes), "length_differs"}"""
    return dict(_corpus()[1])


def hand_status():
    """{name of a hand-built entry: the GPU inflate's status (0 = accepted)}"""
    return dict(_corpus()[2])


# ---- CBAAC payloads -----------------------------------------------------------------------

def prior_row(sym):
    """Container version 2's prior of a frame's symbols: 1 + floor(hist * 8192 / n)."""
    hist = np.bincount(np.asarray(sym, np.uint8).ravel(), minlength=256).astype(np.uint64)
    return (1 + hist * 8192 // max(int(np.size(sym)), 1)).astype(np.uint16)


def segment_row(prior, seg, nseg):
    """The prior row of segment seg of nseg (version 3: row floor(seg * rows / nseg))."""
    if prior is None or prior.ndim == 1:
        return prior
    return prior[seg * prior.shape[0] // nseg]


PAYLOAD_KINDS = ("valid", "half", "one", "none", "bitflip", "random", "zeros", "ones")


def cbaac_payloads(encode, order, seg_len):
    """[(kind, order, seg_len, n, prior rows or None, seg_bytes, payload, symbols or None)]
    for one order and segment length.  encode(symbols, order, prior row or
    None) -> bytes is the host coder; `symbols` is what the payload encodes
    where it is the host coder's own output, else None."""
    out = []
    rng = _rng(404 + order + seg_len)
    unrelated = [np.clip(np.rint(rng.laplace(m, s, 5000)), 0, 255).astype(np.uint8)
                 for m, s in ((128, 1.0), (120, 6.0), (140, 30.0))]
    priors = (None, prior_row(unrelated[1]), np.stack([prior_row(u) for u in unrelated]))
    for n in (1, 255, 256, 257, 10001):
        sym = np.clip(np.rint(rng.laplace(128, 2.5, n)), 0, 255).astype(np.uint8)
        nseg = (n + seg_len - 1) // seg_len
        for prior in priors:
            segs = [encode(sym[i * seg_len:(i + 1) * seg_len], order, segment_row(prior, i, nseg))
                    for i in range(nseg)]
            for kind in PAYLOAD_KINDS:
                if kind == "valid":
                    cut = segs
                elif kind == "half":
                    cut = [s[:len(s) // 2] for s in segs]
                elif kind == "one":
                    cut = [s[:1] for s in segs]
                elif kind == "none":
                    cut = [b"" for s in segs]
                elif kind == "bitflip":
                    cut = []
                    for s in segs:
                        m = bytearray(s)
                        if m:
                            bit = int(rng.integers(0, 8 * len(m)))
                            m[bit >> 3] ^= 0x80 >> (bit & 7)
                        cut.append(bytes(m))
                elif kind == "random":
                    cut = [bytes(rng.integers(0, 256, int(rng.integers(0, 2 * len(s) + 2)), dtype=np.uint8))
                           for s in segs]
                else:
                    cut = [bytes([0x00 if kind == "zeros" else 0xFF]) * len(s) for s in segs]
                out.append((kind, order, seg_len, n, prior, np.array([len(c) for c in cut], np.int64), b"".join(cut),
                            sym if kind == "valid" else None))
    return out


# ---- index frames for the transforms --------------------------------------------------------

PLANE_CLASSES = ("uniform", "edges", "zeros", "max", "smooth", "equal")


def index_plane(cls, shape, dtype, rng):
    """Index values of one class, of `shape` and dtype uint8 (DCT indices, DWT
    details) or uint16 (the DWT's LL subband):
      uniform  every value of the type, uniformly;
      edges    only {0, 1, mid - 1, mid, mid + 1, max}, mid = 128 or 32768;
      zeros    all 0;          max      all 255 / 65535;
      smooth   a slow ramp plus small noise around the type's middle;
      equal    one random value everywhere."""
    dtype = np.dtype(dtype)
    top = int(np.iinfo(dtype).max)
    mid = (top + 1) // 2
    if cls == "uniform":
        return rng.integers(0, top + 1, shape).astype(dtype)
    if cls == "edges":
        return rng.choice(np.array([0, 1, mid - 1, mid, mid + 1, top]), shape).astype(dtype)
    if cls == "zeros":
        return np.zeros(shape, dtype)
    if cls == "max":
        return np.full(shape, top, dtype)
    if cls == "equal":
        return np.full(shape, int(rng.integers(0, top + 1)), dtype)
    if cls == "smooth":
        y = np.arange(shape[0], dtype=np.float64).reshape((-1,) + (1,) * (len(shape) - 1))
        x = np.arange(shape[1], dtype=np.float64).reshape((1, -1) + (1,) * (len(shape) - 2)) if len(shape) > 1 else 0.0
        v = mid + (top / 6.0) * np.sin(y / 9.0 + x / 23.0) + rng.normal(0, top / 100.0, shape)
        return np.clip(np.rint(v), 0, top).astype(dtype)
    raise ValueError(cls)


def dct_index_frames(Hp, Wp, seed):
    """One Hp x Wp x 3 u8 index frame per class, in PLANE_CLASSES' order."""
    rng = _rng(seed)
    return np.stack([index_plane(c, (Hp, Wp, 3), np.uint8, rng) for c in PLANE_CLASSES])


# (class of the LL subband, class of the details): every class on both, then
# sets whose bands differ, where the inverse kernels' per-band paths differ most
DWT_SETS = tuple((c, c) for c in PLANE_CLASSES) + (("uniform", "max"), ("max", "zeros"), ("zeros", "uniform"),
                                                   ("edges", "smooth"))
DWT_SET_NAMES = tuple(f"{a}/{b}" for a, b in DWT_SETS)


def dwt_subband_sets(shapes, levels, seed):
    """One subband set per entry of DWT_SETS: {LL_levels: u16, LH/HL/HH_r:
    u8}, each h_r x w_r x 3 with shapes[r - 1] = (h_r, w_r) as the encoder
    lays them out."""
    rng = _rng(seed)
    sets = []
    for ll, det in DWT_SETS:
        h, w = shapes[levels - 1]
        sb = {f"LL_{levels}": index_plane(ll, (h, w, 3), np.uint16, rng)}
        for r in range(levels, 0, -1):
            h, w = shapes[r - 1]
            for s in ("LH", "HL", "HH"):
                sb[f"{s}_{r}"] = index_plane(det, (h, w, 3), np.uint8, rng)
        sets.append(sb)
    return sets

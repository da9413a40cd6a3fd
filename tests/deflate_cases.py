"""Shared deflate test inputs (CPU harness and GPU kernel tests): the named
corpus, K1's lazy/non-lazy rule restated for the host, and a token view of a
zlib stream (block kinds, literals, match lengths and distances)."""
import functools

import numpy as np

STRIP = 65536       # vcf_zlib_max_strip
MAX_DIST = 32506    # zlib: wsize - MIN_LOOKAHEAD
NEAR_DIST = 7872    # vcf_deflate.hip kNearDist: chain candidates further back are read from HBM
LEVELS = (4, 5, 6, 7, 8, 9)


# ---- K1's parse-order rule (vcf_deflate.hip zlib_sort_kernel) ---------------
def lazy_rule(b: bytes):
    """-> (distinct, n - 2, is_lazy) as K1 computes them for the strip `b`.

    The positions 0 .. n-3 carry zlib's 15-bit hash of their three bytes.  K1
    sorts them by hash, positions increasing inside a hash, so a position's
    predecessor in that order is the newest earlier position with its hash
    (zlib's head[] as the position is inserted).  A position counts as distinct
    unless that predecessor lies in its own group of 64 positions,
    q >= (p & ~63); the strip takes the lazy parse iff 2 * distinct < n - 2
    (kLazyDiv = 2).  A strip shorter than 3 bytes has no position: 0 < 0 is
    false, it is non-lazy."""
    a = np.frombuffer(bytes(b), np.uint8).astype(np.int64)
    n = a.size
    np_ = max(n - 2, 0)
    if np_ == 0:
        return 0, np_, False
    h = (((a[:-2] & 31) << 10) ^ (a[1:-1] << 5) ^ a[2:]) & 0x7fff
    order = np.argsort(h, kind="stable")
    hs = h[order]
    has_prev = np.zeros(np_, bool)
    has_prev[1:] = hs[1:] == hs[:-1]
    prev = np.zeros(np_, np.int64)
    prev[1:] = order[:-1]
    repeat = has_prev & (prev >= (order & ~63))
    distinct = int(np_ - repeat.sum())
    return distinct, np_, 2 * distinct < np_


# ---- a zlib stream (RFC 1950/1951) as its LZ77 tokens -----------------------
_LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195,
          227, 258]
_LEXT = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
_DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
          4097, 6145, 8193, 12289, 16385, 24577]
_DEXT = [0, 0, 0, 0] + [i // 2 for i in range(2, 28)]
_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
STORED, FIXED, DYNAMIC = 0, 1, 2   # block kinds (BTYPE)


class _Bits:
    """LSB-first bit reader; bytes past the end read as zero (a truncated stream
    then ends in a ValueError of the decoder, not an IndexError)."""

    def __init__(self, data: bytes):
        self.d, self.pos, self.acc, self.n = data, 0, 0, 0

    def need(self, k: int) -> None:
        while self.n < k:
            if self.pos > len(self.d) + 8:
                raise ValueError("stream ends inside a block")
            self.acc |= (self.d[self.pos] if self.pos < len(self.d) else 0) << self.n
            self.pos += 1
            self.n += 8

    def get(self, k: int) -> int:
        self.need(k)
        v = self.acc & ((1 << k) - 1)
        self.acc >>= k
        self.n -= k
        return v

    def align(self) -> None:
        self.get(self.n & 7)


def _decoder(lengths):
    codes = {}
    bl = [0] * 16
    for l in lengths:
        if l:
            bl[l] += 1
    nxt, code = [0] * 16, 0
    for b in range(1, 16):
        code = (code + bl[b - 1]) << 1
        nxt[b] = code
    for s, l in enumerate(lengths):
        if l:
            codes[(l, nxt[l])] = s
            nxt[l] += 1
    return codes


def _sym(bits: _Bits, dec) -> int:
    bits.need(15)
    acc, code = bits.acc, 0
    for l in range(1, 16):
        code = (code << 1) | (acc & 1)
        acc >>= 1
        s = dec.get((l, code))
        if s is not None:
            bits.acc = acc
            bits.n -= l
            return s
    raise ValueError("bad code")


def tokens(stream: bytes):
    """-> (tokens, blocks, inflated bytes).  A token is (position, length,
    distance), length 0 for a literal (distance = the byte; a stored block's
    bytes are literals too); a block is (position of its first byte, kind)."""
    bits = _Bits(stream[2:])
    out, toks, blocks = bytearray(), [], []
    while True:
        final = bits.get(1)
        kind = bits.get(2)
        blocks.append((len(out), kind))
        if kind == STORED:
            bits.align()
            n = bits.get(16)
            if bits.get(16) != n ^ 0xffff:
                raise ValueError("stored block length check")
            for _ in range(n):
                b = bits.get(8)
                toks.append((len(out), 0, b))
                out.append(b)
        elif kind > DYNAMIC:
            raise ValueError("bad block type")
        else:
            if kind == FIXED:
                ll = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
                dl = [5] * 30
            else:
                hlit, hdist, hclen = bits.get(5) + 257, bits.get(5) + 1, bits.get(4) + 4
                cl = [0] * 19
                for i in range(hclen):
                    cl[_ORDER[i]] = bits.get(3)
                cdec = _decoder(cl)
                lens = []
                while len(lens) < hlit + hdist:
                    s = _sym(bits, cdec)
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        lens += [lens[-1]] * (3 + bits.get(2))
                    elif s == 17:
                        lens += [0] * (3 + bits.get(3))
                    else:
                        lens += [0] * (11 + bits.get(7))
                ll, dl = lens[:hlit], lens[hlit:]
            ldec, ddec = _decoder(ll), _decoder(dl)
            while True:
                s = _sym(bits, ldec)
                if s < 256:
                    toks.append((len(out), 0, s))
                    out.append(s)
                elif s == 256:
                    break
                else:
                    i = s - 257
                    ln = _LBASE[i] + bits.get(_LEXT[i])
                    ds = _sym(bits, ddec)
                    dist = _DBASE[ds] + bits.get(_DEXT[ds])
                    if dist > len(out):
                        raise ValueError("distance before the start")
                    toks.append((len(out), ln, dist))
                    for _ in range(ln):
                        out.append(out[-dist])
        if final:
            break
    return toks, blocks, bytes(out)


def first_divergence(a: bytes, b: bytes):
    """(index, token of a, token of b, context) of the first differing token."""
    ta, ba, oa = tokens(a)
    tb, bb, ob = tokens(b)
    for i, (x, y) in enumerate(zip(ta, tb)):
        if x != y:
            return {"token": i, "a": x, "b": y, "prev": ta[max(0, i - 3):i], "blocks_a": ba[:6], "blocks_b": bb[:6],
                    "a_inflates_to_b": oa == ob}
    return {"token": None, "len_a": len(ta), "len_b": len(tb), "blocks_a": ba, "blocks_b": bb,
            "a_inflates_to_b": oa == ob}


def describe_mismatch(got: bytes, want: bytes) -> str:
    """Where `got` (the kernel's stream) leaves `want` (zlib's): the first
    differing token, or how `got` fails to decode."""
    try:
        return repr(first_divergence(bytes(got), bytes(want)))
    except (ValueError, IndexError) as e:
        return f"stream of {len(got)} bytes (zlib: {len(want)}) does not decode: {e!r}"


def slide_nil_strip(n: int = 65400, seed: int = 3) -> bytes:
    """A strip where zlib's slide_hash NIL mapping decides the output.

    zlib 1.2.11 slides the window once, at the first deflate_slow step with
    strstart >= wsize + MAX_DIST = 65274, and slide_hash turns a head entry
    equal to wsize (input position 32768) into NIL.  Here the same 8 bytes
    sit at 32768 and 65274, no position in between shares their hash, and
    unique bytes before 65274 make the parse reach it as a fresh position:
    zlib emits a literal there (and matches from 65275 on), a matcher that
    treats 32768 as a live head emits a match of 8 at distance MAX_DIST.
    The background is a 16-symbol alphabet so the blocks are Huffman coded
    (a stored block would hide the difference)."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 16, n, dtype=np.uint8)
    a[65266:65274] = np.arange(240, 248)
    a[32760:32768] = np.arange(224, 232)
    pat = np.array([101, 99, 120, 105, 110, 103, 117, 107], np.uint8)
    a[32768:32776] = pat
    a[65274:65282] = pat

    def hashes(x):
        b = x.astype(np.int64)
        return (((b[:-2] & 31) << 10) ^ (b[1:-1] << 5) ^ b[2:]) & 0x7fff

    for _ in range(100):
        h = hashes(a)
        bad = [q for q in np.nonzero(h == h[32768])[0] if 32768 < q < 65274]
        if not bad:
            break
        for q in bad:
            a[q + 2 if q + 2 < 65266 and not (32768 <= q + 2 < 32776) else q - 1] ^= 0x5
    else:
        raise AssertionError("could not isolate the planted hash")
    return a.tobytes()


# ---- the corpus ---------------------------------------------------------------
def _rng(name: str) -> np.random.Generator:
    return np.random.default_rng([ord(c) for c in name])


def _u8(a) -> bytes:
    return np.asarray(a).astype(np.uint8).tobytes()


def _image(n: int, rng) -> np.ndarray:
    x = np.arange(n)
    return np.clip(128 + 40 * np.sin(x / 300.0) + rng.normal(0, 3, n), 0, 255).astype(np.uint8)


def _noisyflat(n: int, frac: float, rng) -> np.ndarray:
    a = np.full(n, 128, np.uint8)
    m = rng.random(n) < frac
    a[m] = rng.integers(0, 256, int(m.sum()))
    return a


def _runs(n: int, rng) -> np.ndarray:
    out = bytearray()
    while len(out) < n:
        out += bytes([int(rng.integers(0, 256))]) * int(rng.integers(1, 300))
    return np.frombuffer(bytes(out[:n]), np.uint8)


def _tiled(P: int, n: int, rng) -> np.ndarray:
    return np.resize(rng.integers(0, 256, P, dtype=np.uint8), n)


def _sparse_rows(P: int, n: int, rng) -> np.ndarray:
    """C4's "row above" at a controlled distance: a row of P bytes, 3 % of them
    not 128, tiled, with 0.3 % of the strip's bytes replaced afterwards."""
    row = np.full(P, 128, np.uint8)
    m = rng.random(P) < 0.03
    row[m] = rng.integers(100, 160, int(m.sum()))
    a = np.resize(row, n).copy()
    m = rng.random(n) < 0.003
    a[m] = rng.integers(100, 160, int(m.sum()))
    return a


def random_then_flat(k: int, n: int = STRIP) -> bytes:
    """k random bytes (always the same sequence) followed by flat 128."""
    a = np.full(n, 128, np.uint8)
    a[:k] = _rng("random_then_flat").integers(0, 256, n, dtype=np.uint8)[:k]
    return a.tobytes()


@functools.lru_cache(maxsize=None)
def threshold_pair():
    """-> (k_lazy, k_nonlazy): the prefix lengths of random_then_flat closest to
    K1's threshold from each side.  The distinct count grows by about one per
    random byte, so the smallest non-lazy k is found by bisection and its
    neighbourhood searched for the largest lazy k below it."""
    lo, hi = 0, STRIP   # lo lazy, hi non-lazy
    assert lazy_rule(random_then_flat(lo))[2] and not lazy_rule(random_then_flat(hi))[2]
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if lazy_rule(random_then_flat(mid))[2]:
            lo = mid
        else:
            hi = mid
    k_non = min(k for k in range(max(0, hi - 64), hi + 1) if not lazy_rule(random_then_flat(k))[2])
    k_lazy = max(k for k in range(max(0, k_non - 64), k_non) if lazy_rule(random_then_flat(k))[2])
    return k_lazy, k_non


TILED_P = (300, NEAR_DIST, MAX_DIST, MAX_DIST + 1)
SPARSE_P = (5760, 7616, NEAR_DIST, NEAR_DIST + 1, 8192, 16384, MAX_DIST - 1, MAX_DIST, MAX_DIST + 1, 32768)
FUZZ_KINDS = ("alphabet", "phrase", "pm2", "runs50")
SHORT_LENGTHS = (1, 2, 3, 4, 5, 63, 64, 65, 257, 258, 259, 400)
SLIDE_LENGTHS = (65270, 65273, 65274, 65275, 65280, 65535)


def fuzz_strip(kind: str, n: int, rng) -> bytes:
    """The four generators of test_deflate.py::test_harness_equals_zlib_fuzz."""
    if kind == "alphabet":
        return rng.integers(0, int(rng.integers(1, 256)), n, dtype=np.uint8).tobytes()
    if kind == "phrase":
        ph = rng.integers(0, 256, int(rng.integers(3, 3000)), dtype=np.uint8)
        a = np.resize(ph, n).copy()
        m = rng.random(n) < rng.random() * 0.05
        a[m] = rng.integers(0, 256, int(m.sum()))
        return a.tobytes()
    if kind == "pm2":
        return (128 + rng.integers(-2, 3, n)).astype(np.uint8).tobytes()
    assert kind == "runs50"
    return np.repeat(rng.integers(0, 256, n // 50 + 1, dtype=np.uint8), 50)[:n].tobytes()


@functools.lru_cache(maxsize=None)
def _corpus() -> tuple:
    n = STRIP
    c = {}
    # non-lazy by K1's rule
    c["text"] = (b"the quick brown fox jumps over the lazy dog " * 2000)[:n]
    c["alphabet4"] = _rng("alphabet4").integers(0, 4, 60000, dtype=np.uint8).tobytes()
    p = 0.5 ** np.arange(1, 33)
    c["skewed"] = _rng("skewed").choice(np.arange(32, dtype=np.uint8), n, p=p / p.sum()).tobytes()
    c["pm2"] = _u8(128 + _rng("pm2").integers(-2, 3, n))
    c["image"] = _image(n, _rng("image")).tobytes()
    c["random"] = _rng("random").integers(0, 256, n, dtype=np.uint8).tobytes()
    c["alphabet16"] = _rng("alphabet16").integers(0, 16, n, dtype=np.uint8).tobytes()
    for P in TILED_P:
        c[f"tiled_{P}"] = _tiled(P, n, _rng(f"tiled_{P}")).tobytes()
    # lazy
    c["zeros"] = bytes(n)
    c["runs"] = _runs(n, _rng("runs")).tobytes()
    c["alphabet2"] = _rng("alphabet2").integers(0, 2, n, dtype=np.uint8).tobytes()
    c["pm1"] = _u8(128 + _rng("pm1").integers(-1, 2, n))
    c["noisyflat"] = _noisyflat(n, 0.12, _rng("noisyflat")).tobytes()
    for P in SPARSE_P:
        c[f"sparse_rows_{P}"] = _sparse_rows(P, n, _rng(f"sparse_rows_{P}")).tobytes()
    # either side of K1's threshold
    k_lazy, k_non = threshold_pair()
    c["threshold_lazy"] = random_then_flat(k_lazy)
    c["threshold_nonlazy"] = random_then_flat(k_non)
    # lazy strips of more than one block: enough literals at the front to fill the
    # symbol buffer (16 383 symbols) once, few enough to stay under K1's threshold.
    # 12 000 random bytes: dynamic, dynamic; 20 000: stored, dynamic; 8 000 image
    # bytes: dynamic, then a fixed block
    r = _rng("random_noisyflat")
    c["random_noisyflat"] = (r.integers(0, 256, 12000, dtype=np.uint8).tobytes() +
                             _noisyflat(n - 12000, 0.10, r).tobytes())
    r = _rng("random20k_noisyflat")
    c["random20k_noisyflat"] = (r.integers(0, 256, 20000, dtype=np.uint8).tobytes() +
                                _noisyflat(n - 20000, 0.08, r).tobytes())
    r = _rng("image_noisyflat")
    c["image_noisyflat"] = _image(8000, r).tobytes() + _noisyflat(n - 8000, 0.16, r).tobytes()
    # short strips and strips that end around zlib's window slide (65274)
    for kind in FUZZ_KINDS:
        for ln in SHORT_LENGTHS + SLIDE_LENGTHS:
            c[f"fuzz_{kind}_{ln}"] = fuzz_strip(kind, ln, _rng(f"fuzz_{kind}_{ln}"))
    c["slide_nil"] = slide_nil_strip()
    return tuple(c.items())


def corpus() -> dict:
    """The named strips, in a fixed order, from fixed seeds.  tests/test_deflate.py
    asserts the properties the entries are there for (which parse K1 picks, block
    kinds, far matches, ...): an entry that loses its property is a failure there."""
    return dict(_corpus())


@functools.lru_cache(maxsize=None)
def small_strip_frame(strip_bytes: int, n_nonlazy: int, n_lazy: int, tail: int = 0) -> bytes:
    """One frame that cuts into n_nonlazy + n_lazy strips of strip_bytes and, with
    `tail`, a last strip of `tail` bytes.  The non-lazy strips are image noise and
    random bytes in turn, the lazy ones flat 128 and sparse (3 % non-128) in turn;
    the two kinds are interleaved by a fixed permutation, not alternating.  Which
    parse K1 picks for each strip is for the caller to check with lazy_rule."""
    rng = _rng(f"small_{strip_bytes}_{n_nonlazy}_{n_lazy}")
    total = n_nonlazy + n_lazy
    is_lazy = np.zeros(total, bool)
    is_lazy[rng.permutation(total)[:n_lazy]] = True
    a = np.empty((total, strip_bytes), np.uint8)
    x = np.arange(strip_bytes)
    for s in range(total):
        if is_lazy[s]:
            a[s] = 128
            if s % 2:
                m = rng.random(strip_bytes) < 0.03
                a[s, m] = rng.integers(100, 160, int(m.sum()))
        elif s % 2:
            a[s] = rng.integers(0, 256, strip_bytes, dtype=np.uint8)
        else:
            a[s] = np.clip(128 + 60 * np.sin(x / 37.0 + s) + rng.normal(0, 4, strip_bytes), 0, 255).astype(np.uint8)
    return a.tobytes() + rng.integers(0, 256, tail, dtype=np.uint8).tobytes()


def corpus_by_length() -> dict:
    """{length: [(name, bytes), ...]} in corpus order: the strips of one length go
    through one GPU call, as frames of one strip each."""
    out = {}
    for name, b in _corpus():
        out.setdefault(len(b), []).append((name, b))
    return out

"""The GPU deflate's restatement of zlib (vcf_amd/csrc/vcf_deflate.h), built
for the host with a sequential hash-chain matcher (tests/cpu/deflate_harness.cpp),
against zlib.compress itself -- the oracle of TIFF.py:29's strips (tifffile ->
zlib level 6).  CPU only; the GPU kernel is tests/test_deflate_gpu.py."""
import ctypes
import os
import shutil
import subprocess
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpu", "deflate_harness.cpp")


@pytest.fixture(scope="module")
def dh(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    so = str(tmp_path_factory.mktemp("dh") / "deflate_harness.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", os.path.join(ROOT, "vcf_amd", "csrc"),
                    SRC, "-o", so], check=True)
    lib = ctypes.CDLL(so)
    lib.dh_compress.restype = ctypes.c_longlong
    lib.dh_compress.argtypes = [ctypes.c_char_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_char_p, ctypes.c_longlong]

    def compress(b: bytes, level: int = 6) -> bytes:
        out = ctypes.create_string_buffer(len(b) + len(b) // 8 + 1024)
        r = lib.dh_compress(b, len(b), level, out, len(out))
        assert r >= 0, r
        return out.raw[:r]
    return compress


def _cases():
    rng = np.random.default_rng(0)
    img = np.clip(128 + 40 * np.sin(np.arange(64 * 1100 * 3) / 300.0) + rng.normal(0, 3, 64 * 1100 * 3), 0, 255)
    img = img.astype(np.uint8).tobytes()
    runs = bytearray()
    while len(runs) < 65536:
        runs += bytes([int(rng.integers(0, 256))]) * int(rng.integers(1, 300))
    p = 0.5 ** np.arange(1, 33)
    return {
        "empty": b"", "one": b"\x80", "two": b"ab", "three": b"abc", "flat": b"\x80" * 5000,
        "random": rng.integers(0, 256, 40000, dtype=np.uint8).tobytes(),
        "alphabet4": rng.integers(0, 4, 60000, dtype=np.uint8).tobytes(),
        "text": (b"the quick brown fox jumps over the lazy dog " * 2000)[:65536],
        "runs": bytes(runs[:65536]),
        # skewed symbol distribution: Huffman lengths past 15 bits (gen_bitlen's overflow fix-up)
        "skewed": rng.choice(np.arange(32, dtype=np.uint8), 65536, p=p / p.sum()).tobytes(),
        "image_65536": img[:65536], "image_65300": img[:65300], "image_63360": img[:63360],
        # past wsize + MAX_DIST: zlib's window slides once and its stale bytes follow the end
        "zeros_65536": bytes(65536), "zeros_65280": bytes(65280), "random_65536": rng.integers(
            0, 256, 65536, dtype=np.uint8).tobytes(),
    }


def test_harness_slide_nil_head(dh):
    """slide_hash's NIL mapping of the head entry at input position wsize
    (ADVICE round 3): zlib writes a literal at strstart 65274 there."""
    from deflate_cases import slide_nil_strip
    b = slide_nil_strip()
    for level in (4, 5, 6, 7, 8, 9):
        assert dh(b, level) == zlib.compress(b, level), level


@pytest.mark.parametrize("level", [6, 4, 5, 7, 8, 9])
def test_harness_equals_zlib(dh, level):
    for name, b in _cases().items():
        assert dh(b, level) == zlib.compress(b, level), (name, level)


def test_harness_equals_zlib_fuzz(dh):
    rng = np.random.default_rng(7)
    for it in range(120):
        n = int(rng.choice([rng.integers(0, 400), rng.integers(0, 65537), rng.integers(65270, 65537)]))
        kind = it % 4
        if kind == 0:
            b = rng.integers(0, int(rng.integers(1, 256)), n, dtype=np.uint8).tobytes()
        elif kind == 1:
            ph = rng.integers(0, 256, int(rng.integers(3, 3000)), dtype=np.uint8)
            a = np.resize(ph, n).copy()
            m = rng.random(n) < rng.random() * 0.05
            a[m] = rng.integers(0, 256, int(m.sum()))
            b = a.tobytes()
        elif kind == 2:
            b = (128 + rng.integers(-2, 3, n)).astype(np.uint8).tobytes()
        else:
            b = np.repeat(rng.integers(0, 256, n // 50 + 1, dtype=np.uint8), 50)[:n].tobytes()
        level = int(rng.choice([6, 6, 4, 5, 7, 8, 9]))
        assert dh(b, level) == zlib.compress(b, level), (it, n, level)


def test_lazy_rule_hand_cases():
    """lazy_rule on strips whose count can be worked out by hand."""
    from deflate_cases import lazy_rule
    assert lazy_rule(b"") == (0, 0, False) and lazy_rule(b"ab") == (0, 0, False)
    assert lazy_rule(b"abc") == (1, 1, False)
    # one hash everywhere: only the first position of each group of 64 has no predecessor in its group
    assert lazy_rule(bytes(65536)) == (1024, 65534, True)
    assert lazy_rule(bytes(130)) == (2, 128, True)
    # period 64: every position's predecessor is exactly 64 back, in the group before
    assert lazy_rule(bytes(range(64)) * 4) == (254, 254, False)
    # period 32: in each group the first 32 positions look back into the group before
    assert lazy_rule(bytes(range(32)) * 8) == (32 * 4, 254, False)
    # 2 * distinct == n - 2 is not lazy; position 256 then opens a new group (distinct)
    assert lazy_rule(bytes(range(32)) * 8 + b"\x00\x01") == (32 * 4, 256, False)
    assert lazy_rule(bytes(range(32)) * 8 + b"\x00\x01\x02") == (32 * 4 + 1, 257, False)
    assert lazy_rule(bytes(range(16)) * 16) == (16 * 4, 254, True)

    def naive(b):   # the rule as stated, position by position
        n = len(b)
        h = [((b[p] & 31) << 10 ^ b[p + 1] << 5 ^ b[p + 2]) & 0x7fff for p in range(max(n - 2, 0))]
        distinct = sum(1 for p in range(len(h)) if not any(h[q] == h[p] for q in range(p & ~63, p)))
        return distinct, len(h), 2 * distinct < len(h)

    rng = np.random.default_rng(11)
    for it in range(60):
        n = int(rng.integers(0, 700))
        b = rng.integers(0, int(rng.integers(1, 6)) if it % 2 else 256, n, dtype=np.uint8).tobytes()
        assert lazy_rule(b) == naive(b), (it, n)


def test_token_view_roundtrip():
    """The token view decodes stored, fixed and dynamic blocks and reports them."""
    from deflate_cases import DYNAMIC, FIXED, STORED, tokens
    rng = np.random.default_rng(1)
    for b, kinds in ((b"abcabcabcabc", [FIXED]), (rng.integers(0, 256, 70000, dtype=np.uint8).tobytes(), [STORED] * 5),
                     (b"hello " * 3000, [DYNAMIC])):
        toks, blocks, out = tokens(zlib.compress(b, 6))
        assert out == b and [k for _, k in blocks] == kinds
        assert sum(t[1] or 1 for t in toks) == len(b)
    toks, _, _ = tokens(zlib.compress(b"abcabcabcabc", 6))
    # (position 0 is zlib's NIL: the first match starts at 4, not 3)
    assert toks == [(0, 0, 97), (1, 0, 98), (2, 0, 99), (3, 0, 97), (4, 8, 3)]


def _corpus_facts():
    """Per 64 KiB-class corpus entry: K1's rule and the token view of zlib level 6."""
    from deflate_cases import MAX_DIST, NEAR_DIST, corpus, lazy_rule, tokens
    facts = {}
    for name, b in corpus().items():
        distinct, np_, lazy = lazy_rule(b)
        toks, blocks, out = tokens(zlib.compress(b, 6))
        assert out == b, name
        m = [t for t in toks if t[1]]
        facts[name] = dict(n=len(b), distinct=distinct, np=np_, lazy=lazy, kinds=[k for _, k in blocks],
                           far=sum(t[2] > NEAR_DIST for t in m), seam=sum(7600 <= t[2] <= 8200 for t in m),
                           maxdist=sum(t[2] == MAX_DIST for t in m), l258=sum(t[1] == 258 for t in m))
    return facts


def test_corpus_properties():
    """The corpus holds what the GPU tests rely on it for: strips on both sides
    of K1's lazy rule and of the lazy parse's near/far split, multi-block strips,
    matches at MAX_DIST.  Conditions on the inputs (a seed that loses one is
    changed), re-derived here from lazy_rule and the tokens of zlib level 6."""
    from deflate_cases import DYNAMIC, FUZZ_KINDS, SHORT_LENGTHS, SLIDE_LENGTHS, STORED, STRIP, corpus, threshold_pair
    facts = _corpus_facts()
    full = {k: f for k, f in facts.items() if f["n"] == STRIP}
    lazy = {k: f for k, f in full.items() if f["lazy"]}
    non = {k: f for k, f in full.items() if not f["lazy"]}

    def prop(title, names, need=1):
        names = sorted(names)
        print(f"{title}: {len(names)} (need {need}): {', '.join(names)}")
        assert len(names) >= need, title

    prop("lazy 64 KiB strips", lazy, 10)
    prop("non-lazy 64 KiB strips", non, 10)
    tl, tn = facts["threshold_lazy"], facts["threshold_nonlazy"]
    print("threshold pair: k =", threshold_pair(), "2 * distinct - (n - 2) =", 2 * tl["distinct"] - tl["np"],
          2 * tn["distinct"] - tn["np"], "blocks", tl["kinds"], tn["kinds"])
    assert tl["lazy"] and not tn["lazy"]
    assert abs(2 * tl["distinct"] - tl["np"]) <= 64 and abs(2 * tn["distinct"] - tn["np"]) <= 64
    prop("lazy, >= 2 blocks, the first stored", [k for k, f in lazy.items()
                                                if len(f["kinds"]) >= 2 and f["kinds"][0] == STORED])
    prop("lazy, >= 2 dynamic blocks", [k for k, f in lazy.items() if f["kinds"].count(DYNAMIC) >= 2])
    prop("lazy, >= 50 matches further back than 7 872", [k for k, f in lazy.items() if f["far"] >= 50])
    prop("lazy, matches at distances 7 600 - 8 200", [k for k, f in lazy.items() if f["seam"]])
    prop("lazy, a match at distance 32 506", [k for k, f in lazy.items() if f["maxdist"]])
    prop("non-lazy, a match at distance 32 506", [k for k, f in non.items() if f["maxdist"]])
    prop("lazy, >= 30 matches of length 258", [k for k, f in lazy.items() if f["l258"] >= 30])
    prop("non-lazy, >= 30 matches of length 258", [k for k, f in non.items() if f["l258"] >= 30])
    prop("non-lazy, all blocks stored", [k for k, f in non.items() if set(f["kinds"]) == {STORED}])
    # the named classes are what they are named for
    for name in ("text", "alphabet4", "skewed", "pm2", "image", "random", "tiled_300", "tiled_7872", "tiled_32506",
                 "tiled_32507"):
        assert not facts[name]["lazy"], name
    for name in ["zeros", "runs", "alphabet2", "pm1", "noisyflat"] + [k for k in facts if k.startswith("sparse_rows_")]:
        assert facts[name]["lazy"], name
    assert facts["tiled_32506"]["kinds"] == [STORED, DYNAMIC, DYNAMIC] and facts["tiled_32506"]["l258"] >= 100
    assert facts["tiled_32507"]["far"] == 0 and set(facts["tiled_32507"]["kinds"]) == {STORED}
    assert len(facts["image"]["kinds"]) == 3 and facts["skewed"]["far"] >= 1000
    # the near/far split of the lazy parse: a row one byte longer than kNearDist moves the
    # row-above matches to the far side
    assert facts["sparse_rows_7873"]["far"] >= facts["sparse_rows_7872"]["far"] + 100
    names = set(corpus())
    assert all(f"fuzz_{k}_{n}" in names for k in FUZZ_KINDS for n in SHORT_LENGTHS + SLIDE_LENGTHS)
    assert "slide_nil" in names and len(corpus()["alphabet4"]) == 60000


@pytest.mark.parametrize("level", [6, 4, 5, 7, 8, 9])
def test_harness_equals_zlib_corpus(dh, level):
    """The restated algorithm (vcf_deflate.h, sequential matcher) on every corpus
    entry: a GPU failure on an entry that passes here is the kernels' own."""
    from deflate_cases import corpus, describe_mismatch
    for name, b in corpus().items():
        got, want = dh(b, level), zlib.compress(b, level)
        assert got == want, (name, level, describe_mismatch(got, want))


@pytest.mark.parametrize("case", range(5))
def test_zlib_rejects_corrupt_code_lengths(case):
    """The oracle side of tests/test_inflate_gpu.py::test_rejects_corrupt_code_lengths:
    zlib.decompress rejects each hand-built stream with the named message."""
    from deflate_corrupt import CASES
    name, stream, msg, _ = CASES[case]
    with pytest.raises(zlib.error, match=msg):
        zlib.decompress(stream)
